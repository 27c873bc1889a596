"""ctypes wrapper of the sequential CPU reference of stereo fusion (tests/fusion_ref/fusion_ref.cc, written from
DESIGN.md section 23; it shares pycolmap_amd/csrc/fusion_core.h with the kernel), built on first use into
tests/fusion_ref/_build/ with the flags of tests/ba_ref_lib.py.  The arguments and the result's form are
Context.fuse_depth_maps', so that a test swaps one for the other."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from pycolmap_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "fusion_ref" / "fusion_ref.cc"
DEPS = [ROOT / "pycolmap_amd" / "csrc" / "fusion_core.h", ROOT / "include" / "amc_fusion.h"]
LIB = ROOT / "tests" / "fusion_ref" / "_build" / "libfusionref.so"
REASONS = ("taken", "no_map", "earlier_image", "outside", "claimed", "in_cluster", "no_depth", "depth_error", "normal_error",
           "reproj_error", "cut_short")
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    LIB.parent.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or LIB.stat().st_mtime < max(f.stat().st_mtime for f in [SRC] + DEPS):
        tmp = LIB.with_name(LIB.name + ".tmp")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                        "-Wno-unused-function", "-shared", "-fPIC", str(SRC), "-o", str(tmp)], check=True)
        tmp.replace(LIB)
    lib = C.CDLL(str(LIB))
    V, I, U = C.c_void_p, C.c_int, C.c_uint32
    OP, PB = C.POINTER(_capi.FusionOpts), C.POINTER(_capi.FusionProblem)
    lib.furef_fuse.restype = V
    lib.furef_fuse.argtypes = [OP, PB, I]
    lib.furef_counts.restype = None
    lib.furef_counts.argtypes = [V, V]
    lib.furef_copy.restype = None
    lib.furef_copy.argtypes = [V] * 10
    lib.furef_free.restype = None
    lib.furef_free.argtypes = [V]
    lib.furef_measure.restype = None
    lib.furef_measure.argtypes = [PB, U, I, I, U, I, I, V]
    lib.furef_project.restype = I
    lib.furef_project.argtypes = [PB, U, V, V, V]
    _lib = lib
    return lib


_p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def _checked(o, pb, keep):
    """What the library refuses, the reference refuses too (it indexes without looking)."""
    n = int(pb.num_images)
    if not (o.min_num_pixels >= 0 and o.max_num_pixels >= max(1, o.min_num_pixels)
            and 1 <= o.max_traversal_depth <= _capi.FUSION_MAX_TRAVERSAL_DEPTH):
        raise ValueError("fusion_ref: an option is out of its range")
    if keep[11][:-1].size and int(keep[11][:-1].max()) >= n:
        raise ValueError("fusion_ref: a neighbour names an image out of range")


def fuse_depth_maps(images, K, R, t, depth_maps, normal_maps, neighbours, trace=False, **options):
    """The reference in Context.fuse_depth_maps' place: the same arguments, the same dict without the launch counts and
    timings.  trace=True adds "trace": an (L, 7) int32 array of cluster, parent member, child image, row, col, reason
    (an index into REASONS) and the members so far."""
    o = _capi.fusion_options(**options)
    pb, keep = _capi.fusion_inputs(images, K, R, t, depth_maps, normal_maps, neighbours)
    _checked(o, pb, keep)
    lib = load()
    h = lib.furef_fuse(C.byref(o), C.byref(pb), int(bool(trace)))
    try:
        cnt = np.zeros(5, np.uint64)
        lib.furef_counts(h, _p(cnt))
        n, nv, nt = int(cnt[0]), int(cnt[1]), int(cnt[4])
        one = lambda k, dt: np.zeros(max(k, 1), dt)  # noqa: E731
        xyz, normal, color = one(3 * n, np.float32), one(3 * n, np.float32), one(3 * n, np.uint8)
        simg, spix, nf = one(n, np.uint32), one(n, np.uint32), one(n, np.uint32)
        voff, vis, tr = one(n + 1, np.uint64), one(nv, np.uint32), one(7 * nt, np.int32)
        lib.furef_copy(h, _p(xyz), _p(normal), _p(color), _p(simg), _p(spix), _p(nf), _p(voff), _p(vis), _p(tr))
    finally:
        lib.furef_free(h)
    out = {"num_points": n, "xyz": xyz[:3 * n].reshape(n, 3), "normal": normal[:3 * n].reshape(n, 3),
           "color": color[:3 * n].reshape(n, 3), "seed_image": simg[:n], "seed_pixel": spix[:n], "num_fused": nf[:n],
           "vis_offsets": voff[:n + 1], "vis_images": vis[:nv], "num_seeds": int(cnt[2]), "num_truncated": int(cnt[3])}
    if trace:
        out["trace"] = tr[:7 * nt].reshape(nt, 7)
    return out


def measure(problem, seed_image, seed_row, seed_col, image, row, col):
    """The float32 quantities of the three tests for a seed pixel and a child pixel: (relative depth error, cosine,
    squared reprojection error, the seed's point, the child's point); problem = the arguments of fusion_inputs"""
    pb, keep = _capi.fusion_inputs(*problem)
    out = np.zeros(9, np.float32)
    load().furef_measure(C.byref(pb), seed_image, seed_row, seed_col, image, row, col, _p(out))
    return float(out[0]), float(out[1]), float(out[2]), out[3:6].copy(), out[6:9].copy()


def project(problem, image, X):
    """(u, v, depth) of the world point X in `image` and the pixel (row, col) that holds it, or None"""
    pb, keep = _capi.fusion_inputs(*problem)
    x = np.ascontiguousarray(X, np.float32)
    uvz, rc = np.zeros(3, np.float32), np.zeros(2, np.int32)
    ok = load().furef_project(C.byref(pb), image, _p(x), _p(uvz), _p(rc))
    return uvz, ((int(rc[0]), int(rc[1])) if ok else None)


class Context:
    """The reference where _capi.Context goes (StereoFusion._context_factory)"""

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def fuse_depth_maps(self, *args, **options):
        return fuse_depth_maps(*args, **options)
