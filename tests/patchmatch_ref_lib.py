"""ctypes wrapper of the sequential CPU reference of PatchMatch stereo (tests/patchmatch_ref/patchmatch_ref.cc, written
from DESIGN.md section 22; it shares pycolmap_amd/csrc/patchmatch_core.h with the kernels), built on first use into
tests/patchmatch_ref/_build/ with the flags of tests/ba_ref_lib.py.  The flat problem and the result's form are
_capi.patch_match_inputs' and Context.patch_match's, so that a test swaps one for the other."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from pycolmap_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "patchmatch_ref" / "patchmatch_ref.cc"
DEPS = [ROOT / "pycolmap_amd" / "csrc" / "patchmatch_core.h", ROOT / "include" / "amc_patchmatch.h"]
LIB = ROOT / "tests" / "patchmatch_ref" / "_build" / "libpatchmatchref.so"
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
    V, F, I, U = C.c_void_p, C.c_float, C.c_int, C.c_uint32
    OP, PB = C.POINTER(_capi.PatchMatchOpts), C.POINTER(_capi.PatchMatchProblem)
    lib.pmref_patch_match.restype = C.c_int
    lib.pmref_patch_match.argtypes = [OP, PB, V, V, V, V, V, V]
    lib.pmref_cost.restype = F
    lib.pmref_cost.argtypes = [OP, PB, C.c_uint64, U, I, I, F, V]
    lib.pmref_propagate.restype = F
    lib.pmref_propagate.argtypes = [V, I, I, F, V, I, I]
    lib.pmref_fb_error.restype = F
    lib.pmref_fb_error.argtypes = [PB, C.c_uint64, U, I, I, F]
    lib.pmref_uniform.restype = F
    lib.pmref_uniform.argtypes = [U] * 6
    lib.pmref_exp.restype = F
    lib.pmref_exp.argtypes = [F]
    lib.pmref_acos.restype = F
    lib.pmref_acos.argtypes = [F]
    _lib = lib
    return lib


_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def patch_match(images, K, R, t, ref_images, src_offsets, src_images, depth_ranges, in_depth=None, in_normal=None, **options):
    """The reference in Context.patch_match's place: the same arguments, the same dict without the timings."""
    o = _capi.patch_match_options(**options)
    pb, keep = _capi.patch_match_inputs(images, K, R, t, ref_images, src_offsets, src_images, depth_ranges, in_depth, in_normal)
    w, h, ref, soff = keep[2], keep[3], keep[7], keep[8]
    n = ref.size
    moff, coff = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    for p in range(n):
        hw = int(w[ref[p]]) * int(h[ref[p]])
        moff[p + 1] = moff[p] + np.uint64(hw)
        coff[p + 1] = coff[p] + np.uint64(hw * int(soff[p + 1] - soff[p]))
    npix, ncost = int(moff[-1]), int(coff[-1])
    depth, normal = np.zeros(max(npix, 1), np.float32), np.zeros(3 * max(npix, 1), np.float32)
    cnt = np.zeros(max(npix, 1), np.uint8)
    costs = np.zeros(max(ncost, 1), np.float32) if o.want_costs else None
    load().pmref_patch_match(C.byref(o), C.byref(pb), _p(moff), _p(coff), _p(depth), _p(normal), _p(cnt), _p(costs))
    as_ptr = lambda a, ct: None if a is None else a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    return _capi.patch_match_unpack(keep, n, moff, coff, as_ptr(depth, C.c_float), as_ptr(normal, C.c_float),
                                    as_ptr(cnt, C.c_uint8), as_ptr(costs, C.c_float))


def cost(problem, p, s, row, col, depth, normal, **options):
    """One cost evaluation; problem = the arguments of patch_match_inputs as a tuple or dict"""
    o = _capi.patch_match_options(**options)
    pb, keep = _inputs(problem)
    n = np.ascontiguousarray(normal, dtype=np.float32)
    return float(load().pmref_cost(C.byref(o), C.byref(pb), p, s, row, col, float(np.float32(depth)), _p(n)))


def fb_error(problem, p, s, row, col, depth):
    pb, keep = _inputs(problem)
    return float(load().pmref_fb_error(C.byref(pb), p, s, row, col, float(np.float32(depth))))


def propagate(K, prow, pcol, pdepth, pnormal, row, col):
    k = np.ascontiguousarray(K, dtype=np.float64)
    n = np.ascontiguousarray(pnormal, dtype=np.float32)
    return float(load().pmref_propagate(_p(k), prow, pcol, float(np.float32(pdepth)), _p(n), row, col))


def uniform(seed, image, row, col, sweep, draw):
    return float(load().pmref_uniform(seed, image, row, col, sweep, draw))


def _inputs(problem):
    return _capi.patch_match_inputs(**problem) if isinstance(problem, dict) else _capi.patch_match_inputs(*problem)
