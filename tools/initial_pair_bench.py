"""Timings of the two-view triangulation of image pairs and of the start of a model.  It asserts no
time.

Reports, for the best of --reps repetitions after two untimed calls:

  one_pair      one Context.triangulate_pairs call on one pair of 10^4 correspondences (tests/initpair_cases.problem: a ring
                of SIMPLE_RADIAL cameras, points in the unit cube, 0.5 px noise) against the single-threaded CPU reference
                (tests/initpair_ref, with its lift of the pixels) on the same input, compared bit for bit;
  many_pairs    one call on 10^3 pairs of 10^3 correspondences, likewise;
  methods       register_initial_image_pair on the pair with the most correspondences of a 100-image path scene whose
                images are all candidates, and adjust_global_bundle (--ba-iterations, default 5) on a model of 100 images
                of such a scene, once each through Python, against the same calls with the CPU oracle and the references
                in the library's place, with the models compared.

Prints one JSON line; --out writes it too.

    python tools/initial_pair_bench.py [--reps 3] [--out profiles/initial_pair/initial_pair_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))


def best_of(reps, fn):
    out, best = None, None
    for rep in range(reps + 2):
        t0 = time.perf_counter()
        out = fn()
        ms = 1e3 * (time.perf_counter() - t0)
        if rep >= 2:
            best = ms if best is None else min(best, ms)
    return out, best


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--ba-iterations", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import ba_config_cases as bc
    import ba_config_ref_lib
    import initpair_cases as k
    import mapper_cases as mk
    import pycolmap_amd as pc
    from image_registration_bench import path_state
    from pycolmap_amd import _capi
    from pycolmap_amd import _pycolmap as P

    pc.logging.minloglevel = 2
    out = {}
    fields = ("kernel_ms", "copy_ms", "device_ms", "alloc_ms", "host_ms", "wall_ms", "num_batches")
    with _capi.Context(0) as ctx:
        for name, sizes in (("one_pair", (10000,)), ("many_pairs", (1000,) * 1000)):
            args, kw = k.problem(seed=7, sizes=sizes, nimg=40)
            best = None
            for rep in range(a.reps + 2):
                t0 = time.perf_counter()
                r = ctx.triangulate_pairs(*args, **kw)
                r["wall_ms"] = 1e3 * (time.perf_counter() - t0)
                if rep >= 2 and (best is None or r["device_ms"] + r["host_ms"] < best["device_ms"] + best["host_ms"]):
                    best = r
            want, ref_ms = best_of(min(a.reps, 1), lambda: k.ref.triangulate_pairs(*args, **kw))
            out[name] = dict({f: best[f] for f in fields}, pairs=len(sizes), correspondences=int(sum(sizes)), accepted=best["num_accepted"],
                             end_to_end_ms=best["device_ms"] + best["host_ms"], reference_ms=ref_ms, equals_reference_bit_for_bit=bool(k.same(best, want)))

    # ---- through Python
    # (the path's neighbouring cameras are 0.2 apart at a depth of 5 to 7: the angle threshold comes down from 16 degrees)
    opts = dict(init_min_num_inliers=100, init_min_tri_angle=1.0, local_ba_num_images=6)
    st = path_state(a.images, a.points)
    empty = dict(st, images={}, points={}, candidates={**{i: (im[0], im[3]) for i, im in st["images"].items()}, **st["candidates"]})
    runs = {}
    for how in ("library", "reference"):
        r, g, t, mp = mk.mapper(empty)
        id1, id2 = max(((m[0], m[1]) for m in empty["matches"]), key=lambda ab: (g.num_correspondences_between_images(*ab), -ab[0], -ab[1]))
        if how == "library":
            pc.register_initial_image_pair(mk.mapper(empty)[3], opts, id1, id2)  # an untimed call first: the context and the kernels load
            ok, ms = timed(lambda: pc.register_initial_image_pair(mp, opts, id1, id2))
        else:
            ok, ms = timed(lambda: P._register_initial_image_pair_with(mp, opts, id1, id2, k.oracle_two_view_solver, k.pair_solver))
        runs[how] = dict(ok=ok, ms=ms, stats=dict(pc.last_run_stats()), last=mp.last_initial_pair(), snapshot=mk.model_snapshot(r))
    lib, ref = runs["library"], runs["reference"]
    out["register_initial_image_pair"] = {
        "python_ms": lib["ms"], "reference_ms": ref["ms"], "once": True, "registered": bool(lib["ok"]), "equal": lib["ok"] == ref["ok"] and lib["snapshot"] == ref["snapshot"],
        "num_correspondences": lib["last"]["num_correspondences"], "num_inliers": lib["last"]["num_inliers"], "num_points3D": lib["last"]["num_points3D"],
        "triangulation_device_ms": lib["stats"]["device_ms"], "triangulation_kernel_ms": lib["stats"]["kernel_ms"], "triangulation_copy_ms": lib["stats"]["copy_ms"]}
    model = path_state(2 * a.images, 2 * a.points)
    ba = pc.BundleAdjustmentOptions(refine_focal_length=False, refine_extra_params=False)
    so = ba.solver_options
    so.max_num_iterations = a.ba_iterations
    ba.solver_options = so
    runs = {}
    for how in ("library", "reference"):
        r, g, t, mp = mk.mapper(model)
        if how == "library":
            pc.adjust_global_bundle(mk.mapper(model)[3], opts, ba)
            ok, ms = timed(lambda: pc.adjust_global_bundle(mp, opts, ba))
        else:
            ok, ms = timed(lambda: P._adjust_global_bundle_with(mp, opts, ba, bc.reference_solver(ba_config_ref_lib)))
        runs[how] = dict(ok=ok, ms=ms, stats=dict(pc.last_run_stats()), snapshot=mk.model_snapshot(r))
    lib, ref = runs["library"], runs["reference"]
    out["adjust_global_bundle"] = {
        "python_ms": lib["ms"], "reference_ms": ref["ms"], "once": True, "adjusted": bool(lib["ok"]), "equal": lib["ok"] == ref["ok"] and lib["snapshot"] == ref["snapshot"],
        "images": lib["stats"]["num_images"], "points": lib["stats"]["num_points"], "observations": lib["stats"]["num_observations"],
        "ba_iterations": a.ba_iterations, "ba_device_ms": lib["stats"]["device_ms"], "ba_kernel_ms": lib["stats"]["kernel_ms"], "normalize_scale": lib["stats"]["normalize_scale"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
