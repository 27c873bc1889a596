"""Time of one stereo fusion call (amc_fuse_depth_maps) against the single-threaded CPU reference.

Two workloads, both rendered by tests/patchmatch_cases.py (a slanted textured plane, look-at cameras on a ring) with their
exact depth and normal maps, every image naming all the others, the default options:
  small : 4 maps of 130 x 98 pixels;
  large : --maps (default 20) maps of --width x --height (default 2000 x 1500, 3 megapixels).
Reports, for the best of --reps repetitions after one untimed call: kernel / copy / device / host ms and the end-to-end
time of the call, the points and seeds, the time of tests/fusion_ref on the same input and whether the two agree bit for
bit (for the large workload only with --large-reference: the reference needs many minutes there).  Prints one JSON line;
--out writes it too.

    python tools/stereo_fusion_bench.py [--reps 2] [--skip-large] [--out profiles/fusion/stereo_fusion_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def ring_problem(width, height, cameras):
    """fusion_cases.rendered with `cameras` look-at cameras on a ring of radius 1.2 round the first"""
    import fusion_cases as fc
    import patchmatch_cases as pc
    ang = np.linspace(0.0, 2.0 * np.pi, cameras - 1, endpoint=False)
    pc.CENTRES[:] = [(0.0, 0.0, 0.0)] + [(1.2 * np.cos(a), 1.2 * np.sin(a), 0.1 * np.sin(3 * a)) for a in ang]
    return fc.rendered("slanted", cameras, width, height)


def timed(ctx, args, reps):
    ctx.fuse_depth_maps(*args)  # untimed: code objects, allocations
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        out = ctx.fuse_depth_maps(*args)
        wall = (time.perf_counter() - t) * 1e3
        if best is None or wall < best[0]:
            best = (wall, out)
    wall, out = best
    return out, {"end_to_end_ms": wall, "kernel_ms": out["kernel_ms"], "copy_ms": out["copy_ms"], "device_ms": out["device_ms"],
                 "host_ms": out["host_ms"], "alloc_ms": out["alloc_ms"], "num_launches": out["num_launches"],
                 "num_batches": out["num_batches"], "num_points": out["num_points"], "num_seeds": out["num_seeds"],
                 "num_truncated": out["num_truncated"]}


def against_reference(args, out, row):
    import fusion_cases as fc
    import fusion_ref_lib as ref
    ref.load()
    t = time.perf_counter()
    want = ref.fuse_depth_maps(*args)
    row["cpu_reference_ms"] = (time.perf_counter() - t) * 1e3
    row["bit_identical"] = bool(fc.same(out, want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--width", type=int, default=2000)
    ap.add_argument("--height", type=int, default=1500)
    ap.add_argument("--maps", type=int, default=20)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--large-reference", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from pycolmap_amd import _capi
    result = {}
    with _capi.Context(0) as ctx:
        args = ring_problem(130, 98, 4)
        out, result["small"] = timed(ctx, args, a.reps)
        against_reference(args, out, result["small"])
        result["small"].update(width=130, height=98, maps=4)
        if not a.skip_large:
            args = ring_problem(a.width, a.height, a.maps)
            out, result["large"] = timed(ctx, args, a.reps)
            if a.large_reference:
                against_reference(args, out, result["large"])
            result["large"].update(width=a.width, height=a.height, maps=a.maps)
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
