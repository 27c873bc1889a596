"""SIFT extraction throughput at COLMAP's defaults (first_octave -1, 8192 features) on seeded 1600 x 1200 images: one
JSON line with images/s through Context.sift_extract batches, device ms per image (HIP events) and per stage, an
algorithmic bytes model of the scale space (levels and DoGs written and read), and the CPU reference's time on one
image (this project's single-threaded restatement, tests/sift_ref/sift_ref.cc; not VLFeat or COLMAP), and
extract_features images/s from PGM files into a new SQLite database.  "stream_ms" figures are event intervals on the
stream, which include the host round trips between stages (counts, the feature cut); the kernel time alone comes from
a rocprofv3 --kernel-trace run.

    python tools/sift_bench.py [--images 8] [--steps 3] [--hbm-tbs 6.3] [--no-ref]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def bytes_model(w, h, first_octave=-1, num_octaves=4, S=3):
    """Bytes the scale space must move at least: per octave the base written, every level read twice (two blur
    passes through a scratch image) and written, every DoG written once and read once by detection (float32)."""
    total = 0
    for oi in range(num_octaves):
        o = first_octave + oi
        wo, ho = (w << -o, h << -o) if o < 0 else (w >> o, h >> o)
        if min(wo, ho) < 8:
            break
        px = wo * ho * 4
        levels, dogs = S + 3, S + 2
        total += px + (levels - 1) * 4 * px + dogs * 2 * px
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    ap.add_argument("--no-ref", action="store_true")
    args = ap.parse_args()
    import sift_images as si
    from pycolmap_amd import _capi
    imgs = [si.textured(1000 + i, 1200, 1600) for i in range(args.images)]
    with _capi.Context(0) as ctx:
        ctx.sift_extract(imgs[:1])  # warm-up
        walls, dev, stages, nfeat = [], [], None, 0
        for _ in range(args.steps):
            t = time.perf_counter()
            out, st = ctx.sift_extract(imgs)
            walls.append(time.perf_counter() - t)
            dev.append(st["device_ms"])
            stages = st["stage_ms"]
            nfeat = sum(len(k) for k, _ in out)
    wall = float(np.median(walls))
    dev_ms = float(np.median(dev)) / args.images
    model = bytes_model(1600, 1200)
    res = {"metric": "sift_extract_images_per_s", "value": args.images / wall, "images": args.images,
           "shape": [1200, 1600], "features_per_image": nfeat / args.images, "stream_ms_per_image": dev_ms,
           "stage_stream_ms_per_image": {k: v / args.images for k, v in stages.items()},
           "scale_space_bytes_model_per_image": model,
           "scale_space_model_floor_ms": model / (args.hbm_tbs * 1e12) * 1e3,
           "scale_space_fraction_of_hbm": (model / (args.hbm_tbs * 1e12) * 1e3) / max(stages["scale_space"] / args.images, 1e-9)}
    import tempfile
    import pycolmap_amd as pycolmap
    with tempfile.TemporaryDirectory() as td:
        for i, im in enumerate(imgs):
            (Path(td) / f"{i:03d}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im.tobytes())
        pycolmap.extract_features(Path(td) / "warm.db", td, image_list=["000.pgm"])
        t = time.perf_counter()
        pycolmap.extract_features(Path(td) / "f.db", td)
        res["extract_features_images_per_s"] = args.images / (time.perf_counter() - t)
        res["extract_features_stats"] = pycolmap.last_run_stats()
    if not args.no_ref:
        import sift_ref_lib as ref
        t = time.perf_counter()
        ref.extract(imgs[0])
        res["cpu_reference_s_per_image"] = time.perf_counter() - t
    print(json.dumps(res))


if __name__ == "__main__":
    main()
