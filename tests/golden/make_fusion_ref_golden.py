"""Writes tests/golden/fusion_ref_v1.npz from the CPU reference of stereo fusion (tests/fusion_ref_lib.py): for every
case of tests/fusion_cases.py (the threshold cases included) one digest of its result's arrays and counts; whole, the
points, normals and colours of the `rendered_slanted` case.  Run it from the repository root:
python tests/golden/make_fusion_ref_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import fusion_cases as fc  # noqa: E402
import fusion_ref_lib as ref  # noqa: E402


def main():
    data = {}
    for name, (args, opts) in fc.build_cases().items():
        out = ref.fuse_depth_maps(*args, **opts)
        data[f"digest/{name}"] = np.array(fc.result_digest(out))
        if name == "rendered_slanted":
            for key in ("xyz", "normal", "color", "vis_offsets", "vis_images"):
                data[f"rendered_slanted/{key}"] = out[key]
    for name, (args, opts, who, taken) in fc.threshold_cases(ref).items():
        data[f"digest/threshold_{name}"] = np.array(fc.result_digest(ref.fuse_depth_maps(*args, **opts)))
    out = ROOT / "tests" / "golden" / "fusion_ref_v1.npz"
    np.savez_compressed(out, **data)
    print(f"{out}: {len(data)} entries, {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
