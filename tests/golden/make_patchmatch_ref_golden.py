"""Writes tests/golden/patchmatch_ref_v1.npz from the CPU reference of PatchMatch stereo (tests/patchmatch_ref_lib.py):
for every case of tests/patchmatch_cases.py one digest of its result's arrays; whole, the depth map of the `photometric`
case and the photometric maps of the two-stage case, which the geometric test starts from, with the digest of the
geometric pass.  Run it from the repository root: python tests/golden/make_patchmatch_ref_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import patchmatch_cases as pc  # noqa: E402
import patchmatch_ref_lib as ref  # noqa: E402


def main():
    data = {}
    for name, (pb, opts) in pc.build_cases().items():
        out = ref.patch_match(**pb, **opts)
        data[f"digest/{name}"] = np.array(pc.result_digest(out))
        if name == "photometric":
            data["photometric/depth"] = out["depth"][0]
    sc, pb = pc.two_stage_problem()
    ph = ref.patch_match(**pb, **pc.TWO_STAGE["photometric"])
    data["two_stage/photometric_depth"] = np.stack(ph["depth"])
    data["two_stage/photometric_normal"] = np.stack(ph["normal"])
    ge = ref.patch_match(**pb, in_depth=ph["depth"], in_normal=ph["normal"], **pc.TWO_STAGE["geometric"])
    data["digest/two_stage_geometric"] = np.array(pc.result_digest(ge))
    out = ROOT / "tests" / "golden" / "patchmatch_ref_v1.npz"
    np.savez_compressed(out, **data)
    print(f"{out}: {len(data)} entries, {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
