"""Freeze the oracle's guided matching (oracle/match_oracle.c: oracle_match_guided, through oracle_lib.match_guided) on the
cases of tests/guided_cases.py into tests/golden/guided_ref_v1.npz: per case the match offsets over its pairs, the matches
and one digest of both.  Nothing in the file comes from a kernel.  The GPU tests compare the library with the live oracle
and with this file; tests/test_guided_cases_cpu.py checks that the oracle still reproduces it.  The archive is written
with fixed member dates, so that writing it again gives the same bytes.

    python tests/golden/make_guided_ref_golden.py
"""
import io
import sys
import zipfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import guided_cases as gc  # noqa: E402

OUT = Path(__file__).resolve().parent / "guided_ref_v1.npz"


def write_npz(path, data):
    """np.savez_compressed without the clock: members in the given order, dated 1980-01-01."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, arr in data.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main(out=OUT):
    cases = gc.build_cases()
    data = {"cases": np.array(sorted(cases))}
    total = 0
    for name in sorted(cases):
        off, m = gc.oracle_matches(cases[name])
        data[f"{name}/offsets"] = off
        data[f"{name}/matches"] = m
        data[f"{name}/digest"] = np.array(gc.digest(off, m))
        total += len(m)
    write_npz(out, data)
    print(f"wrote {out} ({Path(out).stat().st_size} bytes, {len(cases)} cases, {total} matches)")


if __name__ == "__main__":
    main(*sys.argv[1:2])
