"""Freeze the Python-visible surface of pycolmap_amd._pycolmap (tests/host_surface.py: kinds, docstrings with their
signatures and defaults, class entries, properties, scalars) into tests/golden/host_surface_v1.json, one digest per
top-level name.  tests/test_host_surface_cpu.py checks that the built module still reproduces it; regenerate only when
the surface is meant to change.

    python tests/golden/make_host_surface_golden.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import host_surface  # noqa: E402

OUT = Path(__file__).resolve().parent / "host_surface_v1.json"


def main():
    surface = host_surface.host_surface()
    OUT.write_text(json.dumps(surface, indent=0, sort_keys=True) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(surface)} names)")


if __name__ == "__main__":
    main()
