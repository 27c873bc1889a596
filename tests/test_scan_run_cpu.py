"""The host's choice of the forward scan's run length (pycolmap_amd/csrc/scan_run.h, called from amc_match.hip's
prepare()): runs only where consecutive streamed images share their X list as a prefix, and only for a batch large
enough that a run per workgroup is a small tail.  Built for the host through tests/shim/scan_run_shim.cc."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SHIM = ROOT / "tests" / "shim" / "_build" / "libscanrunshim.so"
WGS = 512


@pytest.fixture(scope="module")
def shim():
    SHIM.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "shim" / "scan_run_shim.cc"
    hdr = ROOT / "pycolmap_amd" / "csrc" / "scan_run.h"
    if not SHIM.exists() or SHIM.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", str(src), "-o", str(SHIM)], check=True)
    lib = C.CDLL(str(SHIM))
    lib.sr_choose.argtypes = [C.c_void_p, C.c_void_p, C.c_ulong, C.c_ulong, C.c_ulong, C.c_int]
    lib.sr_min_runs_per_workgroup.restype = C.c_ulong
    return lib


def forward_order(s1, s2):
    """What prepare() builds: the pairs by (image 2, image 1), the images 1 in that order and the group cuts."""
    s1, s2 = np.asarray(s1), np.asarray(s2)
    o = np.lexsort((s1, s2))
    k2 = s2[o]
    cuts = np.flatnonzero(np.r_[True, k2[1:] != k2[:-1], True])
    return s1[o].astype(np.uint32), cuts.astype(np.uint32)


def choose(lib, s1, s2, items, forced=0):
    slot1, grp = forward_order(s1, s2)
    return lib.sr_choose(slot1.ctypes.data, grp.ctypes.data, len(grp) - 1, items, WGS, forced)


def test_prefix_lists_take_runs_and_windows_do_not(shim):
    auto = shim.sr_auto()
    big = shim.sr_min_runs_per_workgroup() * auto * WGS
    i, j = np.triu_indices(40, k=1)
    assert auto in (2, 4, 8)
    assert choose(shim, i, j, big) == auto
    # a batch carved out of the i-major list: images 1 from 10 to 19, the last of them cut short (behind image 2 = 30
    # the lists get shorter by that image: the shorter list is still a prefix of the longer)
    keep = (i >= 10) & ((i < 19) | ((i == 19) & (j <= 30)))
    assert choose(shim, i[keep], j[keep], big) == auto
    # the same batch, too small to fill the machine often enough
    assert choose(shim, i[keep], j[keep], big - 1) == 1
    # sequential windows of two: image j holds (j - 2, j - 1), only the first cut is a prefix
    w1 = [a for a in range(40) for b in range(a + 1, min(a + 2, 39) + 1)]
    w2 = [b for a in range(40) for b in range(a + 1, min(a + 2, 39) + 1)]
    assert choose(shim, w1, w2, big) == 1
    # one streamed image: nothing to chain
    assert choose(shim, [0, 1, 2], [3, 3, 3], big) == 1


@pytest.mark.parametrize("forced,want", [(1, 1), (2, 2), (4, 4), (8, 8)])
def test_forced_values_hold_whatever_the_list(shim, forced, want):
    assert choose(shim, [0, 1, 1], [1, 2, 3], 1, forced) == want


def test_other_values_mean_auto(shim):
    i, j = np.triu_indices(40, k=1)
    big = shim.sr_min_runs_per_workgroup() * shim.sr_auto() * WGS
    for forced in (0, 3, 5, 6, 7):
        assert choose(shim, i, j, big, forced) == shim.sr_auto()
        assert choose(shim, i, j, 10, forced) == 1
