"""Guided matching (amc_match_guided_pairs) on the cases of tests/guided_cases.py: the candidate-generation kernel
(match_guided.hip) under the default routing, the dense kernel (match_dot4.hip, AMC_GUIDED_DENSE=1), the live oracle and
the frozen fixture tests/golden/guided_ref_v1.npz agree bit for bit, offsets and matches, on every case; the routing is
the one each case states.  tests/test_guided_cases_cpu.py checks that each case reaches the edge it names."""
import os
from pathlib import Path

import numpy as np
import pytest

import guided_cases as gc
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "guided_ref_v1.npz"
CASES = gc.build_cases()
NAMES = sorted(CASES)


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def upload(ctx, case):
    ctx.reserve_slots(len(case["images"]))
    for k, im in enumerate(case["images"]):
        ctx.upload_descriptors(k, im["descriptors"])
        ctx.upload_keypoints(k, im["keypoints"])


def run(ctx, case, env=None):
    """(offsets, matches, stats) of one call, with the given environment switches set for its duration."""
    env = env or {}
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        s1, s2 = case["pairs"]
        return ctx.match_guided_pairs(s1, s2, case["tvg"], case["max_error"], **case["options"])
    finally:
        for k in env:
            del os.environ[k]


def assert_same(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what}: offsets")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: matches")


@pytest.mark.parametrize("name", NAMES)
def test_both_kernels_equal_the_oracle_and_the_fixture(ctx, golden, name):
    case = CASES[name]
    npairs = len(case["grid"])
    upload(ctx, case)
    off_g, m_g, st_g = run(ctx, case)
    off_d, m_d, st_d = run(ctx, case, {"AMC_GUIDED_DENSE": 1})
    assert st_g["pairs_guided_grid"] == sum(case["grid"]) and st_g["pairs_dot4"] == npairs - sum(case["grid"])
    assert st_d["pairs_guided_grid"] == 0 and st_d["pairs_dot4"] == npairs
    fixture = (golden[f"{name}/offsets"], golden[f"{name}/matches"])
    assert_same((off_g, m_g), fixture, f"{name}: default routing against the fixture")
    assert_same((off_d, m_d), fixture, f"{name}: dense kernel against the fixture")
    assert_same((off_g, m_g), (off_d, m_d), f"{name}: default routing against the dense kernel")
    assert_same(gc.oracle_matches(case), fixture, f"{name}: live oracle against the fixture")
    assert gc.digest(off_g, m_g) == str(golden[f"{name}/digest"])


def solo_results(ctx, case):
    """Every pair of the (uploaded) case in a call of its own."""
    out = []
    for p in range(len(case["grid"])):
        one = gc.reordered(case, [p])
        off, m, st = run(ctx, one)
        assert st["pairs_guided_grid"] == int(case["grid"][p]) and st["pairs_dot4"] == 1 - int(case["grid"][p])
        out.append(m)
    return out


def test_mixed_call_equals_the_solo_calls_in_any_order_and_batching(ctx, golden):
    """Grid and dense pairs interleaved in one call: each pair's matches are those of its solo call, whatever the order
    of the pairs and however AMC_MATCH_BATCH_ENTRIES cuts the call into batches."""
    name = "mixed/interleaved"
    case = CASES[name]
    upload(ctx, case)
    solo = solo_results(ctx, case)
    for p, m in enumerate(solo):
        np.testing.assert_array_equal(m, golden[f"{name}/matches"][int(golden[f"{name}/offsets"][p]):int(golden[f"{name}/offsets"][p + 1])])
    orders = (list(range(len(solo))), list(gc.MIXED_ORDER))
    envs = [{}] + [{"AMC_MATCH_BATCH_ENTRIES": v} for v in gc.MIXED_BATCH_ENTRIES.values()]
    for order in orders:
        c = gc.reordered(case, order)
        for env in envs:
            for dense in ({}, {"AMC_GUIDED_DENSE": 1}):
                off, m, st = run(ctx, c, {**env, **dense})
                if not dense:
                    assert st["pairs_guided_grid"] == 4 and st["pairs_dot4"] == 4
                for k, p in enumerate(order):
                    np.testing.assert_array_equal(m[int(off[k]):int(off[k + 1])], solo[p],
                                                  err_msg=f"order {order} env {env} {dense}: position {k} (pair {p})")


def test_consecutive_calls_with_other_thresholds_rebuild_the_accept_table(ctx, golden):
    """Two option sets alternating on one context: each call's result is its own fixture's."""
    a, b = "tie/seconds/cc", "tie/seconds/ratio08"          # the same images and pairs, (1.5, 2.0) and (0.8, 0.7)
    upload(ctx, CASES[a])
    assert not np.array_equal(golden[f"{a}/matches"], golden[f"{b}/matches"])
    for name in (a, b, a, b):
        off, m, _ = run(ctx, CASES[name])
        assert_same((off, m), (golden[f"{name}/offsets"], golden[f"{name}/matches"]), name)
