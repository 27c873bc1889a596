"""The cases of tests/guided_cases.py on the CPU: the frozen oracle reproduces tests/golden/guided_ref_v1.npz, and every
case reaches the edge of the candidate-generation kernel it names - per-row totals, staging rounds, the list positions
of tied candidates, cell membership and routing - checked on the host build of guided_region.h
(tests/shim/guided_shim.cc) and guided_pair_setup.  tests/test_guided_cases_gpu.py runs the same cases through both
kernels."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import guided_cases as gc

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "guided_ref_v1.npz"
CASES = gc.build_cases()
NAMES = sorted(CASES)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def live():
    """name -> (offsets, matches) of the live oracle, computed once."""
    return {name: gc.oracle_matches(CASES[name]) for name in NAMES}


def pair_matches(off, m, p):
    return m[int(off[p]):int(off[p + 1])]


def test_case_list_is_complete(golden):
    assert golden["cases"].tolist() == NAMES
    fams = {n.split("/")[0] for n in NAMES}
    assert fams == {"staging", "tie", "zero", "rows", "geom", "boundary", "mixed"}
    for n in gc.STAGING_TOTALS:
        assert f"staging/a_{n}" in CASES and f"staging/b_{n}" in CASES
    assert "staging/a_0" in CASES and {"staging/c_300_300", "staging/c_500_13"} <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_fixture(name, golden, live):
    off, m = live[name]
    np.testing.assert_array_equal(off, golden[f"{name}/offsets"])
    np.testing.assert_array_equal(m, golden[f"{name}/matches"])
    assert gc.digest(off, m) == str(golden[f"{name}/digest"])


def test_fixture_regenerates_byte_for_byte(tmp_path):
    spec = importlib.util.spec_from_file_location("make_guided_ref_golden", ROOT / "tests" / "golden" / "make_guided_ref_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "again.npz"
    mod.main(out)
    assert out.read_bytes() == GOLDEN.read_bytes()


@pytest.mark.parametrize("name", NAMES)
def test_routing_is_as_stated(name):
    c = CASES[name]
    for p, want in enumerate(c["grid"]):
        assert gc.routes_to_grid(c, p) == want, f"{name} pair {p}"


# ---- the claims --------------------------------------------------------------------------------------------------------
def check_totals(c, r, live):
    ok, cand = gc.candidates(c, r["pair"], r["dir"])
    assert ok
    tot = cand.sum(axis=1, dtype=np.int64)
    rows = np.arange(len(tot)) if isinstance(r["rows"], str) else np.asarray(r["rows"])
    assert len(rows) > 0
    np.testing.assert_array_equal(tot[rows], np.full(len(rows), r["total"]))


def check_rounds(c, r, live):
    tr = gc.trace(c, r["pair"], r["dir"], r["row"])
    assert tr["rounds"] == [tuple(x) for x in r["rounds"]]


def check_lanes_occupied(c, r, live):
    tr = gc.trace(c, r["pair"], r["dir"], r["row"])
    assert len(np.unique(tr["lane"])) == r["lanes"]


def check_lane_lengths(c, r, live):
    tr = gc.trace(c, r["pair"], r["dir"], r["row"])
    lanes, counts = np.unique(tr["lane"], return_counts=True)
    assert dict(zip(lanes.tolist(), counts.tolist())) == r["lengths"]
    # the second lane's range straddles the round boundary: the kernel cuts it at `base`
    first = r["lengths"][min(r["lengths"])]
    assert first < gc.CAND_CAP < first + r["lengths"][max(r["lengths"])]


def check_tie(c, r, live):
    p, row = r["pair"], r["row"]
    tr = gc.trace(c, p, r["dir"], row)
    a, b = c["images"][int(c["pairs"][0][p])], c["images"][int(c["pairs"][1][p])]
    dots = b["descriptors"].astype(np.int64) @ a["descriptors"][row].astype(np.int64)
    pos_of = {int(j): k for k, j in enumerate(tr["idx"])}
    for tag, where in r["where"].items():
        listed = sorted((pos_of[j] for j in r["tagged"][tag] if j in pos_of))
        got = [(int(tr["round"][k]), int(tr["acc_pos"][k])) for k in listed]
        assert got == [tuple(w) for w in where], (tag, got)
    for tag, n in r.get("survivors", {}).items():
        assert sum(1 for j in r["tagged"][tag] if j in pos_of and tr["ok"][pos_of[j]]) == n
        assert len(r["tagged"][tag]) > n           # and some copy is rejected or never listed
    surv = tr["idx"][tr["ok"]]
    vals = dots[surv]
    if r.get("zeros"):
        z = [j for j in r["tagged"][r["zeros"]]]
        assert all(dots[j] == 0 and j in pos_of and tr["ok"][pos_of[j]] for j in z)
    if r["best"] is None:
        assert len(surv) > 0 and vals.max() == 0   # survivors, and every one of them with dot 0
        return
    best_js = [j for j in r["tagged"][r["best"]] if j in pos_of and tr["ok"][pos_of[j]]]
    best = int(vals.max())
    assert best > 0 and sorted(surv[vals == best].tolist()) == sorted(best_js)
    if len(best_js) > 1:
        # the lowest index is listed last: list order is against index order
        order = sorted(best_js, key=lambda j: pos_of[j])
        assert order == sorted(best_js, reverse=True)
    rest = np.sort(vals)[::-1][1:]
    if r["second"] == r["best"]:
        assert len(best_js) > 1 and rest[0] == best
    elif r["second"] is not None:
        sec_js = r["tagged"][r["second"]]
        assert len(sec_js) == 2 and rest[0] == rest[1] == dots[sec_js[0]] == dots[sec_js[1]] < best
        assert rest[2] < rest[1]
    # what the oracle makes of it, where every row with a candidate is accepted: the lowest index among the bests
    # (with the cross check too: the copies' own best in image 0 is the row they copy)
    off, m = live
    mine = pair_matches(off, m, p).tolist()
    copies = r["best"] == "T"
    if c["options"]["max_ratio"] > 1.0:
        if copies or not c["options"]["cross_check"]:
            assert [row, min(best_js)] in mine
    elif len(best_js) > 1 or r["second"] not in (None, r["best"]):
        assert all(i != row for i, _ in mine)       # a tied or close second: the default ratio test rejects the row
    elif copies:
        assert [row, best_js[0]] in mine


def check_zero_row(c, r, live):
    p = r["pair"]
    a, b = c["images"][int(c["pairs"][0][p])], c["images"][int(c["pairs"][1][p])]
    assert not a["descriptors"][r["row"]].any()
    tr = gc.trace(c, p, 0, r["row"])
    assert tr["ok"].sum() >= 9                      # the zero row has survivors: all of them score 0
    d = a["descriptors"][r["full_row"]].astype(np.int64) @ b["descriptors"][r["full_col"]].astype(np.int64)
    assert d == 512 * 512
    tr = gc.trace(c, p, 0, r["full_row"])
    assert r["full_col"] in tr["idx"][tr["ok"]].tolist()
    off, m = live
    mine = pair_matches(off, m, p).tolist()
    assert all(i != r["row"] for i, _ in mine)
    assert [r["full_row"], r["full_col"]] in mine       # acosf(1) = 0: inside any max_distance, below any ratio bound


def check_sizes(c, r, live):
    s1, s2 = c["pairs"]
    n = [len(im["keypoints"]) for im in c["images"]]
    assert {n[int(a)] for a in s1} == {n[int(b)] for b in s2} == set(r["sizes"])
    # both directions of every pair under one model
    for k in range(0, len(s1), 2):
        assert (s1[k], s2[k]) == (s2[k + 1], s1[k + 1])
        assert c["tvg"][k].tobytes() == c["tvg"][k + 1].tobytes()
    off, m = live
    assert len(m) > 200


def check_on_cell_boundaries(c, r, live):
    kp = c["images"][r["image"]]["keypoints"]
    geom, gx, gy = gc.grid_cells(kp)
    x0, y0, cw, ch, inv_cw, inv_ch, bx1, by1 = (float(v) for v in geom)
    assert bx1 - x0 == by1 - y0 == r["extent"] and cw == ch == r["extent"] / 64 and inv_cw * cw == 1.0
    tx, ty = (kp[:, 0] - np.float32(x0)) * np.float32(inv_cw), (kp[:, 1] - np.float32(y0)) * np.float32(inv_ch)
    assert np.all(tx == np.floor(tx)) and np.all(ty == np.floor(ty))       # every keypoint on a cell boundary
    assert (tx == 64).any() and (ty == 64).any() and gx.max() == gy.max() == 63   # the box maximum, clamped to cell 63
    np.testing.assert_array_equal(gx, np.minimum(tx, 63).astype(np.int32))


def check_degenerate_box(c, r, live):
    kp = c["images"][r["image"]]["keypoints"]
    geom, gx, gy = gc.grid_cells(kp)
    cw, ch = float(geom[2]), float(geom[3])
    tiny = float(np.float32(1e-3))
    want = {"identical": (tiny, tiny), "one": (tiny, tiny), "hline": (None, tiny), "vline": (tiny, None)}[r["what"]]
    assert (want[0] is None and cw > 1.0) or cw == want[0]
    assert (want[1] is None and ch > 1.0) or ch == want[1]
    if r["what"] in ("identical", "one"):
        assert not gx.any() and not gy.any()
    assert len(kp) == (1 if r["what"] == "one" else 70)


def check_exact_zero(c, r, live):
    assert c["max_error"] == 0.0
    acc = gc.accepted_matrix(c, 0)
    kp1, kp2 = gc.pair_keypoints(c, 0)
    assert np.all(kp1 == np.floor(kp1)) and np.all(kp2 == np.floor(kp2))
    if r["accepted"] == "y2 == y1":
        want = kp1[:, None, 1] == kp2[None, :, 1]
    else:
        want = (kp1[:, None, 0] == kp2[None, :, 0]) & (kp1[:, None, 1] == kp2[None, :, 1])
    np.testing.assert_array_equal(acc, want)
    assert want.any(axis=1).sum() >= 40 and not want.all()
    for d in (0, 1):
        ok, cand = gc.candidates(c, 0, d)
        assert ok and not ((acc if d == 0 else acc.T) & (cand == 0)).any()
    off, m = live
    assert len(m) > 20


def check_negative(c, r, live):
    for k in r["images"]:
        assert (c["images"][k]["keypoints"] < 0).all()
    assert len(live[1]) > 100


def check_box_max(c, r, live):
    kp = c["images"][r["image"]]["keypoints"]
    assert float(kp[:, 0].max()) == r["x"] and float(np.abs(kp).max()) == r["x"]


def check_boundary(c, r, live):
    p = r["pair"]
    kind, m, mr = gc.model_of(c, p)
    pts, tw = c["images"][r["points"]]["keypoints"], c["images"][r["twins"]]["keypoints"]
    assert len(pts) == 64 and len(tw) == 128
    for i, q in enumerate(pts):
        rej, acc = tw[2 * i], tw[2 * i + 1]
        axis = int(np.flatnonzero(rej != acc)[0])
        assert (rej != acc).sum() == 1 and np.nextafter(acc[axis], rej[axis]) == rej[axis]     # adjacent floats
        args = (lambda t: (t[0], t[1], q[0], q[1])) if r["swapped"] else (lambda t: (q[0], q[1], t[0], t[1]))
        assert not gc.oracle_rejects(kind, m, mr, *args(acc)) and gc.oracle_rejects(kind, m, mr, *args(rej))
        # the vectorised restatement the other checks use agrees with the frozen filter on its boundary
        assert not gc.filter_rejects(kind, m, mr, *args(acc)) and gc.filter_rejects(kind, m, mr, *args(rej))
    # the host's regions list every accepted twin, in the forward and in the reverse scan
    for d in (0, 1):
        ok, cand = gc.candidates(c, p, d)
        assert ok
        rows_are_points = (d == 0) != r["swapped"]
        for i in range(64):
            assert cand[i, 2 * i + 1] if rows_are_points else cand[2 * i + 1, i], (d, i)
    # and every p matches its accepted twin
    off, mm = live
    mine = pair_matches(off, mm, p)
    i = np.arange(64, dtype=np.uint32)
    want = np.stack([2 * i + 1, i], axis=1) if r["swapped"] else np.stack([i, 2 * i + 1], axis=1)
    np.testing.assert_array_equal(mine, want)


def check_sliver(c, r, live):
    p = r["pair"]
    kind, m, mr = gc.model_of(c, p)
    kp1, kp2 = gc.pair_keypoints(c, p)
    geom, gx, gy = gc.grid_cells(kp2)
    assert (float(geom[0]), float(geom[2]), float(geom[4]), float(geom[6])) == (256.0, 16.0, 0.0625, 1280.0)
    ok, cand = gc.candidates(c, p, 0)
    assert ok
    md = m.astype(np.float64)
    for i in range(r["points"]):
        q, rej, acc = kp1[i], kp2[2 * i], kp2[2 * i + 1]
        assert acc[0] == np.nextafter(rej[0], np.float32(np.inf)) and acc[1] == rej[1]
        assert not gc.oracle_rejects(kind, m, mr, q[0], q[1], acc[0], acc[1])
        assert gc.oracle_rejects(kind, m, mr, q[0], q[1], rej[0], rej[1])
        # the exact box around H p (no slack) starts right of the accepted keypoint, in the next cell
        edge = (md[0] * float(q[0]) + md[1] * float(q[1]) + md[2]) - 4.0
        b = r["found"][i]["boundary"]
        assert float(acc[0]) < edge and np.float32(edge) == np.float32(b)
        assert gx[2 * i + 1] == (b - 256.0) / 16 - 1 and np.floor((np.float32(edge) - geom[0]) * geom[4]) == (b - 256.0) / 16
        assert cand[i, 2 * i + 1]                       # the region WITH its slack lists it
    off, mm = live
    i = np.arange(r["points"], dtype=np.uint32)
    np.testing.assert_array_equal(pair_matches(off, mm, p)[:r["points"]], np.stack([i, 2 * i + 1], axis=1))


def check_mixed(c, r, live):
    assert sum(c["grid"]) == r["grid"] and len(c["grid"]) - sum(c["grid"]) == r["dense"]
    assert c["grid"] == [True, False] * 4           # interleaved
    assert all(len(im["keypoints"]) == gc.MIXED_ROWS for im in c["images"])
    assert sorted(gc.MIXED_ORDER) == list(range(len(c["grid"])))
    off, m = live
    for p in range(len(c["grid"])):                 # every pair but the horizon's has matches to lose or to mix up
        assert (off[p + 1] > off[p] + 20) != (p in r["empty"])


CHECKS = dict(totals=check_totals, rounds=check_rounds, lanes_occupied=check_lanes_occupied, lane_lengths=check_lane_lengths,
              tie=check_tie, zero_row=check_zero_row, sizes=check_sizes, on_cell_boundaries=check_on_cell_boundaries,
              degenerate_box=check_degenerate_box, exact_zero=check_exact_zero, negative=check_negative, box_max=check_box_max,
              boundary=check_boundary, sliver=check_sliver, mixed=check_mixed)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_what_it_claims(name, live):
    c = CASES[name]
    assert c["reach"], "every case states the edge it reaches"
    for r in c["reach"]:
        CHECKS[r["kind"]](c, r, live[name])


@pytest.mark.parametrize("name", [n for n in NAMES if n.split("/")[0] in ("tie", "zero")])
def test_numpy_restatement_gives_the_oracles_matches(name, live):
    """The expectation of the tie and zero cases does not rest on the C oracle's scans alone."""
    c = CASES[name]
    off, m = live[name]
    for p in range(len(c["grid"])):
        np.testing.assert_array_equal(gc.numpy_matches(c, p), pair_matches(off, m, p), err_msg=f"{name} pair {p}")


def test_staging_totals_cover_the_bound():
    """Both sides of kCandCap and of its double, in each of the three builds."""
    for fam in "ab":
        got = sorted(int(n.split("_")[1]) for n in NAMES if n.startswith(f"staging/{fam}_"))
        assert got == sorted(set(gc.STAGING_TOTALS) | ({0} if fam == "a" else set()))
    assert gc.CAND_CAP == 512
    src = (ROOT / "pycolmap_amd" / "csrc" / "match_guided.hip").read_text()
    assert "constexpr int kCandCap = 512;" in src       # the cases are built around this value
