"""The MFMA scan's item boundary (match_mfma.hip): the forward scan stores an X tile's 16 rows of the row table only if
it sets the accept bit of one of them, and an accept word only when it has a bit, because nobody reads anything else; and a workgroup pops
the item queue ahead of its scan.  So these tests ask three things: that exactly the rows somebody reads are there,
whatever an earlier call or batch left in the tables; and that every item is scanned once, however the items divide
among the workgroups.  Every comparison is row for row with the oracle, without tolerance, with the cross check off and
on (the reverse scan shares the queue code and stores every candidate row).

The planting is that of test_match_scan_units128_gpu.py, restated: planted rows use four dimensions, an X row
(255, 255, 255, 255, 0, ...) against a Y row (a, b, c, d, 0, ...) has the dot product 255 (a + b + c + d), and with
d(v) = acos(v / 512^2)
    best   260100 = 255 * 1020    d = 0.12494   (passes max_distance 0.7)
    second 258825 = 255 * 1015    0.8 d = 0.12742 > 0.12494: the ratio test ACCEPTS
An X row of zeros scores 0 everywhere: d = pi / 2, rejected by the scan itself - a tile of such rows is not stored."""
import numpy as np
import pytest

import oracle_lib
from pycolmap_amd import _capi, synth

pytestmark = pytest.mark.gpu

BEST = (255, 255, 255, 255)
SEC_ACCEPT = (255, 255, 255, 250)   # 255 * 1015
OPTS = (0.8, 0.7)


def planted(n, rows):
    """n x 128 zero image with the 4-vectors of `rows` ({row: values}) in dimensions 0..3."""
    im = np.zeros((n, 128), np.uint8)
    for r, v in rows.items():
        im[r, :4] = v
    return im


def upload(ctx, imgs):
    ctx.reserve_slots(len(imgs))
    for k, im in enumerate(imgs):
        ctx.upload_descriptors(k, im)


def run(ctx, imgs, s1, s2, cross_check, want=None):
    """Upload, match on the MFMA path, compare with the oracle (or with `want`, an oracle result computed before)."""
    upload(ctx, imgs)
    s1 = np.asarray(s1, np.uint32)
    s2 = np.asarray(s2, np.uint32)
    off, m, st = ctx.match_pairs(s1, s2, *OPTS, cross_check, kernel="mfma")
    woff, wm = want if want is not None else oracle_lib.match_pairs(imgs, s1, s2, *OPTS, cross_check)
    assert st["pairs_mfma"] == len(s1) and st["pairs_dot4"] == 0
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(m, wm)
    return off, m, st


# ---- 1. which rows are stored ------------------------------------------------------------------------------------------
# X rows 0..159 are two segments (128 + 32); an accept word is 32 rows = two 16-row X tiles, low half | high half << 16.
EVERY = tuple(range(160))
ROW_SETS = [EVERY, (), (0,), (15,), (16,), (31,), tuple(range(16, 32)), (127,), (128,), (159,), (), EVERY]


@pytest.mark.parametrize("cross_check", [False, True])
def test_which_rows_are_stored(amc_ctx, cross_check):
    """Only the X rows of a set are planted, so only they are accepted and only their tiles stored: nothing, one row at
    either end of an accept word's low half (X tile 0), at either end of its high half (X tile 1), the whole high half,
    the last row of a segment, the first and the last row of the second segment, and every row - in one call, a pair
    that stores nothing beside one that stores everything.  Then X images of 1, 17, 33, 127 and 129 rows with every row accepted."""
    y = planted(64, {41: BEST, 9: SEC_ACCEPT})
    xs = [planted(160, {r: BEST for r in rows}) for rows in ROW_SETS]
    imgs = xs + [y]
    npairs = len(xs)
    woff, wm, _ = run(amc_ctx, imgs, np.arange(npairs), np.full(npairs, npairs), cross_check)
    counts = np.diff(woff.astype(np.int64))
    if not cross_check:  # the inputs do what they are built for: exactly the planted rows match, all with Y row 41
        assert counts.tolist() == [len(rows) for rows in ROW_SETS]
        assert wm[:, 0].tolist() == [r for rows in ROW_SETS for r in rows]
        assert np.all(wm[:, 1] == 41)
    else:  # identical X rows tie in the column direction: only a single planted row is mutual
        assert counts.tolist() == [1 if len(rows) == 1 else 0 for rows in ROW_SETS]
    sizes = [1, 17, 33, 127, 129]
    xs = [planted(n, {r: BEST for r in range(n)}) for n in sizes]
    woff, wm, _ = run(amc_ctx, xs + [y], np.arange(len(xs)), np.full(len(xs), len(xs)), cross_check)
    counts = np.diff(woff.astype(np.int64)).tolist()
    assert counts == ([1, 0, 0, 0, 0] if cross_check else sizes)


# ---- 2. stale tables are never read ------------------------------------------------------------------------------------
N_IMG, N_ROWS = 6, 300


@pytest.fixture(scope="module")
def dense_and_sparse():
    """Six near-duplicate images (every image sees the same 300 landmarks: nearly every row is accepted and resolved) and
    six unrelated ones (almost none is), all pairs, with the oracle's answers for both option sets - computed once."""
    rng = np.random.default_rng(2024)
    dense = synth.scene_images(rng, N_IMG, N_ROWS, num_landmarks=N_ROWS, visible_frac=1.0, sigma_d=0.04)
    sparse = [synth.random_descriptors(rng, N_ROWS) for _ in range(N_IMG)]
    s1, s2 = synth.exhaustive_pairs(N_IMG)
    want = {}
    for cc in (False, True):
        want["dense", cc] = oracle_lib.match_pairs(dense, s1, s2, *OPTS, cc)
        want["sparse", cc] = oracle_lib.match_pairs(sparse, s1, s2, *OPTS, cc)
        # the inputs are what the test needs: dense pairs keep most rows, sparse pairs next to none
        assert np.diff(want["dense", cc][0].astype(np.int64)).min() > N_ROWS * 0.7
        assert np.diff(want["sparse", cc][0].astype(np.int64)).max() < N_ROWS * 0.05
    return {"dense": dense, "sparse": sparse, "s1": s1, "s2": s2, "want": want}


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("order", [("dense", "sparse"), ("sparse", "dense")])
def test_a_call_never_reads_the_call_before(dense_and_sparse, cross_check, order):
    """Two calls of the same shapes in one context: the second finds the first one's rows at the same table offsets and
    must not read them.  It equals the oracle and the same call in a fresh context."""
    d = dense_and_sparse
    s1, s2 = d["s1"], d["s2"]
    with _capi.Context(0) as ctx:
        for name in order:
            second = run(ctx, d[name], s1, s2, cross_check, want=d["want"][name, cross_check])
    with _capi.Context(0) as fresh:
        upload(fresh, d[order[1]])
        alone = fresh.match_pairs(s1, s2, *OPTS, cross_check, kernel="mfma")
    np.testing.assert_array_equal(second[0], alone[0])
    np.testing.assert_array_equal(second[1], alone[1])


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("order", [("dense", "sparse"), ("sparse", "dense")])
def test_a_batch_never_reads_the_batch_before(dense_and_sparse, monkeypatch, cross_check, order):
    """The same within one call.  Three images of either kind, the three pairs of one kind and then the three of the
    other; a 300-row image pads to 512 table rows and the budget is three pairs' worth, so the first kind's pairs are
    one batch at table offsets 0, 512 and 1024 and the other kind's follow in the next batches at 0, 512 and 0."""
    d = dense_and_sparse
    imgs = d[order[0]][:3] + d[order[1]][:3]
    s1 = np.array([0, 0, 1, 3, 3, 4], np.uint32)
    s2 = np.array([1, 2, 2, 4, 5, 5], np.uint32)
    want = oracle_lib.match_pairs(imgs, s1, s2, *OPTS, cross_check)
    with _capi.Context(0) as ctx:
        _, _, st_one = run(ctx, imgs, s1, s2, cross_check, want=want)
        monkeypatch.setenv("AMC_MATCH_BATCH_ENTRIES", str(3 * 512))
        _, _, st = run(ctx, imgs, s1, s2, cross_check, want=want)
        assert st["match_kernel_launches"] >= 3 * st_one["match_kernel_launches"]  # it really ran as three batches


# ---- 3. ticket edges ---------------------------------------------------------------------------------------------------
N_ITEMS = [1, 2, 3, 255, 256, 257, 511, 512, 513, 769]


@pytest.fixture(scope="module")
def many_y():
    """769 distinct 32-row Y images: the best at row k mod 32, an accepting second eleven rows on."""
    return [planted(32, {k % 32: BEST, (k + 11) % 32: SEC_ACCEPT}) for k in range(max(N_ITEMS))]


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("n", N_ITEMS)
def test_ticket_edges(amc_ctx, many_y, cross_check, n):
    """One shared 16-row X image against n distinct Y images: n forward items of one live segment each (an item never
    mixes streamed images).  Fewer items than workgroups (one per CU, 256), exactly one each, one left over, and
    workgroups that take a second and a third item and then run dry.  A workgroup takes the next item's ticket while
    it scans (every workgroup over-pops at the end), and every item must still be scanned exactly once."""
    x = planted(16, {r: BEST if r == 0 or not cross_check else (255, 255, 255, 200) for r in range(16)})
    imgs = [x] + many_y[:n]
    woff, wm, _ = run(amc_ctx, imgs, np.zeros(n, np.uint32), np.arange(1, n + 1), cross_check)
    assert np.all(np.diff(woff.astype(np.int64)) == (1 if cross_check else 16))
    assert np.array_equal(wm[woff[:-1].astype(np.int64), 1], np.arange(n) % 32)
