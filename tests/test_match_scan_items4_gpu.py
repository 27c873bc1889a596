"""The MFMA scan with items of four segments and 128-row Y chunks (match_mfma.hip): a workgroup is four waves, two
workgroups share a CU, and the streamed image goes through a ring of four 16 KiB LDS buffers, three chunks ahead, with
counted waits at every chunk crossing.  These tests sit on the edges that shape has: the item edges at multiples of four
segments, the chunk edges from one chunk to two laps of the ring, items of different Y lengths following each other in
one workgroup, more items than resident workgroups, random sizes, and empty images.  Every comparison is row for row
with the oracle, without tolerance, with the cross check off and on (the reverse scan is the same kernel code).

The planting is that of test_match_scan_boundary_gpu.py: planted rows use four dimensions, an X row
(255, 255, 255, 255, 0, ...) against a Y row (a, b, c, d, 0, ...) has the dot product 255 (a + b + c + d), and with
d(v) = acos(v / 512^2)
    best   260100 = 255 * 1020    d = 0.12494   (passes max_distance 0.7)
    second 258825 = 255 * 1015    0.8 d = 0.12742 > 0.12494: the ratio test ACCEPTS
so a Y image with a BEST row and a SEC_ACCEPT row matches every planted X row to the BEST row - and to the SEC_ACCEPT
row (second 0, accepted too) if the scan never sees the BEST row.  An X row (255, 255, 255, 200) scores 246075 against
BEST and 245075 against SEC_ACCEPT: the ratio test rejects it forward, and in the column direction it is the accepting
second of an X row BEST - which is how a pair keeps exactly one mutual match under the cross check."""
import numpy as np
import pytest

import oracle_lib
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

BEST = (255, 255, 255, 255)
SEC_ACCEPT = (255, 255, 255, 250)   # 255 * 1015
WEAK = (255, 255, 255, 200)
OPTS = (0.8, 0.7)


def planted(n, rows):
    """n x 128 zero image with the 4-vectors of `rows` ({row: values}, later entries win) in dimensions 0..3."""
    im = np.zeros((n, 128), np.uint8)
    for r, v in rows.items():
        im[r, :4] = v
    return im


def x_rows(n, cross_check):
    """n planted X rows: all BEST, or - under the cross check, where equal rows tie - BEST in row 0 and WEAK elsewhere."""
    return planted(n, {r: BEST if r == 0 or not cross_check else WEAK for r in range(n)})


def y_ends(n, best_last):
    """n-row Y image with BEST in the last row and SEC_ACCEPT in row 0, or the other way round (one row: BEST)."""
    if best_last:
        return planted(n, {0: SEC_ACCEPT, n - 1: BEST})
    return planted(n, {n - 1: SEC_ACCEPT, 0: BEST})


def upload(ctx, imgs):
    ctx.reserve_slots(len(imgs))
    for k, im in enumerate(imgs):
        ctx.upload_descriptors(k, im)


def run(ctx, imgs, s1, s2, cross_check, want=None, opts=OPTS):
    """Upload, match on the MFMA path, compare with the oracle (or with `want`, an oracle result computed before)."""
    upload(ctx, imgs)
    s1 = np.asarray(s1, np.uint32)
    s2 = np.asarray(s2, np.uint32)
    off, m, st = ctx.match_pairs(s1, s2, *opts, cross_check, kernel="mfma")
    woff, wm = want if want is not None else oracle_lib.match_pairs(imgs, s1, s2, *opts, cross_check)
    # every pair that has rows on both sides went through the MFMA scan (a pair with an empty image has nothing to scan)
    scanned = sum(1 for a, b in zip(s1, s2) if len(imgs[a]) and len(imgs[b]))
    assert st["pairs_mfma"] == scanned and st["pairs_dot4"] == 0
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(m, wm)
    return off, m, st


def workgroups():
    """The scan's resident workgroups: two per CU, 256 CUs on MI355X (test_match_scan_boundary_gpu.py counts on the same
    256).  Not asked of torch: importing it here would bring a second copy of the HIP runtime into the suite's process."""
    return 2 * 256


# ---- 1. item edges at four segments ------------------------------------------------------------------------------------
X_SIZES = [1, 127, 128, 129, 384, 512, 513, 640, 1024, 1025]   # 1, 1, 1, 2, 3, 4 | 5, 5, 8 | 9 segments


@pytest.mark.parametrize("cross_check", [False, True])
def test_item_edges_at_four_segments(amc_ctx, cross_check):
    """One Y image, X images of 1 to 9 segments with every row planted, in one call: 35 segments packed four to an
    item, so the waves of one item belong to different pairs, a pair's rows spread over up to three items, and the last
    item is padded with a null segment."""
    assert sum((n + 127) // 128 for n in X_SIZES) % 4 != 0   # the group really ends with a padded item
    y = planted(64, {41: BEST, 9: SEC_ACCEPT})
    xs = [planted(n, {r: BEST for r in range(n)}) for n in X_SIZES]
    k = len(xs)
    woff, wm, _ = run(amc_ctx, xs + [y], np.arange(k), np.full(k, k), cross_check)
    counts = np.diff(woff.astype(np.int64)).tolist()
    if not cross_check:  # every row of every X image matches Y row 41
        assert counts == X_SIZES
        assert wm[:, 0].tolist() == [r for n in X_SIZES for r in range(n)]
        assert np.all(wm[:, 1] == 41)
    else:  # identical X rows tie in the column direction: only the one-row image keeps its match
        assert counts == [1] + [0] * (k - 1)


# ---- 2. chunk edges and the four-buffer ring ---------------------------------------------------------------------------
# one chunk (1, 127, 128), two (129 .. 256), the three chunks an item starts with exactly (383, 384), one more (385:
# the first fetch inside the loop), one lap of the ring (511, 512), the buffer of chunk 0 reused (513, 640), two laps
# (1024) and the start of the third (1025)
Y_SIZES = [1, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 640, 1024, 1025]


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("best_last", [True, False])
def test_chunk_edges_and_the_ring(amc_ctx, cross_check, best_last):
    """A 160-row X image (two live waves, two idle ones) against Y images whose best and second sit in the first and
    in the last row with data.  A chunk that is skipped, read before it landed or read from another buffer of the ring
    loses one of the two, and then the match moves to the other row or is no longer accepted."""
    x = x_rows(160, cross_check)
    ys = [y_ends(n, best_last) for n in Y_SIZES]
    k = len(ys)
    woff, wm, _ = run(amc_ctx, [x] + ys, np.zeros(k), np.arange(1, k + 1), cross_check)
    counts = np.diff(woff.astype(np.int64))
    assert np.all(counts == (1 if cross_check else 160))
    want_row = np.repeat([n - 1 if best_last else 0 for n in Y_SIZES], counts)
    assert np.array_equal(wm[:, 1], want_row)


# ---- 3. consecutive items with different Y lengths ---------------------------------------------------------------------
Y_CYCLE = [1025, 1, 385, 129]   # nine chunks, one, four (one fetch in the loop), two


@pytest.mark.parametrize("cross_check", [False, True])
def test_items_of_different_y_lengths_follow_each_other(amc_ctx, cross_check):
    """One call whose items alternate between Y images of 1025, 1, 385 and 129 rows - an item never mixes streamed
    images, and items are queued in Y order - three times as many as there are resident workgroups: every workgroup
    scans several, of different lengths, and the ring position and the counted waits start over at each."""
    n = 3 * workgroups() + 8
    x = x_rows(16, cross_check)
    proto = [y_ends(rows, True) for rows in Y_CYCLE]
    imgs = [x] + [proto[k % 4] for k in range(n)]
    woff, wm, _ = run(amc_ctx, imgs, np.zeros(n), np.arange(1, n + 1), cross_check)
    assert np.all(np.diff(woff.astype(np.int64)) == (1 if cross_check else 16))
    first = wm[woff[:-1].astype(np.int64), 1]
    assert np.array_equal(first, np.array([Y_CYCLE[k % 4] - 1 for k in range(n)]))


# ---- 4. more items than resident workgroups ----------------------------------------------------------------------------
@pytest.mark.parametrize("cross_check", [False, True])
def test_more_items_than_resident_workgroups(amc_ctx, cross_check):
    """2 x CUs + 40 pairs, each with a one-row Y image of its own and a 16-row X: every workgroup pops an item, some
    pop two, and two workgroups share every CU.  Every fifth Y image is a zero row, which matches nothing: an item that
    is scanned twice, not at all, or against a neighbour's image shows."""
    n = workgroups() + 40
    x = x_rows(16, cross_check)
    ys = [planted(1, {0: BEST} if k % 5 else {}) for k in range(n)]
    woff, wm, _ = run(amc_ctx, [x] + ys, np.zeros(n), np.arange(1, n + 1), cross_check)
    per = 1 if cross_check else 16
    assert np.diff(woff.astype(np.int64)).tolist() == [per if k % 5 else 0 for k in range(n)]
    assert np.all(wm[:, 1] == 0)


# ---- 5. random images --------------------------------------------------------------------------------------------------
RAND_OPTS = (1.0, 2.0)   # every row whose best beats its second is accepted: the result depends on every row's top two


@pytest.fixture(scope="module")
def random_sets():
    """Two sets of 24 images, n ~ U[1, 700] rows of bytes below 64 (dot products below 512^2, so distances tell rows
    apart), with the oracle's answers for all pairs, cross check off and on - computed once."""
    rng = np.random.default_rng(4)
    sets = []
    i, j = np.triu_indices(24, k=1)
    s1, s2 = i.astype(np.uint32), j.astype(np.uint32)
    for _ in range(2):
        sizes = rng.integers(1, 701, size=24)
        imgs = [rng.integers(0, 64, size=(int(n), 128), dtype=np.uint8) for n in sizes]
        want = {cc: oracle_lib.match_pairs(imgs, s1, s2, *RAND_OPTS, cc) for cc in (False, True)}
        # the inputs are what the test needs: one to six segments, and nearly every row of every pair matched forward
        assert sizes.min() <= 128 and sizes.max() > 512
        assert np.all(np.diff(want[False][0].astype(np.int64)) >= 0.9 * sizes[i])
        assert len(want[True][1]) > 0
        sets.append((imgs, want))
    assert [len(a) for a in sets[0][0]] != [len(a) for a in sets[1][0]]
    return s1, s2, sets


@pytest.mark.parametrize("cross_check", [False, True])
def test_random_sizes_twice_on_one_context(amc_ctx, random_sets, cross_check):
    """All 276 pairs of 24 random images, then the same call with other images of other sizes on the same context:
    the second finds the first one's rows, accept words and descriptors in the tables and must read none of them."""
    s1, s2, sets = random_sets
    for imgs, want in sets:
        run(amc_ctx, imgs, s1, s2, cross_check, want=want[cross_check], opts=RAND_OPTS)


# ---- 6. empty images, a single pair ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross_check", [False, True])
def test_empty_images_and_a_single_pair(amc_ctx, cross_check):
    """An image without rows on either side of a pair (no segments at all, or a group without items) beside pairs that
    match; then a pair list of one pair, whose launch is a single workgroup."""
    x = x_rows(130, cross_check)
    y = y_ends(129, True)
    empty = np.zeros((0, 128), np.uint8)
    imgs = [x, y, empty]
    s1 = [0, 2, 0, 2, 0]
    s2 = [1, 1, 2, 2, 1]
    woff, wm, _ = run(amc_ctx, imgs, s1, s2, cross_check)
    per = 1 if cross_check else 130
    assert np.diff(woff.astype(np.int64)).tolist() == [per, 0, 0, 0, per]
    assert np.all(wm[:, 1] == 128)
    woff, wm, _ = run(amc_ctx, imgs, [0], [1], cross_check)
    assert int(woff[-1]) == per and np.all(wm[:, 1] == 128)
    woff, wm, _ = run(amc_ctx, imgs, [2], [1], cross_check)
    assert int(woff[-1]) == 0
