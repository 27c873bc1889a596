"""The MFMA scan's 128-row blocks: within a block of Y a lane quarter owns 32 contiguous rows - one of the 32-row tiles
resolve_index recomputes - reduces its 32 outputs to their maximum over four steps, and inserts that maximum once per
block; the block code is 7 bits, settled every 64 blocks = 8,192 rows; the scan of an image's last chunk ends at the
last block that holds rows (match_mfma.hip).  These tests plant values at chosen rows of otherwise zero images - zero
rows make every dot product exact and known - and compare the matches row for row with the oracle: equalities, no
tolerance.

The planting is that of test_match_scan_units_gpu.py, restated.  The planted rows use four dimensions: an X row
(255, 255, 255, 255, 0, ...) against a Y row (a, b, c, d, 0, ...) has the dot product 255 (a + b + c + d).  With
d(v) = acos(v / 512^2):
    best   260100 = 255 * 1020    d = 0.12494   (passes max_distance 0.7)
    second 258825 = 255 * 1015    0.8 d = 0.12742 > 0.12494: the ratio test ACCEPTS
    second 259080 = 255 * 1016    0.8 d = 0.12243 < 0.12494: the ratio test REJECTS
    decoy  130050 = 255 *  510    far below: a scan that loses the second and reports the decoy accepts either way
so the outcome of a row depends on the exact second value, and the match index on the exact best row."""
import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

BEST = (255, 255, 255, 255)
SEC_ACCEPT = (255, 255, 255, 250)   # 255 * 1015
SEC_REJECT = (255, 255, 255, 251)   # 255 * 1016
SEC_BELOW = (255, 255, 255, 254)    # one step under the best: passes max_ratio 1.0, a tie does not
DECOY = (255, 255, 0, 0)            # 255 * 510


def planted(n, rows):
    """n x 128 zero image with the 4-vectors of `rows` ({row: values}) in dimensions 0..3."""
    im = np.zeros((n, 128), np.uint8)
    for r, v in rows.items():
        im[r, :4] = v
    return im


def x_image(n, cross_check):
    """n X rows that all score the planted values above.  For the cross check only row 0 does: identical rows would
    tie in the column direction and nothing would be mutual; the others score 255 * 965 against the best."""
    return planted(n, {r: BEST if r == 0 or not cross_check else (255, 255, 255, 200) for r in range(n)})


def run(ctx, imgs, s1, s2, opts):
    ctx.reserve_slots(len(imgs))
    for k, im in enumerate(imgs):
        ctx.upload_descriptors(k, im)
    s1 = np.asarray(s1, np.uint32)
    s2 = np.asarray(s2, np.uint32)
    off, m, st = ctx.match_pairs(s1, s2, *opts, kernel="mfma")
    woff, wm = oracle_lib.match_pairs(imgs, s1, s2, *opts)
    assert st["pairs_mfma"] == len(s1) and st["pairs_dot4"] == 0
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(m, wm)
    return woff, wm


def first_columns(woff, wm, pairs):
    """Column matched by the first row of each of `pairs` (which all have matches)."""
    return wm[woff[:-1].astype(np.int64)[pairs], 1]


@pytest.mark.parametrize("cross_check", [False, True])
def test_best_at_every_output_position(amc_ctx, cross_check):
    """Y image k (256 rows: both blocks of a chunk) holds the best at row k, an accepting second at row (k + 37) mod 256
    and a decoy at (k + 71) mod 256: every block, MFMA tile, lane quarter and accumulator register is the best's place
    once, for every one of the 128 X rows."""
    imgs = [x_image(128, cross_check)]
    imgs += [planted(256, {k: BEST, (k + 37) % 256: SEC_ACCEPT, (k + 71) % 256: DECOY}) for k in range(256)]
    woff, wm = run(amc_ctx, imgs, np.zeros(256, np.uint32), np.arange(1, 257, dtype=np.uint32), (0.8, 0.7, cross_check))
    # without the cross check every X row matches row k of image k; with it only X row 0 is built to
    assert np.all(np.diff(woff.astype(np.int64)) == (1 if cross_check else 128))
    assert np.array_equal(first_columns(woff, wm, np.arange(256)), np.arange(256))


# (row of the best, row of the second): the same 32-row tile (one lane quarter's rows of a block); another quarter of
# the block; the other block of the 256-row chunk; the next chunk - each both ways round
SECOND_PLACES = [(5, 9), (9, 5), (5, 40), (40, 5), (5, 100), (100, 5), (5, 130), (130, 5), (31, 32), (32, 31),
                 (127, 128), (128, 127), (255, 256), (256, 255), (300, 17)]


@pytest.mark.parametrize("cross_check", [False, True])
def test_where_the_second_lies(amc_ctx, cross_check):
    """For every placement the second accepts in one image and rejects in the next (max_ratio 0.8), and at max_ratio
    1.0 a second one step below the best accepts where an exact tie rejects; a decoy far below sits in a third tile."""
    n = 320
    x = x_image(16, cross_check)
    for ratio, seconds in ((0.8, (SEC_ACCEPT, SEC_REJECT)), (1.0, (SEC_BELOW, BEST))):
        imgs = [x]
        for rb, rs in SECOND_PLACES:
            decoy = next(r for r in (70, 200, 310) if r // 32 not in (rb // 32, rs // 32))
            for sec in seconds:
                imgs.append(planted(n, {rb: BEST, rs: sec, decoy: DECOY}))
        npairs = len(imgs) - 1
        woff, wm = run(amc_ctx, imgs, np.zeros(npairs, np.uint32), np.arange(1, npairs + 1), (ratio, 0.7, cross_check))
        rows = 1 if cross_check else 16
        assert np.array_equal(np.diff(woff.astype(np.int64)), np.tile([rows, 0], len(SECOND_PLACES)))  # accept, reject, ...
        assert np.array_equal(first_columns(woff, wm, np.arange(0, npairs, 2)), [rb for rb, _ in SECOND_PLACES])


@pytest.mark.parametrize("cross_check", [False, True])
def test_ties_for_the_best_keep_the_lowest_index(amc_ctx, cross_check):
    """The same best value twice or three times (max_ratio above 1 lets a tie through the ratio test): in one lane
    quarter's tile, in two quarters of one block, in two blocks of a chunk, and in two chunks."""
    x = x_image(16, cross_check)
    cases = [(128, (3, 20)), (128, (3, 50)), (128, (40, 100)), (128, (31, 32)), (128, (60, 127)), (256, (130, 250)),
             (256, (10, 200)), (256, (127, 128)), (256, (96, 224)), (600, (200, 290)), (600, (255, 256)),
             (600, (100, 356)), (600, (7, 263, 519))]
    imgs = [x] + [planted(n, {r: BEST for r in rows}) for n, rows in cases]
    npairs = len(cases)
    woff, wm = run(amc_ctx, imgs, np.zeros(npairs, np.uint32), np.arange(1, npairs + 1), (1.01, 0.7, cross_check))
    assert np.all(np.diff(woff.astype(np.int64)) == (1 if cross_check else 16))
    assert np.array_equal(first_columns(woff, wm, np.arange(npairs)), [min(rows) for _, rows in cases])


@pytest.mark.parametrize("cross_check", [False, True])
def test_the_64_block_code_group(amc_ctx, cross_check):
    """Y of 8,448 rows = 33 chunks = 66 blocks: blocks 0..63 are the first code group, 64 and 65 reuse its codes behind
    the flush.  Bests at the group's last row, the next group's first row and its second block; a tie across the
    groups keeps the lower row; a second in the other group than the best, both ways round, accepting and rejecting."""
    n = 8448
    x = x_image(16, cross_check)
    cases = [({8191: BEST, 8192: SEC_ACCEPT, 40: DECOY}, 8191, True),
             ({8191: BEST, 8192: SEC_REJECT, 40: DECOY}, 8191, False),
             ({8192: BEST, 8191: SEC_ACCEPT, 40: DECOY}, 8192, True),
             ({8192: BEST, 8191: SEC_REJECT, 40: DECOY}, 8192, False),
             ({8320: BEST, 130: SEC_ACCEPT, 8400: DECOY}, 8320, True),   # block 65 and block 1: the same code
             ({8320: BEST, 130: SEC_REJECT, 8400: DECOY}, 8320, False),
             ({50: BEST, 8300: SEC_ACCEPT, 4000: DECOY}, 50, True),
             ({50: BEST, 8300: SEC_REJECT, 4000: DECOY}, 50, False),
             ({8300: BEST, 50: SEC_ACCEPT, 4000: DECOY}, 8300, True),
             ({8300: BEST, 50: SEC_REJECT, 4000: DECOY}, 8300, False)]
    imgs = [x] + [planted(n, rows) for rows, _, _ in cases]
    npairs = len(cases)
    woff, wm = run(amc_ctx, imgs, np.zeros(npairs, np.uint32), np.arange(1, npairs + 1), (0.8, 0.7, cross_check))
    rows = 1 if cross_check else 16
    assert np.array_equal(np.diff(woff.astype(np.int64)), [rows if ok else 0 for _, _, ok in cases])
    hit = np.array([k for k, c in enumerate(cases) if c[2]])
    assert np.array_equal(first_columns(woff, wm, hit), [cases[k][1] for k in hit])
    # the tie: rows 100 (block 0) and 8200 (block 64) carry the same code on either side of the flush; row 100 wins
    ties = [x, planted(n, {100: BEST, 8200: BEST}), planted(n, {100: BEST, 8200: BEST, 4200: BEST})]
    woff, wm = run(amc_ctx, ties, np.zeros(2, np.uint32), np.arange(1, 3), (1.01, 0.7, cross_check))
    assert np.all(np.diff(woff.astype(np.int64)) == rows)
    assert np.array_equal(first_columns(woff, wm, np.arange(2)), [100, 100])


N_Y_EDGES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385]
N_X_EDGES = [1, 127, 128, 129]


@pytest.mark.parametrize("cross_check", [False, True])
def test_size_edges(amc_ctx, cross_check):
    """Every n_x x n_y of the edge sizes, the best in the last real row and the second in row 0 (accepting in one image,
    rejecting in the next; a one-row image has no second).  n_y = 129 and 385 are the pad-skip's edge: a last block
    with a single real row, which holds the best."""
    xs = [x_image(n, cross_check) for n in N_X_EDGES]
    ys, ok = [], []
    for n in N_Y_EDGES:
        for sec in (SEC_ACCEPT, SEC_REJECT):
            ys.append(planted(n, {0: sec, n - 1: BEST} if n > 1 else {0: BEST}))
            ok.append(n == 1 or sec is SEC_ACCEPT)
    imgs = xs + ys
    s1 = np.repeat(np.arange(len(xs)), len(ys))
    s2 = np.tile(np.arange(len(ys)) + len(xs), len(xs))
    woff, wm = run(amc_ctx, imgs, s1, s2, (0.8, 0.7, cross_check))
    want = [(1 if cross_check else nx) if a else 0 for nx in N_X_EDGES for a in ok]
    assert np.array_equal(np.diff(woff.astype(np.int64)), want)
    hit = np.flatnonzero(want)
    assert np.array_equal(first_columns(woff, wm, hit), [len(imgs[s2[k]]) - 1 for k in hit])
