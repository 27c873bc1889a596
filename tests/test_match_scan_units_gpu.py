"""The MFMA scan's units: a lane reduces the 16 outputs of a 16-row unit of Y to their maximum, keeps the top two of
those maxima and the unit of the best, and four lanes per X row are merged at the end (match_mfma.hip).  These
tests plant values at chosen rows of otherwise zero images - zero rows make every dot product exact and known - and
compare the matches row for row with the oracle.

The planted rows use four dimensions: an X row (255, 255, 255, 255, 0, ...) against a Y row (a, b, c, d, 0, ...) has the
dot product 255 (a + b + c + d).  With d(v) = acos(v / 512^2):
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
DECOY = (255, 255, 0, 0)


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


def run(ctx, imgs, s1, s2, opts, min_matches=None):
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
    if min_matches is not None:
        assert int(woff[-1]) >= min_matches  # the scene says what it was built to say
    return woff, wm


@pytest.mark.parametrize("cross_check", [False, True])
def test_best_at_every_output_position(amc_ctx, cross_check):
    """Y image k holds the best at row k and an accepting second at row (k + 37) mod 128: every MFMA tile, lane
    quarter and accumulator register is the best's place once, for every one of the 128 X rows."""
    imgs = [x_image(128, cross_check)]
    imgs += [planted(128, {k: BEST, (k + 37) % 128: SEC_ACCEPT, (k + 71) % 128: DECOY}) for k in range(128)]
    s1 = np.zeros(128, np.uint32)
    s2 = np.arange(1, 129, dtype=np.uint32)
    woff, wm = run(amc_ctx, imgs, s1, s2, (0.8, 0.7, cross_check))
    # without the cross check every X row matches row k of image k; with it only X row 0 is built to
    per_pair = np.diff(woff.astype(np.int64))
    assert np.all(per_pair == (1 if cross_check else 128))
    assert np.array_equal(wm[woff[:-1].astype(np.int64), 1], np.arange(128))


# (row of the best, row of the second): same 16-row unit; the other unit of the 32-row tile; the other tile of the
# 64-row block; the next block; the next 256-row chunk - each both ways round
SECOND_PLACES = [(5, 9), (9, 5), (5, 20), (20, 5), (5, 40), (40, 5), (5, 70), (70, 5), (255, 256), (256, 255),
                 (130, 143), (47, 48), (63, 64), (191, 192), (300, 17)]


@pytest.mark.parametrize("cross_check", [False, True])
def test_where_the_second_lies(amc_ctx, cross_check):
    """For every placement the second accepts in one image and rejects in the next (max_ratio 0.8), and at max_ratio
    1.0 a second one step below the best accepts where an exact tie rejects; a decoy far below sits in a third unit."""
    n = 320
    x = x_image(16, cross_check)
    for ratio, seconds in ((0.8, (SEC_ACCEPT, SEC_REJECT)), (1.0, (SEC_BELOW, BEST))):
        imgs = [x]
        for rb, rs in SECOND_PLACES:
            decoy = next(r for r in (100, 200, 310) if abs(r - rb) > 64 and abs(r - rs) > 64)
            for sec in seconds:
                imgs.append(planted(n, {rb: BEST, rs: sec, decoy: DECOY}))
        npairs = len(imgs) - 1
        woff, wm = run(amc_ctx, imgs, np.zeros(npairs, np.uint32), np.arange(1, npairs + 1), (ratio, 0.7, cross_check))
        per_pair = np.diff(woff.astype(np.int64))
        rows = 1 if cross_check else 16
        assert np.array_equal(per_pair, np.tile([rows, 0], len(SECOND_PLACES)))  # accept, reject, accept, ...
        assert np.array_equal(wm[woff[:-1:2].astype(np.int64), 1], [rb for rb, _ in SECOND_PLACES])


@pytest.mark.parametrize("cross_check", [False, True])
def test_ties_for_the_best_keep_the_lowest_index(amc_ctx, cross_check):
    """The same best value twice (max_ratio above 1 lets a tie through the ratio test): in two lane quarters of one
    block, in two blocks, and in blocks 64 apart, which carry the same 7-bit code on either side of the flush."""
    x = x_image(16, cross_check)
    n_big = 4096 + 64
    cases = [(128, (3, 50)), (128, (20, 40)), (128, (17, 30)), (128, (60, 66)), (320, (10, 100)), (320, (200, 290)),
             (320, (255, 256)), (n_big, (30, 4096 + 30)), (n_big, (4095, 4096)), (n_big, (100, 4100)),
             (n_big, (4000, 4150)), (n_big, (7, 2055, 4103))]
    imgs = [x] + [planted(n, {r: BEST for r in rows}) for n, rows in cases]
    npairs = len(cases)
    woff, wm = run(amc_ctx, imgs, np.zeros(npairs, np.uint32), np.arange(1, npairs + 1), (1.01, 0.7, cross_check))
    assert np.all(np.diff(woff.astype(np.int64)) == (1 if cross_check else 16))
    assert np.array_equal(wm[woff[:-1].astype(np.int64), 1], [min(rows) for _, rows in cases])


N2_EDGES = [1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 256, 257]
N1_EDGES = [1, 15, 17, 127, 128, 129]


@pytest.mark.parametrize("cross_check", [False, True])
def test_edge_sizes_random_bytes(amc_ctx, cross_check):
    """Every n1 x n2 of the edge sizes, random bytes.  Bytes below 48 keep the dot products under 512^2 (the distance
    saturates above it and nothing would be told apart); (1.0, 2.0) accepts every row whose best is not tied, the
    default options nearly none: both are compared.  Full-range bytes and a mix of both signs follow."""
    rng = np.random.default_rng(2024)
    imgs = [rng.integers(0, 48, size=(n, 128), dtype=np.uint8) for n in N1_EDGES + N2_EDGES]
    s1 = np.repeat(np.arange(len(N1_EDGES)), len(N2_EDGES))
    s2 = np.tile(np.arange(len(N2_EDGES)) + len(N1_EDGES), len(N1_EDGES))
    run(amc_ctx, imgs, s1, s2, (1.0, 2.0, cross_check), min_matches=len(s1))
    run(amc_ctx, imgs, s1, s2, (0.8, 0.7, cross_check))
    run(amc_ctx, imgs, s2, s1, (1.0, 2.0, cross_check), min_matches=len(s1))
    # Both sides of the a - 128 zero point.  Full-range bytes first: every dot product is above 512^2, every distance
    # 0, so only rows against a one-row image (second = 0) are accepted.  Then the small bytes with two entries of
    # 128..255 per row: operands of either sign through the C operand and the row mapping, and rows that still tell apart.
    full = [rng.integers(0, 256, size=(n, 128), dtype=np.uint8) for n in N1_EDGES + N2_EDGES]
    run(amc_ctx, full, s1, s2, (1.0, 2.0, cross_check), min_matches=1)
    mixed = [im.copy() for im in imgs]
    for im in mixed:
        cols = rng.integers(0, 128, size=(len(im), 2))
        im[np.arange(len(im))[:, None], cols] = rng.integers(128, 256, size=(len(im), 2), dtype=np.uint8)
    run(amc_ctx, mixed, s1, s2, (1.0, 2.0, cross_check), min_matches=len(s1))
    run(amc_ctx, mixed, s2, s1, (1.0, 2.0, cross_check), min_matches=len(s1))


def line_patterns():
    """132 subsets of four dimensions, any two sharing at most one: the first four points of the lines of the affine
    plane over Z_11 (dimension = 11 x + y).  Equal patterns score 4 * 255^2, different ones at most 255^2."""
    pats = [[11 * xx + (a * xx + b) % 11 for xx in range(4)] for a in range(11) for b in range(11)]
    pats += [[11 * c + yy for yy in range(4)] for c in range(11)]
    return pats


def test_reverse_scan_candidate_counts(amc_ctx):
    """Cross check on: c planted mutual matches are c accepted rows pointing at c distinct columns, so the reverse
    scan (MODE 1) gets exactly c candidate rows - around its 16-row X tiles and its 128-row segments."""
    rng = np.random.default_rng(7)
    pats = line_patterns()
    counts = [1, 15, 16, 17, 127, 128, 129]
    imgs, want = [], []
    for c in counts:
        a = np.zeros((300, 128), np.uint8)
        b = np.zeros((333, 128), np.uint8)
        ra = np.sort(rng.choice(300, c, replace=False))
        rb = rng.permutation(333)[:c]
        for j in range(c):
            a[ra[j], pats[j]] = 255
            b[rb[j], pats[j]] = 255
        imgs += [a, b]
        want.append(np.stack([ra, rb], axis=1))
    s1 = np.arange(0, 2 * len(counts), 2)
    woff, wm = run(amc_ctx, imgs, s1, s1 + 1, (0.8, 0.7, True))
    assert np.array_equal(np.diff(woff.astype(np.int64)), counts)
    np.testing.assert_array_equal(wm, np.concatenate(want))
