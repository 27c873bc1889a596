"""The end of an item in the match scan (match_mfma.hip): the four lane quarters' top-2 states of a wave's eight X tiles
are merged by a reduce-scatter (v_permlane32_swap for the tiles xt and xt + 4, v_permlane16_swap for the pairs left),
after which every lane holds one row of the segment - lane quarter q of register set k the X tile 2k + (q & 1) +
4 (q >> 1) - and decodes, tests and stores it.  A wrong lane is a wrong row, a wrong word of the accept mask a lost or
an invented match: every case goes through amc_match_pairs and is compared with the oracle row for row, without
tolerance, forward only and with the cross check (the reverse scan stores through candidate lists)."""
import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

OPTS = (1.0, 2.0)   # every row whose best beats its second is accepted: the result depends on every row's top two


def random_image(rng, n, high=64):
    return rng.integers(0, high, size=(int(n), 128), dtype=np.uint8)


def unit_image(rng, n):
    """n rows of norm 512, as an extractor writes them: a copy of a row is at distance ~0, any other row at ~0.7."""
    v = rng.random((int(n), 128))
    return np.rint(v * (512.0 / np.linalg.norm(v, axis=1, keepdims=True))).astype(np.uint8)


def run(ctx, imgs, s1, s2, cross_check, opts=OPTS):
    ctx.reserve_slots(len(imgs))
    for k, im in enumerate(imgs):
        ctx.upload_descriptors(k, im)
    s1 = np.asarray(s1, np.uint32)
    s2 = np.asarray(s2, np.uint32)
    off, m, st = ctx.match_pairs(s1, s2, *opts, cross_check, kernel="mfma")
    woff, wm = oracle_lib.match_pairs(imgs, s1, s2, *opts, cross_check)
    assert st["pairs_mfma"] == len(s1) and st["pairs_dot4"] == 0
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(m, wm)
    return woff, wm


# X rows: a segment is 128 rows = eight tiles of 16; counts at the tile edges of either register set, of either half
X_ROWS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 79, 81, 95, 97, 112, 113, 127, 128, 129, 200]


@pytest.mark.parametrize("cross_check", [False, True])
def test_segments_that_end_at_every_tile_edge(amc_ctx, cross_check):
    """X images of 1 .. 200 rows against one Y image of 300 rows (three chunks, every lane quarter sees rows of every
    block) in which each X row has its own copy: row i of every X image matches a known Y row, in a tile that depends on
    i, so a row decoded in the wrong lane quarter or stored at the wrong place shows."""
    rng = np.random.default_rng(41)
    y = random_image(rng, 300)
    perm = rng.permutation(300)
    xs = [y[perm[:n]].copy() for n in X_ROWS]
    imgs = xs + [y]
    s1 = np.arange(len(xs))
    s2 = np.full(len(xs), len(xs))
    woff, wm = run(amc_ctx, imgs, s1, s2, cross_check)
    counts = np.diff(woff.astype(np.int64))
    assert np.all(counts >= 0.9 * np.array(X_ROWS) - 1)   # the inputs are what the test needs: nearly every row matched


@pytest.mark.parametrize("cross_check", [False, True])
def test_equal_bests_in_different_lane_quarters_are_rejected_or_kept_like_the_oracle(amc_ctx, cross_check):
    """Y rows that repeat 32, 64 and 96 rows further on - another lane quarter of the same block - and 128 further on -
    the same quarter of the next block: the best of an X row that is one of them is found twice with the same value, so
    its second equals its best (rejected), whichever quarter the merge takes first; the X rows beside it are kept."""
    rng = np.random.default_rng(42)
    y = random_image(rng, 384)
    for d, rows in ((32, range(0, 8)), (64, range(8, 16)), (96, range(16, 24)), (128, range(40, 48))):
        for r in rows:
            y[r + d] = y[r]
    x = y[rng.permutation(384)[:150]].copy()
    woff, wm = run(amc_ctx, [x, y], [0], [1], cross_check)
    assert 60 <= int(woff[1]) < 150


@pytest.mark.parametrize("cross_check", [False, True])
def test_accept_words_of_tiles_without_an_accepted_row(amc_ctx, cross_check):
    """A 128-row X image of which only the rows of some tiles can match (the others are far from every Y row under a
    distance bound of 0.3): accept words with one empty half, empty words between full ones, and tiles that are not
    stored beside tiles that are - in both register sets and both halves of the wave."""
    rng = np.random.default_rng(43)
    y = unit_image(rng, 260)
    x = unit_image(rng, 128)                     # nothing like a Y row
    for tile in (0, 3, 4, 6):                    # X tiles whose rows are copies of Y rows
        x[16 * tile:16 * tile + 16] = y[rng.permutation(260)[:16]]
    x[16 * 7 + 5] = y[7]                         # and one single row of tile 7
    woff, wm = run(amc_ctx, [x, y], [0], [1], cross_check, opts=(0.8, 0.3))
    got = set(int(r) // 16 for r in wm[:, 0])
    assert got == {0, 3, 4, 6, 7}
