"""The MFMA scan's chunk loop (match_mfma.hip) is peeled: a steady loop whose every step fetches a piece of the chunk three
ahead and whose crossing waits with one fixed count, a drain loop for the last up to three chunks, a loop of its own for
waves without rows, read addresses that move round the ring of four LDS buffers in place, and DMA addresses that advance
on the scalar unit.  These tests sit where that structure can go wrong, not at the workload's shapes: every region of
the peeled loop at every ring position, every DMA piece of every ring buffer, the 64-block flush, the C operand on
full-range bytes, and items whose waves are all idle but one.  Every comparison is row for row with the oracle, without
tolerance, with the cross check off and on (the reverse scan is the same kernel code).

The planting is that of test_match_scan_items4_gpu.py: planted rows use four dimensions, an X row
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
from pycolmap_amd import _capi  # noqa: F401  (the library must load: there is no fallback)

pytestmark = pytest.mark.gpu

BEST = (255, 255, 255, 255)
SEC_ACCEPT = (255, 255, 255, 250)   # 255 * 1015
WEAK = (255, 255, 255, 200)
OPTS = (0.8, 0.7)
CHUNK = 128


def planted(n, rows):
    """n x 128 zero image with the 4-vectors of `rows` ({row: values}, later entries win) in dimensions 0..3."""
    im = np.zeros((n, 128), np.uint8)
    for r, v in rows.items():
        im[r, :4] = v
    return im


def x_rows(n, cross_check):
    """n planted X rows: all BEST, or - under the cross check, where equal rows tie - BEST in row 0 and WEAK elsewhere."""
    return planted(n, {r: BEST if r == 0 or not cross_check else WEAK for r in range(n)})


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


def check_best_rows(off, m, best_rows, x_n, cross_check):
    """Pair k matched all its X rows (one under the cross check) to Y row best_rows[k]."""
    counts = np.diff(off.astype(np.int64))
    assert np.all(counts == (1 if cross_check else x_n))
    assert np.array_equal(m[:, 1], np.repeat(np.asarray(best_rows), counts))


# ---- 1. every region of the peeled loop, every ring position -----------------------------------------------------------
# one chunk (no crossing), two and three (drain only), four (one steady chunk), five to eight (the steady loop walks the
# ring once), nine, twelve and thirteen (it wraps; thirteen leaves the steady loop at another ring position than twelve)
CHUNK_COUNTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]


def chunk_walk_images():
    """For every k of CHUNK_COUNTS, every size 128 k - 127, 128 k - 1, 128 k and every chunk c of the image: a Y image
    with BEST in a row of chunk c and SEC_ACCEPT in a row of chunk (c + 1) mod k.  The row within the chunk cycles
    through 0, 9, 18, ... mod 128 from image to image (taken modulo the rows the chunk holds), so all four steps and both
    MFMA tiles of a step are hit.  Returns the images and their BEST rows."""
    ys, best_rows = [], []
    r = 0
    for k in CHUNK_COUNTS:
        for n in (CHUNK * k - 127, CHUNK * k - 1, CHUNK * k):
            for c in range(k):
                def row_in(chunk, within):
                    held = min(CHUNK, n - CHUNK * chunk)
                    return CHUNK * chunk + within % held
                b = row_in(c, r)
                s = row_in((c + 1) % k, r)
                if s == b:   # one chunk: both rows are in it
                    s = row_in(c, r + 64) if n > 1 else None
                    if s == b:
                        s = row_in(c, r + 1)
                rows = {b: BEST} if s is None else {s: SEC_ACCEPT, b: BEST}
                ys.append(planted(n, rows))
                best_rows.append(b)
                r = (r + 9) % CHUNK
    return ys, best_rows


@pytest.fixture(scope="module")
def chunk_walk():
    ys, best_rows = chunk_walk_images()
    assert len(ys) == 3 * sum(CHUNK_COUNTS)
    # the rows within a chunk really spread over the four steps and the two tiles of a step
    assert {(b % CHUNK) % 32 // 8 for b in best_rows} == {0, 1, 2, 3}
    assert {(b % CHUNK) % 8 // 4 for b in best_rows} == {0, 1}
    return ys, best_rows


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("x_n", [16, 160])
def test_every_region_of_the_peeled_loop_at_every_ring_position(amc_ctx, chunk_walk, x_n, cross_check):
    """An X image of 16 rows (one live wave, three that only feed the ring) or of 160 (two and two) against all images
    of chunk_walk_images in one call.  A chunk read from the wrong buffer, skipped, or read before it landed moves the
    match to the SEC_ACCEPT row or loses it."""
    ys, best_rows = chunk_walk
    k = len(ys)
    off, m, _ = run(amc_ctx, [x_rows(x_n, cross_check)] + ys, np.zeros(k), np.arange(1, k + 1), cross_check)
    check_best_rows(off, m, best_rows, x_n, cross_check)


# ---- 2. every DMA piece of every ring buffer ---------------------------------------------------------------------------
@pytest.mark.parametrize("cross_check", [False, True])
def test_every_dma_piece_of_every_ring_buffer(amc_ctx, cross_check):
    """Y images of 641 rows: six chunks, so the buffers of chunks 0 and 1 are used twice.  A DMA piece is 1 KiB, eight
    rows; image p has BEST in row 8 p + (p mod 8), a row of piece p, for p = 0 .. 80, and SEC_ACCEPT in row 0 (row 640
    for p = 0).  A piece fetched from the wrong global offset or written to the wrong slot shows at exactly that p."""
    n = 641
    best_rows = [8 * p + p % 8 for p in range(81)]
    assert best_rows[-1] == n - 1
    ys = [planted(n, {(0 if p else n - 1): SEC_ACCEPT, b: BEST}) for p, b in enumerate(best_rows)]
    k = len(ys)
    off, m, _ = run(amc_ctx, [x_rows(16, cross_check)] + ys, np.zeros(k), np.arange(1, k + 1), cross_check)
    check_best_rows(off, m, best_rows, 16, cross_check)


# ---- 3. the 64-block flush ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross_check", [False, True])
def test_the_64_block_flush(amc_ctx, cross_check):
    """Y images of 8,192, 8,193, 8,320 and 8,449 rows (64, 65, 65 and 67 chunks): the block codes start over behind
    block 63.  BEST in row 8,191, the last row of the first group, or in row 8,192, the first of the second, with
    SEC_ACCEPT in row 0 or in the last row."""
    ys, best_rows = [], []
    for n in (8192, 8193, 8320, 8449):
        for b in (8191, 8192):
            for s in (0, n - 1):
                if b < n and s != b:
                    ys.append(planted(n, {s: SEC_ACCEPT, b: BEST}))
                    best_rows.append(b)
    assert len(ys) == 12
    k = len(ys)
    off, m, _ = run(amc_ctx, [x_rows(16, cross_check)] + ys, np.zeros(k), np.arange(1, k + 1), cross_check)
    check_best_rows(off, m, best_rows, 16, cross_check)


# ---- 4. the C operand per chunk on full-range bytes --------------------------------------------------------------------
RAND_OPTS = (1.0, 2.0)   # every row whose best beats its second is accepted: the result depends on every row's top two


@pytest.fixture(scope="module")
def full_range_sets():
    """Two sets of 16 images, n ~ U[1, 700] rows, every row four non-zero bytes from 128 .. 255 at random dimensions:
    dot products stay below 512^2 (4 * 255^2 = 260,100), the row sums - the C operand - differ from row to row, and
    every non-zero byte crosses the zero point.  With the oracle's answers for all 120 pairs, computed once."""
    rng = np.random.default_rng(0)
    i, j = np.triu_indices(16, k=1)
    s1, s2 = i.astype(np.uint32), j.astype(np.uint32)
    sets = []
    for _ in range(2):
        sizes = rng.integers(1, 701, size=16)
        imgs = []
        for n in sizes:
            n = int(n)
            im = np.zeros((n, 128), np.uint8)
            dims = np.argsort(rng.random((n, 128)), axis=1)[:, :4]
            im[np.arange(n)[:, None], dims] = rng.integers(128, 256, size=(n, 4), dtype=np.uint8)
            imgs.append(im)
        want = {cc: oracle_lib.match_pairs(imgs, s1, s2, *RAND_OPTS, cc) for cc in (False, True)}
        assert {int(c) % 4 for c in (sizes + CHUNK - 1) // CHUNK} == {0, 1, 2, 3}
        assert len(want[False][1]) >= 0.5 * sizes[i].sum()
        assert len(want[True][1]) > 0
        sets.append((imgs, want))
    return s1, s2, sets


@pytest.mark.parametrize("cross_check", [False, True])
def test_c_operand_on_full_range_bytes(amc_ctx, full_range_sets, cross_check):
    """All 120 pairs of a set, then the second set on the same context."""
    s1, s2, sets = full_range_sets
    for imgs, want in sets:
        run(amc_ctx, imgs, s1, s2, cross_check, want=want[cross_check], opts=RAND_OPTS)


# ---- 5. an item whose waves are all idle but one, beside full items -----------------------------------------------------
@pytest.mark.parametrize("cross_check", [False, True])
def test_items_with_one_live_wave_beside_full_items(amc_ctx, cross_check):
    """X images of 1, 128, 129 and 512 rows, every row planted, against Y images of 385 rows (four chunks: one steady,
    three drained) and of 1,025 (nine) in one call: per Y image one item with a single live wave, two full ones, and
    one whose first wave is full and whose second holds one row."""
    x_sizes = [1, 128, 129, 512]
    xs = [planted(n, {r: BEST for r in range(n)}) for n in x_sizes]
    ys = [planted(n, {0: SEC_ACCEPT, n - 1: BEST}) for n in (385, 1025)]
    s1 = [a for a in range(4) for _ in range(2)]
    s2 = [4 + b for _ in range(4) for b in range(2)]
    off, m, _ = run(amc_ctx, xs + ys, s1, s2, cross_check)
    counts = np.diff(off.astype(np.int64)).tolist()
    if not cross_check:
        assert counts == [n for n in x_sizes for _ in range(2)]
        assert np.array_equal(m[:, 1], np.repeat([384, 1024] * 4, counts))
    else:  # identical X rows tie in the column direction: only the one-row image keeps its match
        assert counts == [1, 1] + [0] * 6
