"""Runs of items in the forward match scan (match_mfma.hip, "Runs"): a workgroup scans item t of up to R consecutive
streamed images one after the other, and where the run table marks an entry as holding the X segments of the entry
before it, the X rows stay in the registers and only the top-2 state starts over.  The mark is proved on the device
from the descriptors, the order of the table only makes it frequent.  These tests sit on what that adds: runs with
missing entries, state that must not survive from one streamed image to the next, the tile of the best across the
64-block flush, a pair list the order does not fit, batches that cut the blocks of groups, and the reverse scan, which
takes no runs.  Every case goes through amc_match_pairs and is compared with the oracle row for row, without tolerance.

AMC_SCAN_RUN forces the run length (2, 4, 8) or turns runs off (1); left alone, the host only takes runs for batches
large enough to fill the machine many times over (scan_run.h), which no test shape is."""
import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

OPTS = (1.0, 2.0)   # every row whose best beats its second is accepted: the result depends on every row's top two


def random_image(rng, n, high=64):
    """n rows of bytes below `high`: dot products stay below 512^2, so distances tell rows apart."""
    return rng.integers(0, high, size=(int(n), 128), dtype=np.uint8)


def run(ctx, imgs, s1, s2, cross_check, want_run):
    ctx.reserve_slots(len(imgs))
    for k, im in enumerate(imgs):
        ctx.upload_descriptors(k, im)
    s1 = np.asarray(s1, np.uint32)
    s2 = np.asarray(s2, np.uint32)
    off, m, st = ctx.match_pairs(s1, s2, *OPTS, cross_check, kernel="mfma")
    woff, wm = oracle_lib.match_pairs(imgs, s1, s2, *OPTS, cross_check)
    assert st["pairs_mfma"] == len(s1) and st["pairs_dot4"] == 0
    assert st["scan_run"] == want_run
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(m, wm)
    return woff, wm, st


# ---- 1. groups of unequal item counts ----------------------------------------------------------------------------------
UNEQUAL = [129, 260, 515, 700, 130]   # segments 2, 3, 5, 6: the streamed images 1..4 have 1, 2, 3 and 4 items


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("run_len", [2, 4])
def test_groups_of_unequal_item_counts(amc_ctx, monkeypatch, cross_check, run_len):
    """All pairs of five images.  Streamed image j holds the segments of the images below it, so every group has one
    item more than the one before: under R = 2 the run of item 1 of the groups (1, 2) and of item 3 of (3, 4) starts
    with a missing entry, under R = 4 the runs of items 1, 2 and 3 do, and every group's last item differs from the item
    at its place in the next group (a padded item against a full one, other rows: no mark) while the items before it
    are the same rows (marked)."""
    monkeypatch.setenv("AMC_SCAN_RUN", str(run_len))
    rng = np.random.default_rng(11)
    imgs = [random_image(rng, n) for n in UNEQUAL]
    i, j = np.triu_indices(len(imgs), k=1)
    woff, _, _ = run(amc_ctx, imgs, i, j, cross_check, run_len)
    if not cross_check:   # the inputs are what the test needs: nearly every row of every pair matched
        assert np.all(np.diff(woff.astype(np.int64)) >= 0.9 * np.array(UNEQUAL)[i])


# ---- 2. stale state ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("strong_first", [True, False])
def test_no_state_survives_into_the_next_streamed_image(amc_ctx, monkeypatch, cross_check, strong_first):
    """One X image against a Y image whose rows are X's own rows (every best is the row's squared norm) and a Y image
    of small bytes (every best far below that), consecutive entries of one run, in either order.  A best, a second or
    a tile kept from the strong image beats everything the weak one holds; kept from the weak one it is only found
    out by the second value."""
    monkeypatch.setenv("AMC_SCAN_RUN", "2")
    rng = np.random.default_rng(12)
    x = random_image(rng, 300)
    strong = x[rng.permutation(300)[:200]].copy()
    weak = random_image(rng, 200, high=16)
    ys = [strong, weak] if strong_first else [weak, strong]
    woff, wm, _ = run(amc_ctx, [x] + ys, [0, 0], [1, 2], cross_check, 2)
    counts = np.diff(woff.astype(np.int64))
    # both images match: the weak one by its own, lower values (one to one under the cross check: fewer)
    assert np.all(counts >= (1 if cross_check else 270))


# ---- 3. the tile of the best across the 64-block flush -----------------------------------------------------------------
@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("long_first", [True, False])
def test_best_tile_starts_over_behind_a_long_image(amc_ctx, monkeypatch, cross_check, long_first):
    """An 8,300-row Y image (65 blocks: the scan settles the tile of the best at block 64 and again at the end) whose
    rows from 8,192 on are X's rows, chained with a 200-row one.  The long image's bests lie in the second group of 64
    blocks; a tile kept into the short image points far past its end, and a tile not started over in the long one
    misses the carry across the flush."""
    monkeypatch.setenv("AMC_SCAN_RUN", "2")
    rng = np.random.default_rng(13)
    x = random_image(rng, 130)
    long_y = random_image(rng, 8300, high=16)
    long_y[8192:8192 + 100] = x[:100]
    short_y = random_image(rng, 200)
    ys = [long_y, short_y] if long_first else [short_y, long_y]
    woff, wm, _ = run(amc_ctx, [x] + ys, [0, 0], [1, 2], cross_check, 2)
    k = 0 if long_first else 1
    rows = wm[int(woff[k]):int(woff[k + 1])]
    assert np.sum(rows[:, 1] >= 8192) >= (90 if not cross_check else 50)


# ---- 4. a pair list the order does not fit -----------------------------------------------------------------------------
def window_pairs(n, w):
    s1 = [i for i in range(n) for j in range(i + 1, min(i + w, n - 1) + 1)]
    s2 = [j for i in range(n) for j in range(i + 1, min(i + w, n - 1) + 1)]
    return s1, s2


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("forced", [4, 0])
def test_windows_of_two_over_six_images(amc_ctx, monkeypatch, cross_check, forced):
    """Sequential windows: streamed image j holds the images j - 2 and j - 1, so consecutive groups share no prefix
    and nearly no entry is marked.  Forced to R = 4 the results are the same; left alone the host takes no runs."""
    monkeypatch.setenv("AMC_SCAN_RUN", str(forced))
    rng = np.random.default_rng(14)
    imgs = [random_image(rng, n) for n in (140, 260, 129, 300, 131, 257)]
    s1, s2 = window_pairs(6, 2)
    assert len(s1) == 9
    run(amc_ctx, imgs, s1, s2, cross_check, 4 if forced else 1)


# ---- 5. blocks of groups cut by a batch end ----------------------------------------------------------------------------
@pytest.mark.parametrize("cross_check", [False, True])
def test_batches_cut_the_blocks_of_groups(amc_ctx, monkeypatch, cross_check):
    """All 15 pairs of six images in batches of at most five pairs (300 rows are padded to 512): a batch holds the
    pairs of one or two images 1, its groups are cut where the list was carved, and every batch builds a run table of
    its own in the scratch the one before it used."""
    monkeypatch.setenv("AMC_SCAN_RUN", "4")
    monkeypatch.setenv("AMC_MATCH_BATCH_ENTRIES", str(5 * 512))
    rng = np.random.default_rng(15)
    imgs = [random_image(rng, 300) for _ in range(6)]
    i, j = np.triu_indices(6, k=1)
    _, _, st = run(amc_ctx, imgs, i, j, cross_check, 4)
    assert st["match_kernel_launches"] >= 3


# ---- 6. the launch's last block of groups, handed out item by item ------------------------------------------------------
@pytest.mark.parametrize("cross_check", [False, True])
def test_last_block_of_many_is_runs_of_one_item(amc_ctx, monkeypatch, cross_check):
    """All 171 pairs of 19 images under R = 2: nine blocks of two streamed images, and from eight blocks on the last
    one is written as one run per item (the launch ends on items, not on runs).  The blocks before it keep their runs;
    every item is still scanned exactly once."""
    monkeypatch.setenv("AMC_SCAN_RUN", "2")
    rng = np.random.default_rng(16)
    imgs = [random_image(rng, n) for n in rng.integers(100, 300, size=19)]
    i, j = np.triu_indices(19, k=1)
    run(amc_ctx, imgs, i, j, cross_check, 2)
