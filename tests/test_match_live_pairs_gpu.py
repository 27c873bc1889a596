"""The cross-check chain behind the forward scan visits live pairs only (match_common.hip: live_flag_kernel,
compact_count_kernel, compact_scatter_kernel): a pair with no accept bit is classed dead by one sweep and the per-pair kernels index
compacted lists.  A pair wrongly classed dead loses its matches, a stale counter of a dead pair invents some - so every
case here is compared row for row with the CPU oracle, and the auto / mfma results with kernel="dot4" on the same input.

Dead pairs by construction: an image whose descriptors are non-zero only in dimensions 0..63 against one non-zero only
in 64..127 has every dot product 0.  Live pairs are noisy copies of shared prototypes.  Each case first asserts on the
oracle's output that the pairs meant dead have no match and the pairs meant live have some."""
import numpy as np
import pytest

import oracle_lib
from pycolmap_amd import _capi, synth  # noqa: F401

pytestmark = pytest.mark.gpu

SMALL = (97, 130, 161, 100)       # a 128-row segment or two, no multiple of 32
MIXED = (96, 300, 600, 257, 131)  # up to five segments; 96 and 257 sit at the edges of a tile and of a block


def upload(ctx, imgs):
    ctx.reserve_slots(len(imgs))
    for k, im in enumerate(imgs):
        ctx.upload_descriptors(k, im)


def prototypes(rng, n):
    p = rng.gamma(0.7, 1.0, size=(n, 64))
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def half_image(rng, n, low, proto=None):
    """n descriptors that are zero outside dimensions 0..63 (low) or 64..127: noisy copies of n of the prototypes,
    or i.i.d. ones."""
    x = np.zeros((n, 128))
    cols = slice(0, 64) if low else slice(64, 128)
    if proto is None:
        x[:, cols] = rng.gamma(0.7, 1.0, size=(n, 64))
    else:
        vis = rng.choice(len(proto), size=n, replace=False)
        x[:, cols] = proto[vis] + rng.normal(0, 0.05, size=(n, 64)) * proto[vis].mean()
    return synth.quantize_descriptors(x)


def make_pool(rng, sizes):
    """Slot 2k: a low-half image, slot 2k + 1: a high-half image, of sizes[k] rows; the images of a half share
    prototypes.  Two images of one half are a live pair, one of each a dead pair."""
    plo, phi = prototypes(rng, max(sizes) * 5 // 4), prototypes(rng, max(sizes) * 5 // 4)
    imgs = []
    for n in sizes:
        imgs += [half_image(rng, n, True, plo), half_image(rng, n, False, phi)]
    return imgs


def pairs_for(rng, nimg, live):
    """One pair per entry of `live` over a make_pool() of nimg images."""
    k = nimg // 2
    s1 = np.empty(len(live), np.uint32)
    s2 = np.empty(len(live), np.uint32)
    for p, lv in enumerate(live):
        a, b = rng.choice(k, size=2, replace=False)
        h1 = int(rng.integers(2))
        h2 = h1 if lv else 1 - h1
        s1[p], s2[p] = 2 * a + h1, 2 * b + h2
    return s1, s2


_oracle_cache = {}


def oracle(key, imgs, s1, s2, opts):
    """The reference of a case, computed once per (case, options) and shared by the kernels that are held against it."""
    if key not in _oracle_cache:
        woff, wm = oracle_lib.match_pairs(imgs, s1, s2, *opts)
        woff.setflags(write=False)
        wm.setflags(write=False)
        _oracle_cache[key] = (woff, wm)
    return _oracle_cache[key]


def check(ctx, key, imgs, s1, s2, live, opts=(0.8, 0.7, True), kernels=("dot4", "auto", "mfma")):
    live = np.asarray(live, dtype=bool)
    woff, wm = oracle(key, imgs, s1, s2, opts)
    cnt = np.diff(woff.astype(np.int64))
    assert (cnt[~live] == 0).all(), "a pair meant dead has matches in the oracle"
    assert (cnt[live] > 0).all(), "a pair meant live has no match in the oracle"
    out = None
    for kernel in kernels:
        off, m, st = ctx.match_pairs(s1, s2, *opts, kernel=kernel)
        np.testing.assert_array_equal(off, woff)
        np.testing.assert_array_equal(m, wm)
        if kernel == "mfma":
            nonempty = sum(1 for a, b in zip(s1, s2) if len(imgs[a]) and len(imgs[b]))
            assert st["pairs_mfma"] == nonempty and st["pairs_dot4"] == 0
        out = (off, m, st)
    return out


def test_all_dead(amc_ctx):
    rng = np.random.default_rng(1)
    imgs = make_pool(rng, MIXED)
    upload(amc_ctx, imgs)
    live = np.zeros(40, bool)
    s1, s2 = pairs_for(rng, len(imgs), live)
    off, m, _ = check(amc_ctx, "all_dead", imgs, s1, s2, live)
    assert len(m) == 0 and (off == off[0]).all()


# slots: 0, 3, 6 low images that share prototypes with slot 7 (low); 1, 2 low and 4, 5 high images of their own.
# The dead pairs stream image 1, 2, 4 or 5, so the live pair (7, 0) is the first of the streamed-image order, (7, 3) in
# its middle and (7, 6) its last - wherever it stands in the pair list.
@pytest.mark.parametrize("stream_pos", ["first", "middle", "last"])
@pytest.mark.parametrize("list_pos", ["first", "middle", "last"])
def test_one_live_pair(amc_ctx, list_pos, stream_pos):
    rng = np.random.default_rng(2)
    proto = prototypes(rng, 400)
    sizes = [300, 131, 257, 333, 96, 161, 290, 321]
    imgs = [half_image(rng, n, s not in (4, 5), proto if s in (0, 3, 6, 7) else None) for s, n in enumerate(sizes)]
    upload(amc_ctx, imgs)
    npairs = 37
    lo, hi = rng.choice([1, 2], size=npairs), rng.choice([4, 5], size=npairs)
    flip = rng.integers(2, size=npairs).astype(bool)
    s1 = np.where(flip, lo, hi).astype(np.uint32)
    s2 = np.where(flip, hi, lo).astype(np.uint32)
    at = {"first": 0, "middle": npairs // 2, "last": npairs - 1}[list_pos]
    s1[at], s2[at] = 7, {"first": 0, "middle": 3, "last": 6}[stream_pos]
    # (image 2 major, image 1 minor) is the forward scan's order: where the live pair falls in it
    order = np.lexsort((s1, s2))
    want = {"first": 0, "middle": None, "last": npairs - 1}[stream_pos]
    got = int(np.nonzero(order == at)[0][0])
    assert got == want if want is not None else 0 < got < npairs - 1
    live = np.zeros(npairs, bool)
    live[at] = True
    check(amc_ctx, ("one", list_pos, stream_pos), imgs, s1, s2, live)


def test_all_live(amc_ctx):
    rng = np.random.default_rng(3)
    imgs = make_pool(rng, MIXED)
    upload(amc_ctx, imgs)
    live = np.ones(33, bool)
    s1, s2 = pairs_for(rng, len(imgs), live)
    check(amc_ctx, "all_live", imgs, s1, s2, live)


@pytest.fixture(scope="module")
def small_pool():
    return make_pool(np.random.default_rng(4), SMALL)


# the wave and block edges of the flag kernel (a wave per pair, four to a block) and of the compaction (eight entries per
# thread, 2,048 per block): a thread, a wave, a block, one entry short of and beyond each, several blocks
@pytest.mark.parametrize("npairs", [1, 63, 64, 65, 255, 256, 257, 1025, 2047, 2048, 2049, 6145])
def test_compaction_edges(amc_ctx, small_pool, npairs):
    rng = np.random.default_rng(100 + npairs)
    upload(amc_ctx, small_pool)
    live = rng.random(npairs) < (0.3 if npairs < 2000 else 0.05)
    if npairs > 1:
        live[rng.integers(npairs)] = True
        live[-1] = not live[-2]
    if npairs > 2048:
        live[2047], live[2048] = False, True  # the last entry of a block dead, the first of the next live
    s1, s2 = pairs_for(rng, len(small_pool), live)
    check(amc_ctx, ("edges", npairs), small_pool, s1, s2, live, kernels=("dot4", "auto") if npairs < 2000 else ("auto",))


def test_dead_after_resolve(amc_ctx):
    """A pair that is live behind the scan and dead behind resolve_index(side 0): row 5 of image X has two near-equal
    best candidates in ONE 32-row tile of Y (rows 40 and 41).  The scan's second value leaves out the winning tile, so
    its accept test passes (second = 0); the exact second sits in that tile and fails the ratio test.  Zero matches."""
    rng = np.random.default_rng(6)
    proto = prototypes(rng, 500)
    x = half_image(rng, 200, True)
    y = half_image(rng, 300, False)
    d = half_image(rng, 1, True)[0]
    d2 = d.copy()
    k = int(np.argmax(d))
    d2[k] -= 1
    x[5] = d
    y[40], y[41] = d2, d
    # the construction, in numbers: the two largest products of row 5 are in tile 1 of Y, nothing outside it
    dots = x[5].astype(np.int64) @ y.astype(np.int64).T
    top = np.argsort(-dots)[:2]
    assert set(top.tolist()) == {40, 41} and 40 // 32 == 41 // 32
    outside = np.delete(dots, np.arange(32, 64)).max()
    lut = lambda v: np.arccos(np.float32(min(v / 262144.0, 1.0)))  # noqa: E731
    assert lut(dots[41]) <= 0.7 and lut(dots[41]) < 0.8 * lut(outside)      # accepted with the scan's second
    assert not lut(dots[41]) < 0.8 * lut(dots[40])                          # rejected with the exact one
    # around it: live and dead pairs, and the same pair with the sides exchanged (then the two rows are X rows)
    imgs = [x, y, half_image(rng, 257, True, proto), half_image(rng, 131, True, proto), half_image(rng, 96, False)]
    upload(amc_ctx, imgs)
    s1 = np.array([2, 0, 3, 4, 1, 0, 2], np.uint32)
    s2 = np.array([3, 1, 4, 2, 0, 1, 3], np.uint32)
    live = np.array([1, 0, 0, 0, 0, 0, 1], bool)
    off, m, _ = check(amc_ctx, "dead_after_resolve", imgs, s1, s2, live)
    assert off[2] == off[1] and off[6] == off[5]
    check(amc_ctx, "dead_after_resolve_alone", imgs, s1[1:2], s2[1:2], live[1:2])
    # without the cross check the exchanged pair matches (rows 40 and 41 of Y each have one candidate, row 5 of X)
    live[4] = True
    check(amc_ctx, "dead_after_resolve_nocross", imgs, s1, s2, live, opts=(0.8, 0.7, False))


def test_empty_images(amc_ctx):
    rng = np.random.default_rng(7)
    imgs = make_pool(rng, MIXED[:3]) + [np.zeros((0, 128), np.uint8)]
    upload(amc_ctx, imgs)
    e = len(imgs) - 1
    s1 = np.array([e, 0, 2, e, 0, 1, 4, e, 3], np.uint32)
    s2 = np.array([0, e, 4, e, 3, 5, e, 2, 5], np.uint32)
    live = np.array([0, 0, 1, 0, 0, 1, 0, 0, 1], bool)
    check(amc_ctx, "empty", imgs, s1, s2, live)
    # nothing but pairs with an empty image
    off, m, _ = amc_ctx.match_pairs(s1[[0, 1, 3]], s2[[0, 1, 3]])
    assert off.tolist() == [0] * 4 and len(m) == 0


def test_no_cross_check(amc_ctx):
    """cross_check=False: no candidate selection and no reverse scan; the chain is resolve + finalize."""
    rng = np.random.default_rng(8)
    imgs = make_pool(rng, MIXED)
    upload(amc_ctx, imgs)
    live = rng.random(70) < 0.3
    live[0], live[-1] = True, False
    s1, s2 = pairs_for(rng, len(imgs), live)
    check(amc_ctx, "nocross", imgs, s1, s2, live, opts=(0.8, 0.7, False))


@pytest.mark.parametrize("entries", [1, 2000, 6000])
def test_several_batches(amc_ctx, monkeypatch, entries):
    """AMC_MATCH_BATCH_ENTRIES cuts the call into batches of a few pairs that reuse one scratch set: runs of live
    pairs, runs of dead ones and mixed stretches, so that a batch of dead pairs follows a batch of live ones at the
    same positions (a stale cand_cnt / pair_cnt would show) and the other way round."""
    rng = np.random.default_rng(9)
    imgs = make_pool(rng, MIXED)
    upload(amc_ctx, imgs)
    live = np.concatenate([np.ones(9, bool), np.zeros(9, bool), rng.random(14) < 0.5, np.zeros(5, bool),
                           np.ones(3, bool), np.zeros(1, bool)])
    s1, s2 = pairs_for(rng, len(imgs), live)
    ref = amc_ctx.match_pairs(s1, s2)
    monkeypatch.setenv("AMC_MATCH_BATCH_ENTRIES", str(entries))
    off, m, st = check(amc_ctx, "batches", imgs, s1, s2, live)
    assert st["match_kernel_launches"] > ref[2]["match_kernel_launches"]  # it really ran as several batches
    check(amc_ctx, "batches_nocross", imgs, s1, s2, live, opts=(0.8, 0.7, False), kernels=("dot4", "auto"))


def test_reused_context(amc_ctx):
    """Two calls on one context with different pair lists, the second shorter than the first, and the first again."""
    rng = np.random.default_rng(10)
    imgs = make_pool(rng, MIXED)
    upload(amc_ctx, imgs)
    live_a = rng.random(90) < 0.5
    live_a[:4] = True
    a1, a2 = pairs_for(rng, len(imgs), live_a)
    live_b = np.zeros(17, bool)
    live_b[[3, 16]] = True
    b1, b2 = pairs_for(rng, len(imgs), live_b)
    for kernel in ("auto", "dot4"):
        check(amc_ctx, "reuse_a", imgs, a1, a2, live_a, kernels=(kernel,))
        check(amc_ctx, "reuse_b", imgs, b1, b2, live_b, kernels=(kernel,))
        check(amc_ctx, "reuse_a", imgs, a1, a2, live_a, kernels=(kernel,))
