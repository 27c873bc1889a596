"""GPU parity tests: libamc.so (HIP kernels through the C ABI) vs the CPU oracle on identical
seeded inputs.  Bit-exact: integer match indices must be identical (BASELINE.json north_star).
Both kernels (int8-MFMA and u8 dot4) are exercised explicitly and via AUTO routing."""
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
from pycolmap_amd import _capi, synth

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden" / "match_golden_v1.npz"


def upload(ctx, imgs):
    ctx.reserve_slots(len(imgs))
    for k, im in enumerate(imgs):
        ctx.upload_descriptors(k, im)


def assert_same(ctx, imgs, s1, s2, kernel, opts=(0.8, 0.7, True), expect_kernel=None):
    off, m, st = ctx.match_pairs(s1, s2, *opts, kernel=kernel)
    woff, wm = oracle_lib.match_pairs(imgs, s1, s2, *opts)
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(m, wm)
    rows = np.array([len(i) for i in imgs], dtype=np.int64)
    assert st["num_distances"] == int((rows[s1] * rows[s2]).sum())
    if expect_kernel == "mfma":
        assert st["pairs_mfma"] > 0 and st["pairs_dot4"] == 0
    if expect_kernel == "dot4":
        assert st["pairs_dot4"] > 0 and st["pairs_mfma"] == 0
    return off, m, st


def test_acos_lut_is_the_host_libm_table(amc_ctx):
    np.testing.assert_array_equal(amc_ctx.acos_lut().view(np.uint32),
                                  oracle_lib.acos_lut().view(np.uint32))


@pytest.mark.parametrize("kernel", ["dot4", "mfma", "auto"])
def test_golden_fixture_all_settings(amc_ctx, kernel):
    g = np.load(GOLDEN)
    imgs = [g[f"desc_{k}"] for k in range(int(g["num_images"]))]
    upload(amc_ctx, imgs)
    for name in ("default", "nocross", "loose", "tight"):
        r, d, cc = g[f"{name}_opts"]
        off, m, _ = amc_ctx.match_pairs(g["slot1"], g["slot2"], float(r), float(d), bool(cc),
                                        kernel=kernel)
        np.testing.assert_array_equal(off, g[f"{name}_offsets"])
        np.testing.assert_array_equal(m, g[f"{name}_matches"])


@pytest.mark.parametrize("kernel", ["dot4", "mfma"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scene_pairs_ragged_sizes(amc_ctx, kernel, seed):
    rng = np.random.default_rng(seed)
    sizes = [512, 300, 777, 64, 1, 1025]
    imgs = []
    for n in sizes:
        imgs += synth.scene_images(rng, 1, n, num_landmarks=900, visible_frac=0.4)
    # same landmark prototypes across images need one generator call; add a coherent group too
    imgs += synth.scene_images(rng, 3, 640, num_landmarks=1000, visible_frac=0.5)
    s1, s2 = synth.exhaustive_pairs(len(imgs))
    upload(amc_ctx, imgs)
    off, m, _ = assert_same(amc_ctx, imgs, s1, s2, kernel, expect_kernel=kernel)
    assert off[-1] > 100  # the coherent group matches
    # reversed pair order (image 2 has fewer/more rows than image 1)
    assert_same(amc_ctx, imgs, s2, s1, kernel, expect_kernel=kernel)


@pytest.mark.parametrize("kernel", ["dot4", "mfma"])
@pytest.mark.parametrize("opts", [(0.8, 0.7, False), (0.95, 1.3, True), (1.0, 2.0, True),
                                  (0.5, 0.4, True)])
def test_option_variants(amc_ctx, kernel, opts):
    rng = np.random.default_rng(11)
    imgs = synth.scene_images(rng, 4, 600, num_landmarks=1000, visible_frac=0.5)
    s1, s2 = synth.exhaustive_pairs(4)
    upload(amc_ctx, imgs)
    assert_same(amc_ctx, imgs, s1, s2, kernel, opts, expect_kernel=kernel)


@pytest.mark.parametrize("kernel", ["dot4", "mfma"])
def test_adversarial_ties_zeros_duplicates(amc_ctx, kernel):
    rng = np.random.default_rng(5)
    a = synth.random_descriptors(rng, 300)
    b = a[rng.permutation(300)].copy()
    b[10] = b[11]            # duplicated column: tie for best of one row
    b[20] = 0                # zero column
    a[30] = 0                # zero row
    a[40] = a[41]            # duplicated rows: tie in the column direction
    c = np.concatenate([a[:100], a[:100]])   # every row duplicated
    imgs = [a, b, c, np.zeros((0, 128), np.uint8), a[:1].copy()]
    s1 = np.array([0, 1, 0, 2, 2, 0, 3, 4, 4, 0], np.uint32)
    s2 = np.array([1, 0, 2, 0, 2, 3, 0, 0, 4, 0], np.uint32)
    upload(amc_ctx, imgs)
    for opts in [(0.8, 0.7, True), (0.99, 3.0, True), (0.99, 3.0, False)]:
        assert_same(amc_ctx, imgs, s1, s2, kernel, opts)


def test_unnormalised_and_saturated_descriptors(amc_ctx):
    """Raw random bytes and saturated rows (dot up to 128*255^2) are exact on BOTH kernels: the
    mfma scan works on full-range int32 values, no norm precondition."""
    rng = np.random.default_rng(6)
    a = rng.integers(0, 256, size=(200, 128), dtype=np.uint8)
    b = rng.integers(0, 256, size=(150, 128), dtype=np.uint8)
    sat = np.full((70, 128), 255, np.uint8)
    mixed = np.concatenate([sat[:5], a[:40], np.zeros((3, 128), np.uint8), b[:30]])
    big = rng.integers(0, 256, size=(4096, 128), dtype=np.uint8)
    imgs = [a, b, sat, mixed, big]
    s1, s2 = synth.exhaustive_pairs(len(imgs))
    upload(amc_ctx, imgs)
    for kernel in ("mfma", "dot4"):
        for opts in [(0.8, 0.7, True), (0.99, 3.0, True), (0.99, 3.0, False)]:
            assert_same(amc_ctx, imgs, s1, s2, kernel, opts, expect_kernel=kernel)
            assert_same(amc_ctx, imgs, s2, s1, kernel, opts, expect_kernel=kernel)


def test_max_ratio_above_one_ties_pass_the_ratio_test(amc_ctx):
    """max_ratio > 1 lets tied bests through the ratio test: the lowest index among the ties
    must be reported in both directions (exact index cross check on both kernels)."""
    rng = np.random.default_rng(7)
    a = synth.random_descriptors(rng, 128)
    b = np.concatenate([a, a])  # every column duplicated -> ties everywhere
    imgs = [a, b]
    upload(amc_ctx, imgs)
    s1 = np.array([0, 1], np.uint32); s2 = np.array([1, 0], np.uint32)
    for kernel in ("mfma", "dot4"):
        assert_same(amc_ctx, imgs, s1, s2, kernel, (1.5, 3.0, True), expect_kernel=kernel)
        assert_same(amc_ctx, imgs, s1, s2, kernel, (1.5, 3.0, False), expect_kernel=kernel)


@pytest.mark.parametrize("kernel", ["dot4", "mfma"])
def test_without_cross_check_more_matches_than_columns(amc_ctx, kernel):
    rng = np.random.default_rng(12)
    b = synth.random_descriptors(rng, 40)
    a = np.concatenate([b] * 5)[rng.permutation(200)]
    imgs = [a, b]
    upload(amc_ctx, imgs)
    off, m, _ = assert_same(amc_ctx, imgs, np.array([0], np.uint32), np.array([1], np.uint32),
                            kernel, (0.99, 3.0, False))
    assert off[-1] == 200


def test_invalid_arguments_raise(amc_ctx):
    amc_ctx.reserve_slots(2)
    amc_ctx.upload_descriptors(0, np.zeros((4, 128), np.uint8))
    with pytest.raises(_capi.AmcError) as e:      # slot 1 never uploaded
        amc_ctx.match_pairs([0], [1])
    assert e.value.code == _capi.AMC_E_STATE
    with pytest.raises(_capi.AmcError) as e:      # slot out of range
        amc_ctx.match_pairs([0], [7])
    assert e.value.code == _capi.AMC_E_INVALID
    with pytest.raises(_capi.AmcError):
        amc_ctx.upload_descriptors(5, np.zeros((4, 128), np.uint8))
    off, m, _ = amc_ctx.match_pairs([], [])
    assert off.tolist() == [0] and m.shape == (0, 2)


def test_full_size_properties_4096(amc_ctx):
    """BASELINE config-2 image size (4096 descriptors): too slow for the scalar oracle on every
    pair, so (a) one pair against the oracle, (b) the two independent kernels against each other
    on all pairs, (c) transpose symmetry of the cross-checked match set, (d) self-match identity."""
    rng = np.random.default_rng(8)
    imgs = synth.scene_images(rng, 6, 4096, num_landmarks=8000, visible_frac=0.35)
    s1, s2 = synth.exhaustive_pairs(6)
    upload(amc_ctx, imgs)
    off_m, m_m, st_m = amc_ctx.match_pairs(s1, s2, kernel="mfma")
    off_d, m_d, st_d = amc_ctx.match_pairs(s1, s2, kernel="dot4")
    assert st_m["pairs_mfma"] == len(s1) and st_d["pairs_dot4"] == len(s1)
    np.testing.assert_array_equal(off_m, off_d)
    np.testing.assert_array_equal(m_m, m_d)
    assert off_m[-1] > 1000
    # (a) oracle on the first pair
    np.testing.assert_array_equal(m_m[off_m[0]:off_m[1]], oracle_lib.match(imgs[0], imgs[1]))
    # (c) transpose symmetry
    off_t, m_t, _ = amc_ctx.match_pairs(s2, s1, kernel="mfma")
    for p in range(len(s1)):
        a = {(int(i), int(j)) for i, j in m_m[off_m[p]:off_m[p + 1]]}
        b = {(int(j), int(i)) for i, j in m_t[off_t[p]:off_t[p + 1]]}
        assert a == b
    # (d) self match: every accepted row maps to itself
    off_s, m_s, _ = amc_ctx.match_pairs([0], [0], kernel="mfma")
    assert len(m_s) > 0 and np.all(m_s[:, 0] == m_s[:, 1])


def test_8192_rows(amc_ctx):
    rng = np.random.default_rng(9)
    imgs = synth.scene_images(rng, 2, 8192, num_landmarks=16000, visible_frac=0.4)
    upload(amc_ctx, imgs)
    off, m, st = amc_ctx.match_pairs([0], [1], kernel="auto")
    assert st["pairs_mfma"] == 1
    off_d, m_d, _ = amc_ctx.match_pairs([0], [1], kernel="dot4")
    np.testing.assert_array_equal(m, m_d)
    assert len(m) > 500
    # BASELINE configs[3]'s image size against the oracle itself (the vectorised variant where the host has AVX-512
    # VNNI - checked against the literal one in tests/test_oracle_match.py - else the literal one: ~10 s)
    want = oracle_lib.match_vnni(imgs[0], imgs[1]) if oracle_lib.vnni_available() else oracle_lib.match(imgs[0], imgs[1])
    np.testing.assert_array_equal(m, want)


def test_more_than_8192_rows_matches_oracle(amc_ctx):
    """Images larger than BASELINE's biggest config (8192): still the mfma kernel, both kernels against the oracle.
    Ragged, non-multiple-of-32 sizes."""
    rng = np.random.default_rng(19)
    big = synth.scene_images(rng, 2, 9001, num_landmarks=14000, visible_frac=0.4)
    small = synth.scene_images(rng, 1, 777, num_landmarks=14000, visible_frac=0.4)[0]
    imgs = [big[0], big[1][:8999], small]
    upload(amc_ctx, imgs)
    s1, s2 = [0, 2, 0], [1, 1, 2]
    off, m, st = amc_ctx.match_pairs(s1, s2, kernel="auto")
    assert st["pairs_mfma"] == 3
    off_d, m_d, st_d = amc_ctx.match_pairs(s1, s2, kernel="dot4")
    np.testing.assert_array_equal(off, off_d)
    np.testing.assert_array_equal(m, m_d)
    for p, (a, b) in enumerate(zip(s1, s2)):
        np.testing.assert_array_equal(m[off[p]:off[p + 1]], oracle_lib.match(imgs[a], imgs[b]))
    off_n, m_n, st_n = amc_ctx.match_pairs(s1, s2, kernel="auto", cross_check=False)
    assert st_n["pairs_mfma"] == 3
    for p, (a, b) in enumerate(zip(s1, s2)):
        np.testing.assert_array_equal(m_n[off_n[p]:off_n[p + 1]], oracle_lib.match(imgs[a], imgs[b], cross_check=False))


def test_40000_rows_stay_on_the_mfma_kernel(amc_ctx):
    """Cross-checked images beyond 32,768 descriptors (round 3's limit: the candidate bitmap of select_candidates was 4 KiB
    of static LDS) keep the mfma kernel: 40,000 x 39,871 rows, ragged against a small image, both directions; the per-row
    resolve kernel takes over from the tile-grouped one above 65,536 rows, not here.  Against the dot4 kernel and, where the
    host has AVX-512 VNNI (the literal oracle needs minutes at this size), the oracle itself."""
    rng = np.random.default_rng(41)
    big = synth.scene_images(rng, 2, 40000, num_landmarks=60000, visible_frac=0.4)
    small = synth.scene_images(rng, 1, 1000, num_landmarks=60000, visible_frac=0.4)[0]
    imgs = [big[0], big[1][:39871], small]
    upload(amc_ctx, imgs)
    s1, s2 = [0, 2, 0], [1, 1, 2]
    off, m, st = amc_ctx.match_pairs(s1, s2, kernel="auto")
    assert st["pairs_mfma"] == 3 and st["pairs_dot4"] == 0
    off_d, m_d, _ = amc_ctx.match_pairs(s1, s2, kernel="dot4")
    np.testing.assert_array_equal(off, off_d)
    np.testing.assert_array_equal(m, m_d)
    assert off[1] - off[0] > 2000
    if oracle_lib.vnni_available():
        for p, (a, b) in enumerate(zip(s1, s2)):
            np.testing.assert_array_equal(m[off[p]:off[p + 1]], oracle_lib.match_vnni(imgs[a], imgs[b]))
    else:
        np.testing.assert_array_equal(m[off[1]:off[2]], oracle_lib.match(imgs[2], imgs[1]))


@pytest.mark.parametrize("kernel", ["auto", "dot4"])
@pytest.mark.parametrize("entries", [1, 1500, 4000])
def test_many_batches_pipeline(amc_ctx, monkeypatch, kernel, entries):
    """A call is cut into batches by device-scratch budget and the batches are software-pipelined
    (batch k+1 prepared and enqueued while batch k's matches are copied out).  AMC_MATCH_BATCH_ENTRIES
    shrinks the budget so that a small input runs as many ragged batches - one pair each for 1 - and the
    result must not depend on where the cuts fall; empty images and empty results included."""
    rng = np.random.default_rng(11)
    imgs = synth.scene_images(rng, 6, 400, num_landmarks=700, visible_frac=0.5)
    imgs += [synth.random_descriptors(rng, 130), np.zeros((0, 128), np.uint8), synth.random_descriptors(rng, 600)]
    upload(amc_ctx, imgs)
    s1, s2 = synth.exhaustive_pairs(len(imgs))
    ref = amc_ctx.match_pairs(s1, s2, kernel=kernel)
    monkeypatch.setenv("AMC_MATCH_BATCH_ENTRIES", str(entries))
    for opts in ((0.8, 0.7, True), (0.9, 1.0, False)):
        off, m, st = assert_same(amc_ctx, imgs, s1, s2, kernel, opts)
    off, m, st = amc_ctx.match_pairs(s1, s2, kernel=kernel)
    np.testing.assert_array_equal(off, ref[0])
    np.testing.assert_array_equal(m, ref[1])
    assert st["match_kernel_launches"] > ref[2]["match_kernel_launches"]      # it really ran as several batches
    # reversed pair order, and only pairs with an empty image: batches with no work at all
    off, m, _ = assert_same(amc_ctx, imgs, s2[::-1].copy(), s1[::-1].copy(), kernel)
    e = np.full(5, 7, dtype=np.uint32)
    off, m, _ = amc_ctx.match_pairs(e, np.arange(5, dtype=np.uint32), kernel=kernel)
    assert off.tolist() == [0] * 6 and len(m) == 0
    # the three ways a batch's matches reach the host: riding in the next batch's scan (forced for these small
    # batches), the small copy kernel on the copy stream, the runtime's copy
    for env in ({"AMC_D2H_FUSE_MIN_BYTES": "8"}, {"AMC_D2H": "stream"}, {"AMC_D2H": "memcpy"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        off, m, st = amc_ctx.match_pairs(s1, s2, kernel=kernel)
        np.testing.assert_array_equal(off, ref[0])
        np.testing.assert_array_equal(m, ref[1])
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("cross_check", [True, False])
def test_dense_overlap_and_both_resolve_kernels(amc_ctx, monkeypatch, cross_check):
    """Every pair overlapping (a third of the rows accepted, many accepted rows per Y tile): the tile-grouped
    resolve_index kernel on the matrix core (the default), on v_dot4 (AMC_RESOLVE_DOT4=1), the per-row one
    (AMC_RESOLVE_UNGROUPED=1) and the oracle agree; ragged sizes, an image
    above 4096 rows (two chunks of the grouped kernel's row list), the zero-copy result view."""
    rng = np.random.default_rng(42)
    sizes = [700, 1300, 4096, 5000, 64, 1]
    L = 9000
    proto = rng.gamma(0.7, 1.0, size=(L, 128))
    proto /= np.linalg.norm(proto, axis=1, keepdims=True)
    imgs = []
    for n in sizes:
        vis = rng.choice(L, size=n, replace=False)
        imgs.append(synth.quantize_descriptors(proto[vis] + rng.normal(0, 0.05, size=(n, 128)) * proto[vis].mean()))
    upload(amc_ctx, imgs)
    s1 = np.array([0, 1, 2, 3, 2, 3, 4, 5, 0, 3], dtype=np.uint32)
    s2 = np.array([1, 2, 3, 2, 0, 0, 2, 3, 4, 3], dtype=np.uint32)
    opts = (0.8, 0.7, cross_check)
    off, m, st = assert_same(amc_ctx, imgs, s1, s2, "mfma", opts, expect_kernel="mfma")
    assert int(off[3] - off[2]) > 300                       # 4096 x 5000 with hundreds of mutual matches
    voff, vm, _ = amc_ctx.match_pairs(s1, s2, *opts, kernel="mfma", copy=False)
    np.testing.assert_array_equal(np.asarray(voff), off)
    np.testing.assert_array_equal(np.asarray(vm), m)
    del voff, vm
    # the tile-grouped form on v_dot4 (round 2; the default above is its matrix-core form), then the per-row form
    monkeypatch.setenv("AMC_RESOLVE_DOT4", "1")
    off3, m3, _ = amc_ctx.match_pairs(s1, s2, *opts, kernel="mfma")
    np.testing.assert_array_equal(off3, off)
    np.testing.assert_array_equal(m3, m)
    monkeypatch.delenv("AMC_RESOLVE_DOT4")
    monkeypatch.setenv("AMC_RESOLVE_UNGROUPED", "1")
    off2, m2, _ = amc_ctx.match_pairs(s1, s2, *opts, kernel="mfma")
    np.testing.assert_array_equal(off2, off)
    np.testing.assert_array_equal(m2, m)


def test_trim_releases_scratch_and_the_context_keeps_working(amc_ctx):
    """amc_ctx_trim: per-call scratch, staging and idle result buffers go, uploaded images stay - the next call
    re-allocates what it needs and returns the same result."""
    rng = np.random.default_rng(23)
    imgs = synth.scene_images(rng, 4, 500, num_landmarks=700, visible_frac=0.5)
    upload(amc_ctx, imgs)
    s1, s2 = synth.exhaustive_pairs(len(imgs))
    off, m, _ = amc_ctx.match_pairs(s1, s2)
    amc_ctx.trim()
    amc_ctx.trim()
    off2, m2, _ = amc_ctx.match_pairs(s1, s2)
    np.testing.assert_array_equal(off, off2)
    np.testing.assert_array_equal(m, m2)
    woff, wm = oracle_lib.match_pairs(imgs, s1, s2)
    np.testing.assert_array_equal(m2, wm)


def test_slots_uploaded_again_and_again(amc_ctx):
    """The slots' device memory comes from a slab allocator (amc_ctx.h, SlotArena: best fit, blocks split on
    allocation and merged with their free neighbours when freed, idle slabs given back at amc_ctx_trim): slots
    re-uploaded with other sizes keep holding what was uploaded last, and the keypoint / grid buffers beside them as
    well; a trim between two rounds changes nothing."""
    rng = np.random.default_rng(31)
    n = 6
    amc_ctx.reserve_slots(n)
    pool = synth.scene_images(rng, n, 2600, num_landmarks=3200, visible_frac=0.6)   # rows are shuffled: a prefix is a random subset
    imgs = [None] * n
    for round_ in range(8):
        for k in rng.permutation(n)[: int(rng.integers(2, n + 1))] if round_ else range(n):
            rows = int(rng.choice([0, 1, 37, 300, 301, 650, 1200, 2600])) if round_ else 400
            imgs[k] = np.ascontiguousarray(pool[int(rng.integers(n))][:rows])
            amc_ctx.upload_descriptors(int(k), imgs[k])
            amc_ctx.upload_keypoints(int(k), rng.uniform(0, 1000, (rows, 2)).astype(np.float32))
        s1, s2 = synth.exhaustive_pairs(n)
        assert_same(amc_ctx, imgs, s1, s2, "auto")
        if round_ in (3, 6):
            amc_ctx.trim()                                     # scratch and idle slabs go; the uploaded images stay
            assert_same(amc_ctx, imgs, s1, s2, "auto")
    amc_ctx.reserve_slots(2)                                   # everything released; the context starts over
    small = [synth.random_descriptors(rng, 200), synth.random_descriptors(rng, 100)]
    upload(amc_ctx, small)
    assert_same(amc_ctx, small, np.array([0], np.uint32), np.array([1], np.uint32), "auto")
