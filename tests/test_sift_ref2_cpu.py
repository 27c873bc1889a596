"""The SIFT reference against an independent float64 restatement (tests/ref2/sift_ref2.py: scipy blurs, vectorised
extremum test, LAPACK solves, whole-window numpy sums, libm), without a GPU.

First the judge itself on known answers (the analytic Gaussian, a blob, a patch of one gradient direction), so that it
is not taken on trust; then tests/sift_ref/sift_ref.cc held to it on a fast sample of the image set of
tests/ref2/sift_compare.py, within the committed budget tests/ref2/sift_deviation_budget.json
(DESIGN.md section 10.10).  tests/test_sift_ref2_gpu.py holds Context.sift_extract to the same judge and limits."""
import math

import numpy as np
import pytest
from scipy.special import erf

import sift_images as si
import sift_ref_lib as ref
from ref2 import sift_compare as sc
from ref2 import sift_ref2 as r2

BUDGET = sc.budget()
CASES = sc.CASES


# ---- the judge on known answers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 5])
def test_scale_space_of_an_impulse_has_the_levels_variances(S):
    """Blurs add in quadrature, so level s of an impulse (no input blur) is a Gaussian of variance sigma_s^2.  The taps
    are a Gaussian sampled at the integers and cut at R = ceil(4 sigma) >= 4 sigma: the cut removes at most
    2 * 4 * phi(4) / erf(4 / sqrt 2) = 1.07e-3 of a step's variance (the tails' second moment), the endpoint term of the
    sampled sum (Euler-Maclaurin, (1 / 24) * |d/dx x^2 g| at 4 sigma, twice) is at most 56 phi(4) / (12 sigma^2) <
    0.8e-3 of it for the smallest step here (sigma 0.9), and aliasing, exp(-2 pi^2 sigma^2), is below 1e-5.  Variances
    of successive steps add, so every level is within 2e-3."""
    n = 161
    img = np.zeros((n, n))
    img[n // 2, n // 2] = 1.0
    (o, levels), = r2.scale_space(img, first_octave=0, num_octaves=1, S=S, input_sigma=0.0, scale=1.0)
    assert o == 0 and levels.shape == (S + 3, n, n)
    c = np.arange(n) - n // 2
    for i, L in enumerate(levels):
        want = (1.6 * 2.0 ** (1.0 / S) * 2.0 ** ((i - 1) / S)) ** 2
        assert L.sum() == pytest.approx(1.0, abs=1e-12)
        assert abs((L.sum(axis=0) * c).sum()) < 1e-12 and abs((L.sum(axis=1) * c).sum()) < 1e-12
        for axis in (0, 1):
            var = (L.sum(axis=axis) * c * c).sum()
            print(f"S {S} level {i - 1} axis {axis}: variance / sigma^2 - 1 = {var / want - 1:+.2e}")
            assert var == pytest.approx(want, rel=2e-3)
        assert L[n // 2, n // 2 + 3] == pytest.approx(L[n // 2 + 3, n // 2], rel=1e-12)      # isotropic


def test_first_level_accounts_for_the_input_blur():
    # an input that already has the nominal blur: a Gaussian of sigma 0.5 * 2 at octave -1 reaches level -1's sigma
    n = 81
    yy, xx = np.mgrid[0:n, 0:n] - n // 2
    g = np.exp(-(xx * xx + yy * yy) / (2 * 1.0 ** 2))
    levels = r2.octave_levels(g / g.sum(), 3, sigma_in=1.0)
    c = np.arange(n) - n // 2
    for i in (0, 1, 5):
        assert (levels[i].sum(axis=0) * c * c).sum() == pytest.approx(r2.level_sigma(i - 1, 3) ** 2, rel=2e-3)


def test_doubling_and_decimation_of_the_base():
    a = np.arange(12, dtype=np.float64).reshape(3, 4) ** 2
    up = r2.octave_base(a, -1)
    assert up.shape == (6, 8) and np.array_equal(up[::2, ::2], a)
    assert up[0, 1] == (a[0, 0] + a[0, 1]) / 2 and up[1, 0] == (a[0, 0] + a[1, 0]) / 2
    assert up[1, 1] == (a[0, 0] + a[0, 1] + a[1, 0] + a[1, 1]) / 4
    assert np.array_equal(up[:, 7], up[:, 6]) and np.array_equal(up[5], up[4])       # last column / row replicated
    b = np.arange(63, dtype=np.float64).reshape(7, 9)
    assert np.array_equal(r2.octave_base(b, 1), b[0:6:2, 0:8:2])
    assert np.array_equal(r2.octave_base(b, 2), b[0:1, 0:5:4])


def test_blobs_are_found_at_their_centre_and_scale():
    S = 3
    spots = [(40.3, 50.7, 3.0), (100.2, 80.4, 5.0), (60.0, 30.0, 2.0)]
    kp, desc = r2.extract(si.blobs(128, 160, spots), approx=False, upright=True)
    assert desc.shape == (len(kp), 128)
    for x, y, s in spots:
        d = np.hypot(kp[:, 0] - (x + 0.5), kp[:, 1] - (y + 0.5))
        k = int(np.argmin(d))
        assert d[k] < 0.1, (x, y, d[k])
        # a keypoint's sigma is its DoG level's lower sigma: the blob's scale lies half a level above it
        assert kp[k, 2] * 2 ** (1 / (2 * S)) == pytest.approx(s, rel=0.04)


def _ramp(direction, n=65, tau=5.0):
    """A level whose gradient points along `direction` (a unit vector) everywhere, with a Gaussian envelope of tau
    pixels across the centre line: 0.5 + 0.4 erf(u / (sqrt 2 tau)), u the coordinate along the direction."""
    yy, xx = np.mgrid[0:n, 0:n] - n // 2
    u = xx * direction[0] + yy * direction[1]
    return 0.5 + 0.4 * erf(u / (math.sqrt(2.0) * tau))


@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("phi", [0.05, 0.3, 1.0, 1.6, 2.5, 4.0, 5.5, 6.2])      # off the bin edges: there two bins tie
def test_one_gradient_direction_gives_one_orientation(phi, approx):
    """Central differences of f(u) point along (c + k c^3, s + k s^3), k = f''' / (6 f'), |k| <= 1 / (6 tau^2) where the
    window's weight lies: at most k / 4 = 1.7e-3 rad off phi.  The histogram of a single direction is a two-bin vote
    smoothed six times (close to a Gaussian of two bins); the parabola through its top three bins misplaces such a peak
    by less than a tenth of a bin (0.0175 rad).  The rational atan2 adds up to 0.008 rad."""
    n = 65
    field = r2.gradient_field(_ramp((math.cos(phi), math.sin(phi))), approx)
    angles = r2.orientations(field, n // 2 + 0.2, n // 2 - 0.3, 2.0, approx)
    assert len(angles) == 1
    err = abs((angles[0] - phi + math.pi) % (2 * math.pi) - math.pi)
    print(f"phi {phi:.3f} approx {approx}: {err:.2e} rad")
    assert err < 1.7e-3 + 0.0175 + (0.008 if approx else 0.0)
    hist = r2.orientation_histogram(field, n // 2, n // 2, 2.0, approx)
    assert int(np.argmax(hist)) == int(math.floor(36 * phi / (2 * math.pi)))      # bin i covers 10 i .. 10 i + 10 degrees


def _cells(hist):
    return np.asarray(hist).reshape(4, 4, 8)       # [by, bx, t]


def test_descriptor_energy_lies_in_one_orientation_bin():
    n = 65
    c = n // 2
    # gradient along +x, keypoint angle 0: gy is exactly 0, so every sample votes for t = 0 alone
    h = _cells(r2.raw_histogram(r2.gradient_field(_ramp((1.0, 0.0)), False), c, c, 2.0, 0.0, False))
    assert np.all(h[:, :, 0] > 0) and np.all(h[:, :, 1:] == 0)
    # the envelope lies across x: the inner columns carry more than the outer ones by more than the window alone
    # (which is all that separates the rows), and the pattern is symmetric in both
    cols, rows = h[:, :, 0].sum(axis=0), h[:, :, 0].sum(axis=1)
    assert cols[1] / cols[0] > 2.0 * rows[1] / rows[0] > 2.0
    assert np.allclose(h[:, :, 0], h[::-1, :, 0], rtol=1e-12) and np.allclose(h[:, :, 0], h[:, ::-1, 0], rtol=1e-12)
    # the rational atan2 is within 0.008 rad: at most 8 * 0.008 / 2 pi of the energy in the neighbouring bins
    ha = _cells(r2.raw_histogram(r2.gradient_field(_ramp((1.0, 0.0)), True), c, c, 2.0, 0.0, True))
    assert np.all(ha[:, :, 1:].sum(axis=2) <= 8 * 0.008 / (2 * math.pi) * ha.sum(axis=2))
    # the frame turns with the keypoint: gradient and keypoint both at 0.7 rad put the energy in t = 0 again (up to the
    # direction error of central differences, k / 4 with k = |u^2 / tau^4 - 1 / tau^2| / 6 < 0.06 inside the window:
    # 8 * 0.015 / 2 pi = 2 %), the envelope across the frame's x, and the point symmetry of the sampling grid holds
    th = 0.7
    hr = _cells(r2.raw_histogram(r2.gradient_field(_ramp((math.cos(th), math.sin(th))), False), c, c, 2.0, th, False))
    assert hr[:, :, 0].sum() > 0.98 * hr.sum()
    assert np.allclose(hr, hr[::-1, ::-1, :], rtol=1e-9)
    cols, rows = hr[:, :, 0].sum(axis=0), hr[:, :, 0].sum(axis=1)
    assert cols[1] / cols[0] > 2.0 * rows[1] / rows[0] > 2.0


def test_turning_the_patch_by_45_degrees_moves_one_orientation_bin():
    n = 65
    c = n // 2
    d = 1.0 / math.sqrt(2.0)
    h0 = _cells(r2.raw_histogram(r2.gradient_field(_ramp((1.0, 0.0)), False), c, c, 2.0, 0.0, False))
    # turned towards +y (down): the angle atan2(gy, gx) grows, VLFeat's order counts t upwards with it
    h1 = _cells(r2.raw_histogram(r2.gradient_field(_ramp((d, d)), False), c, c, 2.0, 0.0, False))
    assert np.all(h1[:, :, 1] > 0) and np.all(np.delete(h1, 1, axis=2) <= 1e-12 * h1[:, :, 1:2])
    # turned towards -y (up on the screen): one bin the other way, circularly
    h7 = _cells(r2.raw_histogram(r2.gradient_field(_ramp((d, -d)), False), c, c, 2.0, 0.0, False))
    assert np.all(h7[:, :, 7] > 0) and np.all(h7[:, :, :7] <= 1e-12 * h7[:, :, 7:8])
    # Lowe's layout reverses the orientations: bytes at index 0 of every cell, then at index 7 (down), index 1 (up)
    for h, t in ((h0, 0), (h1, 7), (h7, 1)):
        b = r2.descriptor_bytes(h.ravel()).reshape(16, 8)
        assert np.all(b[:, t] > 0) and b.sum() == b[:, t].sum()
    # and flips y: the keypoint's upper cells (by = 0) are the last 32 bytes
    top = h0.copy()
    top[2:] = 0
    b = r2.descriptor_bytes(top.ravel())
    assert b[:64].sum() == 0 and b[64:].sum() > 0


def test_bytes_of_a_histogram_agree_with_the_reference():
    rng = np.random.default_rng(11)
    for norm in (0, 1):
        for _ in range(20):
            h = rng.random(128) ** 4 * rng.choice([1e-3, 1.0, 50.0])
            got = ref.finish_descriptor(h.astype(np.float32), norm).astype(int)
            want = r2.descriptor_bytes(h.astype(np.float32).astype(np.float64), norm)
            assert np.abs(got - want).max() <= 1 and (got != want).mean() < 0.05


def test_the_restated_approximations_match_the_references():
    rng = np.random.default_rng(12)
    for x in np.concatenate([rng.random(200) * 25.0, [0.0, 24.99, 25.0, 25.5, 100.0]]):
        assert float(r2.expn_table(np.float32(x))) == pytest.approx(ref.expn(float(np.float32(x))), abs=2e-7)
    for y, x in rng.normal(size=(400, 2)):
        assert float(r2.atan2_rational(np.float32(y), np.float32(x))) == pytest.approx(
            ref.atan2(float(np.float32(y)), float(np.float32(x))), abs=2e-6)


def test_options_and_feature_cut():
    img = sc.image("textured")
    kp, desc = r2.extract(img, first_octave=0, max_num_features=0)
    ends = [len(r2.extract(img, first_octave=0, max_num_features=0, num_octaves=k)[0]) for k in (1, 2, 3)]
    assert ends == sorted(ends) and ends[-1] <= len(kp) and ends[0] > 0
    k2, d2 = r2.extract(img, first_octave=0, max_num_features=len(kp) - ends[0] + 5)
    assert np.array_equal(k2, np.concatenate([kp[:5], kp[ends[0]:]])) and np.array_equal(d2[:5], desc[:5])
    k1, _ = r2.extract(img, first_octave=0, max_num_orientations=1, max_num_features=0)
    assert 0 < len(k1) < len(kp)
    with pytest.raises(ValueError, match="unknown option"):
        r2.extract(img, no_such_option=1)


# ---- the committed budget -------------------------------------------------------------------------------------------
def test_committed_budget_meets_the_conditions():
    entries, limits = BUDGET["entries"], BUDGET["limits"]
    assert set(entries) == {f"{tag}/{mode}" for tag in CASES for mode in ("approx", "libm")}
    assert limits == sc.limits_of(entries)
    for tag, e in entries.items():
        name = tag.split("/")[0]
        upright = "/upright/" in tag
        assert name in sc.ORIENTED or upright          # blobs: upright only
        if tag.endswith("/approx"):
            assert e["unpaired"] == [0, 0] and e["byte_diff_max"] <= 1, tag
        elif upright:
            assert e["unpaired"] == [0, 0], tag
        else:
            assert max(e["unpaired_share"]) <= 0.02, tag
    assert sum(e["features"][0] for t, e in entries.items() if t.endswith("/approx")) > 1000
    # deviation S10 is live and small: with Lowe's rule after the fifth solve some features lose their partner
    s10 = BUDGET["s10"]
    assert set(s10) == set(CASES)
    lost, total = sum(max(e["unpaired"]) for e in s10.values()), sum(e["features"][0] for e in s10.values())
    assert 0 < lost <= 0.02 * total


@pytest.mark.parametrize("tag", sc.FAST)
def test_reference_within_the_budget(tag):
    name, opts = CASES[tag]
    sc.check_against_budget(tag, ref.extract(sc.image(name), **opts))


def test_compare_tool_reproduces_the_committed_entries():
    result = sc.evaluate(tags=sc.FAST[:3], verbose=False)
    got = result["entries"]
    assert len(got) == 6
    assert result["s10"] == {tag: BUDGET["s10"][tag] for tag in sc.FAST[:3]}
    for tag, e in got.items():
        want = BUDGET["entries"][tag]
        for key, v in e.items():
            if isinstance(v, float):
                assert v == pytest.approx(want[key], rel=1e-6, abs=1e-9), (tag, key)
            elif key == "unpaired_share":
                assert v == pytest.approx(want[key], rel=1e-9), (tag, key)
            else:
                assert v == want[key], (tag, key)
