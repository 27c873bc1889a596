"""Deterministic camera-model edge scenes for tests/test_camera_edges_cpu.py,
tests/test_camera_edges_gpu.py, tests/ref2/compare_camera_edges.py and tests/golden/make_camera_edges_ref_golden.py: small
flat scenes whose observations sit on, next to and far beyond the branch cuts of the three camera-model restatements and
of the fdlibm atan / sin / cos under them, and a census of which branch every observation takes.

Every scene has at most 6 images, 130 points and 600 observations.  Image 0 is the identity pose at the origin and a
point placed for a radius r is (r z, 0, z), (0, r z, z), (-r z, 0, z) or (0, -r z, z) with z a power of two, so that
u = X / Z, v = Y / Z and sqrt(u u + v v) are r exactly in doubles.  The other images are rotated about the optical axis
and moved by a translation with t_z > 0 only: every point in front of image 0 is in front of them as well.  The observed
pixels are the bundle adjustment reference's own projections at these start values plus Gaussian noise of half a pixel.
The geometry (poses, directions) is built with + - * / alone, so it does not depend on a numpy build's sin, cos, exp or
log; the radii of the log-uniform fillers go through np.ldexp and np.log2 of literal bounds, the noise through
rng.standard_normal, and the pixels through the compiled reference: a build that moved any of them would show up in the
fixture test, not silently.

The wide regimes run iterations (bundle adjustment, pose refinement) only for the models whose projection stays well
conditioned there, WIDE_ITERATION_MODELS: the two pinholes, the four fisheye models and FOV.  For the polynomial models
(SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV) the wide regimes are filter and projection only.  depth_tiny, behind,
rational_pole and strong_poly are filter and projection (strong_poly: lift) only for every model, and so are the two
fov_large_omega cases whose omega / 2 sits next to pi / 2 (round2, round3): with tan(omega / 2) beyond 1e6 every point
projects onto one circle and the Jacobian has lost its radial rank, as it has for a radius beyond 2^66."""
from __future__ import annotations

import functools
import zlib
from pathlib import Path

import numpy as np

import ba_cases

MODEL_NAMES = ba_cases.MODEL_NAMES
NUM_FOCAL = ba_cases.NUM_FOCAL
_M = {n: k for k, n in enumerate(MODEL_NAMES)}
DBL_EPSILON = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)

# the cuts of fdlibm's atan (s_atan.c), restated here from the specification and not read from the code under test
ATAN_TINY = 2.0 ** -29
ATAN_CUTS = (0.4375, 0.6875, 1.1875, 2.4375)
ATAN_HUGE = 2.0 ** 66
FOV_CUT = 1e-4

PINHOLES = (_M["SIMPLE_PINHOLE"], _M["PINHOLE"])
POLYNOMIAL = (_M["SIMPLE_RADIAL"], _M["RADIAL"], _M["OPENCV"], _M["FULL_OPENCV"])
FISHEYE = (_M["OPENCV_FISHEYE"], _M["SIMPLE_RADIAL_FISHEYE"], _M["RADIAL_FISHEYE"], _M["THIN_PRISM_FISHEYE"])
FOV = _M["FOV"]
WIDE_ITERATION_MODELS = PINHOLES + FISHEYE + (FOV,)
ATAN_MODELS = FISHEYE + (FOV,)
NO_ITERATION_REGIMES = ("depth_tiny", "behind", "rational_pole", "strong_poly")
NO_ITERATION_CASES = ("fov_large_omega/round2", "fov_large_omega/round3")

_prev = lambda x: float(np.nextafter(x, -np.inf))  # noqa: E731
_next = lambda x: float(np.nextafter(x, np.inf))  # noqa: E731


def around(x):
    return [_prev(x), float(x), _next(x)]


def _square_cut(cut=FOV_CUT):
    """(a, b): a the largest double whose rounded square is below cut, b the next double"""
    a = float(np.sqrt(cut))
    while a * a < cut:
        a = _next(a)
    while not a * a < cut:
        a = _prev(a)
    return a, _next(a)


SQ_LO, SQ_HI = _square_cut()


# ---- the census's selectors ---------------------------------------------------------------------------------------------
def atan_branch(x):
    """the branch of fdlibm's atan for the argument x, by its cuts"""
    a = abs(float(x))
    if a >= ATAN_HUGE:
        return "atan_huge"
    if a < ATAN_CUTS[0]:
        return "atan_tiny" if a < ATAN_TINY else "atan_poly"
    if a < ATAN_CUTS[1]:
        return "atan_id0"
    if a < ATAN_CUTS[2]:
        return "atan_id1"
    return "atan_id2" if a < ATAN_CUTS[3] else "atan_id3"


def _hi_exp(x):
    return int((np.float64(x).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7ff))


def rem_pio2_round(x):
    """0: |x| <= pi / 4 (no reduction); 1, 2, 3: the cancellation round of e_rem_pio2.c's medium-argument path at which
    the reduction of x ends (the second begins when the first difference lost more than 16 bits, the third more than 49)"""
    t = abs(float(x))
    if (np.float64(t).view(np.uint64) >> np.uint64(32)) <= np.uint64(0x3fe921fb):
        return 0
    invpio2, p1, p1t = 6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050650619224932e-11
    p2, p2t = 6.07710050630396597660e-11, 2.02226624879595063154e-21
    fn = float(int(t * invpio2 + 0.5))
    r = t - fn * p1
    y = r - fn * p1t
    j = _hi_exp(t)
    if j - _hi_exp(y) <= 16:
        return 1
    w = fn * p2
    r2 = r - w
    y = r2 - (fn * p2t - ((r - r2) - w))
    return 2 if j - _hi_exp(y) <= 49 else 3


def rational_denominator(extra, r2):
    """FULL_OPENCV's 1 + k4 r^2 + k5 r^4 + k6 r^6 in the projection's own order of operations"""
    r4 = r2 * r2
    r6 = r4 * r2
    return 1.0 + extra[5] * r2 + extra[6] * r4 + extra[7] * r6


def camera_frame(sc):
    """(N, 3) camera-frame points of the observations, Eigen's q * X + t in doubles"""
    q, t = sc["qvec"][sc["obs_image"]], sc["tvec"][sc["obs_image"]]
    X = sc["xyz"][obs_point(sc)]
    uv = 2.0 * np.cross(q[:, :3], X)
    return (X + q[:, 3:4] * uv) + np.cross(q[:, :3], uv) + t


def obs_point(sc):
    off = sc["track_offsets"].astype(np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.uint32)


def census(case):
    """name -> number of observations in the branch, by selectors applied to the case's inputs alone.  r is
    sqrt(u u + v v) of the start values; the atan branch is r's for the fisheye models (for FOV the argument comes out of
    the projection and is only observed, see observed_fov_atan)."""
    sc = case_scene(case) if isinstance(case, str) else case
    Xc = camera_frame(sc)
    with np.errstate(all="ignore"):
        u, v = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
        r2 = u * u + v * v
        r = np.sqrt(r2)
    out = {}

    def add(name, n=1):
        out[name] = out.get(name, 0) + int(n)
    cam = sc["image_cameras"][sc["obs_image"]]
    for k in range(len(r)):
        model = sc["models"][cam[k]]
        extra = sc["camera_params"][cam[k]][NUM_FOCAL[model] + 2:]
        add("depth_negative" if Xc[k, 2] < 0 else "depth_below_eps" if Xc[k, 2] < DBL_EPSILON else "depth_ok")
        add(atan_branch(r[k]))
        add("r_zero" if r[k] == 0.0 else "r_le_eps" if not r[k] > DBL_EPSILON else "r_gt_eps")
        for c in ATAN_CUTS + (DBL_EPSILON, ATAN_HUGE):
            for nm, val in zip(("prev", "at", "next"), around(c)):
                if r[k] == val:
                    add(f"r_{nm}_{c!r}")
        if model == FOV:
            om = float(extra[0])
            add("fov_omega_series" if om * om < FOV_CUT else "fov_radius_series" if r2[k] < FOV_CUT else "fov_atan")
            add(f"rem_pio2_round{rem_pio2_round(om / 2.0)}")
            for nm, val in (("lo", SQ_LO), ("hi", SQ_HI)):
                if r[k] == val:
                    add(f"fov_radius_{nm}")
        if model == _M["FULL_OPENCV"]:
            d = rational_denominator(extra, r2[k])
            add("denominator_negative" if d < 0 else "denominator_positive")
            if abs(d) < 1e-12:
                add("denominator_zero")
    return out


def observed_fov_atan(sc):
    """the atan branch of FOV's actual argument radius * 2 * tan(omega / 2) per observation (numpy's tan): observed"""
    Xc = camera_frame(sc)
    out = {}
    cam = sc["image_cameras"][sc["obs_image"]]
    for k in range(len(Xc)):
        model = sc["models"][cam[k]]
        if model != FOV:
            continue
        om = float(sc["camera_params"][cam[k]][4])
        with np.errstate(all="ignore"):
            r = float(np.hypot(Xc[k, 0] / Xc[k, 2], Xc[k, 1] / Xc[k, 2]))
            b = atan_branch(r * 2.0 * np.tan(om / 2.0))
        out[b] = out.get(b, 0) + 1
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------
_AXES = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
_DEPTHS = (1.0, 2.0, 0.5, 4.0)


def exact_points(rs, copies=2, depth=None):
    """`copies` points per radius, on different half-axes, with u, v and the radius exact"""
    pts = []
    for k, r in enumerate(r for r in rs for _ in range(copies)):
        ax, z = _AXES[k % 4], (_DEPTHS[(k // 4) % 4] if depth is None else depth)
        pts.append([ax[0] * r * z, ax[1] * r * z, z])
    return pts


def unit_vectors(rng, n):
    """(n, 2) directions over the whole circle by the rational parametrisation ((1 - s^2) / (1 + s^2), 2 s / (1 + s^2)):
    + - * / alone, so that the directions do not depend on a numpy build's sin and cos"""
    s = rng.uniform(-1.0, 1.0, n)
    flip = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
    return np.stack([flip * ((1.0 - s * s) / (1.0 + s * s)), flip * ((2.0 * s) / (1.0 + s * s))], axis=1)


def general_points(rng, n, lo, hi, log=False, sign=1.0):
    """n points with radii in [lo, hi): uniform, or with log a uniform mantissa times a uniform power of two"""
    if log:
        elo, ehi = int(np.ceil(np.log2(lo))), int(np.floor(np.log2(hi)))  # (of the literal bounds: exact for powers of two)
        r = np.clip(np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(elo - 1, ehi + 1, n)), lo, hi)
    else:
        r = rng.uniform(lo, hi, n)
    d = unit_vectors(rng, n)
    z = sign * np.array(_DEPTHS)[rng.integers(0, 4, n)]
    return np.stack([r * d[:, 0] * z, r * d[:, 1] * z, z], axis=1).tolist()


def build(name, model, params, points, nimg=5, noise=0.5):
    """The flat problem (filter_cases.problem's form) of one camera of `model` seen from nimg images; each point is seen
    by image 0 and two others."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    X = np.array(points, np.float64).reshape(-1, 3)
    q, t = [[0.0, 0.0, 0.0, 1.0]], [[0.0, 0.0, 0.0]]
    for i in range(1, nimg):
        h = rng.uniform(-0.25, 0.25)  # the tangent of a quarter of the angle: a rotation of up to 56 degrees about the axis
        n = 1.0 + h * h
        q.append([0.0, 0.0, (2.0 * h) / n, (1.0 - h * h) / n])
        t.append([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.05, 0.4)])
    q, t = np.array(q), np.array(t)
    prm = np.array(params, np.float64)
    off, oi, xy = [0], [], []
    for j in range(len(X)):
        for i in [0] + sorted(rng.choice(np.arange(1, nimg), 2, replace=False).tolist()):
            x, y = project_ref(model, prm, q[i], t[i], X[j])
            oi.append(i)
            xy.append(np.array([x, y]) + noise * rng.standard_normal(2))
        off.append(len(oi))
    sc = dict(name=name, model=int(model), models=[int(model)], camera_params=[prm], image_cameras=np.zeros(nimg, np.uint32),
              qvec=q, tvec=t, xyz=X, track_offsets=np.array(off, np.uint64), obs_image=np.array(oi, np.uint32),
              obs_xy=np.array(xy, np.float64).reshape(-1, 2))
    assert nimg <= 6 and len(X) <= 130 and len(oi) <= 600
    return sc


def project_ref(model, prm, q, t, X):
    """the bundle adjustment reference's projection: its residual against the pixel (0, 0)"""
    import ba_ref_lib
    _, r, _, _, _ = ba_ref_lib.observation(model, prm, q, t, X, [0.0, 0.0])
    return float(r[0]), float(r[1])


def _fov_params(omega):
    p = ba_cases.model_params(FOV).copy()
    p[4] = omega
    return p


def _pole_params():
    p = ba_cases.model_params(_M["FULL_OPENCV"]).copy()
    p[4:12] = [0.05, -0.02, 0.001, -0.001, 0.005, -0.5, 0.02, -0.001]
    return p


def pole_radius(extra):
    """the double r on the positive side of the denominator's zero nearest to it, found by bisection on r"""
    lo, hi = 1.0, 2.0
    assert rational_denominator(extra, lo * lo) > 0 > rational_denominator(extra, hi * hi)
    while _next(lo) < hi:
        mid = 0.5 * (lo + hi)
        if rational_denominator(extra, mid * mid) > 0:
            lo = mid
        else:
            hi = mid
    return lo, hi


STRONG = {_M["SIMPLE_RADIAL"]: [-0.3], _M["RADIAL"]: [-0.3, 0.02], _M["OPENCV"]: [-0.3, 0.02, 0.001, -0.001],
          _M["FULL_OPENCV"]: [-0.3, 0.02, 0.001, -0.001, 0.004, 0.01, -0.005, 0.002]}


def strong_params(model):
    p = ba_cases.model_params(model).copy()
    p[NUM_FOCAL[model] + 2:] = STRONG[model]
    return p


# the smallest normalised radius at which x + Distortion(x) = x0 has no solution for k1 = -0.3 alone is
# max r (1 - 0.3 r^2) = 0.7027 at r = 1.054 (the fold); the other coefficients move it by a few per cent
FOLD_INSIDE, FOLD_OUTSIDE = 0.6, 0.8


@functools.lru_cache(maxsize=None)
def strong_pixels(model):
    """(257, 2) pixels for the lift: the principal point twice, the four pixels one float32 step from it, 120 pixels
    inside the fold, 131 past it (as float32 values, which is what a feature's pixel is)."""
    rng = np.random.default_rng(4000 + model)
    p = strong_params(model)
    nf = NUM_FOCAL[model]
    f, cx, cy = p[0], np.float32(p[nf]), np.float32(p[nf + 1])
    px = [[cx, cy], [cx, cy], [np.nextafter(cx, np.float32(np.inf)), cy], [np.nextafter(cx, np.float32(-np.inf)), cy],
          [cx, np.nextafter(cy, np.float32(np.inf))], [cx, np.nextafter(cy, np.float32(-np.inf))]]
    for lo, hi, n in ((0.0, FOLD_INSIDE, 120), (FOLD_OUTSIDE, 1.6, 131)):
        r, d = rng.uniform(lo, hi, n), unit_vectors(rng, n)
        px += np.stack([cx + f * r * d[:, 0], cy + f * r * d[:, 1]], axis=1).astype(np.float32).tolist()
    out = np.array(px, np.float32).astype(np.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def strong_uv(model):
    """(257, 2) normalised points for the projection: the axis, and radii up to 1.6"""
    rng = np.random.default_rng(4100 + model)
    uv = rng.uniform(-1.15, 1.15, (257, 2))
    uv[0] = 0.0
    uv.setflags(write=False)
    return uv


def strong_census(model):
    px = strong_pixels(model)
    p = strong_params(model)
    nf = NUM_FOCAL[model]
    r = np.hypot((px[:, 0] - p[nf]) / p[0], (px[:, 1] - p[nf + 1]) / p[nf - 1])
    one = float(np.spacing(np.float32(max(p[nf], p[nf + 1]))))
    return dict(principal_point=int((r == 0).sum()), principal_point_neighbour=int(((r > 0) & (r * p[0] <= one)).sum()),
                inside_fold=int(((r * p[0] > one) & (r < FOLD_INSIDE + 1e-3)).sum()), past_fold=int((r > FOLD_OUTSIDE - 1e-3).sum()))


def _filler(rng, n=8):
    return general_points(rng, n, 0.02, 0.35)


def _specs():
    """name -> (regime, model, parameters, points, floors): floors name the census counts the regime is there for"""
    S = {}

    def put(regime, model, points, floors, params=None, tag=None):
        name = f"{regime}/{tag if tag is not None else MODEL_NAMES[model]}"
        S[name] = (regime, model, ba_cases.model_params(model) if params is None else params, points, floors)

    for m in range(11):
        rng = np.random.default_rng(7000 + m)
        fish = m in FISHEYE
        if m in ATAN_MODELS:
            rs = [r for c in ATAN_CUTS for r in around(c)]
            pts = exact_points(rs)
            for lo, hi, n in ((2e-9, 0.43, 8), (0.44, 0.68, 4), (0.69, 1.18, 4), (1.19, 2.43, 4), (2.44, 8.0, 6)):
                pts += general_points(rng, n, lo, hi)
            fl = {f"r_{nm}_{c!r}": 2 for c in ATAN_CUTS for nm in ("prev", "at", "next")}
            if fish:
                fl.update({b: 8 for b in ("atan_poly", "atan_id0", "atan_id1", "atan_id2", "atan_id3")})
            put("atan_cuts", m, pts, fl)
            put("axis_tiny", m, general_points(rng, 12, 2.0 ** -51, 2.0 ** -30, log=True) + _filler(rng, 6),
                {"atan_tiny": 8, "r_gt_eps": 8} if fish else {"atan_tiny": 8, "fov_radius_series": 8})
            rs = [_prev(ATAN_HUGE), ATAN_HUGE, _next(ATAN_HUGE), 2.0 ** 70, 2.0 ** 80, 2.0 ** 100]
            put("depth_tiny", m, exact_points(rs, depth=2.0 ** -50) + _filler(rng),
                {"atan_huge": 8, f"r_at_{ATAN_HUGE!r}": 2, f"r_prev_{ATAN_HUGE!r}": 2, f"r_next_{ATAN_HUGE!r}": 2})
        if fish:
            put("axis_eps", m, exact_points(around(DBL_EPSILON)) + _filler(rng, 10),
                {f"r_{nm}_{DBL_EPSILON!r}": 2 for nm in ("prev", "at", "next")})
        put("wide_50_68", m, exact_points([ATAN_CUTS[2], _prev(ATAN_CUTS[3])]) + general_points(rng, 20, 1.19, 2.43),
            {"atan_id2": 8})
        put("wide_68_89", m, exact_points([ATAN_CUTS[3], 60.0]) + general_points(rng, 20, 2.44, 59.9, log=True),
            {"atan_id3": 8})
        put("axis", m, [[0.0, 0.0, z] for z in _DEPTHS] + _filler(rng, 12) +
            (general_points(rng, 6, 1e-4, 0.0099) if m == FOV else []),
            dict({"r_zero": 2}, **({"fov_radius_series": 8} if m == FOV else {})))
        put("behind", m, general_points(rng, 12, 0.05, 1.0, sign=-1.0) + _filler(rng), {"depth_negative": 8, "depth_ok": 8})
    rng = np.random.default_rng(7100)
    mixed = general_points(rng, 16, 0.01, 1.5) + [[0.0, 0.0, 1.0], [0.0, 0.0, 2.0]]
    for tag, om in (("zero", 0.0), ("plus", 0.005), ("minus", -0.005), ("below_cut", SQ_LO), ("minus_below_cut", -SQ_LO)):
        put("fov_small_omega", FOV, mixed, {"fov_omega_series": 8}, _fov_params(om), tag)
    put("fov_small_omega", FOV, mixed + general_points(rng, 8, 1e-4, 0.0099), {"fov_atan": 8, "fov_radius_series": 8},
        _fov_params(SQ_HI), "above_cut")
    put("fov_small_radius", FOV, exact_points([SQ_LO, SQ_HI]) + general_points(rng, 8, 1e-4, 0.0099) +
        general_points(rng, 8, 0.0101, 0.5), {"fov_radius_series": 8, "fov_atan": 8, "fov_radius_lo": 2, "fov_radius_hi": 2},
        _fov_params(0.6))
    # omega / 2 = fl(pi / 2) loses 54 bits in the first difference and 53 in the second: round 3; pi / 2 + 2^-20 loses 21
    # and ends in round 2 (test_camera_edges_cpu.py asserts both by rem_pio2_round)
    for tag, om, rnd in (("1.6", 1.6, 1), ("2.0", 2.0, 1), ("3.0", 3.0, 1), ("round2", 2.0 * (float(np.pi / 2) + 2.0 ** -20), 2),
                         ("round3", float(np.pi), 3)):
        put("fov_large_omega", FOV, mixed, {f"rem_pio2_round{rnd}": 8}, _fov_params(om), tag)
    pole = _pole_params()
    lo, hi = pole_radius(pole[4:])
    put("rational_pole", _M["FULL_OPENCV"], exact_points([lo, hi], depth=1.0) + general_points(rng, 10, 0.05, lo - 0.01) +
        general_points(rng, 10, hi + 0.01, 2.5), {"denominator_positive": 8, "denominator_negative": 8, "denominator_zero": 2},
        pole)
    for m in POLYNOMIAL:
        put("strong_poly", m, general_points(rng, 24, 0.0, 1.0) + general_points(rng, 6, 1.1, 1.5) + [[0.0, 0.0, 1.0]], {},
            strong_params(m))
    return S


SPECS = _specs()
CASES = sorted(SPECS)
REGIMES = sorted({v[0] for v in SPECS.values()})
# the regimes whose defining values are exact doubles: the fixture keeps their squared errors as arrays
EXACT_REGIMES = ("atan_cuts", "axis", "axis_eps", "fov_small_radius")


def regime(name):
    return SPECS[name][0]


def floors(name):
    return dict(SPECS[name][4])


def iteration_safe(name):
    """bundle adjustment and pose refinement run their iterations on this case"""
    reg, model = SPECS[name][0], SPECS[name][1]
    if reg in NO_ITERATION_REGIMES or name in NO_ITERATION_CASES:
        return False
    return model in WIDE_ITERATION_MODELS if reg.startswith("wide_") else True


ITERATION_CASES = [n for n in CASES if iteration_safe(n)]


@functools.lru_cache(maxsize=None)
def case_scene(name):
    reg, model, prm, pts, _ = SPECS[name]
    sc = build(name, model, prm, pts)
    for v in sc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc


def filter_problem(sc):
    return (list(sc["models"]), sc["camera_params"], sc["image_cameras"], sc["qvec"], sc["tvec"], sc["xyz"],
            sc["track_offsets"], sc["obs_image"], sc["obs_xy"])


def ba_problem(sc):
    """Context.bundle_adjust's positional arguments: every camera parameter and every pose variable but the gauge (image
    0 and image 1's x translation, ba_cases.masks' pattern)"""
    nimg = len(sc["image_cameras"])
    cc = np.ones((1, 12), np.uint8)
    cc[0, :len(sc["camera_params"][0])] = 0
    pc = np.zeros((nimg, 6), np.uint8)
    pc[0, :] = 1
    pc[1, 3] = 1
    return (list(sc["models"]), sc["camera_params"], cc, sc["image_cameras"], sc["qvec"], sc["tvec"], pc, sc["xyz"],
            sc["obs_image"], obs_point(sc), sc["obs_xy"])


# trivial_6: in eight cases (FOV next to its series' cuts and at omega = 3, two axis_tiny cases) the first two steps are
# rejected, and a run without an accepted step hands the Jacobian to nothing the result shows but a PCG count; within six
# iterations every case accepts one (tests/test_camera_edges_cpu.py asserts it by the reference)
BA_OPTIONS = {"trivial_0": dict(max_num_iterations=0), "trivial_2": dict(max_num_iterations=2),
              "trivial_6": dict(max_num_iterations=6),
              "cauchy_2": dict(max_num_iterations=2, loss_function_type="CAUCHY", loss_function_scale=2.0)}
CAUCHY_CASE = "wide_50_68/OPENCV_FISHEYE"


def ba_options_of(name):
    """the keys of BA_OPTIONS the case runs under: the trivial loss with 0, 2 and 6 iterations, and CAUCHY for one case"""
    return ("trivial_0", "trivial_2", "trivial_6") + (("cauchy_2",) if name == CAUCHY_CASE else ())


def abspose_problem(sc, off_axis=True):
    """One refinement query per image over its observations: (offsets, models, params, points2D, points3D, qvec, tvec,
    mask).  off_axis: the start poses are the scene's turned by about three degrees and moved by 0.02; otherwise the
    scene's own, where the radii are the exact ones."""
    rng = np.random.default_rng(zlib.crc32(sc["name"].encode()) + 1)
    nimg = len(sc["image_cameras"])
    order = np.argsort(sc["obs_image"], kind="stable")
    counts = np.bincount(sc["obs_image"], minlength=nimg)
    q, t = sc["qvec"].copy(), sc["tvec"].copy()
    if off_axis:
        for i in range(nimg):
            q[i] = q[i] + rng.uniform(-0.015, 0.015, 4)
            q[i] = q[i] / np.sqrt(q[i][0] * q[i][0] + q[i][1] * q[i][1] + q[i][2] * q[i][2] + q[i][3] * q[i][3])
            t[i] = t[i] + rng.uniform(-0.02, 0.02, 3)
    return dict(offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64),
                camera_models=np.full(nimg, sc["model"], np.int32), camera_params=[sc["camera_params"][0]] * nimg,
                points2D=sc["obs_xy"][order], points3D=sc["xyz"][obs_point(sc)[order]], qvec=q, tvec=t,
                inlier_mask=np.ones(len(order), bool))


ABSPOSE_REFINEMENT = dict(gradient_tolerance=0.0, max_num_iterations=3)


def estimate_problem(model):
    """One estimation query on the strong_poly scene's image 0: its observations, and 12 more whose pixels lie past the
    fold (no point projects there; the device lift runs its hundred iterations on them)."""
    sc = case_scene(f"strong_poly/{MODEL_NAMES[model]}")
    sel = np.flatnonzero(sc["obs_image"] == 0)
    far = strong_pixels(model)[-12:]
    rng = np.random.default_rng(4200 + model)
    p2 = np.concatenate([sc["obs_xy"][sel], far])
    p3 = np.concatenate([sc["xyz"][obs_point(sc)[sel]], general_points(rng, 12, 0.1, 0.9)])
    return dict(offsets=np.array([0, len(p2)], np.uint64), camera_models=np.array([model], np.int32),
                camera_params=[sc["camera_params"][0]], points2D=p2, points3D=p3)


ESTIMATION = dict(min_num_trials=30, max_num_trials=500)

ABSPOSE_FIELDS = ("success", "qvec", "tvec", "num_inliers", "num_trials", "focal_factor", "inlier_mask")


# ---- references and digests ---------------------------------------------------------------------------------------------
def bits(a):
    """the doubles' bits, every NaN as the one canonical NaN (filter_cases.bits)"""
    a = np.array(a, dtype=np.float64).reshape(-1)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def filter_reference(name, errors_only=False):
    import filter_ref_lib
    return _freeze(filter_ref_lib.filter_points3d(*filter_problem(case_scene(name)), errors_only=errors_only))


@functools.lru_cache(maxsize=None)
def ba_reference(name, options):
    import ba_ref_lib
    return _freeze(ba_ref_lib.bundle_adjust(*ba_problem(case_scene(name)), options=BA_OPTIONS[options]))


@functools.lru_cache(maxsize=None)
def abspose_reference(name, off_axis):
    import abspose_ref_lib
    p = abspose_problem(case_scene(name), off_axis)
    return _freeze(abspose_ref_lib.refine(p["offsets"], p["camera_models"], p["camera_params"], p["points2D"], p["points3D"],
                                          p["qvec"], p["tvec"], p["inlier_mask"], refinement=ABSPOSE_REFINEMENT))


@functools.lru_cache(maxsize=None)
def estimate_reference(model):
    import abspose_ref_lib
    p = estimate_problem(model)
    return _freeze(abspose_ref_lib.estimate(p["offsets"], p["camera_models"], p["camera_params"], p["points2D"],
                                            p["points3D"], estimation=ESTIMATION))


@functools.lru_cache(maxsize=None)
def lift_reference(model):
    """(cam_from_img of strong_pixels, img_from_cam of strong_uv) by the oracle"""
    import oracle_lib
    cam = oracle_lib.make_camera(MODEL_NAMES[model], 1000, 800, strong_params(model))
    a, b = oracle_lib.cam_from_img(cam, strong_pixels(model)), oracle_lib.img_from_cam(cam, strong_uv(model))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _sha(parts):
    import hashlib
    h = hashlib.sha256()
    for p in parts:
        h.update(p)
    return h.hexdigest()


def filter_digest(res):
    import filter_cases
    return filter_cases.digest(res)


def ba_digest(res):
    return _sha([bits(res[k]).tobytes() for k in ba_cases.RESULT_ARRAYS] +
                [bits([res[k]]).tobytes() if isinstance(res[k], float) else str(res[k]).encode() for k in ba_cases.RESULT_STATS])


def abspose_digest(res):
    return _sha([bits(res[k]).tobytes() if res[k].dtype == np.float64 else np.ascontiguousarray(res[k]).astype(np.int64).tobytes()
                 for k in ABSPOSE_FIELDS])


def lift_digest(a):
    return _sha([bits(a).tobytes()])


GOLDEN = Path(__file__).resolve().parent / "golden" / "camera_edges_ref_v1.npz"


@functools.lru_cache(maxsize=None)
def golden():
    """(key -> digest, the fixture's arrays)"""
    z = np.load(GOLDEN)
    return dict(zip(z["digest_keys"].tolist(), z["digest_values"].tolist())), z
