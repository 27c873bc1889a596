"""Cases of the stereo fusion tests: name -> (the arguments of _capi.fusion_inputs, the options of
amc_fuse_depth_maps).  Two kinds of scene: a stack of cameras at one pose with dyadic intrinsics and depths, where every
number comes out exactly and a cluster is one pixel per image, and the rendered planes of patchmatch_cases with their
exact maps.  EXPECT says what the reference's trace must show for a case, so that a case reaches what its name says."""
from __future__ import annotations

import numpy as np

import patchmatch_cases as pc

MAX_CLUSTER = 256
ALL = dict(min_num_pixels=1)  # every cluster gives a point


def stack(n, w=2, h=2, depth=2.0, focal=4.0, neighbours=None, colors=None):
    """n cameras at the world's origin, fx = fy = focal, the principal point in the middle: images (grey ramps unless
    `colors` gives a value per image), K, R, t, depth maps of `depth`, normal maps of (0, 0, -1) and, unless given, every
    later image as a neighbour (the first 64)"""
    images = []
    for i in range(n):
        a = np.zeros((h, w, 3), np.uint8)
        a[..., 0] = (np.arange(w)[None, :] * 7 + np.arange(h)[:, None] * 13 + 5 * i) % 256
        a[..., 1] = (40 + 3 * i) % 256
        a[..., 2] = (200 - i) % 256
        if colors is not None:
            a[...] = np.asarray(colors[i], np.uint8)
        images.append(a)
    K = np.array([[focal, focal, w / 2.0, h / 2.0]] * n)
    R = np.array([np.eye(3)] * n)
    t = np.zeros((n, 3))
    dm = [np.full((h, w), depth, np.float32) for _ in range(n)]
    nm = [np.stack([np.zeros((h, w)), np.zeros((h, w)), -np.ones((h, w))]).astype(np.float32) for _ in range(n)]
    if neighbours is None:
        neighbours = [[j for j in range(n) if j != i][:64] for i in range(n)]
    return [images, K, R, t, dm, nm, [list(x) for x in neighbours]]


def rendered(kind="slanted", cams=3, w=12, h=9):
    """A scene of patchmatch_cases with its exact maps in float32; every image names all the others"""
    sc = pc.scene(kind, cams, w, h)
    images = [np.stack([a, 255 - a, (a.astype(np.int32) * 3 % 256).astype(np.uint8)], axis=-1) for a in sc["images"]]
    dm = [np.asarray(d, np.float32) for d in sc["depth"]]
    nm = [np.asarray(x, np.float32) for x in sc["normal"]]
    return [images, sc["K"].copy(), sc["R"].copy(), sc["t"].copy(), dm, nm, [[j for j in range(cams) if j != i] for i in range(cams)]]


def _copy(args):
    images, K, R, t, dm, nm, nb = args
    return [[a.copy() for a in images], K.copy(), R.copy(), t.copy(), [None if d is None else d.copy() for d in dm],
            [None if x is None else x.copy() for x in nm], [list(x) for x in nb]]


def reordered(args, order):
    """the same problem with image order[k] at position k"""
    images, K, R, t, dm, nm, nb = args
    where = {old: new for new, old in enumerate(order)}
    return [[images[i] for i in order], K[list(order)], R[list(order)], t[list(order)], [dm[i] for i in order], [nm[i] for i in order],
            [[where[j] for j in nb[i]] for i in order]]


LOOSE = dict(min_num_pixels=1, max_reproj_error=2.0, max_depth_error=0.05, max_normal_error=25.0)


def build_cases():
    cases = {}
    # image and neighbour counts: 64 images give lists of 63, 65 give lists of 64
    for n in (1, 2, 3, 64, 65):
        cases[f"images_{n}"] = (stack(n, 2, 1), dict(ALL))
    cases["neighbours_0"] = (stack(3, neighbours=[[], [], []]), dict(ALL))
    cases["neighbours_1"] = (stack(3, neighbours=[[1], [2], [0]]), dict(ALL))
    cases["neighbours_twice"] = (stack(3, neighbours=[[1, 1, 2, 1], [2, 2], []]), dict(ALL))
    cases["neighbours_self_and_earlier"] = (stack(3, neighbours=[[0, 1], [0, 1, 2], [2, 1, 0]]), dict(ALL))
    # seeds per step and image shapes
    for w, h in ((1, 1), (2, 1), (63, 1), (64, 1), (65, 1), (257, 1), (1, 2), (1, 63), (1, 64), (1, 65), (5, 13)):
        cases[f"shape_{w}x{h}"] = (stack(2, w, h), dict(ALL))
    none = stack(2, 3, 2)
    none[4][0][...] = 0.0
    cases["seeds_0"] = (none, dict(ALL))
    # cluster sizes
    for m in (3, 4):
        cases[f"min_num_pixels_{m}_of_3"] = (stack(3), dict(min_num_pixels=m))
    for m in (1, 2):
        cases[f"max_num_pixels_{m}"] = (stack(4), dict(min_num_pixels=1, max_num_pixels=m))
    for n in (MAX_CLUSTER - 1, MAX_CLUSTER, MAX_CLUSTER + 1, MAX_CLUSTER + 2):  # many tiny images at one pose
        nb = [list(range(i + 1, min(n, i + 65))) for i in range(n)]
        cases[f"cluster_{n}"] = (stack(n, 1, 1, neighbours=nb), dict(ALL))
    cases["cluster_257_bound_256"] = (stack(257, 1, 1, neighbours=[list(range(i + 1, min(257, i + 65))) for i in range(257)]),
                                      dict(min_num_pixels=1, max_num_pixels=256))
    # traversal depth: a chain, each image naming only the next
    chain = [[i + 1] if i + 1 < 5 else [] for i in range(5)]
    for d in (1, 2, 3, 5):
        cases[f"chain_depth_{d}"] = (stack(5, neighbours=chain), dict(min_num_pixels=1, max_traversal_depth=d))
    cases["cycle"] = (stack(3, neighbours=[[1], [2], [1]]), dict(ALL))
    # bad values
    base = rendered("slanted", 3, 12, 9)
    cases["rendered_slanted"] = (base, dict(LOOSE))
    cases["rendered_step_defaults"] = (rendered("step", 4, 16, 12), dict(min_num_pixels=2))
    for what, value in (("nan", np.nan), ("inf", np.inf), ("neg_inf", -np.inf), ("zero", 0.0), ("negative", -2.0)):
        a = _copy(base)
        a[4][0][2, 3] = value  # a seed
        a[4][1][4, 5] = value  # a child
        a[4][2][1, 1:4] = value
        cases[f"depth_{what}"] = (a, dict(LOOSE))
    for what, value in (("nan", np.nan), ("inf", np.inf), ("zero", 0.0)):
        a = _copy(base)
        a[5][0][:, 2, 3] = value
        a[5][1][0, 4, 5] = value
        a[5][2][2, 1, 1:4] = value
        cases[f"normal_{what}"] = (a, dict(LOOSE))
    for what, value in (("nan", np.nan), ("inf", np.inf)):
        a = _copy(base)
        a[3][1][0] = value
        cases[f"pose_{what}"] = (a, dict(LOOSE))
        a = _copy(base)
        a[1][0][0] = value  # the first image's focal length
        cases[f"intrinsic_{what}"] = (a, dict(LOOSE))
    behind = stack(3)
    behind[2][1] = np.diag([-1.0, 1.0, -1.0])  # image 1 turned round: every point is behind it
    cases["behind_a_neighbour"] = (behind, dict(ALL))
    edge = stack(2, 4, 2)
    edge[1][1][2] += 0.5  # image 1's principal point half a pixel on: every projection falls on a pixel edge, the last on the border
    cases["projection_on_edge_and_border"] = (edge, dict(ALL))
    # claims
    again = stack(3, 4, 2, neighbours=[[2], [2], []])
    again[4][0][:, 2:] = 0.0  # image 0 seeds its left half only; image 1 then meets what image 0 took of image 2
    cases["claimed_met_again"] = (again, dict(ALL))
    shared = stack(2, 4, 2)
    shared[0][1] = shared[0][1][:1, :2].copy()
    shared[4][1], shared[5][1] = shared[4][1][:1, :2].copy(), shared[5][1][:, :1, :2].copy()
    shared[1][1] = [2.0, 2.0, 1.0, 0.5]  # half the focal length: two pixels of image 0 fall into one of image 1
    cases["two_seeds_share_a_member"] = (shared, dict(ALL))
    # structure
    hole = _copy(base)
    hole[4][1] = hole[5][1] = None
    cases["no_maps_in_the_middle"] = (hole, dict(LOOSE))
    cases["box_drops_everything"] = (base, dict(LOOSE, bounding_box=((10.0, 10.0, 10.0), (11.0, 11.0, 11.0))))
    cases["box_keeps_a_part"] = (base, dict(LOOSE, bounding_box=((-0.5, -10.0, 0.0), (0.5, 10.0, 10.0))))
    cases["reordered_210"] = (reordered(base, (2, 1, 0)), dict(LOOSE))
    cases["reordered_120"] = (reordered(base, (1, 2, 0)), dict(LOOSE))
    return cases


# what the trace of a case must hold: case -> reasons that must occur
EXPECT = {
    "neighbours_twice": ("in_cluster",), "neighbours_self_and_earlier": ("earlier_image",), "cycle": ("in_cluster",),
    "depth_nan": ("no_depth",), "depth_zero": ("no_depth",), "depth_negative": ("no_depth",), "depth_inf": ("depth_error",),
    "normal_nan": ("normal_error",), "pose_nan": ("outside",), "behind_a_neighbour": ("outside",),
    "projection_on_edge_and_border": ("outside", "taken"), "claimed_met_again": ("claimed",),
    "no_maps_in_the_middle": ("no_map",), "cluster_257": ("cut_short",), "cluster_258": ("cut_short",),
    "rendered_step_defaults": ("depth_error", "taken"),
}


def threshold_cases(ref):
    """Each of the three tests exactly on its threshold and one float beyond it: the quantity of one (seed, child) pair
    is measured on the reference, and the option is set so that its float32 threshold is that value, then the next float
    on the failing side.  name -> (arguments, options, (seed pixel, child image, child row, child col), taken)"""
    args = rendered("slanted", 2, 8, 6)
    args[4][1] = (args[4][1] * np.float32(1.003)).astype(np.float32)  # a depth error to measure
    tilt = np.array([0.05, -0.03, -1.0])
    args[5][1] = np.broadcast_to((tilt / np.linalg.norm(tilt)).astype(np.float32)[:, None, None], args[5][1].shape).copy()
    wide = dict(min_num_pixels=1, max_reproj_error=4.0, max_depth_error=0.5, max_normal_error=60.0)
    srow, scol = 3, 4
    out0 = ref.fuse_depth_maps(*args, trace=True, **wide)
    line = next(ln for ln in out0["trace"] if ln[2] == 1 and ln[5] == 0 and out0["seed_pixel"][ln[0]] == srow * 8 + scol and ln[1] == 0)
    row, col = int(line[3]), int(line[4])
    derr, cosn, rsq, _, _ = ref.measure(args, 0, srow, scol, 1, row, col)
    f = np.float32
    out = {}
    who = (srow * 8 + scol, 1, row, col)
    out["depth_on"] = (args, dict(wide, max_depth_error=float(f(derr))), who, True)
    out["depth_beyond"] = (args, dict(wide, max_depth_error=float(np.nextafter(f(derr), f(0)))), who, False)
    deg = lambda c: float(np.degrees(np.arccos(np.float64(c))))  # noqa: E731
    out["normal_on"] = (args, dict(wide, max_normal_error=deg(f(cosn))), who, True)
    out["normal_beyond"] = (args, dict(wide, max_normal_error=deg(np.nextafter(f(cosn), f(2)))), who, False)
    out["reproj_on"] = (args, dict(wide, max_reproj_error=float(np.sqrt(np.float64(f(rsq))))), who, True)
    out["reproj_beyond"] = (args, dict(wide, max_reproj_error=float(np.sqrt(np.float64(np.nextafter(f(rsq), f(0)))))), who, False)
    return out


KEYS = ("xyz", "normal", "color", "seed_image", "seed_pixel", "num_fused", "vis_offsets", "vis_images")


def same(a, b) -> bool:
    """two results agree bit for bit"""
    if a["num_points"] != b["num_points"] or a["num_seeds"] != b["num_seeds"] or a["num_truncated"] != b["num_truncated"]:
        return False
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in KEYS)


def result_digest(out) -> str:
    """one digest of a result's arrays and counts, in a fixed order"""
    import hashlib
    h = hashlib.sha256()
    for key in KEYS:
        h.update(np.ascontiguousarray(out[key]).tobytes())
    h.update(np.array([out["num_points"], out["num_seeds"], out["num_truncated"]], np.uint64).tobytes())
    return h.hexdigest()
