"""The shapes at which guided matching (amc_match_guided_pairs: match_guided.hip, guided_region.h, the GUIDED build of
match_dot4.hip) can go wrong, shared by tests/test_guided_cases_cpu.py, tests/test_guided_cases_gpu.py and
tests/golden/make_guided_ref_golden.py.  Everything is built from fixed integers and small seeded draws.

build_cases() returns name -> dict(images=[dict(descriptors, keypoints)], pairs=(s1, s2), tvg=TVG_DTYPE array, max_error,
options, grid, reach): `grid` says per pair whether guided_pair_setup lets the candidate-generation kernel take it, `reach`
is the list of claims about which edge of that kernel the case reaches.  The CPU suite checks every claim on the host
build of guided_region.h (tests/shim/guided_shim.cc) - trace() below replays the kernel's staging rounds from it - so a
case cannot silently stop reaching its edge.

The kernel's hidden state, as the claims name it: a row's candidates are LISTED grid row by grid row (lane = grid row,
cells left to right, ascending index inside a cell) in rounds of 512 (kCandCap); every listed keypoint goes through the
float32 filter; the survivors of a round are compacted in list order and survivor k of the round gets its dot product
in lane k % 64, which folds it into that lane's (best, index, second); after the last round a butterfly merges the 64
lanes.  So two candidates meet in the per-lane fold when they survive in the same lane (same round or not) and in the
butterfly otherwise."""
from __future__ import annotations

import ctypes as C
import functools
import hashlib
import subprocess
from pathlib import Path

import numpy as np

import oracle_lib as o
from pycolmap_amd import synth
from pycolmap_amd._capi import TVG_DTYPE

ROOT = Path(__file__).resolve().parent.parent
SHIM = ROOT / "tests" / "shim" / "_build" / "libguidedshim.so"
CAND_CAP = 512          # match_guided.hip: kCandCap
KIND_F, KIND_H = 1, 2
DEFAULTS = dict(max_ratio=0.8, max_distance=0.7, cross_check=True)
TIE_OPTIONS = dict(max_ratio=1.5, max_distance=2.0)     # a tied best still yields a match: the index shows
STAGING_TOTALS = (1, 63, 64, 65, 511, 512, 513, 1024, 1025)
ROW_SIZES = (1, 15, 16, 17, 63, 64, 65, 128, 129)
BOUNDARY_THRESHOLDS = (0.5, 4.0, 50.0)
H_HORIZON = np.array([[1, 0, 0], [0, 1, 0], [1.0 / 800, 0, -1.0]])     # w = x / 800 - 1 changes sign inside the images
F_TX = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])                # [t]_x, t = (1, 0, 0): accepts y2 == y1


# ---- the host build of guided_region.h ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shim() -> C.CDLL:
    SHIM.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "shim" / "guided_shim.cc"
    hdr = ROOT / "pycolmap_amd" / "csrc" / "guided_region.h"
    if not SHIM.exists() or SHIM.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-shared", "-fPIC", str(src),
                        "-o", str(SHIM)], check=True)
    lib = C.CDLL(str(SHIM))
    for f in (lib.shim_guided_candidates, lib.shim_grid_cells, lib.shim_guided_listing):
        f.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def kind_of(config: int) -> int:
    return KIND_F if config in (2, 3) else KIND_H


def model_of(case, p: int):
    """(kind, the 9 float32 coefficients of the filter, float32 max_residual) of pair p, as the library forms them."""
    t = case["tvg"][p]
    kind = kind_of(int(t["config"]))
    m = np.ascontiguousarray((t["F"] if kind == KIND_F else t["H"]).reshape(9), dtype=np.float32)
    return kind, m, np.float32(case["max_error"] * case["max_error"])


def pair_keypoints(case, p: int):
    a, b = int(case["pairs"][0][p]), int(case["pairs"][1][p])
    return (np.ascontiguousarray(case["images"][a]["keypoints"], np.float32),
            np.ascontiguousarray(case["images"][b]["keypoints"], np.float32))


def candidates(case, p: int, direction: int):
    """(routes to the grid kernel, [rows, cols] uint8: listed) for pair p; rows are image-1 points for direction 0."""
    kind, m, mr = model_of(case, p)
    kp1, kp2 = pair_keypoints(case, p)
    nr, nc = (len(kp1), len(kp2)) if direction == 0 else (len(kp2), len(kp1))
    cand = np.zeros((nr, nc), dtype=np.uint8)
    if len(kp1) == 0 or len(kp2) == 0:
        return False, cand
    rc = shim().shim_guided_candidates(kind, _p(m), C.c_float(mr), _p(kp1), len(kp1), _p(kp2), len(kp2), direction, _p(cand))
    return rc == 1, cand


def routes_to_grid(case, p: int) -> bool:
    return candidates(case, p, 0)[0]


def grid_cells(kp):
    """(geom = x0, y0, cw, ch, inv_cw, inv_ch, bx1, by1; gx; gy) of an image's keypoint grid."""
    kp = np.ascontiguousarray(kp, np.float32)
    geom = np.zeros(8, np.float32)
    gx, gy = np.zeros(len(kp), np.int32), np.zeros(len(kp), np.int32)
    assert shim().shim_grid_cells(_p(kp), len(kp), _p(geom), _p(gx), _p(gy)) == 1
    return geom, gx, gy


def filter_rejects(kind, m, mr, x1, y1, x2, y2):
    """oracle_guided_filter restated on float32 arrays: every product and sum rounded to float32, left to right."""
    f = np.float32
    x1, y1, x2, y2 = (np.asarray(v, f) for v in (x1, y1, x2, y2))
    one = f(1.0)
    with np.errstate(all="ignore"):
        if kind == KIND_F:
            a0 = m[0] * x1 + m[1] * y1 + m[2] * one
            a1 = m[3] * x1 + m[4] * y1 + m[5] * one
            a2 = m[6] * x1 + m[7] * y1 + m[8] * one
            b0 = m[0] * x2 + m[3] * y2 + m[6] * one
            b1 = m[1] * x2 + m[4] * y2 + m[7] * one
            e = x2 * a0 + y2 * a1 + one * a2
            return e * e / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1) > mr
        h0 = m[0] * x1 + m[1] * y1 + m[2] * one
        h1 = m[3] * x1 + m[4] * y1 + m[5] * one
        h2 = m[6] * x1 + m[7] * y1 + m[8] * one
        e0 = h0 / h2 - x2
        e1 = h1 / h2 - y2
        return e0 * e0 + e1 * e1 > mr


def oracle_rejects(kind, m, mr, x1, y1, x2, y2) -> bool:
    """The frozen filter itself (oracle/match_oracle.c), one pairing."""
    lib = o.load()
    lib.oracle_guided_filter.restype = C.c_int
    lib.oracle_guided_filter.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]
    return bool(lib.oracle_guided_filter(kind, _p(m), C.c_float(mr), C.c_float(x1), C.c_float(y1), C.c_float(x2), C.c_float(y2)))


def accepted_matrix(case, p: int):
    """[n1, n2] bool: the float32 filter does not reject (image-1 point, image-2 point) of pair p."""
    kind, m, mr = model_of(case, p)
    kp1, kp2 = pair_keypoints(case, p)
    return ~filter_rejects(kind, m, mr, kp1[:, None, 0], kp1[:, None, 1], kp2[None, :, 0], kp2[None, :, 1])


def trace(case, p: int, direction: int, row: int):
    """The kernel's staging of one row, replayed: dict(idx: listed keypoints in list order, lane: the grid row each came
    from, ok: survives the filter, round, acc_pos: position among its round's survivors (-1: rejected),
    rounds: [(cnt, nacc)])."""
    kind, m, mr = model_of(case, p)
    kp1, kp2 = pair_keypoints(case, p)
    ncols = len(kp2) if direction == 0 else len(kp1)
    idx, lane = np.zeros(ncols, np.uint32), np.zeros(ncols, np.int32)
    total = shim().shim_guided_listing(kind, _p(m), C.c_float(mr), _p(kp1), len(kp1), _p(kp2), len(kp2), direction, row,
                                       _p(idx), _p(lane))
    assert total >= 0, "the pair does not take the candidate-generation kernel"
    idx, lane = idx[:total], lane[:total]
    if direction == 0:
        rej = filter_rejects(kind, m, mr, kp1[row, 0], kp1[row, 1], kp2[idx, 0], kp2[idx, 1])
    else:
        rej = filter_rejects(kind, m, mr, kp1[idx, 0], kp1[idx, 1], kp2[row, 0], kp2[row, 1])
    ok = ~np.asarray(rej, bool).reshape(total)
    rnd = np.arange(total) // CAND_CAP
    acc_pos = np.full(total, -1, np.int64)
    rounds = []
    for r in range((total + CAND_CAP - 1) // CAND_CAP):
        sel = np.flatnonzero((rnd == r) & ok)
        acc_pos[sel] = np.arange(len(sel))
        rounds.append((int((rnd == r).sum()), len(sel)))
    return dict(idx=idx.astype(np.int64), lane=lane, ok=ok, round=rnd, acc_pos=acc_pos, rounds=rounds)


# ---- the expectation ---------------------------------------------------------------------------------------------------
def oracle_matches(case):
    """The frozen oracle's matches of every pair: (offsets uint64 [npairs + 1], matches uint32 [M, 2])."""
    s1, s2 = case["pairs"]
    chunks = []
    for p in range(len(s1)):
        a, b = case["images"][int(s1[p])], case["images"][int(s2[p])]
        t = case["tvg"][p]
        m = o.match_guided(a["descriptors"], a["keypoints"], b["descriptors"], b["keypoints"], int(t["config"]), t["F"], t["H"],
                           case["max_error"], **case["options"])
        assert m is not None
        chunks.append(m)
    off = np.zeros(len(s1) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in chunks])
    return off, (np.concatenate(chunks) if int(off[-1]) else np.zeros((0, 2), np.uint32))


def digest(off, matches) -> str:
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(off, np.uint64).tobytes())
    h.update(np.ascontiguousarray(matches, np.uint32).tobytes())
    return h.hexdigest()


def numpy_one_way(d, max_ratio, max_distance):
    """FindBestMatchesOneWayBruteForce on an int matrix whose rejected entries are 0, in plain numpy: per row the first
    index of the maximum, the second WITH multiplicity (a tied best is its own second), the float32 acos tests."""
    f = np.float32
    out = np.full(d.shape[0], -1, np.int64)
    if d.shape[1] == 0:
        return out
    for i, r in enumerate(d):
        best = int(r.max())
        if best <= 0:
            continue
        j = int(np.argmax(r))
        rest = np.delete(r, j)
        second = max(int(rest.max()), 0) if len(rest) else 0
        k = f(1.0) / (f(512.0) * f(512.0))
        a_best = np.arccos(np.minimum(k * f(best), f(1.0)), dtype=f)
        a_second = np.arccos(np.minimum(k * f(second), f(1.0)), dtype=f)
        if a_best > f(max_distance) or a_best >= f(max_ratio) * a_second:
            continue
        out[i] = j
    return out


def numpy_matches(case, p: int):
    """MatchGuided of pair p from the filtered dot-product matrix, without the C oracle's scans."""
    s1, s2 = case["pairs"]
    a, b = case["images"][int(s1[p])], case["images"][int(s2[p])]
    d = a["descriptors"].astype(np.int64) @ b["descriptors"].astype(np.int64).T
    d = np.where(accepted_matrix(case, p), d, 0)
    opt = case["options"]
    m12 = numpy_one_way(d, opt["max_ratio"], opt["max_distance"])
    m21 = numpy_one_way(d.T, opt["max_ratio"], opt["max_distance"]) if opt["cross_check"] else None
    out = [(i, j) for i, j in enumerate(m12) if j >= 0 and (m21 is None or m21[j] == i)]
    return np.array(out, np.uint32).reshape(-1, 2)


# ---- building blocks ---------------------------------------------------------------------------------------------------
def descs(seed: int, n: int):
    return synth.random_descriptors(np.random.default_rng(seed), n)


def image(descriptors, keypoints):
    d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 128)
    k = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 2)
    assert len(d) == len(k)
    return dict(descriptors=d, keypoints=k)


def translation(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])


def cross_matrix(e):
    return np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0.0]])


def case(images, pairs, models, max_error, grid, reach=(), **options):
    """models: per pair (configuration, 3 x 3 matrix); configuration 2, 3: F, 4, 5, 6: H."""
    tvg = np.zeros(len(pairs), dtype=TVG_DTYPE)
    for k, (cfg, mat) in enumerate(models):
        tvg["config"][k] = cfg
        tvg["F" if kind_of(cfg) == KIND_F else "H"][k] = mat
    assert len(grid) == len(pairs) == len(models)
    return dict(images=list(images), pairs=(np.array([a for a, _ in pairs], np.uint32), np.array([b for _, b in pairs], np.uint32)),
                tvg=tvg, max_error=float(max_error), options={**DEFAULTS, **options}, grid=[bool(g) for g in grid],
                reach=list(reach))


def permuted_copy(img, seed):
    """The same features in another order: row i of the copy is feature perm[i] of img."""
    perm = np.random.default_rng(seed).permutation(len(img["keypoints"]))
    return image(img["descriptors"][perm], img["keypoints"][perm]), perm


# ---- family 1: the staging bound ---------------------------------------------------------------------------------------
def spread_layout(n):
    """n keypoints over the grid rows of the box [0, 640]^2 (10-pixel cells): keypoint i in grid row i % 64."""
    i = np.arange(n)
    gy = i % 64
    gx = (i // 64 * 5 + gy * 3) % 64
    y = np.where(gy == 0, 0.0, np.where(gy == 63, 640.0, 10.0 * gy + 5))
    x = np.where(gx == 0, 0.0, np.where(gx == 63, 640.0, 10.0 * gx + 5))
    return np.stack([x, y], axis=1)


ANCHORS = np.array([[0.0, 0.0], [6400.0, 6400.0]])     # stretch the box: 100-pixel cells


def staging_cases(cases):
    ident = (4, np.eye(3))
    # (a) every keypoint of the box listed and accepted: total = cnt = nacc = n
    for n in STAGING_TOTALS:
        y = image(descs(1000 + n, n), spread_layout(n))
        x, perm = permuted_copy(y, 2000 + n)
        reach = [dict(kind="totals", pair=0, dir=d, rows="all", total=n) for d in (0, 1)]
        reach.append(dict(kind="rounds", pair=0, dir=0, row=0,
                          rounds=[(min(CAND_CAP, n - b), min(CAND_CAP, n - b)) for b in range(0, n, CAND_CAP)]))
        reach.append(dict(kind="lanes_occupied", pair=0, dir=0, row=0, lanes=min(n, 64)))
        cases[f"staging/a_{n}"] = case([x, y], [(0, 1)], [ident], 1000.0, [True], reach)
    y = image(descs(1000, 65), spread_layout(65))
    x = image(y["descriptors"][:3], [[5000.0, 5000.0], [5001.0, 5000.0], [5002.0, 5000.0]])
    cases["staging/a_0"] = case([x, y], [(0, 1)], [ident], 4.0, [True],
                                [dict(kind="totals", pair=0, dir=d, rows="all", total=0) for d in (0, 1)])
    # (b) the whole list in ONE cell (one lane owns it through every round); 4 pixels keep a part of it
    for n in STAGING_TOTALS:
        k = np.arange(n)
        cluster = np.stack([3234.0 + k % 33, 3234.0 + k // 33], axis=1)
        y = image(descs(3000 + n, n + 2), np.concatenate([ANCHORS, cluster]))
        x, perm = permuted_copy(y, 4000 + n)
        inv = np.argsort(perm)
        members = np.flatnonzero(perm >= 2)
        reach = []
        for d in (0, 1):
            reach.append(dict(kind="totals", pair=0, dir=d, rows=members if d == 0 else np.arange(2, n + 2), total=n))
            reach.append(dict(kind="totals", pair=0, dir=d, rows=inv[:2] if d == 0 else np.arange(2), total=1))
        reach.append(dict(kind="lanes_occupied", pair=0, dir=0, row=int(members[0]), lanes=1))
        if n == 1025:
            # the rows at the cluster's first and last keypoint: survivors in round 0 only / in rounds 1 and 2 only
            reach.append(dict(kind="rounds", pair=0, dir=0, row=int(inv[2]), rounds=[(512, 17), (512, 0), (1, 0)]))
            reach.append(dict(kind="rounds", pair=0, dir=0, row=int(inv[2 + 1024]), rounds=[(512, 0), (512, 16), (1, 1)]))
        if n == 513:
            reach.append(dict(kind="rounds", pair=0, dir=0, row=int(inv[2 + 512]), rounds=[(512, 24), (1, 1)]))
        cases[f"staging/b_{n}"] = case([x, y], [(0, 1)], [ident], 4.0, [True], reach)
    # (c) two grid rows whose ranges meet inside a round: the second lane's range is cut at `base`
    for na, nb in ((300, 300), (500, 13)):
        ka, kb = np.arange(na), np.arange(nb)
        grp_a = np.stack([3230.0 + ka % 40, 2099.0 - ka // 40], axis=1)     # grid row 20
        grp_b = np.stack([3230.0 + kb % 40, 2101.0 + kb // 40], axis=1)     # grid row 21
        y = image(descs(5000 + na, na + nb + 2), np.concatenate([ANCHORS, grp_a, grp_b]))
        x, perm = permuted_copy(y, 6000 + na)
        members = np.flatnonzero(perm >= 2)
        n = na + nb
        reach = [dict(kind="totals", pair=0, dir=0, rows=members, total=n),
                 dict(kind="totals", pair=0, dir=1, rows=np.arange(2, n + 2), total=n),
                 dict(kind="lane_lengths", pair=0, dir=0, row=int(members[0]), lengths={20: na, 21: nb}),
                 dict(kind="rounds", pair=0, dir=0, row=int(members[0]), rounds=[(512, 512), (n - 512, n - 512)])]
        cases[f"staging/c_{na}_{nb}"] = case([x, y], [(0, 1)], [ident], 60.0, [True], reach)


# ---- family 2: ties and zeros ------------------------------------------------------------------------------------------
QUERY = np.array([3250.0, 3250.0])      # the middle of cell (32, 32) of the ANCHORS box
TIE_ERROR = 180.0                       # lists grid rows and columns 30 .. 34; accepts the 3 x 3 cells around the query


def cell_points(gy, gx, count):
    k = np.arange(count)
    return np.stack([100.0 * gx + 50 + 0.25 * (k % 48), 100.0 * gy + 50 + 0.25 * (k // 48)], axis=1)


def tie_layout(cells):
    """cells: [(gy, gx, count or list of tags)] in LIST order (grid rows ascending, columns ascending).  Indices are
    handed out against the list order - the cell listed last gets the lowest indices - and the two anchors come last.
    Returns (keypoints, tags: per keypoint None or its tag)."""
    assert [c[:2] for c in cells] == sorted(c[:2] for c in cells)
    kps, tags = [], []
    for gy, gx, what in reversed(cells):
        t = [None] * what if isinstance(what, int) else list(what)
        kps.append(cell_points(gy, gx, len(t)))
        tags += t
    kps.append(ANCHORS)
    tags += [None, None]
    return np.concatenate(kps), tags


def reduced_query_descriptor(seed):
    """A descriptor with |q|^2 well below 512^2 (entries zeroed from the front), so that acos(best) > 0 and the ratio
    test looks at the second."""
    q = descs(seed, 1)[0].copy()
    k = 0
    while int((q.astype(np.int64) ** 2).sum()) > 240000:
        q[k] = 0
        k += 1
    return q


def tie_case(name, cells, cases, expect, zero_query=False):
    """One query row of image 0 at QUERY; image 1 from tie_layout.  Tags: 'T' a copy of the query's descriptor, 'S' the
    query's descriptor less one step in one entry (the same for every S), 'O' a descriptor on a support disjoint from the
    query's (dot exactly 0), 'W' a weak partner (dot > 0, far below a filler's), None a seeded filler.  `expect`:
    the claims besides the list positions."""
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:6], 16)
    kp2, tags = tie_layout(cells)
    q = reduced_query_descriptor(seed)
    d2 = descs(seed + 1, len(kp2))
    second = q.copy()
    second[int(np.argmax(q))] -= 1
    lo = q.copy()
    lo[64:] = 0                          # the query of the zero cases lives on entries 0 .. 63
    ortho = np.zeros(128, np.uint8)
    ortho[64:] = d2[0][:64]
    weak = np.zeros(128, np.uint8)
    weak[int(np.argmax(lo))] = 1
    weak[64:] = 3
    qd = lo if zero_query else q
    for j, t in enumerate(tags):
        if t == "T":
            d2[j] = qd
        elif t == "S":
            d2[j] = second
        elif t == "O":
            d2[j] = ortho
        elif t == "W":
            d2[j] = weak
    # image 0: the query, two more rows with seeded descriptors next to it, and the anchors
    kp1 = np.concatenate([[QUERY], [QUERY + [1.0, 0.0]], [QUERY + [0.0, 1.0]], ANCHORS])
    d1 = descs(seed + 2, len(kp1))
    d1[0] = qd
    tagged = {t: [j for j, u in enumerate(tags) if u == t] for t in set(tags) if t is not None}
    reach = [dict(kind="tie", pair=0, dir=0, row=0, tagged=tagged, **expect)]
    imgs = [image(d1, kp1), image(d2, kp2)]
    pairs, models, grid = [(0, 1), (1, 0)], [(4, np.eye(3))] * 2, [True, True]
    cases[f"{name}/cc"] = case(imgs, pairs, models, TIE_ERROR, grid, reach, **TIE_OPTIONS, cross_check=True)
    cases[f"{name}/nocc"] = case(imgs, pairs, models, TIE_ERROR, grid, reach, **TIE_OPTIONS, cross_check=False)
    cases[f"{name}/ratio08"] = case(imgs, pairs, models, TIE_ERROR, grid, reach)


def tie_cases(cases):
    # `where`: per tagged candidate in LIST order (round, position among the round's survivors); lane = position % 64
    # two bests in one lane of one round: the per-lane fold
    tie_case("tie/lane", [(31, 31, ["T"]), (31, 32, 63), (31, 33, ["T"])], cases,
             dict(where={"T": [(0, 0), (0, 64)]}, best="T", second="T"))
    # two bests in different grid rows, different lanes: the butterfly
    tie_case("tie/butterfly", [(31, 32, ["T"]), (32, 32, 10), (33, 32, ["T"])], cases,
             dict(where={"T": [(0, 0), (0, 11)]}, best="T", second="T"))
    # two bests more than 512 list places apart, in the same lane of two rounds (275 of the fillers are listed and
    # rejected) and in different lanes of two rounds
    tie_case("tie/rounds_lane", [(31, 32, ["T"]), (32, 30, 275), (32, 32, 300), (33, 32, ["T"])], cases,
             dict(where={"T": [(0, 0), (1, 64)]}, best="T", second="T"))
    tie_case("tie/rounds_butterfly", [(31, 32, ["T"]), (32, 30, 275), (32, 32, 310), (33, 32, ["T"])], cases,
             dict(where={"T": [(0, 0), (1, 74)]}, best="T", second="T"))
    tie_case("tie/three", [(31, 32, ["T"]), (32, 31, 63), (32, 32, ["T"]), (32, 33, 5), (33, 32, ["T"])], cases,
             dict(where={"T": [(0, 0), (0, 64), (0, 70)]}, best="T", second="T"))
    # a unique best between two equal seconds, one of them in the best's lane
    tie_case("tie/seconds", [(31, 32, ["S"]), (32, 31, 63), (32, 32, ["T"]), (32, 33, 5), (33, 32, ["S"])], cases,
             dict(where={"S": [(0, 0), (0, 70)], "T": [(0, 64)]}, best="T", second="S"))
    # copies of the query the filter rejects - one listed (200 pixels away), one never listed - with lower indices than
    # the accepted copy: they must not count, so the match comes through the default ratio test
    tie_case("tie/rejected", [(31, 32, 4), (32, 32, ["T"]), (32, 34, ["T"]), (50, 50, ["T"])], cases,
             dict(where={"T": [(0, 4), (0, -1)]}, best="T", second=None, survivors={"T": 1}))
    # zeros
    tie_case("zero/orthogonal", [(31, 32, ["O", "O"]), (32, 32, ["W"]), (33, 32, ["O"])], cases,
             dict(where={"O": [(0, 0), (0, 1), (0, 3)], "W": [(0, 2)]}, best="W", second=None, zeros="O"), zero_query=True)
    tie_case("zero/only", [(32, 30, 3), (32, 32, ["O"]), (32, 34, 2)], cases,
             dict(where={"O": [(0, 0)]}, best=None, second=None, zeros="O"), zero_query=True)
    # an all-zero descriptor row in image 0 (and, for the reverse scans, an all-zero candidate), and a best of exactly
    # 512 * 512: acosf gives exactly 0 there (0 >= max_ratio * second is false for any second below: the row matches),
    # so the device's table and the host's acosf have to agree at the table's last entry
    kp2, _ = tie_layout([(31, 32, 6), (32, 32, 6), (33, 32, 6)])
    d2 = descs(77, len(kp2))
    full = np.zeros(128, np.uint8)
    full[:64] = 64                         # 64 * 64^2 = 512^2
    d2[5] = full
    kp1 = np.concatenate([[QUERY], [QUERY + [1.0, 0.0]], [QUERY + [0.0, 1.0]], ANCHORS])
    d1 = descs(78, len(kp1))
    d1[0] = 0
    d1[1] = full
    imgs = [image(d1, kp1), image(d2, kp2)]
    for tag, opt in (("cc", dict(TIE_OPTIONS)), ("nocc", dict(TIE_OPTIONS, cross_check=False)), ("ratio08", {})):
        cases[f"zero/x_row/{tag}"] = case(imgs, [(0, 1), (1, 0)], [(4, np.eye(3))] * 2, TIE_ERROR, [True, True],
                                          [dict(kind="zero_row", pair=0, row=0, full_row=1, full_col=5)], **opt)


# ---- family 3: row-block edges -----------------------------------------------------------------------------------------
def row_block_cases(cases):
    rng = np.random.default_rng(300)
    nl = max(ROW_SIZES)
    land_xy = rng.uniform([100, 100], [1500, 1100], size=(nl, 2))
    land_d = descs(301, nl)
    imgs, shifts = [], []
    for k, n in enumerate(ROW_SIZES):
        t = np.array([1.0 * k, -0.75 * k])      # (small steps: the swapped pair, off by twice the step, keeps a part)
        order = rng.permutation(n)
        noise = rng.uniform(-1.0, 1.0, size=(n, 2))
        imgs.append(image(land_d[order], land_xy[order] + t + noise))
        shifts.append(t)
    pairs, h_models, f_models = [], [], []
    e = np.array([3000.0, 500.0, 1.0])
    for k in range(len(ROW_SIZES)):
        a, b = k, (k + 1) % len(ROW_SIZES)
        hm = translation(*(shifts[b] - shifts[a]))
        fm = cross_matrix(e) @ hm
        fm = fm / np.abs(fm).max()
        pairs += [(a, b), (b, a)]          # and the two images swapped under the same model
        h_models += [(4, hm)] * 2
        f_models += [(3, fm)] * 2
    reach = [dict(kind="sizes", sizes=ROW_SIZES)]
    cases["rows/H"] = case(imgs, pairs, h_models, 4.0, [True] * len(pairs), reach)
    cases["rows/F"] = case(imgs, pairs, f_models, 4.0, [True] * len(pairs), reach)


# ---- family 4: grid geometry -------------------------------------------------------------------------------------------
def both_ways(imgs, model, max_error, grid=True, reach=(), **options):
    return case(imgs, [(0, 1), (1, 0)], [model, model], max_error, [grid, grid], reach, **options)


def geometry_cases(cases):
    rng = np.random.default_rng(400)
    # integer keypoints on a box of extent 64 * 2: 2-pixel cells, every keypoint on a cell boundary, the corners included
    n = 300
    xy = 2.0 * rng.integers(0, 65, size=(n, 2))
    xy[0], xy[1] = (0, 0), (128, 128)
    y = image(descs(401, n), xy)
    x, _ = permuted_copy(y, 402)
    x = image(x["descriptors"], x["keypoints"] - [2.0, 0.0])
    cases["geom/pow2"] = both_ways([x, y], (4, translation(2, 0)), 3.0,
                                   reach=[dict(kind="on_cell_boundaries", image=k, extent=128.0) for k in (0, 1)])
    # all keypoints of the searched image identical, on a horizontal line, on a vertical line; a single keypoint
    m = 70
    xd, off = descs(403, 40), rng.uniform(-2.5, 2.5, size=(40, 2))
    t = np.arange(m, dtype=np.float64)
    for name, pts in (("identical", np.tile([500.0, 500.0], (m, 1))), ("hline", np.stack([465 + t, 0 * t + 500], axis=1)),
                      ("vline", np.stack([0 * t + 500, 465 + t], axis=1)), ("one", np.array([[500.0, 500.0]]))):
        # row i of image 0 sits within 2.5 pixels of its partner, keypoint 39 - i (the only one), whose descriptor it has
        partner = np.minimum(39 - np.arange(40), len(pts) - 1)
        d = descs(404, len(pts))
        d[partner] = xd
        x = image(xd, pts[partner] + off)
        cases[f"geom/{name}"] = both_ways([x, image(d, pts)], (4, np.eye(3)), 4.0,
                                          reach=[dict(kind="degenerate_box", image=1, what=name)])
    # max_error = 0: F = [t]_x accepts exactly y2 == y1 on integer coordinates, H = I exactly the coincident keypoints
    n = 120
    xy1 = rng.integers(0, 40, size=(n, 2)).astype(np.float64)
    xy2 = np.stack([rng.integers(0, 40, size=n), xy1[rng.permutation(n), 1]], axis=1).astype(np.float64)
    d1 = descs(405, n)
    cases["geom/err0_F"] = both_ways([image(d1, xy1), image(d1[::-1], xy2)], (3, F_TX), 0.0,
                                     reach=[dict(kind="exact_zero", accepted="y2 == y1")], **TIE_OPTIONS)
    xy2 = xy1[::-1].copy()
    xy2[::3] += [1.0, 0.0]
    cases["geom/err0_H"] = both_ways([image(d1, xy1), image(d1[::-1], xy2)], (4, np.eye(3)), 0.0,
                                     reach=[dict(kind="exact_zero", accepted="coincident")], **TIE_OPTIONS)
    # negative coordinates
    n = 200
    xy = rng.uniform([-1600, -1200], [-50, -50], size=(n, 2))
    y = image(descs(406, n), xy)
    x, _ = permuted_copy(y, 407)
    x = image(x["descriptors"], x["keypoints"] - [30.0, -20.0] + rng.uniform(-2, 2, size=(n, 2)))
    cases["geom/negative"] = both_ways([x, y], (4, translation(30, -20)), 4.0, reach=[dict(kind="negative", images=(0, 1))])
    # the coordinate limit of guided_pair_setup: a box corner at 1e7 - 1 keeps the grid kernel, at 1e7 + 1 the dense one
    n = 90
    base = np.stack([1e7 - 200 + rng.integers(0, 199, size=n), 1000.0 + rng.integers(0, 150, size=n)], axis=1)
    base[0, 0] = 1e7 - 1
    a = image(descs(408, n), base)
    b, _ = permuted_copy(a, 409)
    over = b["keypoints"].astype(np.float64)
    over[:, 0] += 2.0
    c = image(b["descriptors"], over)
    cases["geom/limit_1e7"] = case([a, b, c], [(0, 1), (0, 2), (2, 0), (1, 0)],
                                   [(4, np.eye(3)), (4, translation(2, 0)), (4, translation(-2, 0)), (4, np.eye(3))], 4.0,
                                   [True, False, False, True],
                                   [dict(kind="box_max", image=0, x=1e7 - 1), dict(kind="box_max", image=1, x=1e7 - 1),
                                    dict(kind="box_max", image=2, x=1e7 + 1)])


# ---- family 5: the acceptance boundary ---------------------------------------------------------------------------------
def _f32_ordinal(v):
    """float32 -> an integer that orders like the float (adjacent floats differ by 1)."""
    i = int(np.float32(v).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def _f32_from_ordinal(i):
    return np.array([i if i >= 0 else (-i) | 0x80000000], dtype=np.uint32).view(np.float32)[0]


def boundary_twins(kind, m, mr, p, start, axis, step, swapped):
    """From `start` (accepted) move coordinate `axis` by `step` (rejected there) and bisect over the float32 values in
    between to the adjacent pair (accepted, rejected).  The filter is oracle_guided_filter(p, twin), or (twin, p) when
    `swapped`."""
    def rejects(q):
        return oracle_rejects(kind, m, mr, *((q[0], q[1], p[0], p[1]) if swapped else (p[0], p[1], q[0], q[1])))

    s = np.array(start, np.float32)
    far = s.copy()
    for _ in range(3):      # (the Sampson error grows slowly with the distance when p's line is short: go further out)
        far[axis] = np.float32(s[axis] + np.float32(step))
        if rejects(far):
            break
        step *= 4.0
    if rejects(s) or not rejects(far):
        return None         # no boundary within reach: near the epipole the Sampson error stays below a wide threshold
    lo, hi = _f32_ordinal(s[axis]), _f32_ordinal(far[axis])
    while abs(hi - lo) > 1:
        mid = (lo + hi) // 2
        q = s.copy()
        q[axis] = _f32_from_ordinal(mid)
        if rejects(q):
            hi = mid
        else:
            lo = mid
    acc, rej = s.copy(), s.copy()
    acc[axis], rej[axis] = _f32_from_ordinal(lo), _f32_from_ordinal(hi)
    return acc, rej


def boundary_images(kind, model, max_error, swapped, seed):
    """64 points p and, for each, the adjacent float32 pair on the filter's boundary: the rejected twin at index 2 i, the
    accepted one at 2 i + 1, both with p's descriptor.  Returns (image of the p, image of the twins)."""
    rng = np.random.default_rng(seed)
    m = np.ascontiguousarray(np.asarray(model, np.float64).reshape(9), dtype=np.float32)
    mr = np.float32(max_error * max_error)
    md = m.astype(np.float64).reshape(3, 3)
    d = descs(seed + 1, 64)
    pts = np.zeros((64, 2), np.float32)
    twins = np.zeros((128, 2), np.float32)
    i = 0
    while i < 64:           # (a draw without a boundary within reach is skipped: see boundary_twins)
        p = rng.uniform([100, 100], [1500, 1100]).astype(np.float32)
        ph = np.array([p[0], p[1], 1.0], np.float64)
        if kind == KIND_F:
            a, b, c = (md.T if swapped else md) @ ph                  # the line of p in the twins' image
            anchor = rng.uniform([300, 300], [1300, 900])
            foot = anchor - (a * anchor[0] + b * anchor[1] + c) / (a * a + b * b) * np.array([a, b])
            axis = 0 if abs(a) >= abs(b) else 1
        else:
            q = (np.linalg.inv(md) if swapped else md) @ ph
            foot = q[:2] / q[2]
            axis = i % 2
        step = (8.0 * max_error + 4.0) * (1 if i % 4 < 2 else -1)
        found = boundary_twins(kind, m, mr, p, foot, axis, step, swapped)
        if found is None:
            continue
        pts[i], twins[2 * i], twins[2 * i + 1] = p, found[1], found[0]
        i += 1
    return image(d, pts), image(np.repeat(d, 2, axis=0), twins)


def boundary_cases(cases):
    a_mat = np.eye(3) + np.array([[0.02, -0.01, 12.0], [0.015, 0.01, -9.0], [2e-6, -3e-6, 0.0]])
    f_out = cross_matrix([3100.0, 700.0, 1.0]) @ a_mat
    f_in = cross_matrix([820.0, 640.0, 1.0]) @ a_mat
    models = {"F_out": (3, f_out / np.abs(f_out).max()), "F_in": (3, f_in / np.abs(f_in).max()), "H": (4, a_mat)}
    for mname, (cfg, mat) in models.items():
        for t, thr in enumerate(BOUNDARY_THRESHOLDS):
            # one call: images 0, 1 with the twins in image 2's role, images 2, 3 with the twins in image 1's role
            p0, t0 = boundary_images(kind_of(cfg), mat, thr, False, 500 + 10 * t + len(mname))
            p1, t1 = boundary_images(kind_of(cfg), mat, thr, True, 600 + 10 * t + len(mname))
            reach = [dict(kind="boundary", pair=0, points=0, twins=1, swapped=False),
                     dict(kind="boundary", pair=1, points=2, twins=3, swapped=True)]
            cases[f"boundary/{mname}/{thr:g}"] = case([p0, t0, p1, t1], [(0, 1), (3, 2)], [(cfg, mat)] * 2, thr, [True, True],
                                                      reach)
    cases["boundary/sliver_H"] = sliver_case()


SLIVER_ULP = 2.0 ** -14      # float32 spacing in [512, 1024)
SLIVER_H = np.array([[1.013, 0.021, 7.3], [-0.017, 0.991, -5.1], [0.0, 0.0, 1.0]])


def sliver_case():
    """Accepted keypoints OUTSIDE the exact box around H p, in another cell than the box's edge: what the regions' slack
    (2 % and one pixel) is for.  H is affine and max_error = 4.  The float32 filter computes hx = fl(H p)_x with three
    roundings and accepts the keypoint at exactly hx - 4; in exact arithmetic H p has cx = hx + d with d about one
    float32 step, so the box [cx - 4, cx + 4] ends d to the right of that keypoint.  The searched image's box is
    [256, 1280] (16-pixel cells, boundaries at multiples of 16) and every p is searched for such that hx - 4 is the
    last float32 below a cell boundary B: the keypoint is in the cell left of B, the exact box's edge rounds to B.
    A candidate region without slack starts listing at the cell of B and drops the accepted keypoint."""
    f = np.float32
    m = SLIVER_H.reshape(9).astype(f)
    md = m.astype(np.float64)
    pts, twins, found = [], [], []
    for b in (528.0, 592.0, 656.0, 752.0, 848.0, 1008.0):
        hx_want = f(b + 4.0 - SLIVER_ULP)
        y1 = (f(300.0) + f(0.37) * np.arange(400, dtype=f))[:, None]
        x_mid = ((np.float64(hx_want) - md[1] * y1 - md[2]) / md[0]).astype(f)
        x1 = x_mid
        for _ in range(8):
            x1 = np.nextafter(x1, f(-np.inf))
        cols = [x1]
        for _ in range(16):
            cols.append(np.nextafter(cols[-1], f(np.inf)))
        x1 = np.concatenate(cols, axis=1)
        y1 = np.broadcast_to(y1, x1.shape)
        hx = (m[0] * x1 + m[1] * y1) + m[2] * f(1.0)
        d = (md[0] * x1.astype(np.float64) + md[1] * y1.astype(np.float64) + md[2]) - hx.astype(np.float64)
        hit = np.argwhere((hx == hx_want) & (d >= 0.8 * SLIVER_ULP) & (d <= 1.2 * SLIVER_ULP))
        assert len(hit), b
        i, j = hit[0]
        p = np.array([x1[i, j], y1[i, j]], f)
        hy = (m[3] * p[0] + m[4] * p[1]) + m[5] * f(1.0)
        pts.append(p)
        twins += [[f(hx_want - f(4.0)) - f(SLIVER_ULP), hy], [hx_want - f(4.0), hy]]      # rejected, accepted
        found.append(dict(boundary=b, d=float(d[i, j])))
    n = len(pts)
    d1 = descs(650, n + 2)
    d2 = np.concatenate([np.repeat(d1[:n], 2, axis=0), descs(651, 2)])
    kp1 = np.concatenate([np.array(pts, np.float64), [[200.0, 200.0], [1300.0, 600.0]]])
    kp2 = np.concatenate([np.array(twins, np.float64), [[256.0, 100.0], [1280.0, 740.0]]])
    return case([image(d1, kp1), image(d2, kp2)], [(0, 1)], [(4, SLIVER_H)], 4.0, [True],
                [dict(kind="sliver", pair=0, points=n, found=found)])


# ---- family 6: grid and dense pairs in one call ------------------------------------------------------------------------
MIXED_ROWS = 128        # every image: one kRowPad (256) of the batch budget each, so AMC_MATCH_BATCH_ENTRIES counts pairs


def mixed_cases(cases):
    rng = np.random.default_rng(700)
    land_xy = rng.uniform([100, 100], [1500, 1100], size=(MIXED_ROWS, 2))
    land_d = descs(701, MIXED_ROWS)
    imgs, shifts = [], []
    for k in range(4):
        t = np.array([9.0 * k, 4.0 * k])
        order = rng.permutation(MIXED_ROWS)
        imgs.append(image(land_d[order], land_xy[order] + t + rng.uniform(-1, 1, size=(MIXED_ROWS, 2))))
        shifts.append(t)
    far = imgs[3]["keypoints"].astype(np.float64)
    far[0] = [1e7 + 1, 500.0]                     # image 4: image 3 with one keypoint past the coordinate limit
    imgs.append(image(imgs[3]["descriptors"], far))
    e = np.array([-2500.0, 300.0, 1.0])
    pairs, models, grid = [], [], []

    def add(a, b, kind, is_grid):
        hm = translation(*(shifts[min(b, 3)] - shifts[min(a, 3)]))
        fm = cross_matrix(e) @ hm
        pairs.append((a, b))
        # "scaled": the same homography times 1e13 - the same filter verdicts, but past the setup's limit on a model's
        # magnitude; "horizon": w changes sign inside image 1 (the one pair here without matches)
        models.append({"H": (4, hm), "F": (3, fm / np.abs(fm).max()), "scaled": (6, hm * 1e13), "horizon": (5, H_HORIZON)}[kind])
        grid.append(is_grid)

    add(0, 1, "H", True)
    add(0, 2, "scaled", False)
    add(1, 2, "F", True)
    add(1, 4, "H", False)
    add(2, 3, "H", True)
    add(3, 0, "horizon", False)
    add(2, 0, "F", True)
    add(4, 1, "F", False)
    cases["mixed/interleaved"] = case(imgs, pairs, models, 4.0, grid, [dict(kind="mixed", grid=4, dense=4, empty=[5])])


MIXED_ORDER = (5, 2, 7, 0, 3, 6, 1, 4)          # the second order of mixed/interleaved's pairs
MIXED_BATCH_ENTRIES = {"two": 7 * 256, "one_per_pair": 1}   # 8 pairs x 256 padded rows: 7 + 1 pairs, 1 pair per batch


def reordered(c, order):
    order = np.asarray(order)
    out = dict(c)
    out["pairs"] = (c["pairs"][0][order], c["pairs"][1][order])
    out["tvg"] = c["tvg"][order]
    out["grid"] = [c["grid"][k] for k in order]
    return out


@functools.lru_cache(maxsize=None)
def build_cases():
    cases = {}
    staging_cases(cases)
    tie_cases(cases)
    row_block_cases(cases)
    geometry_cases(cases)
    boundary_cases(cases)
    mixed_cases(cases)
    for c in cases.values():
        for im in c["images"]:
            assert len(im["keypoints"]) <= 1100
            im["descriptors"].setflags(write=False)
            im["keypoints"].setflags(write=False)
    return cases
