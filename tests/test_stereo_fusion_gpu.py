"""GPU parity of stereo fusion (include/amc_fusion.h, csrc/fusion.hip): the library against the
sequential CPU reference (tests/fusion_ref) and the frozen fixture, bit for bit, on the smallest shapes at which the kernel
can go wrong (tests/fusion_cases.py): image, neighbour and seed counts at the lane edges, cluster sizes at the bounds,
traversal depths, the three tests on their thresholds, bad values, claims; independence of the launch size and dependence
on the image order exactly as the reference says; refused input; and StereoFusion at the end of the dense walk against
the same walk with the references in the library's place."""
from pathlib import Path

import numpy as np
import pytest

import fusion_cases as fc
import fusion_ref_lib as ref
import patchmatch_cases as pc
import patchmatch_ref_lib as pmref
import pycolmap_amd as pycolmap
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "fusion_ref_v1.npz"
CASES = fc.build_cases()


@pytest.fixture(scope="module")
def ctx():
    with _capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def references():
    """every case's reference result, computed once"""
    return {name: ref.fuse_depth_maps(*args, **opts) for name, (args, opts) in CASES.items()}


def launches(args, want, batch):
    """23.6 restated: per image with maps the seed launch; per `batch` of a step's seeds a cluster launch and, when it
    gave a point, a gather launch.  Returns (cluster launches, all launches)."""
    images, dm = args[0], args[4]
    clusters = total = 0
    counted = 0
    for i in range(len(images)):
        if dm[i] is None:
            continue
        total += 1
        # the step's seeds in order: the reference does not report them per step, so count them from its clusters
        seeds = want["seeds_per_step"][i]
        points = want["point_seed_rank"][i]  # of each point of the step, the rank of its seed among the step's seeds
        for s0 in range(0, seeds, batch):
            clusters += 1
            total += 1 + (1 if any(s0 <= r < s0 + batch for r in points) else 0)
        counted += seeds
    assert counted == want["num_seeds"]
    return clusters, total


def seed_ranks(args, opts):
    """per step the seeds and, per point, its seed's rank among them, from the reference's trace-free result: a run
    with min_num_pixels = 0 and no box gives a point per seed"""
    every = ref.fuse_depth_maps(*args, **dict(opts, min_num_pixels=0, bounding_box=_capi.FUSION_DEFAULTS["bounding_box"]))
    some = ref.fuse_depth_maps(*args, **opts)
    n = len(args[0])
    per_step = [int(np.sum(every["seed_image"] == i)) for i in range(n)]
    finite = every["num_points"] == every["num_seeds"]
    ranks = [[] for _ in range(n)]
    if finite:
        for i in range(n):
            order = {int(p): k for k, p in enumerate(every["seed_pixel"][every["seed_image"] == i])}
            ranks[i] = [order[int(p)] for p in some["seed_pixel"][some["seed_image"] == i]]
    return dict(some, seeds_per_step=per_step, point_seed_rank=ranks), finite


# ---- every case ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_reference_and_fixture(name, ctx, golden, references):
    args, opts = CASES[name]
    got = ctx.fuse_depth_maps(*args, **opts)
    want = references[name]
    assert fc.same(got, want), name
    assert fc.result_digest(got) == str(golden[f"digest/{name}"])
    assert got["device_ms"] >= got["kernel_ms"] > 0 and got["device_ms"] >= got["copy_ms"] > 0 and got["host_ms"] >= got["alloc_ms"] >= 0
    assert not np.isnan(got["xyz"]).any() and not np.isnan(got["normal"]).any()
    if name == "rendered_slanted":
        for key in ("xyz", "normal", "color", "vis_offsets", "vis_images"):
            assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(golden[f"rendered_slanted/{key}"]).tobytes()
    if name.startswith("images_"):
        n = int(name.split("_")[1])
        assert got["num_points"] == 2 and list(got["num_fused"]) == [n, n] and list(got["vis_images"][:n]) == list(range(n))
    if name.startswith("cluster_"):
        n = int(name.split("_")[1])
        assert got["num_fused"][0] == min(n, fc.MAX_CLUSTER)
        assert got["num_truncated"] == (1 if n > fc.MAX_CLUSTER and "bound" not in name else 0)
    if name.startswith("chain_depth_"):
        assert got["num_fused"][0] == int(name.split("_")[2])
    if name in ("box_drops_everything", "min_num_pixels_4_of_3"):
        assert got["num_points"] == 0 and got["num_seeds"] > 0
    if name == "seeds_0":
        assert not (got["seed_image"] == 0).any() and got["num_seeds"] == 6


@pytest.mark.parametrize("name", ["depth_on", "depth_beyond", "normal_on", "normal_beyond", "reproj_on", "reproj_beyond"])
def test_thresholds_to_the_float(name, ctx, golden):
    args, opts, (spix, image, row, col), taken = fc.threshold_cases(ref)[name]
    got = ctx.fuse_depth_maps(*args, **opts)
    want = ref.fuse_depth_maps(*args, trace=True, **opts)
    assert fc.same(got, want) and fc.result_digest(got) == str(golden[f"digest/threshold_{name}"])
    line = [ln for ln in want["trace"] if want["seed_pixel"][ln[0]] == spix and want["seed_image"][ln[0]] == 0 and ln[1] == 0
            and tuple(ln[2:5]) == (image, row, col)]
    assert len(line) == 1 and (ref.REASONS[line[0][5]] == "taken") == taken


# ---- launch sizes and order -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 64])
def test_the_result_does_not_depend_on_the_launch_size(batch, ctx, monkeypatch, references):
    monkeypatch.setenv("AMC_FUSION_BATCH_SEEDS", str(batch))
    for name in sorted(CASES):
        args, opts = CASES[name]
        got = ctx.fuse_depth_maps(*args, **opts)
        assert fc.same(got, references[name]), (name, batch)
        want, exact = seed_ranks(args, opts)
        if exact:  # (a seed that is not finite gives no point even with every gate open: its rank is not known here)
            assert (got["num_batches"], got["num_launches"]) == launches(args, want, batch), (name, batch)


def test_default_launch_counts(ctx):
    args, opts = CASES["shape_257x1"]
    got = ctx.fuse_depth_maps(*args, **opts)
    assert got["num_seeds"] == 257 and got["num_batches"] == 1 and got["num_launches"] == 2 + 1 + 1  # image 1 has no seeds left


def test_reordering_changes_the_result_as_the_reference_says(ctx, references):
    base = references["rendered_slanted"]
    for name in ("reordered_210", "reordered_120"):
        got = ctx.fuse_depth_maps(*CASES[name][0], **CASES[name][1])
        assert fc.same(got, references[name]) and not fc.same(got, base)


# ---- empty and refused input ------------------------------------------------------------------------------------------------------
def test_a_call_without_images_touches_no_device(ctx):
    got = ctx.fuse_depth_maps([], np.zeros((0, 4)), np.zeros((0, 3, 3)), np.zeros((0, 3)), [], [], [])
    assert got["num_points"] == 0 and got["num_launches"] == 0 and got["device_ms"] == 0 and list(got["vis_offsets"]) == [0]


def test_refused_input(ctx):
    good = fc.stack(3)
    far = fc.stack(3, neighbours=[[3], [], []])
    for args, opts, text in [(far, {}, "out of range"), (good, dict(max_traversal_depth=129), "max_traversal_depth"),
                             (good, dict(max_traversal_depth=0), "max_traversal_depth"), (good, dict(max_num_pixels=0), "max_num_pixels"),
                             (good, dict(min_num_pixels=-1), "min_num_pixels"), (good, dict(min_num_pixels=7, max_num_pixels=6), "max_num_pixels"),
                             (good, dict(max_depth_error=-1.0), "error bound"), (good, dict(max_normal_error=np.nan), "error bound")]:
        with pytest.raises(_capi.AmcError, match=text) as e:
            ctx.fuse_depth_maps(*args, **opts)
        assert e.value.code == _capi.AMC_E_INVALID
    with pytest.raises(ValueError, match="65 neighbours, more than 64"):
        ctx.fuse_depth_maps(*fc.stack(2, neighbours=[[1] * 65, []]))


# ---- the end of the dense walk ----------------------------------------------------------------------------------------------------
class ReferenceContext:
    """the CPU references in the library's place; the angles of __auto__ still come from the device"""

    def __init__(self, device):
        self.ctx = _capi.Context(device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def shared_point_angles(self, *a, **k):
        return self.ctx.shared_point_angles(*a, **k)

    def patch_match(self, *a, **k):
        return pmref.patch_match(*a, **k)

    def fuse_depth_maps(self, *a, **k):
        return ref.fuse_depth_maps(*a, **k)


def tree(path):
    return {str(p.relative_to(path)): p.read_bytes() for p in sorted(Path(path).rglob("*")) if p.is_file()}


def test_undistort_patch_match_fusion_equals_the_walk_with_the_references(tmp_path):
    sc = pc.scene("fronto", 4, 64, 48)
    src = tmp_path / "src"
    pc.write_workspace(str(src), sc, "")
    outs = {}
    for kind in ("gpu", "ref"):
        ws = tmp_path / kind
        pycolmap.undistort_images(str(ws), str(src / "sparse"), str(src / "images"))
        pm = pycolmap.PatchMatchController(dict(num_iterations=1, window_radius=2, filter_min_num_consistent=1), str(ws))
        fu = pycolmap.StereoFusion(dict(min_num_pixels=2, max_reproj_error=2.0, max_depth_error=0.05, max_normal_error=30.0), str(ws))
        if kind == "ref":
            pm._context_factory = fu._context_factory = ReferenceContext
        pm.run()
        before = tree(ws)
        fu.run()
        assert tree(ws) == before  # run() writes nothing
        (ws / "fused").mkdir()
        fu.write(str(ws / "fused"))
        fu.write(str(ws / "fused.ply"))
        outs[kind] = (fu, tree(ws))
    (g, gt), (r, rt) = outs["gpu"], outs["ref"]
    assert gt == rt
    assert g.fused_points.tobytes() == r.fused_points.tobytes() and len(g.fused_points) > 100
    assert [list(v) for v in g.fused_points_visibility] == [list(v) for v in r.fused_points_visibility]
    assert g.summary["kernel_ms"] > 0 and g.summary["num_points"] == len(g.fused_points)
    assert pycolmap.last_run_stats()["num_points"] == len(r.fused_points)
    assert {"fused.ply", "fused.ply.vis", "fused/points3D.bin"} <= set(gt)
