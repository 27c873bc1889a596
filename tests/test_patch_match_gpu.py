"""GPU parity of PatchMatch stereo (include/amc_patchmatch.h, csrc/patchmatch.hip): the library against
the sequential CPU reference (tests/patchmatch_ref) and the frozen fixture, bit for bit, on the smallest shapes at which
the kernels can go wrong (tests/patchmatch_cases.py): initial costs, full passes, lane and line edges, degenerate input;
independence of how the problems are spread over calls and launches; refused input; and PatchMatchController on a
workspace against the same walk with the reference in the library's place."""
import os
from pathlib import Path

import numpy as np
import pytest

import patchmatch_cases as pc
import patchmatch_ref_lib as ref
import pycolmap_amd as pycolmap
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "patchmatch_ref_v1.npz"
CASES = pc.build_cases()
KEYS = ("depth", "normal", "num_consistent", "costs")


@pytest.fixture(scope="module")
def ctx():
    with _capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    """every array of two results, bit for bit"""
    for key in KEYS:
        g, w = got.get(key), want.get(key)
        if (g is None) != (w is None) or (g is not None and len(g) != len(w)):
            return False
        for x, y in zip(g or [], w or []):
            if x.shape != y.shape or not np.array_equal(bits(x), bits(y)):
                return False
    return True


def launches(options, batches):
    """22.8 restated: per batch the initialisation, four sweeps per iteration, the final costs when the filter or the
    caller wants them, the filter"""
    o = dict(_capi.PATCHMATCH_DEFAULTS, **options)
    return batches * (1 + 4 * o["num_iterations"] + (1 if o["filter"] or o["want_costs"] else 0) + (1 if o["filter"] else 0))


# ---- every case: initial costs, full passes, lane and line edges, degenerate input ----------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_reference_and_fixture(name, ctx, golden):
    pb, opts = CASES[name]
    got = ctx.patch_match(**pb, **opts)
    assert same(got, ref.patch_match(**pb, **opts)), name
    assert pc.result_digest(got) == str(golden[f"digest/{name}"])
    assert got["num_batches"] == 1 and got["num_launches"] == launches(opts, 1)
    assert got["device_ms"] >= got["kernel_ms"] > 0 and got["device_ms"] >= got["copy_ms"] > 0 and got["host_ms"] >= got["alloc_ms"] >= 0
    if name == "photometric":
        assert np.array_equal(bits(got["depth"][0]), bits(golden["photometric/depth"]))
    if name == "constant_image":  # every cost is the maximum
        assert np.all(got["costs"][0] == 2.0) and not got["depth"][0].any()
    if name == "filter_keeps_nothing":
        assert not got["depth"][0].any() and not got["normal"][0].any()
    if name == "filter_keeps_everything":
        assert np.all(got["depth"][0] > 0)
    if name == "depth_min_equals_max":
        assert np.all(got["depth"][0] == 5.0)


def test_geometric_pass_from_the_photometric_fixture(ctx, golden):
    sc, pb = pc.two_stage_problem()
    ph = ctx.patch_match(**pb, **pc.TWO_STAGE["photometric"])
    assert np.array_equal(bits(np.stack(ph["depth"])), bits(golden["two_stage/photometric_depth"]))
    assert np.array_equal(bits(np.stack(ph["normal"])), bits(golden["two_stage/photometric_normal"]))
    maps = dict(in_depth=list(golden["two_stage/photometric_depth"]), in_normal=list(golden["two_stage/photometric_normal"]))
    got = ctx.patch_match(**pb, **maps, **pc.TWO_STAGE["geometric"])
    assert same(got, ref.patch_match(**pb, **maps, **pc.TWO_STAGE["geometric"]))
    assert pc.result_digest(got) == str(golden["digest/two_stage_geometric"])
    assert any(d.any() for d in got["depth"]) and not all(d.all() for d in got["depth"])  # the filter keeps some, not all


# ---- independence from the spreading of the work ----------------------------------------------------------------------------
OPTS = dict(pc.QUICK, filter=1, filter_min_num_consistent=1, want_costs=1)


def nine_problems():
    sc = pc.scene("slanted", 4, *pc.SMALL)
    refs = [0, 1, 2, 3, 0, 1, 2, 3, 0]
    srcs = [[j for j in range(4) if j != r][: 1 + k % 3] for k, r in enumerate(refs)]
    return sc, refs, srcs


@pytest.fixture(scope="module")
def singles(ctx):
    sc, refs, srcs = nine_problems()
    return [ctx.patch_match(**pc.problem(sc, refs=[r], sources=[s]), **OPTS) for r, s in zip(refs, srcs)]


@pytest.mark.parametrize("order", [[0], [3, 7], list(range(9)), [8, 2, 5, 0, 7, 1, 6, 4, 3]])
def test_a_call_of_many_problems_equals_the_single_calls(order, ctx, singles):
    sc, refs, srcs = nine_problems()
    got = ctx.patch_match(**pc.problem(sc, refs=[refs[k] for k in order], sources=[srcs[k] for k in order]), **OPTS)
    for at, k in enumerate(order):
        for key in KEYS:
            assert np.array_equal(bits(got[key][at]), bits(singles[k][key][0])), (key, k)


def test_the_result_does_not_depend_on_the_batch_bound(ctx, monkeypatch):
    sc, refs, srcs = nine_problems()
    pb = pc.problem(sc, refs=refs[:3], sources=[srcs[0], srcs[0], srcs[0]])  # three problems of one source each
    state = pc.SMALL[0] * pc.SMALL[1] * (16 + 4 * 1)  # 22.8: the state bytes of one of them
    whole = ctx.patch_match(**pb, **OPTS)
    assert whole["num_batches"] == 1
    for bound, batches in ((1, 3), (2 * state, 2), (2 * state - 1, 3), (3 * state, 1)):
        monkeypatch.setenv("AMC_PATCHMATCH_BATCH_BYTES", str(bound))
        got = ctx.patch_match(**pb, **OPTS)
        assert got["num_batches"] == batches and got["num_launches"] == launches(OPTS, batches), bound
        assert same(got, whole), bound


def test_a_call_without_problems_touches_no_device(ctx):
    sc = pc.scene("fronto", 2, 4, 3)
    got = ctx.patch_match(**pc.problem(sc, refs=[], sources=[]))
    assert got["depth"] == [] and got["num_batches"] == 0 and got["num_launches"] == 0 and got["device_ms"] == 0


def test_refused_input(ctx):
    sc = pc.scene("fronto", 2, 4, 3)
    good = pc.problem(sc)
    many = pc.problem(sc, sources=[[1] * (_capi.PATCHMATCH_MAX_SOURCES + 1)])
    for pb, opts, text in [(many, {}, "33 sources"), (pc.problem(sc, sources=[[]]), {}, "0 sources"),
                           (dict(good, depth_ranges=np.array([[0.0, 5.0]])), {}, "depth range"),
                           (dict(good, depth_ranges=np.array([[6.0, 5.0]])), {}, "depth range"),
                           (dict(good, depth_ranges=np.array([[np.nan, 5.0]])), {}, "depth range"),
                           (dict(good, src_images=np.array([2], np.uint32)), {}, "out of range"),
                           (good, dict(window_radius=33), "window_radius"), (good, dict(window_step=0), "window_step"),
                           (good, dict(num_samples=0), "num_samples"), (good, dict(ncc_sigma=0.0), "sigma")]:
        with pytest.raises(_capi.AmcError, match=text) as e:
            ctx.patch_match(**pb, **opts)
        assert e.value.code == _capi.AMC_E_INVALID


# ---- the controller -----------------------------------------------------------------------------------------------------------
class ReferenceContext:
    """the CPU reference in the library's place; the angles of __auto__ still come from the device"""

    def __init__(self, device):
        self.ctx = _capi.Context(device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def shared_point_angles(self, *a, **k):
        return self.ctx.shared_point_angles(*a, **k)

    def patch_match(self, *a, **k):
        return ref.patch_match(*a, **k)


CONFIG = "im0.pgm\n__auto__, 2\nim1.pgm\n__all__\n# a comment\nim2.pgm\nim0.pgm, im3.pgm\n"
CONTROLLER_OPTIONS = dict(num_iterations=1, window_radius=2, filter_min_num_consistent=1)


def tree(path):
    return {str(p.relative_to(path)): p.read_bytes() for p in sorted(Path(path).rglob("*")) if p.is_file()}


def test_controller_equals_the_walk_with_the_reference(tmp_path):
    sc = pc.scene("fronto", 4, 24, 18)
    for sub in ("gpu", "ref"):
        pc.write_workspace(str(tmp_path / sub), sc, CONFIG)
    before = tree(tmp_path / "gpu")
    c = pycolmap.PatchMatchController(CONTROLLER_OPTIONS, str(tmp_path / "gpu"))
    c.run()
    r = pycolmap.PatchMatchController(pycolmap.PatchMatchOptions(CONTROLLER_OPTIONS), str(tmp_path / "ref"))
    r._context_factory = ReferenceContext
    r.run()
    after, want = tree(tmp_path / "gpu"), tree(tmp_path / "ref")
    assert after == want
    new = sorted(set(after) - set(before))
    assert new == sorted(f"stereo/{kind}_maps/im{i}.pgm.{stage}.bin" for kind in ("depth", "normal") for i in range(3)
                         for stage in ("photometric", "geometric"))
    assert all(after[k] == before[k] for k in before)
    assert c.summary["problems_run"] == 6 and c.summary["problems_skipped"] == 0 and c.summary["kernel_ms"] > 0
    assert c.summary["bytes_written"] == sum(len(after[k]) for k in new)
    assert pycolmap.last_run_stats()["problems_run"] == 6
    depth = pycolmap.read_array(tmp_path / "gpu" / "stereo" / "depth_maps" / "im0.pgm.photometric.bin")
    assert depth.shape == (18, 24) and np.all((depth >= 0.75 * 4.9) & (depth <= 1.25 * 5.1))  # the points' range, widened
    # a second run writes nothing
    stamps = {k: os.stat(tmp_path / "gpu" / k).st_mtime_ns for k in after}
    c.run()
    assert c.summary["problems_run"] == 0 and c.summary["problems_skipped"] == 6 and c.summary["bytes_written"] == 0
    assert tree(tmp_path / "gpu") == after and stamps == {k: os.stat(tmp_path / "gpu" / k).st_mtime_ns for k in after}


@pytest.mark.parametrize("options, kwargs, text", [
    ({}, dict(workspace_format="PMVS"), "workspace_format"),
    (dict(write_consistency_graph=True), {}, "write_consistency_graph"),
    (dict(gpu_index="0,1"), {}, "gpu_index"),
    (dict(max_image_size=16), {}, "max_image_size"),
    (dict(window_step=3), {}, "Check Failed: window_step <= 2"),
])
def test_controller_refusals_leave_the_folder_untouched(options, kwargs, text, tmp_path):
    pc.write_workspace(str(tmp_path), pc.scene("fronto", 3, 24, 18), "im0.pgm\n__all__\n")
    before = tree(tmp_path)
    with pytest.raises(ValueError, match=text):
        pycolmap.PatchMatchController(options, str(tmp_path), **kwargs).run()
    assert tree(tmp_path) == before


def test_controller_refuses_a_camera_that_is_not_pinhole_and_a_bad_config(tmp_path):
    sc = pc.scene("fronto", 3, 24, 18)
    pc.write_workspace(str(tmp_path), sc, "im0.pgm\nim0.pgm\n")
    before = tree(tmp_path)
    with pytest.raises(ValueError, match="lists itself"):
        pycolmap.PatchMatchController({}, str(tmp_path)).run()
    assert tree(tmp_path) == before
    rec = pycolmap.Reconstruction()
    rec.read(str(tmp_path / "sparse"))
    cam = rec.cameras[1]
    rec.cameras[1] = pycolmap.Camera("SIMPLE_RADIAL", cam.width, cam.height, [26.0, 12.0, 9.0, 0.01], 1)
    rec.write(str(tmp_path / "sparse"))
    before = tree(tmp_path)
    with pytest.raises(ValueError, match="PINHOLE"):
        pycolmap.PatchMatchController({}, str(tmp_path)).run()
    assert tree(tmp_path) == before
