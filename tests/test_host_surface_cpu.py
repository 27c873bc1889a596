"""The binding layer's contract without a GPU: the Python-visible surface of pycolmap_amd._pycolmap against its frozen
digests, what the entry points that go to the library do when there is no device, and the scope guard that frees the
library's result structs, in a stand-alone program under ASan + UBSan."""
import copy
import json
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ba_cases
import host_surface
import pycolmap_amd as pc
import triangulator_cases as tc
from pycolmap_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "host_surface_v1.json"


def test_surface_reproduces_fixture():
    want = json.loads(GOLDEN.read_text())
    got = host_surface.host_surface()
    differing = sorted(n for n in set(want) | set(got) if want.get(n) != got.get(n))
    assert not differing, f"surface changed for: {differing} (missing: {sorted(set(want) - set(got))}, new: {sorted(set(got) - set(want))})"
    assert list(got) == sorted(got) and len(got) == len(want) > 90  # every class, function and constant of the module


def test_without_a_gpu_triangulate_image_raises_and_leaves_the_model():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the CPU-only container")
    sc = tc.scene(seed=9, nimg=5, npts=6, views=(4, 5), wrong=1)  # the smallest scene of triangulator_cases
    r, g = tc.reconstruction(sc)
    image_id = next(iter(sc["images"]))
    # the call plans at least one item: with the reference in the library's place, on a copy
    trial = pc.IncrementalTriangulator(g, copy.deepcopy(r))
    trial._triangulate_image_with({}, image_id, tc.reference_solver)
    assert pc.last_run_stats()["num_items"] >= 1
    t = pc.IncrementalTriangulator(g, r)
    t.add_modified_point3D(12345)  # an id the model does not hold: recorded, not reported
    before = tc.reconstruction_points(r)
    ids = {i: [p.point3D_id for p in im.points2D] for i, im in r.images.items()}
    with pytest.raises(_capi.AmcError):
        t.triangulate_image({}, image_id)
    after = tc.reconstruction_points(r)
    assert list(after) == list(before) and tc.scene_digest([], after) == tc.scene_digest([], before)
    assert {i: [p.point3D_id for p in im.points2D] for i, im in r.images.items()} == ids
    assert t.get_modified_points3D() == set()


def test_without_a_gpu_bundle_adjustment_raises_and_leaves_the_model():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the CPU-only container")
    r = ba_cases.reconstruction(ba_cases.scene(seed=1, nimg=2, npts=8, model=2, noise=0.3))
    assert r.num_images() == 2

    def state():
        return ([list(c.params) for c in r.cameras.values()],
                [(list(im.cam_from_world.rotation.quat), list(im.cam_from_world.translation), [p.point3D_id for p in im.points2D])
                 for im in r.images.values()],
                {pid: (list(p.xyz), p.error, [(e.image_id, e.point2D_idx) for e in p.track.elements]) for pid, p in r.points3D.items()})

    before = state()
    with pytest.raises(RuntimeError, match=r"^amc_ctx_create: ") as e:
        pc.bundle_adjustment(r)
    assert type(e.value) is RuntimeError  # not AmcError: the blocks that go through EstCheck raise RuntimeError
    assert state() == before


def test_result_guard_frees_once_under_asan(tmp_path):
    """The scope guard of csrc/host/result_guard.h in a stand-alone program under ASan + UBSan
    (tests/shim/result_guard_check.cc): the free function runs exactly once on a normal exit, once when an exception
    passes through the guard, and once when the struct was never filled."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "result_guard_check"
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", f"-I{ROOT / 'pycolmap_amd' / 'csrc' / 'host'}",
                        str(ROOT / "tests" / "shim" / "result_guard_check.cc"), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("sanitizer runtime not installed: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and "result guard ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
