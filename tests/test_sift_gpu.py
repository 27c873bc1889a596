"""The SIFT extractor on the GPU (libamc.so's amc_sift_extract, pycolmap_amd.Sift) against its CPU reference
(tests/sift_ref/sift_ref.cc): keypoint float bits and descriptor bytes identical, for seeded textured, noise, blob and
rendered images, every option the extractor reads, odd and tiny sizes, the kernels' tile edges, batches and repeated
runs."""
import numpy as np
import pytest

import sift_images as si
import sift_ref_lib as ref

pytestmark = pytest.mark.gpu


def assert_same(got, want, what=""):
    kp, desc = got
    wkp, wdesc = want
    assert kp.shape == wkp.shape, f"{what}: {kp.shape[0]} features, reference {wkp.shape[0]}"
    assert np.array_equal(kp.view(np.uint32), wkp.view(np.uint32)), f"{what}: keypoint bits differ"
    assert np.array_equal(desc, wdesc), f"{what}: descriptor bytes differ"


IMAGES = {
    "textured_240x320": lambda: si.textured(1, 240, 320),
    "noise_97x131": lambda: si.noise(2, 97, 131),
    "blobs_128x160": lambda: si.blobs(128, 160, [(40.3, 50.7, 3.0), (100.2, 80.4, 5.0), (60.0, 30.0, 2.0)]),
    "rendered_200x260": lambda: si.render(si.plane_texture(3, 512), si.similarity(12.0, 0.9, 5.0, -3.0, 130, 100), 200,
                                          260),
}


@pytest.mark.parametrize("name", sorted(IMAGES))
@pytest.mark.parametrize("first_octave", [-1, 0, 1])
def test_bit_exact_to_reference(amc_ctx, name, first_octave):
    img = IMAGES[name]()
    got, st = amc_ctx.sift_extract(img, first_octave=first_octave)
    want = ref.extract(img, first_octave=first_octave)
    assert_same(got, want, f"{name} first_octave={first_octave}")
    if first_octave <= 0 and name.startswith(("textured", "rendered")):
        assert len(got[0]) > 10
    assert st["device_ms"] > 0


@pytest.mark.parametrize("opts", [
    dict(upright=True),
    dict(normalization="L2"),
    dict(max_num_orientations=1),
    dict(max_num_orientations=3),
    dict(max_num_orientations=4),
    dict(max_num_features=60),
    dict(max_num_features=1),
    dict(octave_resolution=2, num_octaves=3),
    dict(peak_threshold=0.01, edge_threshold=5.0),
])
def test_options_bit_exact(amc_ctx, opts):
    img = si.textured(7, 180, 230)
    got, _ = amc_ctx.sift_extract(img, **opts)
    ropts = dict(opts)
    if ropts.get("normalization") == "L2":
        ropts["normalization"] = 1
    want = ref.extract(img, **ropts)
    assert_same(got, want, str(opts))
    if "max_num_features" in opts:
        assert len(got[0]) == opts["max_num_features"]


@pytest.mark.parametrize("shape", [(5, 7), (8, 8), (9, 33), (31, 17), (1, 40)])
def test_tiny_and_odd_sizes(amc_ctx, shape):
    img = si.noise(11, *shape)
    got, _ = amc_ctx.sift_extract(img)
    assert_same(got, ref.extract(img), str(shape))


# The kernels' tile edges, at first_octave = 0 so that the octave has exactly these sizes: the 64-pixel strip of k_vblur
# (63 .. 65), the 256-pixel segment of k_hblur and the 256-pixel chunk of k_detect over pixels 1 .. w - 2 (255 .. 259),
# two segments and one pixel (513); the 16-row tile (15 .. 18), three tiles (33), and the smallest octave that is
# processed (8, 9: deviation S3).  Every width once, every height once.
TILE_EDGE_SHAPES = [(15, 63), (16, 64), (17, 65), (18, 255), (33, 256), (8, 257), (9, 258), (15, 259), (16, 513)]


@pytest.mark.parametrize("shape", TILE_EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_edge_sizes_bit_exact(amc_ctx, shape):
    img = si.textured(60, *shape)
    got, _ = amc_ctx.sift_extract(img, first_octave=0)
    want = ref.extract(img, first_octave=0)
    assert_same(got, want, str(shape))
    assert len(want[0]) > 0
    # the same octave sizes reached through the doubling and through decimation
    half = np.ascontiguousarray(img[:(shape[0] + 1) // 2, :(shape[1] + 1) // 2])
    assert_same(amc_ctx.sift_extract(half, first_octave=-1, num_octaves=1)[0],
                ref.extract(half, first_octave=-1, num_octaves=1), f"{half.shape} doubled")


@pytest.mark.parametrize("opts", [
    dict(octave_resolution=1),              # the widest blur aprons: 45 taps each side
    dict(octave_resolution=5),
    dict(num_octaves=1),
    dict(num_octaves=8),                    # more than fit: the octaves below 8 pixels are not processed
    dict(first_octave=2),
    dict(first_octave=1, octave_resolution=1, num_octaves=2),
], ids=str)
def test_octave_options_bit_exact(amc_ctx, opts):
    img = si.textured(61, 150, 200)
    got, _ = amc_ctx.sift_extract(img, **opts)
    want = ref.extract(img, **opts)
    assert_same(got, want, str(opts))
    assert len(want[0]) > 0


@pytest.mark.parametrize("name,opts", [
    ("noise", dict(peak_threshold=0.0)),
    # white noise has few extrema across scale (its DoG shrinks with sigma); a texture with no contrast or edge test
    # keeps nearly every one: many hits per 256-pixel detection chunk, rows with hits in both chunks, keypoints whose
    # windows reach every border
    ("textured", dict(peak_threshold=0.0, edge_threshold=1e6, max_num_features=0)),
    ("textured", dict(peak_threshold=0.0, edge_threshold=1e6, max_num_features=0, octave_resolution=5)),
], ids=["noise_tp0", "textured_keep_all", "textured_keep_all_S5"])
def test_zero_peak_threshold_bit_exact(amc_ctx, name, opts):
    img = si.noise(62, 64, 300) if name == "noise" else si.textured(63, 64, 300)
    got, _ = amc_ctx.sift_extract(img, first_octave=0, **opts)
    want = ref.extract(img, first_octave=0, **opts)
    assert_same(got, want, f"{name} {opts}")
    kp = want[0]
    assert len(kp) > 0
    if name == "textured":
        assert len(kp) > 150 and (kp[:, 0] < 256).sum() > 50 and (kp[:, 0] > 258).sum() > 10
        assert kp[:, 0].min() < 8 and kp[:, 0].max() > 292 and kp[:, 1].min() < 8 and kp[:, 1].max() > 56


def test_constant_image_has_no_features(amc_ctx):
    (kp, desc), _ = amc_ctx.sift_extract(np.full((64, 80), 128, np.uint8))
    assert kp.shape == (0, 4) and desc.shape == (0, 128)


def test_batch_of_mixed_sizes_equals_single_calls(amc_ctx):
    imgs = [si.textured(20, 120, 150), si.noise(21, 61, 45), np.zeros((16, 16), np.uint8), si.textured(22, 201, 99)]
    batch, st = amc_ctx.sift_extract(imgs)
    assert len(batch) == len(imgs)
    for im, b in zip(imgs, batch):
        single, _ = amc_ctx.sift_extract(im)
        assert_same(b, single, f"{im.shape}")
    assert set(st["stage_ms"]) == {"scale_space", "detection", "orientation", "descriptors"}


def test_strided_input_equals_contiguous(amc_ctx):
    big = si.textured(30, 150, 300)
    view = big[:, 10:150]  # row pitch 300 bytes, width 140
    (kp, desc), _ = amc_ctx.sift_extract(np.ascontiguousarray(view))
    ctx_kp, ctx_desc = amc_ctx.sift_extract(view)[0]
    assert np.array_equal(kp, ctx_kp) and np.array_equal(desc, ctx_desc)


def test_two_runs_identical(amc_ctx):
    img = si.textured(40, 260, 300)
    a, _ = amc_ctx.sift_extract(img)
    b, _ = amc_ctx.sift_extract(img)
    assert_same(a, b, "rerun")


def test_larger_than_max_image_size_is_refused(amc_ctx):
    from pycolmap_amd import _capi
    with pytest.raises(_capi.AmcError):
        amc_ctx.sift_extract(np.zeros((40, 50), np.uint8), max_image_size=45)


# ---- pycolmap_amd.Sift (the host layer over the C ABI) ---------------------------------------------------------------
def test_sift_extract_uint8_and_float32():
    import pycolmap_amd as pycolmap
    img = si.textured(50, 210, 250)
    sift = pycolmap.Sift()  # {peak_threshold: 0.01, first_octave: 0, max_image_size: 7000}
    kp, desc = sift.extract(img)
    wkp, wdesc = ref.extract(img, peak_threshold=0.01, first_octave=0)
    assert kp.dtype == np.float32 and desc.dtype == np.float32 and kp.shape[1] == 4 and desc.shape[1] == 128
    assert np.array_equal(kp.view(np.uint32), wkp.view(np.uint32))
    assert np.array_equal(desc, wdesc.astype(np.float32) / 512.0)
    # float32 input: (image * 255) clamped and truncated to bytes
    f = (img.astype(np.float32) + 0.25) / 255.0
    f[0, :5] = [-1.0, 2.0, np.nan, 0.5, 1.0]
    u8 = np.nan_to_num(np.clip(f * np.float32(255.0), 0, 255), nan=0.0).astype(np.uint8)
    fkp, fdesc = sift.extract(f)
    wkp, wdesc = ref.extract(u8, peak_threshold=0.01, first_octave=0)
    assert np.array_equal(fkp.view(np.uint32), wkp.view(np.uint32))
    assert np.array_equal(fdesc, wdesc.astype(np.float32) / 512.0)
    assert sift.last_device_ms > 0


def test_sift_default_options_and_refusal():
    import pycolmap_amd as pycolmap
    sift = pycolmap.Sift(pycolmap.SiftExtractionOptions(normalization="L2", max_num_features=40, max_image_size=300))
    img = si.textured(51, 190, 230)
    kp, desc = sift.extract(img)
    wkp, wdesc = ref.extract(img, normalization=1, max_num_features=40)
    assert len(kp) == 40 and np.array_equal(kp.view(np.uint32), wkp.view(np.uint32))
    assert np.array_equal(desc, wdesc.astype(np.float32) / 512.0)
    with pytest.raises(ValueError, match="max_image_size"):
        sift.extract(np.zeros((301, 20), np.uint8))
