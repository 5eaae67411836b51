"""GPU: the book-3 MIS integrator (shade_b3, lights_pdf, lights_random; kernel class 4) against the oracle on
the scenes of tests/book3_scenes.py: five lights of both kinds with an inexact 1 / n, an emissive sphere
that is sampled, a light seen from behind, media under book 3 (the Isotropic branch), a Perlin material,
a far light sphere (cos_max == 1), a list of one sphere, and hit points inside a light sphere, whose NaN
the kernel must carry through the sample sums, the chunk sums and the quantisers as the reference does.

Every frame is held bit for bit to the oracle's walk of the tree the scene holds (KBVH) and to the oracle's
own tree (TWIN) with equal ray and path counts, in both placements and through both entries.
tests/test_book3_scenes.py checks on the CPU that the scenes are what this file assumes.
"""
import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle

import book3_scenes as B
from test_book2_class_scenes import PLACEMENT_IDS, PLACEMENTS, place
from test_book3_scenes import check_class4, kbvh, twin
from test_gpu_device_bvh import gpu_render_with_rays
from test_gpu_parity import _torch, assert_bit_exact, gpu_tile

pytestmark = pytest.mark.gpu

SEED = B.FIELD_SEED["inside_light"]
CHUNKED = ("inside_light", SEED, 81, 24)  # 81 spp: chunks of 64, 16 and 1 samples (rrt_accum_chunk)


def assert_frames_equal(gpu, ref, spp, rays=None, ref_rays=None):
    """assert_bit_exact for frames with NaN sums: the same channels are NaN, every other channel has the
    same bits, w is the sample count on both sides, and the ray counts (when given) are equal."""
    ref32, finite = ref.astype(np.float32), ~np.isnan(ref)
    assert np.array_equal(np.isnan(ref32), ~finite), "oracle sums must be exact f32"
    assert np.array_equal(ref32.astype(np.float64)[finite], ref[finite]), "oracle sums must be exact f32"
    gn, rn = np.isnan(gpu), np.isnan(ref32)
    assert np.array_equal(gn, rn), f"NaN channels differ: {int(gn.sum())} on the GPU, {int(rn.sum())} in the oracle"
    assert not gn[..., 3].any() and np.array_equal(gpu[..., 3], ref32[..., 3]) and np.all(gpu[..., 3] == spp)
    same = gpu.view(np.uint32)[~gn] == ref32.view(np.uint32)[~rn]
    assert same.all(), f"{int((~same).sum())} finite channels differ"
    if rays is not None:
        assert rays == ref_rays


def _tile_and_compare(in_lds, name, *args):
    """One tile render with counters and the counting twin against KBVH and TWIN; returns the frame."""
    scene = B.built(in_lds, name, *args)[0]
    gpu, idx, ctr, work = gpu_tile(scene, count=True)
    assert len(idx) == scene.height
    ref, krays = kbvh(in_lds, name, *args)
    tw, trays = twin(name, *args)
    if name == "inside_light":
        assert_frames_equal(gpu, ref, scene.spp, ctr["rays"], krays)
        assert_frames_equal(gpu, tw, scene.spp, ctr["rays"], trays)
    else:
        assert_bit_exact(gpu, ref, scene.spp)
        assert_bit_exact(gpu, tw, scene.spp)
        assert np.all(gpu[..., 3] == scene.spp)
    assert ctr["rays"] == krays == trays == work["rays"]
    assert ctr["paths"] == work["paths"] == scene.width * scene.height * scene.spp
    return gpu


# ---- every scene, both placements, both entries ------------------------------------------------------
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("name", B.SCENES)
def test_scenes(monkeypatch, name, in_lds):
    place(monkeypatch, in_lds)
    scene, _, order, info = B.built(in_lds, name)
    check_class4(scene, info, order, in_lds)
    tile = _tile_and_compare(in_lds, name)
    one_shot = rrt.render(scene)
    assert np.array_equal(one_shot.view(np.uint32), tile.view(np.uint32))  # NaN sums included, bit for bit
    if name == "inside_light":
        n = int(B.nan_mask(tile).sum())
        assert 20 <= n <= scene.width * scene.height // 10
    else:
        assert np.isfinite(tile).all()
    if name == "multi_light_noise":  # the Perlin tables left in global memory: the same frame
        place(monkeypatch, in_lds, "0")
        check_class4(scene, info, order, in_lds, "0")
        assert np.array_equal(_tile_and_compare(in_lds, name), tile)


# ---- NaN sums through the quantisers and the chunk sums -----------------------------------------------
def test_quantisers_on_nan_sums(monkeypatch):
    """render_io.rs sends a non-finite mean to 0; color.rs's write_color has no such test and takes a NaN
    through its own sqrt, clamp and cast. Device bytes equal the host quantisers' on the oracle's frame."""
    place(monkeypatch, None)
    scene = B.built(None, "inside_light")[0]
    ref = twin("inside_light")[0].astype(np.float32)
    nan_px = B.nan_mask(ref)
    assert nan_px.sum() >= 20
    want = rrt.quantize_accum(scene.width, scene.height, ref, scene.spp)
    assert np.array_equal(want.reshape(-1, 3), oracle.quantize_render_io(ref, scene.spp))
    got = rrt.render_rgb8(scene)
    assert np.array_equal(got, want)
    assert (got[np.isnan(ref[..., :3])] == 0).all()
    torch = _torch()
    n_px = scene.width * scene.height
    d_acc = torch.from_numpy(rrt.render(scene)).to("cuda:0")
    d_rgb = torch.zeros(3 * n_px, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rrt.quantize_accum_books_async(n_px, d_acc.data_ptr(), scene.spp, d_rgb.data_ptr(), stream)
    torch.cuda.synchronize()
    books = rrt.quantize_accum_books(scene.width, scene.height, ref, scene.spp)
    assert np.array_equal(d_rgb.cpu().numpy().reshape(books.shape), books)


@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
def test_nan_crosses_the_chunk_sums(monkeypatch, in_lds):
    """81 spp: three accumulation chunks, so a NaN sample sum goes through rrt_combine_chunks. (The
    24 x 24 frame's partial sums are 21 KB: RRT_PARTIAL_MB=1 would not split it into passes.)"""
    place(monkeypatch, in_lds)
    gpu = _tile_and_compare(in_lds, *CHUNKED)
    n = int(B.nan_mask(gpu).sum())
    assert 20 <= n < gpu.shape[0] * gpu.shape[1]
    assert np.array_equal(rrt.render(B.built(in_lds, *CHUNKED)[0]).view(np.uint32), gpu.view(np.uint32))


# ---- the device-built tree ------------------------------------------------------------------------------
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
def test_device_built_tree(monkeypatch, in_lds):
    place(monkeypatch, in_lds)
    scene = B.multi_light()
    gpu, rays, (nodes, order, info) = gpu_render_with_rays(scene)
    check_class4(scene, info, order, in_lds)
    ref, krays, _ = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    assert_bit_exact(gpu, ref, scene.spp)
    tw, trays = twin("multi_light")
    assert_bit_exact(gpu, tw, scene.spp)
    assert rays == krays == trays and np.all(gpu[..., 3] == scene.spp)


# ---- sample-range tiles under stratification ------------------------------------------------------------
def test_sample_range_tiles(monkeypatch):
    """Sample s of a pixel is stratum (s % sqrt_spp, s / sqrt_spp): a tile of samples [s0, s1) renders those
    strata alone."""
    place(monkeypatch, None)
    scene = B.built(None, "multi_light", B.FIELD_SEED["multi_light"], 16)[0]
    assert scene.spp == 16
    for s0, s1 in ((0, 16), (5, 13), (15, 16), (3, 3)):
        gpu, _, ctr, _ = gpu_tile(scene, s0=s0, s1=s1)
        ref, rays, _ = oracle.render(scene, oracle.TWIN, samples=(s0, s1), threads=16)
        assert_bit_exact(gpu, ref, s1 - s0)
        assert np.all(gpu[..., 3] == s1 - s0) and ctr["rays"] == rays
        assert ctr["paths"] == scene.width * scene.height * (s1 - s0)
    with pytest.raises(rrt.RrtError, match="sample_end exceeds"):
        gpu_tile(scene, s0=0, s1=17)


@pytest.mark.parametrize("spp,eff", [(1, 1), (10, 9)])
def test_sqrt_spp_edges(monkeypatch, spp, eff):
    """sqrt_spp = 1, and 10 samples rounded down to 3 x 3."""
    place(monkeypatch, None)
    args = ("multi_light", B.FIELD_SEED["multi_light"], spp)
    assert B.built(None, *args)[0].spp == eff
    _tile_and_compare(None, *args)
