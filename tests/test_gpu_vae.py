"""GPU parity of the VAE decode (pytest -m gpu): C ABI (s2v_vae_*) vs the reference's golden vectors and vs the CPU
oracle on the same seeded inputs.  Tolerances: fp32 max-abs <= 1e-3 (measured ~1e-5); bf16 relative L2 <= 3e-2 against
the oracle's own bf16 run (conv stacks accumulate a few bf16 ulps per layer)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, weights_of
from oracle import vae_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(block_out_channels=(16, 16, 32, 32), layers_per_block=1, norm_num_groups=4, latent_channels=16,
            sample_height=96, sample_width=160, scaling_factor=0.7, temporal_compression_ratio=4)


def t(x, dt=torch.float32):
    return torch.from_numpy(np.asarray(x)).to(dt)


def make_vae(s2v, cfgd, dt, sd, force_simple=False):
    cfg = s2v.VAEConfig(block_out_channels=cfgd["block_out_channels"], layers_per_block=cfgd["layers_per_block"],
                        norm_num_groups=cfgd["norm_num_groups"], latent_channels=cfgd["latent_channels"],
                        sample_height=cfgd["sample_height"], sample_width=cfgd["sample_width"],
                        scaling_factor=cfgd["scaling_factor"], temporal_compression_ratio=cfgd["temporal_compression_ratio"])
    vae = s2v.HipAutoencoderKLCogVideoX(cfg, dt, DEV, force_simple)
    vae.load_state_dict(sd)
    return vae


@pytest.mark.parametrize("tiling", [False, True])
def test_vae_tiny_fp32_vs_reference_golden(s2v, tiling):
    g = load_golden("vae_tiny.npz")
    vae = make_vae(s2v, TINY, torch.float32, weights_of(g))
    if tiling:
        vae.enable_tiling()
    y = vae.decode_latents(t(g["latents"]).to(DEV))
    torch.cuda.synchronize()
    name = "dec_tiled" if tiling else "dec_untiled"
    assert tuple(y.shape) == (1, 3, 17, 96, 160)
    y = y.cpu()
    assert torch.isfinite(y).all()
    assert np.abs(y[..., ::3, ::3].numpy() - g[name + "_s3"]).max() <= 1e-3
    np.testing.assert_allclose(y.double().sum(dim=(0, 1, 3, 4)).numpy(), g[name + "_sum"], rtol=1e-4, atol=0.5)
    np.testing.assert_allclose((y.double() ** 2).sum(dim=(0, 1, 3, 4)).numpy(), g[name + "_sq"], rtol=1e-4)


def test_vae_tiny_tiled_ragged_grid_vs_oracle(s2v):
    """7 x 9 latents, the smallest tiled decode whose grid has two tile sizes in both axes (6 | 2 rows, 9 | 1 columns of latents) and an edge
    tile smaller than the blend extent: the last column decodes to 8 pixels where the horizontal blend takes 16 (the 12 x 20 decode above has
    edge tiles of 16 x 32 pixels against blends of 8 and 16) -- fp32 against the oracle's tiled decode, every pixel"""
    g = load_golden("vae_tiny.npz")
    sd = weights_of(g)
    lat = t(g["latents"])[:, :2, :, :7, :9].contiguous()
    with torch.no_grad():
        exp = vae_ref.decode_latents(sd, TINY, lat, True)
    vae = make_vae(s2v, TINY, torch.float32, sd)
    vae.enable_tiling()
    y = vae.decode_latents(lat.to(DEV)).cpu()
    torch.cuda.synchronize()
    assert y.shape == exp.shape and y.shape[3:] == (56, 72)  # crops of 40 + 16 rows, 64 + 8 columns
    err = (y - exp).abs().max().item()
    print(f"MEASURED vae tiny ragged tiled decode vs oracle: max-abs {err:.3e}")
    assert err <= 1e-3, err


def test_vae_even_single_frame_and_postprocess_vs_reference_golden(s2v):
    g = load_golden("vae_tiny.npz")
    vae = make_vae(s2v, TINY, torch.float32, weights_of(g))
    lat = t(g["latents"]).to(DEV)
    y2 = vae.decode_latents(lat[:, :2, :, :6, :8].contiguous())
    y1 = vae.decode_latents(lat[:, :1, :, :6, :8].contiguous())
    # the vae.decode(z) seam: z = latents / scaling_factor in [B,C,F,h,w]
    z = (lat[:, :2, :, :6, :8] / 0.7).permute(0, 2, 1, 3, 4)
    y2z = vae.decode(z).sample
    torch.cuda.synchronize()
    assert np.abs(y2.cpu().numpy() - g["dec_2f"]).max() <= 1e-3
    assert np.abs(y1.cpu().numpy() - g["dec_1f"]).max() <= 1e-3
    assert np.abs(y2z.cpu().numpy() - g["dec_2f"]).max() <= 1e-3
    post = vae.postprocess_video(t(g["dec_2f"]).to(DEV), "np")
    assert np.abs(post - g["post_np"]).max() <= 1e-6
    with pytest.raises(s2v.S2VError):  # decoder-only state dict: the encode half has no weights
        vae.encode(lat)


@pytest.mark.parametrize("dt_name", ["bf16", "f16"])
def test_vae_tiny_reduced_precision_vs_reference_golden(s2v, dt_name):
    """the reference decoder itself run in bf16 / fp16 on the CPU (fixtures dec_2f_bf16 / dec_2f_f16, round 5): the HIP decoder in that dtype on the
    same latent window, every pixel.  (Tiny channel counts: these convolutions take the generic kernels; the MFMA widths are held to the oracle below.)"""
    g = load_golden("vae_tiny.npz")
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[dt_name]
    vae = make_vae(s2v, TINY, dt, weights_of(g))
    lat = t(g["latents"]).to(dt)[:, :2, :, :6, :8].contiguous().to(DEV)
    y = vae.decode_latents(lat).float().cpu()
    torch.cuda.synchronize()
    exp = t(g[f"dec_2f_{dt_name}"])
    assert y.shape == exp.shape and torch.isfinite(y).all()
    rel = ((y - exp).double().norm() / exp.double().norm()).item()
    err = (y - exp).abs().max().item() / exp.abs().max().item()
    print(f"MEASURED vae tiny {dt_name} vs reference: rel-l2 {rel:.3e} max-abs/max|ref| {err:.3e}")
    br, ba = (1.8e-2, 2.5e-2) if dt_name == "bf16" else (2.5e-3, 3.5e-3)  # the CPU oracle's own distance to these fixtures is 9.0e-3 / 1.2e-3
    assert rel <= br and err <= ba, (rel, err)


@pytest.mark.parametrize("dt_name,simple", [("bf16", False), ("bf16", True), ("f32", False)])
@pytest.mark.parametrize("tiling", [False, True])
def test_vae_mfma_channels_vs_oracle(s2v, dt_name, simple, tiling):
    """channel counts that take the MFMA implicit-GEMM path (64/128), 5 latent frames of 12x20 -> 17 frames 96x160"""
    dt = torch.float32 if dt_name == "f32" else torch.bfloat16
    cfgd = dict(block_out_channels=(64, 64, 128, 128), layers_per_block=1, norm_num_groups=8, latent_channels=16,
                sample_height=96, sample_width=160, scaling_factor=1.15258426, temporal_compression_ratio=4)
    cfg = s2v.VAEConfig(**{k: cfgd[k] for k in ("block_out_channels", "layers_per_block", "norm_num_groups",
                                                "latent_channels", "sample_height", "sample_width", "scaling_factor",
                                                "temporal_compression_ratio")})
    sd = s2v.weights.synthetic_vae_state_dict(cfg, seed=8)
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(1, 5, 16, 12, 20, generator=g).to(dt)
    with torch.no_grad():
        exp = vae_ref.decode_latents({k: v.to(dt) for k, v in sd.items()}, cfgd, lat, tiling).float()
    vae = make_vae(s2v, cfgd, dt, sd, simple)
    if tiling:
        vae.enable_tiling()
    y = vae.decode_latents(lat.to(DEV)).float().cpu()
    torch.cuda.synchronize()
    assert y.shape == exp.shape
    assert torch.isfinite(y).all()
    err = (y - exp).abs().max().item()
    if dt_name == "f32":
        assert err <= 1e-3, err
    else:
        rel = ((y - exp).double().norm() / exp.double().norm()).item()
        assert rel <= 3e-2 and err <= 6e-2 * exp.abs().max().item(), (rel, err)


DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
REAL = dict(block_out_channels=(128, 256, 256, 512), layers_per_block=3, norm_num_groups=32, latent_channels=16,
            sample_height=480, sample_width=720, scaling_factor=0.7, temporal_compression_ratio=4)


@pytest.mark.parametrize("dt_name", ["f32", "bf16", "f16"])
def test_vae_real_width_decoder_vs_oracle(s2v, dt_name):
    """the decoder the checkpoints ship -- (128, 256, 256, 512) channels, 3 resnets per block, 32 groups
    (autoencoder_kl_cogvideox.py:921-981) -- on a small latent (3 x 8 x 12 -> 9 frames 64 x 96), against the fp32 oracle"""
    dt = DT[dt_name]
    cfg = s2v.VAEConfig(**REAL)
    sd = {k: v.to(dt).float() for k, v in s2v.weights.synthetic_vae_state_dict(cfg, seed=61).items()}
    lat = torch.randn(1, 3, 16, 8, 12, generator=torch.Generator().manual_seed(62)).to(dt).float()
    with torch.no_grad():
        exp = vae_ref.decode_latents(sd, REAL, lat, False)
    vae = make_vae(s2v, REAL, dt, sd)
    y = vae.decode_latents(lat.to(DEV, dt)).float().cpu()
    torch.cuda.synchronize()
    assert y.shape == exp.shape == (1, 3, 9, 64, 96)
    assert torch.isfinite(y).all()
    err = (y - exp).abs().max().item()
    if dt_name == "f32":
        assert err <= 1e-3, err
    else:  # fp16 (round 5): the same rounding points, 8 x finer ulps
        rel = ((y - exp).double().norm() / exp.double().norm()).item()
        br, ba = (1.7e-2, 2.1e-2) if dt_name == "bf16" else (2.1e-3, 2.5e-3)   # 2 x measured in round 5 (bf16 8.4e-3 / 1.05e-2, fp16 1.04e-3 / 1.23e-3)
        print(f"MEASURED vae {dt_name}: rel-l2 {rel:.3e} max-abs/max|ref| {err / exp.abs().max().item():.3e}")
        assert rel <= br and err <= ba * exp.abs().max().item(), (rel, err)


@pytest.mark.parametrize("dt_name", ["f32", "bf16", "f16"])
def test_vae_real_width_tiled_decoder_vs_oracle(s2v, dt_name):
    """the reference enables VAE tiling by default (src/inference.py:56-57, 206-207): the real-width decoder in its TILED form
    (autoencoder_kl_cogvideox.py:1374-1455) -- sample size 96 x 128, so a 5 x 10 x 14 latent (17 frames 80 x 112) is cut into
    overlapping 6 x 8 latent tiles, blended in both directions, over two frame batches with the conv cache -- against the oracle"""
    dt = DT[dt_name]
    cfgd = dict(REAL, sample_height=96, sample_width=128)
    cfg = s2v.VAEConfig(**cfgd)
    sd = {k: v.to(dt).float() for k, v in s2v.weights.synthetic_vae_state_dict(cfg, seed=63).items()}
    lat = torch.randn(1, 5, 16, 10, 14, generator=torch.Generator().manual_seed(64)).to(dt).float()
    with torch.no_grad():
        exp = vae_ref.decode_latents(sd, cfgd, lat, True)
    vae = make_vae(s2v, cfgd, dt, sd)
    vae.enable_tiling()
    y = vae.decode_latents(lat.to(DEV, dt)).float().cpu()
    torch.cuda.synchronize()
    # the reference's tile arithmetic decides the output extent (tiles x cropped tile size: 3 x 40 = 120 columns for 14 latent
    # columns, where the untiled decode gives 112) -- the drop-in reproduces that, quirk included
    assert y.shape == exp.shape and y.shape[:3] == (1, 3, 17) and y.shape[4] != 112
    assert torch.isfinite(y).all()
    err = (y - exp).abs().max().item()
    if dt_name == "f32":
        assert err <= 1e-3, err
    else:  # fp16 (round 5): the same rounding points, 8 x finer ulps
        rel = ((y - exp).double().norm() / exp.double().norm()).item()
        br, ba = (1.7e-2, 2.1e-2) if dt_name == "bf16" else (2.1e-3, 2.5e-3)   # 2 x measured in round 5 (bf16 8.4e-3 / 1.05e-2, fp16 1.04e-3 / 1.23e-3)
        print(f"MEASURED vae {dt_name}: rel-l2 {rel:.3e} max-abs/max|ref| {err / exp.abs().max().item():.3e}")
        assert rel <= br and err <= ba * exp.abs().max().item(), (rel, err)


def test_frames_uint8_matches_export_to_video_conversion(s2v, tmp_path):
    """(postprocess_video(..., "np")[0] * 255).astype(np.uint8) of utils/export_utils.py:175, bit-exact, both dtypes"""
    g = load_golden("vae_tiny.npz")
    vae = make_vae(s2v, TINY, torch.float32, weights_of(g))
    for dt in (torch.float32, torch.bfloat16):
        video = t(g["dec_2f"]).to(dt).to(DEV)
        video[0, 0, 0, 0, :4] = torch.tensor([5.0, -5.0, 1.0, -1.0], dtype=dt)  # clamp edges: 255, 0, 255, 0
        u8 = vae.frames_uint8(video).cpu().numpy()
        ref = (vae.postprocess_video(video, "np")[0] * 255).astype(np.uint8)
        assert u8.dtype == np.uint8 and u8.shape == ref.shape
        assert np.array_equal(u8, ref)
    out = s2v.video_generate.export_to_video(u8, str(tmp_path / "s2v_test_clip.mp4"), fps=8)
    if out.endswith(".avi"):  # no imageio-ffmpeg on the box: Motion-JPEG AVI with the same frames
        n, fps, w, h, first = s2v.video_generate.read_avi_info(out)
        assert (n, w, h) == (u8.shape[0], u8.shape[2], u8.shape[1]) and fps == 8.0


def test_tiled_decode_workspace_byte_cap_and_regrowth(s2v, monkeypatch):
    """prepare_tile_capacity: the number of workspace sets (tiles in flight) is bounded by S2V_VAE_WORKSPACE_MAX_GB as well as
    by the free memory; capacity is committed only after its sets exist, so a context that was granted ONE set decodes (bit-identically
    to six in flight) and grows when a later, larger window asks for more"""
    import os

    g = load_golden("vae_tiny.npz")
    lat = t(g["latents"]).to(DEV)
    free = make_vae(s2v, TINY, torch.float32, weights_of(g))
    free.enable_tiling()
    y_free = free.decode_latents(lat)
    n_free, set_bytes = free.workspace_info()
    assert n_free >= 2 and set_bytes > 0
    monkeypatch.setenv("S2V_VAE_WORKSPACE_MAX_GB", str(1.5 * set_bytes / 1e9))
    capped = make_vae(s2v, TINY, torch.float32, weights_of(g))
    capped.enable_tiling()
    y_cap = capped.decode_latents(lat)
    torch.cuda.synchronize()
    assert capped.workspace_info()[0] == 1
    assert torch.equal(y_cap, y_free)
    monkeypatch.delenv("S2V_VAE_WORKSPACE_MAX_GB")
    capped.disable_tiling()      # the untiled decode needs a larger window: the workspace is rebuilt, and the decode is the golden one
    y_un = capped.decode_latents(lat).cpu()
    assert np.abs(y_un[..., ::3, ::3].numpy() - g["dec_untiled_s3"]).max() <= 1e-3
    capped.enable_tiling()
    assert torch.equal(capped.decode_latents(lat), y_free)


def test_tiled_decode_survives_a_workspace_set_that_fails_part_way(s2v, monkeypatch):
    """set 1 of the tiled decode's workspace fails after a few allocations (injected: S2V_VAE_FAULT_GEO_ALLOC counts the workspace
    allocations of one prepare_tile_capacity call).  The partial set is freed, ONE set survives -- and the live members must be reloaded from
    it, not left on the freed pointers: the decode runs and is bit-identical to the unconstrained one."""
    g = load_golden("vae_tiny.npz")
    lat = t(g["latents"]).to(DEV)
    free = make_vae(s2v, TINY, torch.float32, weights_of(g))
    free.enable_tiling()
    y_free = free.decode_latents(lat)
    n_free, _ = free.workspace_info()
    assert n_free >= 2
    # count the allocations of one set: fail at the first allocation -> no capacity at all, loudly
    monkeypatch.setenv("S2V_VAE_FAULT_GEO_ALLOC", "1")
    none = make_vae(s2v, TINY, torch.float32, weights_of(g))
    none.enable_tiling()
    with pytest.raises(s2v._lib.S2VError):
        none.decode_latents(lat)
    # fail a few allocations INTO the second set (a set of this tiny decoder has > 20 buffers; 200 is past the first set for every level count)
    hit = False
    for n in (30, 40, 60, 90):
        monkeypatch.setenv("S2V_VAE_FAULT_GEO_ALLOC", str(n))
        v = make_vae(s2v, TINY, torch.float32, weights_of(g))
        v.enable_tiling()
        try:
            y = v.decode_latents(lat)
        except s2v._lib.S2VError:
            continue  # n fell inside the FIRST set: nothing to survive on
        torch.cuda.synchronize()
        sets = v.workspace_info()[0]
        assert torch.equal(y, y_free), n
        if sets < n_free:
            hit = True
            assert torch.equal(v.decode_latents(lat), y_free)  # and again on the surviving sets
    monkeypatch.delenv("S2V_VAE_FAULT_GEO_ALLOC")
    assert hit, "no injected failure landed inside a later set"


@pytest.mark.parametrize("dt_name", ["bf16", "f16"])
@pytest.mark.parametrize("frames,h,w", [(1, 5, 7), (2, 5, 7), (4, 3, 9)])
def test_direct_conv_out_kernel_edge_shapes_vs_oracle(s2v, dt_name, frames, h, w):
    """the direct conv_out kernel (round 6; csrc/vae.hip conv_out_direct_k: runs when the last block has a multiple of 32 channels) on what its
    plane walk has to get right at the edges: ONE latent frame (three planes, a single output frame), two (8 frames), an even batch after an odd one
    (4 latent frames = 3 + 1: the second batch is a single frame behind a conv cache), output sizes that are ragged against the 4 x 32 patch
    (40 x 56, 24 x 72), 32 input channels (one 32-channel block per tap) -- against the CPU oracle"""
    dt = DT[dt_name]
    cfgd = dict(block_out_channels=(32, 32, 32, 32), layers_per_block=1, norm_num_groups=4, latent_channels=16,
                sample_height=480, sample_width=720, scaling_factor=0.7, temporal_compression_ratio=4)
    cfg = s2v.VAEConfig(**cfgd)
    sd = {k: v.to(dt).float() for k, v in s2v.weights.synthetic_vae_state_dict(cfg, seed=81).items()}
    lat = torch.randn(1, frames, 16, h, w, generator=torch.Generator().manual_seed(82)).to(dt).float()
    with torch.no_grad():
        exp = vae_ref.decode_latents(sd, cfgd, lat, False)
    vae = make_vae(s2v, cfgd, dt, sd)
    y = vae.decode_latents(lat.to(DEV, dt)).float().cpu()
    torch.cuda.synchronize()
    assert y.shape == exp.shape
    assert torch.isfinite(y).all()
    rel = ((y - exp).double().norm() / exp.double().norm()).item()
    err = (y - exp).abs().max().item() / exp.abs().max().item()
    print(f"MEASURED direct conv_out {dt_name} F={frames} {h}x{w}: rel-l2 {rel:.3e} max-abs/max|ref| {err:.3e}")
    br, ba = (1.7e-2, 2.1e-2) if dt_name == "bf16" else (2.1e-3, 2.5e-3)   # the real-width decoder's bars above
    assert rel <= br and err <= ba, (rel, err)
