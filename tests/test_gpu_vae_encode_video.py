"""GPU parity of the video encode and the video-to-video start (pytest -m gpu): s2v_vae_encode_video against the CPU oracle's
encoder driven by a restatement of AutoencoderKLCogVideoX._encode / tiled_encode frame batching (autoencoder_kl_cogvideox.py:1177-1202,
1300-1372), s2v_add_noise against torch's own ops, and S2VPipeline(video=..., strength=...) against a CPU composition of the oracles
(pipeline_cogvideox_video2video.py)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, weights_of
from oracle import sched_ref, transformer_ref as tr, vae_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(block_out_channels=(16, 16, 32, 32), layers_per_block=1, norm_num_groups=4, latent_channels=16,
            sample_height=96, sample_width=160, scaling_factor=0.7, temporal_compression_ratio=4)
DTS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# max-abs deviation from the fp32 oracle (fed the dtype-rounded weights and video), relative to max(1, |moments|): 2 x measured
BAR = {"f32": 5e-6, "bf16": 3e-2, "f16": 3.6e-3}


# ---- CPU restatement of the reference's frame batching over the oracle's encoder ---------------------------------------------
def enc_batches(F):
    """_encode :1184-1195: num_sample_frames_batch_size 8, the remainder goes to the first batch"""
    fbs = 8
    nb = max(F // fbs, 1)
    rem = F % fbs
    return [(fbs * i + (0 if i == 0 else rem), fbs * (i + 1) + rem) for i in range(nb)]


def encode_untiled(sd, cfg, x):
    cache, out = None, []
    for s, e in enc_batches(x.shape[2]):
        y, cache = vae_ref.encoder_forward(sd, cfg, x[:, :, s:e], cache)
        out.append(y)
    return torch.cat(out, dim=2)


def encode_tiled(sd, cfg, x):
    """tiled_encode :1300-1372: every tile runs its own frame batches and caches over all frames; latent-space blends"""
    tg = vae_ref.encode_tile_geometry(cfg)
    H, W = x.shape[3], x.shape[4]
    rows = []
    for i in range(0, H, tg["ov_h"]):
        rows.append([encode_untiled(sd, cfg, x[:, :, :, i:i + tg["ts_h"], j:j + tg["ts_w"]]) for j in range(0, W, tg["ov_w"])])
    res_rows = []
    for i, row in enumerate(rows):
        res = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = vae_ref._blend_v(rows[i - 1][j], tile, tg["bl_h"])
            if j > 0:
                tile = vae_ref._blend_h(row[j - 1], tile, tg["bl_w"])
            res.append(tile[:, :, :, :tg["lim_h"], :tg["lim_w"]])
        res_rows.append(torch.cat(res, dim=4))
    return torch.cat(res_rows, dim=3)


def make_vae(s2v, dt, sd):
    vae = s2v.HipAutoencoderKLCogVideoX(s2v.VAEConfig(**TINY), dt, DEV)
    vae.load_state_dict(sd)
    return vae


def video(F, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, 3, F, H, W, generator=g) * 2 - 1


@pytest.fixture(scope="module")
def sd():
    return weights_of(load_golden("vae_enc_tiny.npz"))


# ---- moments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("F", [9, 17])
@pytest.mark.parametrize("tiling", [False, True])
def test_video_moments_vs_oracle(s2v, sd, name, F, tiling):
    dt = DTS[name]
    H, W = (64, 120) if tiling else (48, 80)  # tiled: 2 x 2 tiles of 48 x 80 pixels with partial edge tiles (24 and 56)
    x = video(F, H, W, 100 + F).to(dt)
    vae = make_vae(s2v, dt, sd)
    if tiling:
        vae.enable_tiling()
    mom = vae.encode(x.to(DEV)).latent_dist.parameters
    torch.cuda.synchronize()
    Fl = (F - 1) // 4 + 1
    assert tuple(mom.shape) == (1, 32, Fl, H // 8, W // 8)
    sdd = {k: v.to(dt).float() for k, v in sd.items()}
    with torch.no_grad():
        exp = (encode_tiled if tiling else encode_untiled)(sdd, TINY, x.float())
    err = (mom.float().cpu() - exp).abs().max().item() / max(1.0, exp.abs().max().item())
    print(f"video encode {name} F={F} tiling={tiling}: max-abs deviation / scale {err:.3e}")
    assert torch.isfinite(mom).all()
    assert err <= BAR[name], err


def _lib_encode(s2v, vae, x, video_entry, tiling):
    lib, L = s2v.lib(), s2v._lib
    F, H, W = x.shape[2], x.shape[3], x.shape[4]
    fl, ho, wo = (ctypes.c_int32() for _ in range(3))
    L.check(lib.s2v_vae_encode_video_shape(vae._enc, F, H, W, tiling, ctypes.byref(fl), ctypes.byref(ho), ctypes.byref(wo)))
    mom = torch.empty((1, 32, fl.value, ho.value, wo.value), dtype=x.dtype, device=DEV)
    if video_entry:
        L.check(lib.s2v_vae_encode_video(vae._enc, L.ptr(x), F, H, W, tiling, L.ptr(mom), L.stream_ptr()))
    else:
        L.check(lib.s2v_vae_encode(vae._enc, L.ptr(x), H, W, tiling, L.ptr(mom), L.stream_ptr()))
    torch.cuda.synchronize()
    return mom


@pytest.mark.parametrize("name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("tiling", [0, 1])
def test_one_frame_through_the_video_entry_is_the_image_encode(s2v, sd, name, tiling):
    dt = DTS[name]
    x = video(1, 96, 160, 7).to(DEV, dt).contiguous()
    vae = make_vae(s2v, dt, sd)
    a = _lib_encode(s2v, vae, x, False, tiling)
    b = _lib_encode(s2v, vae, x, True, tiling)
    assert torch.equal(a, b)
    # and again after a 17-frame encode has grown the workspace of the same handle
    _lib_encode(s2v, vae, video(17, 96, 160, 8).to(DEV, dt).contiguous(), True, tiling)
    assert torch.equal(_lib_encode(s2v, vae, x, True, tiling), a)


def test_video_encode_is_deterministic(s2v, sd):
    x = video(17, 64, 120, 9).to(DEV, torch.bfloat16)
    vae = make_vae(s2v, torch.bfloat16, sd)
    vae.enable_tiling()
    a = vae.encode(x).latent_dist.parameters.clone()
    b = vae.encode(x).latent_dist.parameters.clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_video_frame_counts_refused(s2v, sd):
    vae = make_vae(s2v, torch.float32, sd)
    for F in (2, 10):
        with pytest.raises(NotImplementedError):
            vae.encode(torch.zeros(1, 3, F, 16, 16, device=DEV))
        x = torch.zeros(1, 3, F, 16, 16, device=DEV)
        m = torch.zeros(1, 32, 4, 2, 2, device=DEV)
        with pytest.raises(s2v.S2VError):
            s2v._lib.check(s2v.lib().s2v_vae_encode_video(vae._enc, s2v._lib.ptr(x), F, 16, 16, 0, s2v._lib.ptr(m), s2v._lib.stream_ptr()))


def test_video_posterior_sample_shape(s2v, sd):
    """HipDiagonalGaussianDistribution.sample over [1,2C,Fl,h,w] moments: mean + exp(0.5 clamp(logvar)) * randn, in fp32"""
    vae = make_vae(s2v, torch.float32, sd)
    post = vae.encode(video(9, 48, 80, 11).to(DEV)).latent_dist
    z = post.sample(torch.Generator().manual_seed(3)).cpu()
    noise = torch.randn((1, 16, 3, 6, 10), generator=torch.Generator().manual_seed(3))
    mean, logvar = torch.chunk(post.parameters.cpu(), 2, dim=1)
    exp = mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise
    assert z.shape == (1, 16, 3, 6, 10)
    assert (z - exp).abs().max().item() <= 1e-6


# ---- add_noise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_add_noise_bit_exact_vs_torch(s2v, name, kind):
    dt = DTS[name]
    sch = (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=3.0)
    sch.set_timesteps(50)
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(1, 13, 16, 6, 10, generator=g) * 1.7).to(DEV, dt)
    n = torch.randn(1, 13, 16, 6, 10, generator=g).to(DEV, dt)
    ac = sch.alphas_cumprod.to(DEV).to(dt)  # the reference's add_noise, on the device: fp64 table cast to the sample dtype
    for t in [int(v) for v in sch.timesteps[[0, 10, 25, 40, 49]]]:
        tt = torch.tensor([t], device=DEV)
        sa = (ac[tt] ** 0.5).flatten().reshape(1, 1, 1, 1, 1)
        sb = ((1 - ac[tt]) ** 0.5).flatten().reshape(1, 1, 1, 1, 1)
        exp = sa * x + sb * n
        got = sch.add_noise(x, n, torch.tensor([t]))
        torch.cuda.synchronize()
        assert torch.equal(got, exp), (name, kind, t)


# ---- video-to-video end to end (tiny, fp32) ------------------------------------------------------------------------------------
H, W, FV, TN, STEPS, GS = 64, 96, 9, 7, 4, 6.0


def _tiny_pipeline(s2v, kind, layers=2):
    cfg = s2v.tiny(use_rope=True, heads=2, layers=layers, text_dim=64, temb=64)
    cfg.max_text_seq_length = TN
    sd_tr = s2v.weights.synthetic_state_dict(cfg, seed=81, parity=True)
    model = s2v.HipCogVideoXTransformer3DModel(cfg, torch.float32, DEV)
    model.load_state_dict(sd_tr)
    sd_enc = weights_of(load_golden("vae_enc_tiny.npz"))
    vae = make_vae(s2v, torch.float32, sd_enc)
    sch = (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)
    return s2v.S2VPipeline(model, sch, vae), sd_tr, sd_enc


def _inputs():
    g = torch.Generator().manual_seed(82)
    text = torch.randn(1, TN, 64, generator=g)
    neg = torch.randn(1, TN, 64, generator=g)
    ref = torch.randn(1, 1, 16, H // 8, W // 8, generator=g) * 0.7
    x = video(FV, H, W, 83)
    return text, neg, ref, x


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_video2video_tiny_fp32_vs_oracles(s2v, kind):
    pipe, sd_tr, sd_enc = _tiny_pipeline(s2v, kind)
    text, neg, ref, x = _inputs()
    out = pipe(prompt_embeds=text.to(DEV), negative_prompt_embeds=neg.to(DEV), ref_img_states=ref.to(DEV), height=H, width=W,
               num_inference_steps=STEPS, guidance_scale=GS, generator=torch.Generator().manual_seed(84), video=x.to(DEV),
               strength=0.5, output_type="latent")["frames"]
    torch.cuda.synchronize()
    Fl = (FV - 1) // 4 + 1
    assert out.shape == (1, Fl, 16, H // 8, W // 8)
    # CPU: oracle encode, posterior sample, noise (both from the same generator, in that order), add_noise, truncated loop
    gen = torch.Generator().manual_seed(84)
    shape = (1, Fl, 16, H // 8, W // 8)
    with torch.no_grad():
        mom = encode_untiled(sd_enc, TINY, x)
        eps = torch.randn((1, 16, Fl, H // 8, W // 8), generator=gen)
        mean, logvar = torch.chunk(mom, 2, dim=1)
        z0 = (mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * eps).permute(0, 2, 1, 3, 4)
        noise = torch.randn(shape, generator=gen)
        ac = sched_ref.alphas_cumprod(1.0)
        n = STEPS
        ts = sched_ref.trailing_timesteps(n)
        init_t = min(int(n * 0.5), n)
        ts = ts[max(n - init_t, 0):]
        a0 = torch.as_tensor(ac[int(ts[0])], dtype=torch.float64).to(torch.float32)
        lat = a0**0.5 * (TINY["scaling_factor"] * z0) + (1 - a0) ** 0.5 * noise
        ref_rope, rope = tr.pipeline_rope(H, W, Fl)
        ocfg = dict(num_heads=2, num_layers=2, use_rope=True, norm_eps=1e-5)
        txt = torch.cat([neg, text], dim=0)
        old = None
        for i, t in enumerate(ts):
            tt = torch.tensor([int(t), int(t)])
            npred = tr.transformer_forward(sd_tr, ocfg, torch.cat([lat, lat]), txt, ref, tt, rope, ref_rope).float()
            v = sched_ref.cfg_combine(npred, GS)
            if kind == "ddim":
                lat = sched_ref.ddim_step(ac, n, v, int(t), lat)[0]
            else:
                n1 = torch.randn(shape, generator=gen)
                multistep = old is not None and int(t) - 1000 // n >= 0
                n2 = torch.randn(shape, generator=gen) if multistep else None
                lat, old = sched_ref.dpm_step(ac, n, v, old, int(t), int(ts[i - 1]) if i > 0 else None, lat, n1, n2)
    err = (out.cpu() - lat).abs().max().item() / max(1.0, lat.abs().max().item())
    print(f"video2video {kind} fp32 strength 0.5: max-abs deviation / scale {err:.3e}")
    assert err <= 5e-6, err  # 2 x measured (ddim 2.1e-6, dpm 1.6e-6)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_video2video_strength_one_is_text2video_from_the_noise(s2v, kind):
    """zero-terminal SNR: alphas_cumprod[999] = 0, so add_noise at the first timestep returns the noise itself"""
    pipe, _, _ = _tiny_pipeline(s2v, kind, layers=1)
    text, neg, ref, x = _inputs()
    kw = dict(prompt_embeds=text.to(DEV), negative_prompt_embeds=neg.to(DEV), ref_img_states=ref.to(DEV), height=H, width=W,
              num_inference_steps=STEPS, guidance_scale=GS, output_type="latent")
    v2v = pipe(generator=torch.Generator().manual_seed(85), video=x.to(DEV), strength=1.0, **kw)["frames"]
    gen = torch.Generator().manual_seed(85)
    Fl = (FV - 1) // 4 + 1
    torch.randn((1, 16, Fl, H // 8, W // 8), generator=gen)  # the posterior sample's draw
    noise = torch.randn((1, Fl, 16, H // 8, W // 8), generator=gen)
    t2v = pipe(generator=gen, latents=noise.to(DEV), num_frames=FV, **kw)["frames"]
    torch.cuda.synchronize()
    assert torch.equal(v2v, t2v)


def test_video_latents_is_the_encode_of_the_uint8_video(s2v, sd):
    """video_generate.video_latents: uint8 [F,H,W,3] -> [-1,1] exactly as reference_latents maps the image, then encode + sample"""
    vae = make_vae(s2v, torch.float32, sd)
    v8 = torch.randint(0, 256, (9, 48, 80, 3), generator=torch.Generator().manual_seed(12), dtype=torch.uint8).numpy()
    z = s2v.video_generate.video_latents(vae, v8, torch.Generator().manual_seed(13))
    x = (torch.from_numpy(v8).float() / 255.0 * 2.0 - 1.0).permute(3, 0, 1, 2).unsqueeze(0).to(DEV)
    exp = vae.encode(x).latent_dist.sample(torch.Generator().manual_seed(13))
    torch.cuda.synchronize()
    assert z.shape == (1, 16, 3, 6, 10)
    assert torch.equal(z, exp)
