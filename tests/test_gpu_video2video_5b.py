"""Video-to-video at the real widths (pytest -m gpu): the bf16 encode of a 49 x 480 x 720 video (tiled, as src/inference.py enables
tiling) against the fp32 encode on the matrix pipe (gemm_f32m), and one 5B video-to-video S2VPipeline call on the fused, graph-captured
step through decode to frames."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# max-abs deviation of the bf16 moments from the fp32 ones, relative to max(1, |moments|): 2 x measured
BF16_VS_F32_BAR = 4.2e-2  # measured 2.08e-2


@pytest.fixture(scope="module")
def clip():
    return torch.rand(1, 3, 49, 480, 720, generator=torch.Generator().manual_seed(31)) * 2 - 1


def test_encode_49x480x720_bf16_vs_fp32_matrix_pipe(s2v, clip):
    vcfg = s2v.VAEConfig(scaling_factor=0.7)
    sd = s2v.weights.synthetic_vae_encoder_state_dict(vcfg, seed=32)
    moms = {}
    for dt in (torch.float32, torch.bfloat16):
        vae = s2v.HipAutoencoderKLCogVideoX(vcfg, dt, DEV)
        vae.load_state_dict(sd)
        vae.enable_tiling()
        moms[dt] = vae.encode(clip.to(DEV, dt)).latent_dist.parameters.float().cpu()
        torch.cuda.synchronize()
        vae.close()
        del vae
        torch.cuda.empty_cache()
    ref, got = moms[torch.float32], moms[torch.bfloat16]
    assert ref.shape == (1, 32, 13, 60, 90)
    assert torch.isfinite(ref).all() and torch.isfinite(got).all()
    err = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"encode 49x480x720 bf16 vs fp32: max-abs deviation / scale {err:.3e}")
    assert err <= BF16_VS_F32_BAR, err


def test_video2video_5b_fused_graph_is_finite(s2v, clip):
    cfg = s2v.cogvideox_5b()
    m = s2v.HipCogVideoXTransformer3DModel(cfg, torch.bfloat16, DEV)
    m.load_state_dict(s2v.weights.synthetic_state_dict(cfg, seed=1, device=DEV))
    vcfg = s2v.VAEConfig(scaling_factor=cfg.vae_scaling_factor)
    vae = s2v.HipAutoencoderKLCogVideoX(vcfg, torch.bfloat16, DEV)
    sd = dict(s2v.weights.synthetic_vae_state_dict(vcfg, seed=2, device=DEV))
    sd.update(s2v.weights.synthetic_vae_encoder_state_dict(vcfg, seed=33))
    vae.load_state_dict(sd)
    vae.enable_tiling()
    pipe = s2v.S2VPipeline(m, s2v.CogVideoXDPMScheduler(snr_shift_scale=cfg.snr_shift_scale), vae)
    g = torch.Generator(device=DEV).manual_seed(3)
    pe = torch.randn(1, 226, 4096, generator=g, device=DEV).bfloat16()
    ne = torch.randn(1, 226, 4096, generator=g, device=DEV).bfloat16()
    ref = (torch.randn(1, 1, 16, 60, 90, generator=g, device=DEV) * 0.7).bfloat16()
    steps = []
    frames = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, ref_img_states=ref, height=480, width=720, num_inference_steps=5,
                  guidance_scale=6.0, generator=torch.Generator(device=DEV).manual_seed(4), video=clip.to(DEV, torch.bfloat16),
                  strength=0.6, output_type="pt", use_graph=True,
                  callback_on_step_end=lambda p, i, t, kw: steps.append(int(t)) or {})["frames"]
    torch.cuda.synchronize()
    assert steps == [int(v) for v in pipe.scheduler.timesteps[2:]]  # int(5 * 0.6) = 3 of the 5 timesteps
    assert frames.shape[1:] == (49, 3, 480, 720)
    assert torch.isfinite(frames.float()).all()
