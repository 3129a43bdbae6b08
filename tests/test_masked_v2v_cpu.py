"""Masked video-to-video, the host side that needs no device (pipeline.py: check_mask / blend_plan; schedulers.py: blend_record;
video_generate.inference: mask_uint8): the mask's shape and row logic, the blend record of every step of a plan, every refusal before any
device work, and the new symbols.  The mask reduction itself runs only on the GPU (s2v_mask_to_latent): its values are checked in
tests/test_gpu_masked_v2v.py against the restatement of tests/masked_v2v_ref.py, which is checked here against a per-cell loop."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import masked_v2v_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.bfloat16


def _sched(s2v, kind):
    return (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)


# ------------------------------------------------------------------------------------------------ the mask reduction's restatement
def _by_cell(mask):
    """the "any" rule, cell by cell as the issue words it"""
    m = R.binarise(mask)
    r, F, H, W = m.shape
    out = torch.zeros(r, (F - 1) // 4 + 1, H // 8, W // 8, dtype=torch.uint8)
    for j in range(out.shape[1]):
        frames = [0] if j == 0 else list(range(4 * j - 3, 4 * j + 1))
        for y in range(H // 8):
            for x in range(W // 8):
                out[:, j, y, x] = m[:, frames, 8 * y:8 * y + 8, 8 * x:8 * x + 8].reshape(r, -1).amax(dim=1)
    return out


@pytest.mark.parametrize("F", [1, 9, 17])
def test_the_restatement_of_the_mask_reduction_is_the_any_rule(F):
    g = torch.Generator().manual_seed(F)
    sparse = (torch.rand(2, F, 64, 96, generator=g) > 0.995).float()   # sparse enough that "any" differs from "nearest" and from "all"
    for mask in (sparse, torch.rand(2, F, 64, 96, generator=g), (sparse * 255).to(torch.uint8)):
        got = R.latent_mask(mask)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, (F - 1) // 4 + 1, 8, 12)
        assert torch.equal(got, _by_cell(mask))
    assert 0 < int(R.latent_mask(sparse).sum()) < R.latent_mask(sparse).numel()
    one = torch.zeros(1, F, 64, 96)
    one[0, -1, -1, -1] = 1.0   # a single pixel in the last frame's last row and column: the last cell of the last latent frame, nothing else
    lat = R.latent_mask(one)
    assert int(lat.sum()) == 1 and int(lat[0, -1, -1, -1]) == 1
    assert torch.equal(R.binarise(torch.tensor([0.0, 0.49, 0.5, 1.0])), torch.tensor([0, 0, 1, 1], dtype=torch.uint8))


def test_mask_to_latent_refuses_shapes_it_cannot_reduce_before_any_launch(s2v):
    for shape in ((9, 64, 96), (1, 8, 64, 96), (1, 9, 60, 96), (1, 9, 64, 100)):
        with pytest.raises(s2v.S2VError, match="mask_to_latent"):
            s2v.mask_to_latent(torch.zeros(shape))


# ------------------------------------------------------------------------------------------------ shape and row logic
def test_check_mask_returns_the_rows_and_takes_both_layouts(s2v):
    P = s2v.S2VPipeline
    video = torch.zeros(3, 3, 9, 64, 96)
    m4, m5 = torch.zeros(3, 9, 64, 96), torch.ones(1, 1, 9, 64, 96)
    assert P.check_mask(m4, video, 3) is m4
    got = P.check_mask(m5, video, 3)
    assert tuple(got.shape) == (1, 9, 64, 96) and bool((got == 1).all()), "one row, shared by all videos"
    assert tuple(P.check_mask(torch.zeros(3, 1, 9, 64, 96), video[:1], 3).shape) == (3, 9, 64, 96), "a mask per video over one shared input video"


# ------------------------------------------------------------------------------------------------ the blend plan
def _record(r):
    return (r.sqrt_alpha, r.sqrt_one_minus_alpha, r.last)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_blend_plan_is_add_noise_at_the_next_timestep_and_a_flag_on_the_last_step(s2v, kind, dt):
    P = s2v.S2VPipeline
    sch = _sched(s2v, kind)
    plan = P.video_plan(sch, 4, 0.75, 6.0, False, dt)
    ts = [int(t) for t in plan["timesteps"]]
    assert len(ts) == 3
    recs = P.blend_plan(sch, plan, dt)
    assert len(recs) == 3
    for i in range(2):
        sa, sb = sch.add_noise_scalars(ts[i + 1], dt, "cpu")
        assert _record(recs[i]) == (np.float32(sa), np.float32(sb), 0), f"step {i} blends at t = {ts[i + 1]}"
        assert 0.0 < recs[i].sqrt_alpha < 1.0
    assert recs[2].last == 1 and [r.last for r in recs] == [0, 0, 1]
    # per video, plans of different lengths (strengths 0.5 / 1.0 / 0.75 at 4 steps keep 2 / 4 / 3 timesteps): every video on its OWN next timestep
    # and flagged on its OWN last step
    for strength, n in ((0.5, 2), (1.0, 4), (0.75, 3)):
        plan = P.video_plan(sch, 4, strength, 6.0, False, dt)
        recs = P.blend_plan(sch, plan, dt)
        ts = [int(t) for t in plan["timesteps"]]
        assert len(recs) == n and [r.last for r in recs] == [0] * (n - 1) + [1]
        for i in range(n - 1):
            assert _record(recs[i])[:2] == tuple(np.float32(x) for x in sch.add_noise_scalars(ts[i + 1], dt, "cpu"))
    # a one-step plan is its own last step
    assert [r.last for r in P.blend_plan(sch, P.video_plan(sch, 4, 0.25, 6.0, False, dt), dt)] == [1]


# ------------------------------------------------------------------------------------------------ refusals
def _args():
    T, D = 5, 8
    return dict(prompt_embeds=torch.zeros(2, T, D), negative_prompt_embeds=torch.zeros(2, T, D), ref_img_states=torch.zeros(4, 1, 16, 8, 12),
                num_videos_per_prompt=2, height=64, width=96)


class _Engine:
    """stands where the engine would: any attribute access beyond `geometry` is a refusal that came too late"""
    geometry = (8, 5, 3, 8, 12)

    def __getattr__(self, name):
        raise AssertionError(f"a refused call reached the engine ({name})")


def test_every_refusal_names_its_cause_and_leaves_the_engine_alone(s2v):
    P = s2v.S2VPipeline
    eng = _Engine()
    tr = SimpleNamespace(dtype=DT, device=torch.device("cpu"), engine=eng)
    pipe = P(tr, _sched(s2v, "ddim"), object())   # a VAE that is never asked
    kw = _args()
    video = torch.zeros(4, 3, 9, 64, 96)
    with pytest.raises(ValueError, match=r"`mask` applies only together with `video`"):
        pipe(mask=torch.zeros(4, 5, 64, 96), num_frames=5, **kw)
    with pytest.raises(ValueError, match=r"`mask` must be \[rows, 1, F, H, W\] or \[rows, F, H, W\] with the video's F x H x W = 9 x 64 x 96"):
        pipe(mask=torch.zeros(4, 9, 64, 88), video=video, **kw)
    with pytest.raises(ValueError, match=r"`mask` must be .* with the video's F x H x W"):
        pipe(mask=torch.zeros(4, 5, 64, 96), video=video, **kw)
    with pytest.raises(ValueError, match=r"`mask` must be .* with the video's F x H x W"):
        pipe(mask=torch.zeros(9, 64, 96), video=video, **kw)
    with pytest.raises(ValueError, match=r"`mask` has 3 rows for b = 4 videos: one mask per video, or one row shared by all"):
        pipe(mask=torch.zeros(3, 1, 9, 64, 96), video=video, **kw)
    one = dict(kw, prompt_embeds=kw["prompt_embeds"][:1], negative_prompt_embeds=kw["negative_prompt_embeds"][:1], num_videos_per_prompt=1,
               ref_img_states=kw["ref_img_states"][:1])
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=rf"`mask` together with `{name}`: the masked step runs on one GPU"):
            pipe(mask=torch.zeros(1, 9, 64, 96), video=video[:1], **{name: object()}, **one)
    with pytest.raises(ValueError, match=r"`mask` has 2 rows for b = 1 videos"):
        pipe(mask=torch.zeros(2, 9, 64, 96), video=video[:1], **one)
    assert eng.geometry == (8, 5, 3, 8, 12), "no refusal reached the engine"


def test_inference_passes_the_mask_through_like_the_video(s2v):
    vg = s2v.video_generate
    seen = {}

    class Pipe:
        transformer = SimpleNamespace(device=torch.device("cpu"), dtype=torch.float32)

        def __call__(self, **kw):
            seen.update(kw)
            return {"frames": np.zeros((3, 9, 16, 24, 3), np.float32)}

    pipe = Pipe()
    pipe.vae = SimpleNamespace(device=torch.device("cpu"), dtype=torch.float32, config=SimpleNamespace(scaling_factor=1.0),
                               encode=lambda x: SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda g=None: torch.zeros(1, 16, 1, 2, 3))))
    enc = lambda ids: (torch.zeros(ids.shape[0], 4, 8),)
    rng = np.random.default_rng(6)
    clips = rng.integers(0, 256, (3, 9, 16, 24, 3), dtype=np.uint8)
    masks = rng.integers(0, 256, (3, 9, 16, 24), dtype=np.uint8)
    masks[0, 0, 0, :4] = (0, 127, 128, 255)
    call = lambda **kw: vg.inference(pipe, enc, np.zeros((16, 24, 3), np.uint8), torch.zeros(3, 4, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long),
                                     height=16, width=24, **kw)
    call(video_uint8=clips, mask_uint8=masks)
    assert tuple(seen["mask"].shape) == (3, 9, 16, 24) and seen["mask"].dtype == torch.uint8 and seen["paste_back"] is True
    assert torch.equal(seen["mask"], torch.from_numpy((masks >= 128).astype(np.uint8))), ">= 128 repaints"
    assert seen["mask"][0, 0, 0, :4].tolist() == [0, 0, 1, 1]
    seen.clear()
    call(video_uint8=clips, mask_uint8=masks[1], paste_back=False)
    assert tuple(seen["mask"].shape) == (1, 9, 16, 24) and seen["paste_back"] is False, "[F, H, W]: one row, shared by all videos"
    seen.clear()
    call(video_uint8=clips)
    assert "mask" not in seen and "paste_back" not in seen, "an unmasked call is the call it was"
    with pytest.raises(ValueError, match="mask_uint8 applies only together with video_uint8"):
        call(mask_uint8=masks)
    with pytest.raises(ValueError, match=r"mask_uint8 is .* but the video is"):
        call(video_uint8=clips, mask_uint8=masks[:, :5])
    with pytest.raises(ValueError, match="mask_uint8 must be uint8"):
        call(video_uint8=clips, mask_uint8=masks.astype(np.float32))


# ------------------------------------------------------------------------------------------------ symbols
NEW = ["s2v_mask_to_latent", "s2v_set_blend", "s2v_denoise_step_masked", "s2v_sched_step_masked", "s2v_vae_postprocess_masked",
       "s2v_vae_postprocess_u8_masked"]


def test_the_new_entries_are_declared_bound_and_exported(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = s2v.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert name in s2v._lib._SIGS, f"{name} is not bound"
        assert hasattr(lib, name), f"{name} is not exported"
    assert "typedef struct s2v_blend" in code
    import ctypes

    assert ctypes.sizeof(s2v._lib.BlendC) == 16
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, f"{name} is missing from INTEGRATION.md"


def test_the_library_refuses_bad_blend_arguments_by_name(s2v):
    """argument checks that run before any device work"""
    lib, L = s2v.lib(), s2v._lib
    assert lib.s2v_set_blend(None, None, None, None, 0) != 0 and b"s2v_set_blend: null context" in lib.s2v_last_error()
    assert lib.s2v_denoise_step_masked(None, None, None, None, None, None, None, 0, None) != 0
    assert b"s2v_denoise_step_masked: null argument" in lib.s2v_last_error()
    assert lib.s2v_mask_to_latent(None, 0, 9, 64, 96, None, None, None) != 0 and b"s2v_mask_to_latent: null argument" in lib.s2v_last_error()
    assert lib.s2v_vae_postprocess_masked(None, None, 0, None, 3, 9, 64, 96, None, 0, None) != 0
    assert b"s2v_vae_postprocess_masked: null argument" in lib.s2v_last_error()
    assert lib.s2v_vae_postprocess_u8_masked(None, None, 0, None, 3, 9, 64, 96, None, 0, None) != 0
    assert b"s2v_vae_postprocess_u8_masked: null argument" in lib.s2v_last_error()
