"""Several videos per call, the host side that needs no device (pipeline.py: expand_prompts / cfg_text / randn_videos / S2VPipeline.check_batch):
the prompt-major expansion and the [negative x b | positive x b] order of custom_cogvideox_pipe.py:196, one random stream per video as diffusers'
randn_tensor gives a list of generators, and every refusal that is decided before a device is touched."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pl(s2v):
    return s2v.pipeline


@pytest.mark.parametrize("nv", [1, 2, 3])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_prompt_expansion_is_prompt_major_and_negative_comes_first(s2v, P, nv):
    T, D = 5, 8
    g = torch.Generator().manual_seed(P * 10 + nv)
    pos, neg = torch.randn(P, T, D, generator=g), torch.randn(P, T, D, generator=g)
    exp = pos.repeat(1, nv, 1).view(P * nv, T, -1)   # pipeline_cogvideox.py:230-233
    got = _pl(s2v).expand_prompts(pos, nv)
    assert torch.equal(got, exp)
    for k in range(P * nv):
        assert torch.equal(got[k], pos[k // nv]), "video k belongs to prompt k // num_videos_per_prompt"
    text = _pl(s2v).cfg_text(neg, pos, nv)
    b = P * nv
    assert text.shape == (2 * b, T, D)
    assert torch.equal(text[:b], neg.repeat(1, nv, 1).view(b, T, -1)) and torch.equal(text[b:], exp), "[negative x b | positive x b]"


def _pipe(s2v):
    from types import SimpleNamespace

    tr = SimpleNamespace(config=SimpleNamespace(in_channels=16))
    return s2v.S2VPipeline(tr, s2v.CogVideoXDPMScheduler(snr_shift_scale=1.0))


def test_a_list_of_generators_draws_every_video_from_its_own_stream(s2v):
    b, F, H, W = 3, 5, 64, 96
    pipe = _pipe(s2v)
    gens = [torch.Generator().manual_seed(40 + k) for k in range(b)]
    lat = pipe.prepare_latents(F, H, W, torch.float32, torch.device("cpu"), gens, batch=b)
    assert lat.shape == (b, 2, 16, 8, 12)
    noise = torch.empty_like(lat)
    drawn = []
    for step in range(3):   # DPM: one draw per step, and a second one on the multistep steps (the first is discarded)
        pipe._draw(noise, gens)
        if step > 0:
            pipe._draw(noise, gens)
        drawn.append(noise.clone())
    for k in range(b):
        g = torch.Generator().manual_seed(40 + k)
        one = pipe.prepare_latents(F, H, W, torch.float32, torch.device("cpu"), g)
        assert torch.equal(lat[k:k + 1], one), f"initial latents of video {k}"
        buf = torch.empty_like(one)
        for step in range(3):
            pipe._draw(buf, g)
            if step > 0:
                pipe._draw(buf, g)
            assert torch.equal(drawn[step][k:k + 1], buf), f"step {step}: noise of video {k}"
    assert not torch.equal(lat[0], lat[1])


def test_a_single_generator_draws_the_whole_batch_at_once(s2v):
    b, F, H, W = 3, 5, 64, 96
    pipe = _pipe(s2v)
    lat = pipe.prepare_latents(F, H, W, torch.float32, torch.device("cpu"), torch.Generator().manual_seed(7), batch=b)
    exp = torch.randn((b, 2, 16, 8, 12), generator=torch.Generator().manual_seed(7))
    assert torch.equal(lat, exp * pipe.scheduler.init_noise_sigma)
    noise = torch.empty_like(lat)
    g = torch.Generator().manual_seed(8)
    pipe._draw(noise, g)
    assert torch.equal(noise, torch.randn(noise.shape, generator=torch.Generator().manual_seed(8)))
    with pytest.raises(ValueError, match="list of generators of length 2"):
        pipe.prepare_latents(F, H, W, torch.float32, torch.device("cpu"), [torch.Generator(), torch.Generator()], batch=b)


def test_the_dpm_scheduler_object_takes_the_list_too(s2v):
    """the seam path hands the list to scheduler.step: its draws are refused when the list does not fit the batch (no device needed for that)"""
    sch = s2v.CogVideoXDPMScheduler(snr_shift_scale=1.0)
    sch.set_timesteps(3)
    x = torch.zeros(3, 2, 16, 8, 12)
    with pytest.raises(ValueError, match="list of generators of length 2"):
        sch.step(x, None, sch.timesteps[0], None, x, generator=[torch.Generator(), torch.Generator()])


def test_argument_validation_without_a_device(s2v):
    pipe = s2v.S2VPipeline(None, None)   # nothing below may reach the transformer, the scheduler or a device
    T, D = 5, 8
    pe, ne = torch.zeros(2, T, D), torch.zeros(2, T, D)
    ref = torch.zeros(4, 1, 16, 8, 12)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, height=64, width=96, num_frames=5)
    with pytest.raises(ValueError, match="at most 4 videos"):
        pipe(ref_img_states=ref[:1], num_videos_per_prompt=3, **kw)
    with pytest.raises(ValueError, match="one row per video"):
        pipe(ref_img_states=ref[:3], num_videos_per_prompt=2, **kw)
    with pytest.raises(ValueError, match="one row per video"):
        pipe(ref_img_states=ref[:3], **kw)
    with pytest.raises(ValueError, match="`latents` has 1 rows for 2 videos"):
        pipe(ref_img_states=ref[:2], latents=torch.zeros(1, 2, 16, 8, 12), **kw)
    with pytest.raises(ValueError, match="list of generators of length 3"):
        pipe(ref_img_states=ref[:2], generator=[torch.Generator() for _ in range(3)], **kw)
    for name, arg in (("cfg_parallel", object()), ("ulysses", object()), ("video", torch.zeros(1, 3, 5, 64, 96))):
        with pytest.raises(ValueError, match=f"`{name}` with 2 videos per call.*one video per call"):
            pipe(ref_img_states=ref[:2], **{name: arg}, **kw)
    with pytest.raises(ValueError, match="same shape"):
        pipe(ref_img_states=ref[:2], **dict(kw, negative_prompt_embeds=ne[:1]))
    assert s2v.S2VPipeline.check_batch(pe, 2, ref) == 4 and s2v.S2VPipeline.check_batch(pe, 2, ref[:1]) == 4
    assert s2v.S2VPipeline.check_batch(pe[:1], 1, ref[:1], cfg_parallel=object(), ulysses=object()) == 1   # one video: nothing new is refused


def test_batch_limit_and_new_entry_points_are_declared_and_bound(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    assert re.search(r"#define\s+S2V_MAX_BATCH\s+8\b", hdr)
    assert s2v.S2VEngine.MAX_BATCH == 8 and s2v.pipeline.MAX_VIDEOS == 4
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("s2v_set_conditioning_refs", "s2v_transformer_forward_videos"):
        assert re.search(rf"\b{name}\s*\(", code) and name in s2v._lib._SIGS
        assert hasattr(s2v.lib(), name)
