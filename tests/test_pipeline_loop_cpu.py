"""The one denoise loop of S2VPipeline (pipeline.py: _denoise) against the plans, with a recording stand-in for the engine and no device: a
call with scalars and a call with per-video step counts hand the engine exactly the steps of every video's video_plan -- timestep, coefficient
bytes and the active videos per iteration, longest plan first -- set the geometry once per distinct active count, draw every video's DPM noise
from its own generator as often as its plan says, show `guidance_scale` as the call asked for it and return the videos in the caller's order."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

DT = torch.bfloat16
B, STEPS, GUIDANCE = 3, 4, 6.0
CALLS = {"scalars": STEPS, "per-video": [2, 4, 3]}   # num_inference_steps; the per-video call runs videos 1, 2, 0 in that order and shrinks twice
LATENT = (2, 16, 8, 12)   # 5 frames of 64 x 96 pixels


def _coef_bytes(c):
    return bytes(ctypes.string_at(ctypes.byref(c), ctypes.sizeof(c)))


class Recorder:
    """what the fused loop needs of an S2VEngine; its step halves the latents, so a video's result tells how many steps it ran"""
    fp8_qk_active = False
    cfg = SimpleNamespace(attn_p_format="bf16")

    def __init__(self):
        self.calls, self.steps, self.geometry = [], [], None

    def set_geometry(self, *geo):
        self.geometry = geo
        self.calls.append(("set_geometry", geo))

    def prepare_tables(self, height, width):
        self.calls.append(("prepare_tables", (height, width)))

    def set_conditioning(self, text, ref):
        self.calls.append(("set_conditioning", (text.clone(), ref.clone())))

    def denoise_step(self, latents, timestep, coef, x0_hist=None, noise=None, use_graph=False, blend=None, cache=None, attn_layers=None):
        a = latents.shape[0]
        ts = list(timestep) if isinstance(timestep, (list, tuple)) else [timestep] * a   # scalars and lists of equal entries are the same step
        cs = list(coef) if isinstance(coef, (list, tuple)) else [coef] * a
        assert len(ts) == a and len(cs) == a and blend is None and cache is None and attn_layers is None
        self.calls.append(("step", a))
        self.steps.append(dict(t=[float(t) for t in ts], coef=[_coef_bytes(c) for c in cs], noise=None if noise is None else noise.clone(),
                               x0_hist=None if x0_hist is None else tuple(x0_hist.shape)))
        latents.mul_(0.5)


def _scheduler(s2v, kind):
    return (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)


@functools.lru_cache(maxsize=None)
def _run(s2v, kind, call):
    """one call of the pipeline, made once per (scheduler, call) and shared by the tests below, with the plans it must have followed"""
    eng = Recorder()
    tr = SimpleNamespace(engine=eng, dtype=DT, device=torch.device("cpu"),
                         config=SimpleNamespace(in_channels=16, use_rotary_positional_embeddings=True, num_layers=2))
    pipe = s2v.S2VPipeline(tr, _scheduler(s2v, kind))
    g = torch.Generator().manual_seed(1)
    pos, neg, ref = torch.randn(B, 5, 8, generator=g), torch.randn(B, 5, 8, generator=g), torch.randn(B, 1, 16, 8, 12, generator=g)
    seen = []
    out = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, height=64, width=96, num_frames=5, guidance_scale=GUIDANCE,
               num_inference_steps=CALLS[call], generator=[torch.Generator().manual_seed(50 + k) for k in range(B)],
               callback_on_step_end=lambda p, i, t, tensors: seen.append(p.guidance_scale))["frames"]
    counts = CALLS[call] if isinstance(CALLS[call], list) else [CALLS[call]] * B
    plans = [s2v.S2VPipeline.video_plan(_scheduler(s2v, kind), n, None, GUIDANCE, False, DT) for n in counts]
    order, _ = s2v.S2VPipeline.plan_order(plans)
    return SimpleNamespace(pipe=pipe, eng=eng, out=out, plans=plans, order=order, counts=counts, seen=seen, text=torch.cat([neg, pos]).to(DT),
                           ref=ref.to(DT))


def _active(r, i):
    """the caller's indices of the videos that run iteration i, in the loop's order"""
    return [k for k in r.order if r.counts[k] > i]


KINDS = pytest.mark.parametrize("kind", ["ddim", "dpm"])
BOTH = pytest.mark.parametrize("call", list(CALLS))


@KINDS
@BOTH
def test_the_engine_receives_the_steps_of_every_plan_longest_first(s2v, kind, call):
    r = _run(s2v, kind, call)
    assert r.order == ([0, 1, 2] if call == "scalars" else [1, 2, 0])
    assert len(r.eng.steps) == max(r.counts)
    for i, got in enumerate(r.eng.steps):
        videos = _active(r, i)
        assert got["t"] == [float(r.plans[k]["steps"][i]["t"]) for k in videos], f"iteration {i}: timesteps"
        assert got["coef"] == [_coef_bytes(r.plans[k]["steps"][i]["coef"]) for k in videos], f"iteration {i}: coefficients"
        assert got["x0_hist"] == (None if kind == "ddim" else (len(videos),) + LATENT)
    assert r.pipe.scheduler.num_inference_steps == max(r.counts), "the scheduler object is left on the longest count"


@KINDS
@BOTH
def test_the_geometry_is_set_once_per_distinct_active_count(s2v, kind, call):
    r = _run(s2v, kind, call)
    exp = []
    for i in range(max(r.counts)):
        a = len(_active(r, i))
        if i == 0 or a != len(_active(r, i - 1)):
            exp += ["set_geometry", "prepare_tables", "set_conditioning"]
        exp.append("step")
    assert [c[0] for c in r.eng.calls] == exp
    assert exp.count("set_geometry") == (1 if call == "scalars" else 3)
    counts = sorted({len(_active(r, i)) for i in range(max(r.counts))}, reverse=True)
    assert [c[1] for c in r.eng.calls if c[0] == "set_geometry"] == [(2 * a, 5, 2, 8, 12) for a in counts]
    for a, (text, ref) in zip(counts, [c[1] for c in r.eng.calls if c[0] == "set_conditioning"]):   # the rows of the active videos
        rows = r.order[:a]
        assert torch.equal(text, torch.cat([r.text[:B][rows], r.text[B:][rows]])) and torch.equal(ref, r.ref[rows])


@BOTH
def test_dpm_noise_of_every_video_is_its_own_generator_after_the_draws_of_its_plan(s2v, call):
    r = _run(s2v, "dpm", call)
    assert [s["draws"] for s in r.plans[1]["steps"]] == [1, 2, 2, 1], "multistep steps draw twice and keep the second"
    for k in range(B):
        g = torch.Generator().manual_seed(50 + k)
        torch.randn((1,) + LATENT, generator=g, dtype=DT)   # the initial latents come first
        for i, st in enumerate(r.plans[k]["steps"]):
            for _ in range(st["draws"]):
                exp = torch.randn((1,) + LATENT, generator=g, dtype=DT)
            p = _active(r, i).index(k)
            assert torch.equal(r.eng.steps[i]["noise"][p:p + 1], exp), f"video {k}, step {i}"


@KINDS
def test_guidance_scale_is_a_float_on_a_scalar_call_and_a_list_per_video(s2v, kind):
    r = _run(s2v, kind, "scalars")
    assert r.seen == [GUIDANCE] * STEPS and all(isinstance(g, float) for g in r.seen) and r.pipe.guidance_scale == GUIDANCE
    r = _run(s2v, kind, "per-video")
    assert r.seen == [[GUIDANCE] * B] * max(r.counts) and isinstance(r.pipe.guidance_scale, list)


@KINDS
@BOTH
def test_results_come_back_in_the_callers_order(s2v, kind, call):
    r = _run(s2v, kind, call)
    assert tuple(r.out.shape) == (B,) + LATENT
    for k in range(B):   # video k: the latents of generator k, halved once per step of its own plan (exact in bf16)
        start = torch.randn((1,) + LATENT, generator=torch.Generator().manual_seed(50 + k), dtype=DT)
        assert torch.equal(r.out[k:k + 1], start * 0.5 ** r.counts[k]), f"video {k}"
