"""Per-video guidance, strength and step count in a batched call, the host side that needs no device (pipeline.py: check_per_video / video_plan /
plan_order / check_plans; schedulers.py: timesteps_for and the `num_inference_steps` argument of coef): the plan of every video is the sequence
its one-video call makes -- timesteps after `strength`, and per step the timestep, the coefficients (DPM: timestep_back and first), the guidance
scale and the number of noise draws -- the internal order is longest-first and stable, and every refusal is decided before a device is touched."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.bfloat16


def _sched(s2v, kind):
    return (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)


def _coef_bytes(c):
    return bytes(ctypes.string_at(ctypes.byref(c), ctypes.sizeof(c)))


def _one_video_sequence(s2v, kind, n, strength, guidance, dynamic):
    """what S2VPipeline.__call__ does for ONE video with scalars (the reference's loop, custom_cogvideox_pipe.py:237-296), written out on a scheduler of its own"""
    sch = _sched(s2v, kind)
    sch.set_timesteps(n, device="cpu")
    ts, n_loop = sch.timesteps, n
    if strength is not None:
        ts, n_loop = s2v.S2VPipeline.get_timesteps(n, ts, strength, sch.order)
    seq = []
    for i, t in enumerate(ts):
        g = guidance
        if dynamic:
            g = 1 + guidance * ((1 - math.cos(math.pi * ((n_loop - i) / n_loop) ** 5.0)) / 2)
        if kind == "dpm":
            back = ts[i - 1] if i > 0 else None
            coef = sch.coef(t, back, i == 0, DT, g)
            seq.append((int(t), None if back is None else int(back), i == 0, g, _coef_bytes(coef), 2 if coef.kind == 2 else 1))
        else:
            seq.append((int(t), None, i == 0, g, _coef_bytes(sch.coef(t, DT, g)), 0))
    return [int(t) for t in ts], seq


def _plan_sequence(plan):
    return [(int(s["t"]), None if s["t_back"] is None else int(s["t_back"]), s["first"], s["guidance"], _coef_bytes(s["coef"]), s["draws"])
            for s in plan["steps"]]


@pytest.mark.parametrize("dynamic", [False, True], ids=["fixed-cfg", "dynamic-cfg"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_plans_equal_the_one_video_sequences(s2v, kind, dynamic):
    sch = _sched(s2v, kind)
    sch.set_timesteps(7)   # the shared object sits on another count: a plan may not depend on it, nor change it
    guidance = [3.0, 4.5, 6.0, 7.5]
    for counts, strengths in (([2, 4, 3, 3], [None] * 4), ([4, 4, 4], [0.5, 1.0, 0.75]), ([20, 50, 30, 40], [0.4, 0.6, 0.8, 1.0])):
        for k, (n, st) in enumerate(zip(counts, strengths)):
            plan = s2v.S2VPipeline.video_plan(sch, n, st, guidance[k], dynamic, DT)
            ts, seq = _one_video_sequence(s2v, kind, n, st, guidance[k], dynamic)
            assert [int(t) for t in plan["timesteps"]] == ts and plan["num_inference_steps"] == n
            assert _plan_sequence(plan) == seq, (kind, n, st)
    assert sch.num_inference_steps == 7
    # strength 0.5 / 1.0 / 0.75 at 4 steps keep 2 / 4 / 3 timesteps
    assert [len(s2v.S2VPipeline.video_plan(sch, 4, st, 6.0, False, DT)["steps"]) for st in (0.5, 1.0, 0.75)] == [2, 4, 3]
    if kind == "dpm":   # first step and last step are kind 1 (one draw), the steps between are multistep (two draws)
        plan = s2v.S2VPipeline.video_plan(sch, 4, None, 6.0, False, DT)
        assert [s["coef"].kind for s in plan["steps"]] == [1, 2, 2, 1] and [s["draws"] for s in plan["steps"]] == [1, 2, 2, 1]


def test_coef_with_a_step_count_equals_the_scheduler_set_to_it(s2v):
    for kind in ("ddim", "dpm"):
        a, b = _sched(s2v, kind), _sched(s2v, kind)
        a.set_timesteps(50)
        for n in (2, 3, 20):
            b.set_timesteps(n)
            assert torch.equal(a.timesteps_for(n), b.timesteps)
            for i, t in enumerate(b.timesteps):
                if kind == "ddim":
                    got, exp = a.coef(t, DT, 6.0, num_inference_steps=n), b.coef(t, DT, 6.0)
                else:
                    back = b.timesteps[i - 1] if i else None
                    got, exp = a.coef(t, back, i == 0, DT, 6.0, num_inference_steps=n), b.coef(t, back, i == 0, DT, 6.0)
                assert _coef_bytes(got) == _coef_bytes(exp)
        assert a.num_inference_steps == 50 and len(a.timesteps) == 50


def test_internal_order_is_longest_first_stable_and_the_inverse_restores_the_callers(s2v):
    sch = _sched(s2v, "ddim")
    P = s2v.S2VPipeline
    for counts, exp in (([2, 4, 3, 3], [1, 2, 3, 0]), ([3, 3, 3, 3], [0, 1, 2, 3]), ([1, 2], [1, 0]), ([4, 2, 4], [0, 2, 1]), ([5], [0])):
        plans = [P.video_plan(sch, n, None, 6.0, False, DT) for n in counts]
        order, inverse = P.plan_order(plans)
        assert order == exp
        lens = [counts[k] for k in order]
        assert lens == sorted(lens, reverse=True)
        internal = [f"video{k}" for k in order]
        assert [internal[inverse[k]] for k in range(len(counts))] == [f"video{k}" for k in range(len(counts))]
        x = torch.arange(len(counts))
        assert torch.equal(x[order][inverse], x)
        for i in range(max(counts)):   # the videos that still have a step are a prefix
            alive = [n > i for n in lens]
            assert alive == sorted(alive, reverse=True)


def _args(b=4):
    T, D = 5, 8
    pe, ne = torch.zeros(2, T, D), torch.zeros(2, T, D)
    ref = torch.zeros(4, 1, 16, 8, 12)
    return dict(prompt_embeds=pe, negative_prompt_embeds=ne, ref_img_states=ref, num_videos_per_prompt=2, height=64, width=96, num_frames=5)


def test_every_refusal_names_its_limit_before_any_device_work(s2v):
    P = s2v.S2VPipeline
    pipe = P(None, None)   # no transformer, no scheduler: nothing below may reach either
    kw = _args()
    with pytest.raises(ValueError, match=r"`guidance_scale` is a list of 3 entries for b = 4 videos"):
        pipe(guidance_scale=[3.0, 4.0, 5.0], **kw)
    with pytest.raises(ValueError, match=r"`num_inference_steps` is a list of 2 entries for b = 4 videos"):
        pipe(num_inference_steps=[3, 4], **kw)
    with pytest.raises(ValueError, match=r"`strength` is a list of 5 entries for b = 4 videos"):
        pipe(strength=[0.5] * 5, **kw)
    with pytest.raises(ValueError, match=r"guidance_scale\[2\] = 1.0: every guidance scale must be > 1"):
        pipe(guidance_scale=[3.0, 4.0, 1.0, 5.0], **kw)
    with pytest.raises(ValueError, match=r"strength should in \[0.0, 1.0\] but is 1.5"):
        P(None, None, object())(strength=[0.5, 1.5, 0.5, 0.5], video=torch.zeros(1, 3, 9, 64, 96), **dict(kw, num_frames=9))
    with pytest.raises(ValueError, match=r"`strength` as a list applies only together with `video`"):
        pipe(strength=[0.5, 0.6, 0.7, 0.8], **kw)
    with pytest.raises(ValueError, match=r"`video` must be \[v, 3, F, H, W\] with v = 1 .* or v = b = 4"):
        pipe(video=torch.zeros(3, 3, 9, 64, 96), **kw)
    one = dict(kw, prompt_embeds=kw["prompt_embeds"][:1], negative_prompt_embeds=kw["negative_prompt_embeds"][:1], num_videos_per_prompt=1,
               ref_img_states=kw["ref_img_states"][:1])
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=rf"`guidance_scale` as a list together with `{name}`.*one video per call with scalars"):
            pipe(guidance_scale=[6.0], **{name: object()}, **one)
        with pytest.raises(ValueError, match=rf"`{name}` with 4 videos per call.*one video per call"):
            pipe(guidance_scale=[6.0] * 4, **{name: object()}, **kw)
    # the refusals that need the scheduler (a host object) and nothing else
    from types import SimpleNamespace

    vae, tr = object(), SimpleNamespace(dtype=DT, device=torch.device("cpu"))   # a transformer with no engine: the dtype the plans are made for
    for kind in ("ddim", "dpm"):
        pv = P(tr, _sched(s2v, kind), vae)
        with pytest.raises(ValueError, match=r"strength 0.1 keeps none of the 4 timesteps"):
            pv(strength=[0.5, 0.1, 1.0, 1.0], num_inference_steps=4, video=torch.zeros(1, 3, 9, 64, 96), **dict(kw, num_frames=9))
    dpm = P(tr, _sched(s2v, "dpm"))
    for gen in (None, torch.Generator().manual_seed(1)):
        with pytest.raises(ValueError, match=r"plans of \[2, 4, 3, 3\] steps under the DPM scheduler with a single generator.*list of 4 generators"):
            dpm(num_inference_steps=[2, 4, 3, 3], generator=gen, **kw)
    # DDIM draws nothing in the loop: different lengths with one generator pass the plan check (and then reach for the engine)
    with pytest.raises(AttributeError):
        P(tr, _sched(s2v, "ddim"))(num_inference_steps=[2, 4, 3, 3], generator=torch.Generator().manual_seed(1), **kw)


def test_check_per_video_and_check_batch_return_what_they_did(s2v):
    P = s2v.S2VPipeline
    assert P.check_per_video(3, 6.0, 50, 0.8) == ([6.0] * 3, [50] * 3, [0.8] * 3)
    assert P.check_per_video(2, [3.0, 4.0], 50, [0.5, 1.0], video=object()) == ([3.0, 4.0], [50, 50], [0.5, 1.0])
    kw = _args()
    pe, ref = kw["prompt_embeds"], kw["ref_img_states"]
    assert P.check_batch(pe, 2, ref) == 4 and P.check_batch(pe, 2, ref[:1]) == 4 and P.check_batch(pe, 1, ref[:2]) == 2
    assert P.check_batch(pe[:1], 1, ref[:1], cfg_parallel=object(), ulysses=object()) == 1
    assert P.check_batch(pe[:1], 1, ref[:1], None, None, torch.zeros(1, 3, 9, 64, 96)) == 1
    assert P.check_batch(pe, 2, ref, torch.zeros(4, 2, 16, 8, 12), [torch.Generator() for _ in range(4)]) == 4
    with pytest.raises(ValueError, match="at most 4 videos"):
        P.check_batch(pe, 3, ref[:1])
    with pytest.raises(ValueError, match="one row per video"):
        P.check_batch(pe, 2, ref[:3])
    # new ground: several videos with one shared input video, or one each
    assert P.check_batch(pe, 2, ref, None, None, torch.zeros(1, 3, 9, 64, 96)) == 4
    assert P.check_batch(pe, 2, ref, None, None, torch.zeros(4, 3, 9, 64, 96)) == 4


def test_add_noise_refuses_a_timestep_count_that_is_neither_one_nor_the_rows(s2v):
    sch = _sched(s2v, "ddim")
    x = torch.zeros(3, 2, 16, 8, 12)
    with pytest.raises(ValueError, match="2 timesteps for samples of shape"):
        sch.add_noise(x, x, torch.tensor([999, 500]))


def test_the_new_entry_is_declared_bound_and_exported(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bs2v_denoise_step_videos\s*\(", code) and "s2v_denoise_step_videos" in s2v._lib._SIGS
    assert hasattr(s2v.lib(), "s2v_denoise_step_videos")


def test_inference_passes_one_input_video_per_row_and_the_lists_through(s2v):
    import numpy as np
    from types import SimpleNamespace

    vg = s2v.video_generate
    vae = SimpleNamespace(device=torch.device("cpu"), dtype=torch.float32)
    clips = np.random.default_rng(5).integers(0, 256, (3, 9, 16, 24, 3), dtype=np.uint8)
    x = vg._video_tensor(vae, clips)
    assert tuple(x.shape) == (3, 3, 9, 16, 24)
    for k in range(3):
        assert torch.equal(x[k:k + 1], vg._video_tensor(vae, clips[k]))
    with pytest.raises(ValueError, match="resize"):
        vg.inference(None, None, None, None, None, height=480, width=720, video_uint8=clips)
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
    out = vg.inference(pipe, enc, np.zeros((16, 24, 3), np.uint8), torch.zeros(3, 4, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long),
                       height=16, width=24, video_uint8=clips, strength=[0.5, 1.0, 0.75], guidance_scale=[3.0, 4.5, 6.0],
                       num_inference_steps=[4, 4, 4])
    assert out.shape[0] == 3 and tuple(seen["video"].shape) == (3, 3, 9, 16, 24) and seen["num_frames"] == 9
    assert seen["strength"] == [0.5, 1.0, 0.75] and seen["guidance_scale"] == [3.0, 4.5, 6.0] and seen["num_inference_steps"] == [4, 4, 4]
    seen.clear()
    vg.inference(pipe, enc, np.zeros((16, 24, 3), np.uint8), torch.zeros(3, 4, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long),
                 height=16, width=24, strength=[0.5, 1.0, 0.75])
    assert seen["strength"] == [0.5, 1.0, 0.75], "a strength list without a video reaches the pipeline, which refuses it"
