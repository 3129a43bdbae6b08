"""Temporal windows without a device: the plan (weights, starts, counts, coverage, sums), every refusal of the definition and of the pipeline by
message, the loop with a recording engine, the ABI, and the emulation of the kernel's gather (tests/temporal_windows_ref.py) against the scatter
that defines the blend -- bit for bit, with mutations that the comparison must catch."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import temporal_windows_ref as TW
from conftest import ROOT

DT = torch.bfloat16
G = float(np.float32(6.2831855))   # a full fp32 mantissa: with 6.0 every product of a bf16 value is exact and an fma changes nothing


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ the plan
def test_the_literal_weights(s2v):
    for mod in (s2v.pipeline, TW):
        assert mod.window_weights(13, "pyramid") == [1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1]
        assert mod.window_weights(4, "pyramid") == [1, 2, 2, 1]
        assert mod.window_weights(3, "pyramid") == [1, 2, 1]
        assert mod.window_weights(1, "pyramid") == [1] and mod.window_weights(2, "pyramid") == [1, 1]
        assert mod.window_weights(5, "flat") == [1] * 5
    with pytest.raises(ValueError, match="weighting must be one of"):
        s2v.pipeline.window_weights(3, "delayed_reverse_sawtooth")


PLANS = {
    # (L, F, s): (starts, pyramid sums, flat sums)
    (5, 3, 1): ([0, 1, 2], [1, 3, 4, 3, 1], [1, 2, 3, 2, 1]),
    (7, 3, 2): ([0, 2, 4], [1, 2, 2, 2, 2, 2, 1], [1, 1, 2, 1, 2, 1, 1]),
    (25, 13, 6): ([0, 6, 12], [1, 2, 3, 4, 5, 6, 8, 8, 8, 8, 8, 8, 9, 8, 8, 8, 8, 8, 8, 6, 5, 4, 3, 2, 1], [1] * 6 + [2] * 6 + [3] + [2] * 6 + [1] * 6),
    (13, 13, 5): ([0], [1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1], [1] * 13),
}


@pytest.mark.parametrize("lfs", list(PLANS))
def test_starts_counts_coverage_and_sums(s2v, lfs):
    L, F, s = lfs
    starts, pyramid, flat = PLANS[lfs]
    for weighting, wsum in (("pyramid", pyramid), ("flat", flat)):
        plan = s2v.pipeline.window_plan(L, F, s, weighting)
        assert plan == TW.window_plan(L, F, s, weighting), "the product's plan is the restated one"
        assert plan["starts"] == starts and plan["W"] == len(starts) == (L - F) // s + 1
        assert plan["wsum"] == wsum and all(x > 0 for x in plan["wsum"]), "every frame is covered"
        covered = sorted(set(k0 + j for k0 in starts for j in range(F)))
        assert covered == list(range(L)) and starts[-1] + F == L, "the windows tile the L frames exactly"


def test_every_refusal_of_the_definition_names_its_reason(s2v):
    T, P = s2v.TemporalWindows, s2v.pipeline
    assert T().plan(97)["W"] == 3 and T().plan(49)["W"] == 1 and T().plan(145)["W"] == 5
    assert T(9, 8).plan(25)["starts"] == [0, 2, 4] and (T(9, 8).plan(25)["L"], T(9, 8).plan(25)["F"], T(9, 8).plan(25)["s"]) == (7, 3, 2)
    with pytest.raises(ValueError, match=r"num_frames must be 4k \+ 1, got 98.*nearest valid num_frames are 97 and 121"):
        T().plan(98)
    with pytest.raises(ValueError, match="num_frames = 101 is no whole number of windows.*nearest valid num_frames are 97 and 121"):
        T().plan(101)
    with pytest.raises(ValueError, match="num_frames = 33 is no whole number of windows.*nearest valid num_frames are 49 and 73"):
        T().plan(33)   # L < F
    with pytest.raises(ValueError, match="nearest valid num_frames are 25 and 33"):
        T(9, 8).plan(29)
    for wf in (48, 53, 0, 50):
        with pytest.raises(ValueError, match=r"window_frames must be 4k \+ 1 and at most 49"):
            T(wf, 8).plan(97)
    for sf in (6, 0, -4, 2):
        with pytest.raises(ValueError, match="stride_frames must be a positive multiple of 4"):
            T(9, sf).plan(25)
    with pytest.raises(ValueError, match="beyond the window's 3"):
        T(9, 16).plan(25)
    assert T(9, 12).plan(21)["starts"] == [0, 3], "s = F: the windows abut"
    with pytest.raises(ValueError, match="weighting must be one of"):
        T(9, 8, "sawtooth").plan(25)
    with pytest.raises(ValueError, match="per_forward = 2 does not divide the 3 windows"):
        T(9, 8, per_forward=2).plan(25)
    assert T(9, 8, per_forward=3).plan(25)["per_forward"] == 3
    for pf in (0, 5):
        with pytest.raises(ValueError, match="per_forward must be 1..4"):
            T(9, 4, per_forward=pf).plan(25)
    with pytest.raises(ValueError, match=r"L = 6 latent frames are no whole number.*L = 5 and L = 7"):
        P.window_plan(6, 3, 2)
    with pytest.raises(ValueError, match="stride of 1 <= s <= F"):
        P.window_plan(7, 3, 4)
    with pytest.raises(ValueError, match="stride of 1 <= s <= F"):
        P.window_plan(7, 3, 0)


def test_every_pipeline_refusal_names_its_reason(s2v):
    P, tw = s2v.S2VPipeline, s2v.TemporalWindows(9, 8)
    assert P.check_windows(tw, 25)["W"] == 3
    with pytest.raises(ValueError, match="must be a TemporalWindows"):
        P.check_windows((9, 8), 25)
    for name in ("mask", "change_map", "step_cache", "attention_map", "subject_guidance_scale", "cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=f"`temporal_windows` together with `{name}`"):
            P.check_windows(tw, 25, **{name: object()})
    with pytest.raises(ValueError, match="`temporal_windows` together with a per-video list"):
        P.check_windows(tw, 25, per_video=True)
    with pytest.raises(ValueError, match="`temporal_windows` with 2 videos per call"):
        P.check_windows(tw, 25, b=2)
    with pytest.raises(ValueError, match="`temporal_windows` together with fused=False"):
        P.check_windows(tw, 25, fused=False)
    with pytest.raises(ValueError, match="nearest valid num_frames are 25 and 33"):
        P.check_windows(tw, 29)


# ------------------------------------------------------------------------------------------------ the loop with a recording engine
class Recorder:
    """what the fused loop needs of an S2VEngine; its windowed step halves the long latent"""
    fp8_qk_active = False
    cfg = SimpleNamespace(attn_p_format="bf16")

    def __init__(self):
        self.calls, self.geometry = [], None

    def set_geometry(self, *geo):
        self.geometry = geo
        self.calls.append(("set_geometry", geo))

    def prepare_tables(self, height, width):
        self.calls.append(("prepare_tables", (height, width)))

    def set_conditioning(self, text, ref):
        self.calls.append(("set_conditioning", (text.clone(), ref.clone())))

    def set_windows(self, L, stride, weights, per_forward=1):
        self.calls.append(("set_windows", (L, stride, list(weights), per_forward)))

    def clear_windows(self):
        self.calls.append(("clear_windows", ()))

    def denoise_step(self, latents, timestep, coef, x0_hist=None, noise=None, use_graph=False, blend=None, cache=None, attn_layers=None):
        self.calls.append(("step", tuple(latents.shape)))
        latents.mul_(0.5)

    def denoise_step_windows(self, latents, timestep, coef, x0_hist=None, noise=None, use_graph=False):
        self.calls.append(("step_windows", (tuple(latents.shape), float(timestep), coef.guidance, None if noise is None else tuple(noise.shape))))
        latents.mul_(0.5)


def _pipe(s2v, dpm=False):
    eng = Recorder()
    tr = SimpleNamespace(engine=eng, dtype=DT, device=torch.device("cpu"),
                         config=SimpleNamespace(in_channels=16, use_rotary_positional_embeddings=True, num_layers=2))
    sch = (s2v.CogVideoXDPMScheduler if dpm else s2v.CogVideoXDDIMScheduler)(snr_shift_scale=1.0)
    return s2v.S2VPipeline(tr, sch), eng


def _inputs(b=1, num_frames=25):
    g = torch.Generator().manual_seed(1)
    return dict(prompt_embeds=torch.randn(b, 5, 8, generator=g), negative_prompt_embeds=torch.randn(b, 5, 8, generator=g),
                ref_img_states=torch.randn(1, 1, 16, 8, 12, generator=g), height=64, width=96, num_frames=num_frames,
                generator=torch.Generator().manual_seed(50))


def test_without_temporal_windows_the_length_limit_and_the_calls_are_what_they_were(s2v):
    pipe, eng = _pipe(s2v)
    with pytest.raises(ValueError, match="less than or equal to 49 due to static positional embeddings"):
        pipe(num_inference_steps=2, guidance_scale=6.0, **_inputs(1, 53))
    assert eng.calls == []
    pipe(num_inference_steps=2, guidance_scale=6.0, **_inputs(1, 5))
    assert [c[0] for c in eng.calls] == ["set_geometry", "prepare_tables", "set_conditioning", "step", "step"]


@pytest.mark.parametrize("per_forward", [1, 3])
def test_the_windowed_loop_sets_the_windows_geometry_and_steps_the_long_latent(s2v, per_forward):
    pipe, eng = _pipe(s2v, dpm=True)
    inp = _inputs(1, 25)
    seen = []

    def cb(p, i, t, tensors):
        seen.append(tuple(tensors["latents"].shape))
        return {}

    out = pipe(num_inference_steps=2, guidance_scale=6.0, temporal_windows=s2v.TemporalWindows(9, 8, "pyramid", per_forward),
               callback_on_step_end=cb, **inp)["frames"]
    assert [c[0] for c in eng.calls] == ["set_geometry", "prepare_tables", "set_conditioning", "set_windows", "step_windows", "step_windows",
                                         "clear_windows"]
    assert eng.calls[0][1] == (2 * per_forward, 5, 3, 8, 12), "B = 2 per_forward samples of the WINDOW's frames"
    text, ref = eng.calls[2][1]
    neg, pos = inp["negative_prompt_embeds"].to(DT), inp["prompt_embeds"].to(DT)
    assert torch.equal(text, torch.cat([neg] * per_forward + [pos] * per_forward)) and tuple(ref.shape) == (1, 1, 16, 8, 12)
    assert eng.calls[3][1] == (7, 2, [1.0, 2.0, 1.0], per_forward)
    long = (1, 7, 16, 8, 12)
    assert all(c[1][0] == long and c[1][2] == 6.0 and c[1][3] == long for c in eng.calls if c[0] == "step_windows")
    assert seen == [long, long] and tuple(out.shape) == long
    start = torch.randn(long, generator=torch.Generator().manual_seed(50), dtype=DT)
    assert torch.equal(out, start * 0.25)


def test_a_refused_windowed_call_touches_no_engine(s2v):
    pipe, eng = _pipe(s2v)
    tw = s2v.TemporalWindows(9, 8)
    kw = dict(num_inference_steps=2, guidance_scale=6.0, temporal_windows=tw)
    with pytest.raises(ValueError, match="nearest valid num_frames are 25 and 33"):
        pipe(**kw, **_inputs(1, 29))
    with pytest.raises(ValueError, match="`temporal_windows` with 2 videos per call"):
        pipe(**kw, **_inputs(2, 25))
    with pytest.raises(ValueError, match="`temporal_windows` with 2 videos per call"):
        pipe(num_videos_per_prompt=2, **kw, **_inputs(1, 25))
    with pytest.raises(ValueError, match="`temporal_windows` together with `step_cache`"):
        pipe(step_cache=0.1, **kw, **_inputs(1, 25))
    with pytest.raises(ValueError, match="`temporal_windows` together with `attention_map`"):
        pipe(attention_map=s2v.AttentionMap([0]), **kw, **_inputs(1, 25))
    with pytest.raises(ValueError, match="`temporal_windows` together with `subject_guidance_scale`"):
        pipe(subject_guidance_scale=2.0, **kw, **_inputs(1, 25))
    with pytest.raises(ValueError, match="`temporal_windows` together with a per-video list"):
        pipe(num_inference_steps=[2], guidance_scale=6.0, temporal_windows=tw, **_inputs(1, 25))
    with pytest.raises(ValueError, match="`temporal_windows` together with fused=False"):
        pipe(fused=False, **kw, **_inputs(1, 25))
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=f"`temporal_windows` together with `{name}`"):
            pipe(**{name: object()}, **kw, **_inputs(1, 25))
    assert eng.calls == []


def test_inference_passes_temporal_windows_through(s2v):
    import inspect
    assert inspect.signature(s2v.video_generate.inference).parameters["temporal_windows"].default is None
    assert inspect.signature(s2v.S2VPipeline.__call__).parameters["temporal_windows"].default is None


def test_the_new_symbols_are_declared_and_bound(s2v):
    with open(os.path.join(ROOT, "include", "s2v_hip.h")) as f:
        h = f.read()
    for name, nargs in (("s2v_set_windows", 5), ("s2v_denoise_step_windows", 8), ("s2v_op_window_blend", 13)):
        assert re.search(rf"S2V_API int {name}\(", h), name
        assert len(s2v._lib._SIGS[name]) == nargs, name


# ------------------------------------------------------------------------------------------------ the gather against the scatter
def _windows(plan, dt, seed=7, tail=(16, 35)):
    """the negative and the positive prediction of every window, [W, F, C, HW], with the values dt can hold"""
    g = torch.Generator().manual_seed(seed)
    shape = (plan["W"], plan["F"]) + tail
    return torch.randn(shape, generator=g).to(dt), torch.randn(shape, generator=g).to(dt)


CONFIGS = [(5, 3, 1), (7, 3, 2), (6, 3, 3), (25, 13, 6)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("weighting", ["flat", "pyramid"])
def test_the_gather_equals_the_scatter_bit_for_bit(dt, weighting):
    for L, F, s in CONFIGS:
        plan = TW.window_plan(L, F, s, weighting)
        neg, pos = _windows(plan, dt)
        exp = TW.blend_scatter(neg, pos, G, plan)
        assert torch.isfinite(exp).all()
        for pf in sorted({1, plan["W"]}):
            got = TW.blend_gather(neg, pos, G, plan, pf)
            assert _bits_equal(got, exp), f"(L, F, s) = {(L, F, s)}, per_forward {pf}"


def test_the_scatter_divides_as_numpy_does():
    """the restatement's `/` is IEEE division, not a multiplication by a rounded reciprocal"""
    plan = TW.window_plan(5, 3, 1, "pyramid")
    neg, pos = _windows(plan, torch.float32)
    n, p = neg.numpy(), pos.numpy()
    acc = np.zeros((5,) + n.shape[2:], dtype=np.float32)
    for k in range(3):
        v = (n[k] + (np.float32(G) * (p[k] - n[k]).astype(np.float32)).astype(np.float32)).astype(np.float32)
        for j in range(3):
            acc[k + j] = (acc[k + j] + (np.float32(plan["weights"][j]) * v[j]).astype(np.float32)).astype(np.float32)
    exp = (acc / np.asarray(plan["wsum"], dtype=np.float32)[:, None, None]).astype(np.float32)
    assert np.array_equal(TW.blend_scatter(neg, pos, G, plan).numpy().view(np.uint32), exp.view(np.uint32))


# the configuration on which each mutation must show: (L, F, s), weighting, per_forward
MUTATION_CASES = {
    "descending": ((5, 3, 1), "pyramid", 3),        # three windows over the middle frame in ONE batch: fp32 addition does not associate
    "fma": ((5, 3, 1), "flat", 1),
    "global_weight": ((7, 3, 2), "pyramid", 1),     # window 1 starts at frame 2: w[f mod 3] is not w[j]
    "drop_last_frame": ((7, 3, 2), "flat", 3),
    "batch_wsum": ((5, 3, 1), "pyramid", 1),        # a batch of one window sums one weight
    "reciprocal": ((5, 3, 1), "pyramid", 3),        # sums of 3: 1 / 3 is not an fp32 number
}


@pytest.mark.parametrize("name", list(TW.MUTATIONS))
def test_every_mutation_of_the_gather_differs_from_the_scatter(name):
    assert set(MUTATION_CASES) == set(TW.MUTATIONS) and len(TW.MUTATIONS) >= 5
    (L, F, s), weighting, pf = MUTATION_CASES[name]
    plan = TW.window_plan(L, F, s, weighting)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        neg, pos = _windows(plan, dt)
        exp = TW.blend_scatter(neg, pos, G, plan)
        assert _bits_equal(TW.blend_gather(neg, pos, G, plan, pf), exp), f"{dt}: the unmutated gather passes"
        assert not _bits_equal(TW.blend_gather(neg, pos, G, plan, pf, mutate=name), exp), f"{dt}: the comparison does not catch `{name}`"
