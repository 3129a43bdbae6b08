"""Subject guidance without a device: the torch restatement (tests/subject_guidance_ref.py) against the reference's scheduler bits and against a
numpy emulation of the kernel's combine whose mutations the checks must catch, the host logic of the pipeline (layout, per-video lists, every
refusal by message, the loop with a recording engine) and the ABI (header, ctypes binding)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import subject_guidance_ref as SG
from conftest import ROOT, load_golden

DT = torch.bfloat16
F32 = np.float32
# scales with full fp32 mantissas: with 2.5 and 6.0 every product of a bf16 plane is exact, and a re-association or an fma changes nothing
GS, GT = float(F32(2.7182817)), float(F32(6.2831855))


# ------------------------------------------------------------------------------------------------ the combine: emulation, checks, mutations
def _emu(u, r, f, gs, gt):
    """numpy mirror of the triple combine of sched_step_k: five separately rounded fp32 operations"""
    s = (u + (F32(gs) * (r - u).astype(F32)).astype(F32)).astype(F32)
    return (s + (F32(gt) * (f - r).astype(F32)).astype(F32)).astype(F32)


def _fma(a, b, c):
    """a * b + c with one rounding: the product of two fp32 values is exact in fp64"""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F32)


MUTATIONS = {
    "u and r swapped": lambda u, r, f, gs, gt: _emu(r, u, f, gs, gt),
    "scales swapped": lambda u, r, f, gs, gt: _emu(u, r, f, gt, gs),
    "f - u for f - r": lambda u, r, f, gs, gt: ((u + (F32(gs) * (r - u).astype(F32)).astype(F32)).astype(F32)
                                                + (F32(gt) * (f - u).astype(F32)).astype(F32)).astype(F32),
    "re-associated": lambda u, r, f, gs, gt: (u + ((F32(gs) * (r - u).astype(F32)).astype(F32)
                                                   + (F32(gt) * (f - r).astype(F32)).astype(F32)).astype(F32)).astype(F32),
    "fma": lambda u, r, f, gs, gt: _fma((f - r).astype(F32), F32(gt), _fma((r - u).astype(F32), F32(gs), u)),
}


def _planes(dt=torch.bfloat16, n=1680, seed=5):
    """three independent random planes with the values a model dtype can hold"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(dt).float().numpy() for _ in range(3)]


def _check_restatement(impl):
    """the combine equals the restatement bit for bit on independent planes, g_subject != g_text, neither 1"""
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        u, r, f = _planes(dt)
        exp = SG.combine(*(torch.from_numpy(p) for p in (u, r, f)), GS, GT).numpy()
        if not np.array_equal(impl(u, r, f, GS, GT).view(np.uint32), exp.view(np.uint32)):
            return False
    return True


def _check_degenerate(impl):
    """with the u plane holding the r plane's bits the result is the pair's r + g_text (f - r), whatever g_subject"""
    _, r, f = _planes()
    exp = SG.pair_combine(torch.from_numpy(r), torch.from_numpy(f), 6.0).numpy()
    return all(np.array_equal(impl(r.copy(), r, f, gs, 6.0).view(np.uint32), exp.view(np.uint32)) for gs in (0.5, 1.0, 7.5))


def _check_nested(impl):
    """g_subject = 1 is today's call mathematically: within a few fp32 roundings of the pair's combine on [r | f]"""
    u, r, f = _planes()
    exp = SG.pair_combine(torch.from_numpy(r), torch.from_numpy(f), 6.0).numpy()
    got = impl(u, r, f, 1.0, 6.0)
    scale = np.abs(u) + np.abs(r) + 6.0 * (np.abs(f) + np.abs(r))
    return bool((np.abs(got - exp) <= 4 * np.finfo(F32).eps * scale).all())


CHECKS = (_check_restatement, _check_degenerate, _check_nested)


def test_the_emulated_combine_passes_every_check():
    assert all(c(_emu) for c in CHECKS)


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_every_mutation_changes_an_element_and_fails_a_check(name):
    for dt in (torch.bfloat16, torch.float16, torch.float32):   # the planes of _check_restatement, every dtype of them
        u, r, f = _planes(dt)
        assert not np.array_equal(MUTATIONS[name](u, r, f, GS, GT).view(np.uint32), _emu(u, r, f, GS, GT).view(np.uint32)), \
            f"the {dt} inputs must make the mutation visible"
    assert not all(c(MUTATIONS[name]) for c in CHECKS), f"no check catches: {name}"


def test_the_degenerate_identity_holds_in_the_restatement_for_any_subject_scale():
    _, r, f = (torch.from_numpy(p) for p in _planes())
    exp = SG.pair_combine(r, f, 6.0)
    for gs in (0.5, 1.0, 7.5, -3.0, 1e6):
        assert torch.equal(SG.combine(r.clone(), r, f, gs, 6.0), exp)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["f32", "bf16"])
def test_the_restated_step_reproduces_the_reference_bits_through_the_degenerate_triple(s2v, kind, dt_name):
    """the golden steps of the reference's schedulers (tests/golden/sched_*.npz), run as a triple whose u plane is the r plane: the scheduler
    arithmetic of the restatement is the reference's, bit for bit"""
    g = load_golden(f"sched_{kind}_{dt_name}_10.npz")
    dt = torch.bfloat16 if dt_name == "bf16" else torch.float32
    sch = (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=float(g["snr"]))
    sch.set_timesteps(10)
    ids, checked = list(g["step_ids"]), 0
    for i in ids:
        t = sch.timesteps[i]
        if kind == "ddim":
            c, x0_old, noise = sch.coef(t, dt, 6.0, guidance_subject=3.25), None, None
        else:
            if i > 0 and (i - 1) not in ids:
                continue
            c = sch.coef(t, sch.timesteps[i - 1] if i > 0 else None, i == 0, dt, 6.0, guidance_subject=3.25)
            x0_old = torch.from_numpy(g[f"x0_{i - 1}"]) if i > 0 else None
            noise = torch.from_numpy(g[f"n2_{i}"] if c.kind == 2 else g[f"n1_{i}"]).to(dt)
        assert c.guidance_subject == 3.25
        npred = torch.from_numpy(g[f"noise_pred_{i}"])
        triple = torch.cat([npred[0:1], npred[0:1], npred[1:2]])
        prev, x0 = SG.triple_step(c, triple, torch.from_numpy(g[f"lat_in_{i}"]).to(dt), x0_old, noise, dt)
        assert np.array_equal(x0.numpy(), g[f"x0_{i}"]), f"x0 step {i}"
        assert np.array_equal(SG.rnd(prev, dt).numpy(), g[f"lat_out_{i}"]), f"latents step {i}"
        checked += 1
    assert checked >= 2


# ------------------------------------------------------------------------------------------------ host logic
def test_layout_is_u_r_f_blocks_with_the_negative_text_twice_and_a_table_row_per_sample(s2v):
    for b in (1, 2):
        lay = s2v.pipeline.subject_layout(b)
        assert [e["sample"] for e in lay] == ["u"] * b + ["r"] * b + ["f"] * b
        assert [e["video"] for e in lay] == list(range(b)) * 3
        # text rows of [negative x b | positive x b]: [neg | neg | pos]
        assert [e["text"] for e in lay] == list(range(b)) * 2 + list(range(b, 2 * b))
        assert [e["ref"] for e in lay] == ["null"] * b + ["ref"] * (2 * b)
        assert [e["entry"] for e in lay] == list(range(3 * b)), "one table row per sample: j mod 3b is j"
    for b in (0, 3):
        with pytest.raises(ValueError, match="1..2 videos"):
            s2v.pipeline.subject_layout(b)


def test_per_video_list_validation(s2v):
    P = s2v.S2VPipeline
    ref = torch.zeros(2, 1, 16, 8, 12)
    assert P.check_subject_batch(2, 2.5, None, ref) == [2.5, 2.5]
    assert P.check_subject_batch(2, [0.5, 3], None, ref) == [0.5, 3.0]
    with pytest.raises(ValueError, match="list of 3 entries for b = 2"):
        P.check_subject_batch(2, [1.0, 2.0, 3.0], None, ref)
    with pytest.raises(ValueError, match="at most 2 videos"):
        P.check_subject_batch(3, 2.0, None, ref)
    with pytest.raises(ValueError, match="negative_ref_img_states"):
        P.check_subject_batch(2, 2.0, torch.zeros(3, 1, 16, 8, 12), ref)
    with pytest.raises(ValueError, match="negative_ref_img_states"):
        P.check_subject_batch(2, 2.0, torch.zeros(1, 1, 16, 8, 10), ref)
    with pytest.raises(ValueError, match="finite number"):
        P.check_subject("high", 6.0)
    with pytest.raises(ValueError, match="finite number"):
        P.check_subject([2.0, float("nan")], 6.0)


def test_the_coefficient_sets_carry_the_subject_scale_and_dynamic_cfg_leaves_it_alone(s2v):
    for cls in (s2v.CogVideoXDDIMScheduler, s2v.CogVideoXDPMScheduler):
        sch = cls(snr_shift_scale=1.0)
        plain = s2v.S2VPipeline.video_plan(sch, 4, None, 6.0, True, DT)
        plan = s2v.S2VPipeline.video_plan(sch, 4, None, 6.0, True, DT, guidance_subject=2.5)
        assert [st["coef"].guidance_subject for st in plan["steps"]] == [2.5] * 4
        assert [st["coef"].guidance_subject for st in plain["steps"]] == [0.0] * 4
        assert [st["guidance"] for st in plan["steps"]] == [st["guidance"] for st in plain["steps"]]
        assert len({st["guidance"] for st in plan["steps"]}) > 1, "dynamic CFG moves the text scale"


class Recorder:
    """what the fused loop needs of an S2VEngine; its step halves the latents"""
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

    def set_conditioning_triples(self, text, ref, null):
        self.calls.append(("set_conditioning_triples", (text.clone(), ref.clone(), null.clone())))

    def denoise_step(self, latents, timestep, coef, x0_hist=None, noise=None, use_graph=False, blend=None, cache=None, attn_layers=None,
                     subject=False):
        assert blend is None and cache is None and attn_layers is None
        self.calls.append(("guided_step" if subject else "step", (latents.shape[0], [float(t) for t in timestep],
                                                                  [(c.guidance, c.guidance_subject) for c in coef])))
        latents.mul_(0.5)


def _pipe(s2v, eng=None):
    eng = eng or Recorder()
    tr = SimpleNamespace(engine=eng, dtype=DT, device=torch.device("cpu"),
                         config=SimpleNamespace(in_channels=16, use_rotary_positional_embeddings=True, num_layers=2))
    return s2v.S2VPipeline(tr, s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0)), eng


def _inputs(b):
    g = torch.Generator().manual_seed(1)
    return dict(prompt_embeds=torch.randn(b, 5, 8, generator=g), negative_prompt_embeds=torch.randn(b, 5, 8, generator=g),
                ref_img_states=torch.randn(b, 1, 16, 8, 12, generator=g), height=64, width=96, num_frames=5,
                generator=[torch.Generator().manual_seed(50 + k) for k in range(b)])


def test_none_never_calls_a_triple_entry(s2v):
    pipe, eng = _pipe(s2v)
    pipe(num_inference_steps=[2, 3], guidance_scale=6.0, subject_guidance_scale=None, **_inputs(2))
    names = [c[0] for c in eng.calls]
    assert "set_conditioning_triples" not in names and "guided_step" not in names
    assert names.count("step") == 3 and [c[1] for c in eng.calls if c[0] == "set_geometry"] == [(4, 5, 2, 8, 12), (2, 5, 2, 8, 12)]
    assert all(gs == 0.0 for c in eng.calls if c[0] == "step" for _, gs in c[1][2]), "the pair call's coefficient sets are built as before"


def test_the_triple_loop_follows_the_plans_longest_first_and_shrinks_from_two_videos_to_one(s2v):
    pipe, eng = _pipe(s2v)
    inp = _inputs(2)
    null = torch.randn(2, 1, 16, 8, 12, generator=torch.Generator().manual_seed(9))
    out = pipe(num_inference_steps=[2, 3], guidance_scale=[6.0, 4.0], subject_guidance_scale=[2.5, 0.5], negative_ref_img_states=null, **inp)["frames"]
    names = [c[0] for c in eng.calls]
    assert names == ["set_geometry", "prepare_tables", "set_conditioning_triples", "guided_step", "guided_step",
                     "set_geometry", "prepare_tables", "set_conditioning_triples", "guided_step"]
    assert [c[1] for c in eng.calls if c[0] == "set_geometry"] == [(6, 5, 2, 8, 12), (3, 5, 2, 8, 12)]
    neg, pos, ref = (inp[k].to(DT) for k in ("negative_prompt_embeds", "prompt_embeds", "ref_img_states"))
    conds = [c[1] for c in eng.calls if c[0] == "set_conditioning_triples"]
    # the internal order is longest plan first: video 1 (3 steps), then video 0; the text goes in as [negative x a | positive x a]
    for a, (text, r, n) in zip((2, 1), conds):
        rows = [1, 0][:a]
        assert torch.equal(text, torch.cat([neg[rows], pos[rows]])) and torch.equal(r, ref[rows]) and torch.equal(n, null.to(DT)[rows])
    steps = [c[1] for c in eng.calls if c[0] == "guided_step"]
    assert [s[0] for s in steps] == [2, 2, 1]
    assert [s[2] for s in steps] == [[(4.0, 0.5), (6.0, 2.5)], [(4.0, 0.5), (6.0, 2.5)], [(4.0, 0.5)]]
    for k, n in enumerate((2, 3)):   # the caller's order comes back
        start = torch.randn((1, 2, 16, 8, 12), generator=torch.Generator().manual_seed(50 + k), dtype=DT)
        assert torch.equal(out[k:k + 1], start * 0.5 ** n)


def test_a_scalar_scale_and_the_default_null_reference(s2v):
    pipe, eng = _pipe(s2v)
    inp = _inputs(2)
    pipe(num_inference_steps=2, guidance_scale=6.0, subject_guidance_scale=3.0, **inp)
    text, ref, null = [c[1] for c in eng.calls if c[0] == "set_conditioning_triples"][0]
    assert tuple(null.shape) == (1, 1, 16, 8, 12) and not null.any(), "the default null reference is one row of zeros, the zero latent"
    assert tuple(ref.shape) == (2, 1, 16, 8, 12) and tuple(text.shape) == (4, 5, 8)
    assert [c[1][2] for c in eng.calls if c[0] == "guided_step"] == [[(6.0, 3.0)] * 2] * 2
    # one shared reference row becomes one row per video: the triples entry takes b rows
    pipe, eng = _pipe(s2v)
    inp["ref_img_states"] = inp["ref_img_states"][:1]
    pipe(num_inference_steps=2, guidance_scale=6.0, subject_guidance_scale=3.0, **inp)
    assert tuple([c[1] for c in eng.calls if c[0] == "set_conditioning_triples"][0][1].shape) == (2, 1, 16, 8, 12)


def test_every_refusal_names_its_reason_and_touches_no_engine(s2v):
    pipe, eng = _pipe(s2v)
    kw = dict(num_inference_steps=2, subject_guidance_scale=2.0)
    with pytest.raises(ValueError, match="at most 2 videos"):
        pipe(guidance_scale=6.0, **kw, **_inputs(3))
    for g in (1.0, 0.5, [6.0, 1.0]):
        with pytest.raises(ValueError, match="without CFG there is nothing to extend"):
            pipe(guidance_scale=g, **kw, **_inputs(2))
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=f"`subject_guidance_scale` together with `{name}`"):
            pipe(guidance_scale=6.0, **{name: object()}, **kw, **_inputs(1))
    with pytest.raises(ValueError, match="`subject_guidance_scale` together with `step_cache`"):
        pipe(guidance_scale=6.0, step_cache=0.1, **kw, **_inputs(1))
    with pytest.raises(ValueError, match="`subject_guidance_scale` together with `attention_map`"):
        pipe(guidance_scale=6.0, attention_map=s2v.pipeline.AttentionMap([0]), **kw, **_inputs(1))
    with pytest.raises(ValueError, match="`subject_guidance_scale` together with fused=False"):
        pipe(guidance_scale=6.0, fused=False, **kw, **_inputs(1))
    with pytest.raises(ValueError, match="list of 1 entries for b = 2"):
        pipe(guidance_scale=6.0, num_inference_steps=2, subject_guidance_scale=[2.0], **_inputs(2))
    with pytest.raises(ValueError, match="only together with `subject_guidance_scale`"):
        pipe(guidance_scale=6.0, num_inference_steps=2, negative_ref_img_states=torch.zeros(1, 1, 16, 8, 12), **_inputs(1))
    assert eng.calls == []


def test_inference_passes_the_scale_through_and_leaves_local_reference_scale_alone(s2v):
    import inspect
    sig = inspect.signature(s2v.video_generate.inference)
    assert sig.parameters["subject_guidance_scale"].default is None
    assert "local_reference_scale" not in sig.parameters


# ------------------------------------------------------------------------------------------------ ABI
def _header():
    with open(os.path.join(ROOT, "include", "s2v_hip.h")) as f:
        return f.read()


def test_sched_coef_keeps_its_48_bytes_with_guidance_subject_where_pad_was(s2v):
    h = _header()
    body = re.search(r"typedef struct s2v_sched_coef \{(.*?)\} s2v_sched_coef;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int32_t|float)\s+([^;]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert [n for n, _ in fields] == ["kind", "guidance", "c_x0_x", "c_x0_v", "a_t", "b_t", "m1", "m2", "m3", "m4", "mn", "guidance_subject"]
    assert 4 * len(fields) == 48 and "pad" not in [n for n, _ in fields]
    C = s2v._lib.SchedCoefC
    assert ctypes.sizeof(C) == 48
    assert [(n, {ctypes.c_int32: "int32_t", ctypes.c_float: "float"}[t]) for n, t in C._fields_] == fields
    assert C.guidance_subject.offset == 44
    with open(os.path.join(ROOT, "disentangled-subject-to-vid_amd", "csrc", "kernels.h")) as f:
        k = re.search(r"struct SchedCoef \{(.*?)\};", f.read(), re.S).group(1)
    assert re.search(r"float m1, m2, m3, m4, mn;\s*float guidance_subject;", re.sub(r"//[^\n]*", "", k).replace("c_x0_x, c_x0_v, a_t, b_t, ", ""))


def test_the_new_symbols_are_declared_and_bound_and_max_batch_stays_8(s2v):
    h = _header()
    for name in ("s2v_set_conditioning_triples", "s2v_denoise_step_guided"):
        assert re.search(rf"S2V_API int {name}\(", h), name
        assert name in s2v._lib._SIGS
    assert len(s2v._lib._SIGS["s2v_set_conditioning_triples"]) == 6 and len(s2v._lib._SIGS["s2v_denoise_step_guided"]) == 9
    assert re.search(r"#define S2V_MAX_BATCH 8\b", h) and s2v.S2VEngine.MAX_BATCH == 8
    assert s2v._lib.SCHED_TRIPLE == 8 and "bit3" in h
