"""Temporal windows on the GPU (include/s2v_hip.h: s2v_set_windows, s2v_denoise_step_windows, s2v_op_window_blend;
S2VPipeline(temporal_windows=...)): a long latent stepped as overlapping windows of the geometry's frames, the windows' CFG pairs combined and
averaged where they overlap, one scheduler step on the whole of it.

No tolerance appears in this file: every claim is equality of bits -- the kernel against the torch restatement (tests/temporal_windows_ref.py), the
fused step against hand-driven pieces (the forward on every window slice, the restatement, s2v_sched_step), against plain steps where the
windows degenerate, per_forward = 3 against 1, the pipeline against hand-driven steps -- on the shapes where tests/test_gpu_batch_videos.py already
holds batches to bits (no GEMM splits K there).  The guidance scale has a full fp32 mantissa: with 6.0 every product of a bf16 value is exact and
an fma would change nothing.
"""
import ctypes

import numpy as np
import pytest
import torch

import temporal_windows_ref as TW
import test_gpu_batch_hetero as H
import test_gpu_batch_videos as BV

pytestmark = pytest.mark.gpu
DEV = BV.DEV
DT = BV.DT
STEPS = 3
G = float(np.float32(6.2831855))
CHW = 16 * 5 * 7        # one latent frame [C, H, W] = [16, 5, 7]: 560 elements = 2.19 blocks of 256 threads
SENT = 123.0
SLACK = 64
LFS = (5, 3, 1)         # the engine tests' long latent: three windows of three frames, all three over the middle frame, so the weights matter


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. the kernel against the restatement
def _run_blend(s2v, neg, pos, plan, pf, dt):
    """W / pf launches of s2v_op_window_blend on a plane that starts as NaN (a cell read before it was written poisons the result) with
    sentinels behind it; every launch's noise_pred is followed by NaN rows where the windows outside the batch would be -> plane [n + SLACK]"""
    lib, L = s2v.lib(), s2v._lib
    n = plan["L"] * CHW
    acc = torch.cat([torch.full((n,), float("nan"), device=DEV), torch.full((SLACK,), SENT, device=DEV)])
    w = torch.tensor(plan["weights"] + [float("nan")] * 4, dtype=torch.float32, device=DEV)
    wsum = torch.tensor(plan["wsum"] + [float("nan")] * 4, dtype=torch.float32, device=DEV)
    trap = torch.full((plan["W"] * plan["F"] * CHW,), float("nan"), dtype=dt, device=DEV)
    for k0 in range(0, plan["W"], pf):
        npred = torch.cat([neg[k0:k0 + pf].flatten(), pos[k0:k0 + pf].flatten(), trap]).contiguous()
        L.check(lib.s2v_op_window_blend(L.ptr(npred), L.ptr(acc), L.ptr(w), L.ptr(wsum), G, plan["L"], plan["F"], plan["s"], k0, pf, CHW,
                                        L.DTYPE_OF[dt], L.stream_ptr()))
    torch.cuda.synchronize()
    return acc


@pytest.mark.parametrize("weighting", ["flat", "pyramid"])
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
def test_blend_kernel_equals_the_restatement_bitwise(s2v, dt_name, weighting):
    dt = DT[dt_name]
    for L, F, s in ((7, 3, 2), (5, 3, 1)):
        plan = TW.window_plan(L, F, s, weighting)
        g = torch.Generator(device=DEV).manual_seed(191)
        neg = torch.randn((plan["W"], F, CHW), generator=g, device=DEV).to(dt)
        pos = torch.randn((plan["W"], F, CHW), generator=g, device=DEV).to(dt)
        exp = TW.blend_scatter(neg, pos, G, plan).to(DEV)
        assert torch.isfinite(exp).all()
        for pf in (1, plan["W"]):
            acc = _run_blend(s2v, neg, pos, plan, pf, dt)
            what = f"(L, F, s) = {(L, F, s)}, per_forward {pf}"
            assert torch.isfinite(acc[:L * CHW]).all(), f"{what}: a trap value leaked, or a plane cell was read before it was written"
            assert _same(acc[:L * CHW].view(L, CHW), exp), what
            assert bool((acc[L * CHW:] == SENT).all()), f"{what}: a write past element {L * CHW}"
    # the inputs tell a flat blend from a pyramid one where three windows meet (at (7, 3, 2) the two are the same blend: the overlaps weigh 1 : 1)
    other = TW.blend_scatter(neg, pos, G, TW.window_plan(5, 3, 1, "flat" if weighting == "pyramid" else "pyramid")).to(DEV)
    assert not torch.equal(other, exp)


def test_blend_kernel_refuses_windows_that_do_not_tile_and_batches_outside_them(s2v):
    lib, L = s2v.lib(), s2v._lib
    x = torch.zeros(8 * 3 * CHW, device=DEV)
    args = lambda Lf, F, s, k0, wb: (L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), G, Lf, F, s, k0, wb, CHW, L.DTYPE_F32, None)
    for bad in ((6, 3, 2, 0, 1), (7, 3, 4, 0, 1), (7, 3, 0, 0, 1), (2, 3, 1, 0, 1)):
        assert lib.s2v_op_window_blend(*args(*bad)) != 0 and b"must tile the L frames exactly" in lib.s2v_last_error(), bad
    for bad in ((7, 3, 2, 3, 1), (7, 3, 2, 2, 2), (7, 3, 2, 0, 0), (7, 3, 2, -1, 1)):
        assert lib.s2v_op_window_blend(*args(*bad)) != 0 and b"must lie inside 0 .. W - 1" in lib.s2v_last_error(), bad


# ------------------------------------------------------------------------------------------------ engines and plans
def _engine(s2v, case, dt, B, F):
    """an engine of `case` on B samples of F frames (the case's own F is the batch tests')"""
    m, eng = BV._engine(s2v, case, dt, B)
    _, T, _, Hh, W = BV.CASES[case]
    if eng.geometry != (B, T, F, Hh, W):
        eng.set_geometry(B, T, F, Hh, W)
        eng.prepare_tables(Hh * 8, W * 8)
    return m, eng


_LONG = {}


def _long_inputs(s2v, case, L):
    """a long latent [1, L, C, H, W] and DPM noise for every step, fp32 on the device: made once, never written"""
    if (case, L) not in _LONG:
        _, T, _, Hh, W = BV.CASES[case]
        g = torch.Generator(device=DEV).manual_seed(192)
        _LONG[case, L] = dict(lat=torch.randn(1, L, 16, Hh, W, generator=g, device=DEV), noise=torch.randn(STEPS, 1, L, 16, Hh, W, generator=g, device=DEV))
    return _LONG[case, L]


def _condition(s2v, eng, case, pf=1):
    inp = BV._inputs(s2v, case)
    eng.set_conditioning(torch.cat([inp["neg"][:1].expand(pf, -1, -1), inp["pos"][:1].expand(pf, -1, -1)]).contiguous(), inp["ref"][:1])


def _plan(s2v, kind, dt):
    """STEPS steps of one plan: [(timestep, coefficient set)]; DDIM is kind 0, the DPM plan runs kinds 1 and 2"""
    steps = s2v.S2VPipeline.video_plan(H._sched(s2v, kind), STEPS, None, G, False, dt)["steps"]
    assert {st["coef"].kind for st in steps} == ({0} if kind == "ddim" else {1, 2})
    return [(float(st["t"]), st["coef"]) for st in steps]


def _loop(plan, dt, lat, noise, dpm, step):
    """STEPS steps on a fresh clone of lat: step(x, t, coef, x0_hist, noise) updates x (and x0_hist) in place -> [(latents, x0_hist)] per step"""
    x = lat.to(dt).contiguous().clone()
    x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
    nz = torch.empty_like(x) if dpm else None
    out = []
    for i, (t, coef) in enumerate(plan):
        if dpm:
            nz.copy_(noise[i].to(dt))
        step(x, t, coef, x0, nz)
        torch.cuda.synchronize()
        out.append((x.clone(), x0.clone() if dpm else None))
    assert torch.isfinite(x.float()).all()
    return out


def _windowed(eng, plan, dt, lat, noise, dpm, graph):
    return _loop(plan, dt, lat, noise, dpm, lambda x, t, c, x0, nz: eng.denoise_step_windows(x, t, c, x0, nz, use_graph=graph))


def _equal_steps(got, exp, what):
    for i, ((x, x0), (ex, ex0)) in enumerate(zip(got, exp)):
        assert _same(x, ex), f"{what}, step {i}: latents"
        assert (x0 is None and ex0 is None) or _same(x0, ex0), f"{what}, step {i}: x0 history"


# ------------------------------------------------------------------------------------------------ 2. the step against hand-driven pieces
_HAND = {}


def _hand_driven(s2v, case, dt_name, kind, weighting):
    """the step in pieces on a B = 2 engine without windows: engine.forward on every window slice, the restatement of the blend on the CPU,
    s2v_sched_step on the long latent from the averaged fp32 prediction"""
    key = (case, dt_name, kind, weighting)
    if key not in _HAND:
        lib, Lb = s2v.lib(), s2v._lib
        dt, dpm = DT[dt_name], kind == "dpm"
        L, F, s = LFS
        wp = TW.window_plan(L, F, s, weighting)
        inp = _long_inputs(s2v, case, L)
        m, eng = _engine(s2v, case, dt, 2, F)
        _condition(s2v, eng, case)

        def step(x, t, coef, x0, nz):
            ys = [eng.forward(x[:, k0:k0 + F].contiguous(), torch.tensor([t, t]), shared_latent=True).clone() for k0 in wp["starts"]]
            vbar = TW.blend_scatter(torch.stack([y[0] for y in ys]), torch.stack([y[1] for y in ys]), coef.guidance, wp).to(DEV).contiguous()
            Lb.check(lib.s2v_sched_step(None, ctypes.byref(coef), Lb.ptr(vbar), Lb.SCHED_NP_F32, Lb.ptr(x), Lb.ptr(x), Lb.ptr(x0), Lb.ptr(nz), x.numel(),
                                        Lb.DTYPE_OF[dt], Lb.stream_ptr()))

        _HAND[key] = _loop(_plan(s2v, kind, dt), dt, inp["lat"], inp["noise"], dpm, step)
        eng.close()
    return _HAND[key]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("case,dt_name", [("tiny-rope", "bf16"), ("tiny-rope", "f16"), ("tiny-rope", "f32"), ("mid-rope", "bf16")])
def test_windowed_step_equals_the_hand_driven_pieces_bitwise(s2v, case, dt_name, kind, graph):
    dt, dpm = DT[dt_name], kind == "dpm"
    L, F, s = LFS
    exp = _hand_driven(s2v, case, dt_name, kind, "pyramid")
    inp = _long_inputs(s2v, case, L)
    m, eng = _engine(s2v, case, dt, 2, F)
    _condition(s2v, eng, case)
    eng.set_windows(L, s, TW.window_weights(F, "pyramid"))
    before = eng.lora_state["graph_captures"]
    got = _windowed(eng, _plan(s2v, kind, dt), dt, inp["lat"], inp["noise"], dpm, graph)
    assert eng.lora_state["graph_captures"] - before == (1 if graph else 0), "one captured graph holds every forward and serves every step"
    eng.close()
    _equal_steps(got, exp, f"{case} {dt_name} {kind}")
    assert not torch.equal(got[-1][0], inp["lat"].to(dt))
    if kind == "ddim" and not graph:   # the weights matter: the flat blend of the same windows is another result
        assert not torch.equal(_hand_driven(s2v, case, dt_name, kind, "flat")[0][0], exp[0][0])


# ------------------------------------------------------------------------------------------------ 3. anchors that need no restatement
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("case,dt_name", [("tiny-rope", "bf16"), ("tiny-rope", "f32"), ("mid-rope", "bf16")])
def test_one_flat_window_is_the_plain_step_bitwise(s2v, case, dt_name, kind):
    dt, dpm = DT[dt_name], kind == "dpm"
    F = 3
    inp = _long_inputs(s2v, case, F)
    plan = _plan(s2v, kind, dt)
    m, eng = _engine(s2v, case, dt, 2, F)
    _condition(s2v, eng, case)
    exp = _loop(plan, dt, inp["lat"], inp["noise"], dpm, lambda x, t, c, x0, nz: eng.denoise_step(x, t, c, x0, nz))
    eng.set_windows(F, F, TW.window_weights(F, "flat"))
    for graph in (False, True):
        _equal_steps(_windowed(eng, plan, dt, inp["lat"], inp["noise"], dpm, graph), exp, f"L = F, graph {graph}")
    eng.close()


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("case,dt_name", [("tiny-rope", "bf16"), ("tiny-rope", "f32"), ("mid-rope", "bf16")])
def test_two_abutting_flat_windows_are_two_independent_plain_steps_bitwise(s2v, case, dt_name, kind):
    dt, dpm = DT[dt_name], kind == "dpm"
    F = 3
    inp = _long_inputs(s2v, case, 2 * F)
    plan = _plan(s2v, kind, dt)
    m, eng = _engine(s2v, case, dt, 2, F)
    _condition(s2v, eng, case)
    plain = lambda x, t, c, x0, nz: eng.denoise_step(x, t, c, x0, nz)
    halves = [_loop(plan, dt, inp["lat"][:, h * F:(h + 1) * F], inp["noise"][:, :, h * F:(h + 1) * F], dpm, plain) for h in (0, 1)]
    eng.set_windows(2 * F, F, TW.window_weights(F, "flat"))
    got = _windowed(eng, plan, dt, inp["lat"], inp["noise"], dpm, False)
    eng.close()
    for h in (0, 1):
        _equal_steps([(x[:, h * F:(h + 1) * F], None if x0 is None else x0[:, h * F:(h + 1) * F]) for x, x0 in got], halves[h], f"half {h}")
    assert not torch.equal(got[-1][0][:, :F], got[-1][0][:, F:])


# ------------------------------------------------------------------------------------------------ 4. three windows per forward
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("case,dt_name", [("tiny-rope", "bf16"), ("tiny-rope", "f16"), ("tiny-rope", "f32"), ("mid-rope", "bf16")])
def test_three_windows_per_forward_equal_one_per_forward_bitwise(s2v, case, dt_name, kind):
    dt, dpm = DT[dt_name], kind == "dpm"
    L, F, s = LFS
    inp = _long_inputs(s2v, case, L)
    res = {}
    for pf in (1, 3):
        m, eng = _engine(s2v, case, dt, 2 * pf, F)
        _condition(s2v, eng, case, pf)
        eng.set_windows(L, s, TW.window_weights(F, "pyramid"), pf)
        res[pf] = [_windowed(eng, _plan(s2v, kind, dt), dt, inp["lat"], inp["noise"], dpm, graph) for graph in (False, True)]
        eng.close()
    _equal_steps(res[3][0], res[1][0], "per_forward 3 against 1, eager")
    _equal_steps(res[3][1], res[1][0], "per_forward 3 under hipGraph against 1, eager")
    _equal_steps(res[1][0], _hand_driven(s2v, case, dt_name, kind, "pyramid"), "per_forward 1 against the hand-driven pieces")


# ------------------------------------------------------------------------------------------------ 5. the pipeline
PH, PW, PT, NF = H.PH, H.PW, H.PT, 25   # 25 frames: L, F, s = 7, 3, 2 with TemporalWindows(9, 8)


def _pipe_args(s2v, dt):
    inp = BV._inputs(s2v, "tiny-rope")
    return dict(prompt_embeds=inp["pos"][:1].to(dt), negative_prompt_embeds=inp["neg"][:1].to(dt), ref_img_states=inp["ref"][:1].to(dt),
                height=PH, width=PW, guidance_scale=G)


def _hand_pipeline(s2v, pipe, dt, kind, args, lat, plan, gen):
    """the loop written out on the pipeline's own engine: geometry of one window, the text pair, set_windows, one windowed step per plan step;
    DPM draws the long noise from the call's generator as often as the step's kind says"""
    eng = pipe.transformer.engine
    tw = s2v.TemporalWindows(9, 8).plan(NF)
    eng.set_geometry(2, PT, tw["F"], PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning(torch.cat([args["negative_prompt_embeds"], args["prompt_embeds"]]), args["ref_img_states"])
    eng.set_windows(tw["L"], tw["s"], tw["weights"])
    x = lat.to(dt).contiguous().clone()
    dpm = kind == "dpm"
    x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
    nz = None
    for st in plan["steps"]:
        for _ in range(st["draws"]):
            nz = s2v.pipeline.randn_videos(x.shape, gen, DEV, dt).contiguous()
        eng.denoise_step_windows(x, float(st["t"]), st["coef"], x0, nz)
    torch.cuda.synchronize()
    eng.clear_windows()
    return x


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_returns_the_latents_of_hand_driven_windowed_steps_bitwise(s2v, kind):
    dt = torch.bfloat16
    pipe = H._pipe(s2v, kind, dt)
    args = _pipe_args(s2v, dt)
    gen = torch.Generator().manual_seed(977)
    lat = pipe.prepare_latents(NF, PH, PW, dt, DEV, gen, None, 1)
    assert tuple(lat.shape) == (1, 7, 16, PH // 8, PW // 8)
    plan = s2v.S2VPipeline.video_plan(pipe.scheduler, STEPS, None, G, False, dt)
    exp = _hand_pipeline(s2v, pipe, dt, kind, args, lat, plan, gen)
    with pytest.raises(ValueError, match="less than or equal to 49"):
        pipe(num_frames=53, num_inference_steps=STEPS, **args)
    seen = []
    for graph in (False, True):
        got = pipe(num_frames=NF, num_inference_steps=STEPS, temporal_windows=s2v.TemporalWindows(9, 8), use_graph=graph,
                   generator=torch.Generator().manual_seed(977), callback_on_step_end=lambda p, i, t, tensors: seen.append(tuple(tensors["latents"].shape)) or {},
                   **args)["frames"]
        assert _same(got, exp), f"use_graph {graph}"
        assert pipe.transformer.engine.windows is None, "the windows are cleared when the call ends"
    assert seen == [tuple(exp.shape)] * (2 * STEPS), "the callback sees the long latent"
    pipe.transformer.engine.close()


def test_pipeline_decodes_the_long_latent_in_one_call_and_video_to_video_starts_where_prepare_video_latents_puts_it(s2v):
    dt = torch.bfloat16
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, "ddim", dt, vae)
    args = _pipe_args(s2v, dt)
    kw = dict(num_frames=NF, num_inference_steps=STEPS, temporal_windows=s2v.TemporalWindows(9, 8), use_graph=True, **args)
    lat = pipe(generator=torch.Generator().manual_seed(5), output_type="latent", **kw)["frames"].clone()
    frames = pipe(generator=torch.Generator().manual_seed(5), output_type="np", **kw)["frames"]
    assert frames.shape == (1, NF, PH, PW, 3)
    assert np.array_equal(frames, vae.postprocess_video(vae.decode_latents(lat), "np")), "the frames are the decode of the call's long latent"
    # video-to-video: a 25-frame clip, strength 0.6 of 5 steps = the last 3 timesteps
    video = torch.rand(1, 3, NF, PH, PW, generator=torch.Generator().manual_seed(78)) * 2 - 1
    plan = s2v.S2VPipeline.video_plan(pipe.scheduler, 5, 0.6, G, False, dt)
    assert len(plan["steps"]) == 3
    gen = torch.Generator().manual_seed(6)
    start, _, _ = pipe.prepare_video_latents(video, dt, DEV, gen, [plan["timesteps"][0]])
    assert tuple(start.shape) == (1, 7, 16, PH // 8, PW // 8)
    exp = _hand_pipeline(s2v, pipe, dt, "ddim", args, start, plan, gen)
    got = pipe(video=video, strength=0.6, num_inference_steps=5, temporal_windows=s2v.TemporalWindows(9, 8), generator=torch.Generator().manual_seed(6),
               **args)["frames"]
    assert _same(got, exp)
    with pytest.raises(ValueError, match="less than or equal to 49"):
        pipe(video=torch.zeros(1, 3, 57, PH, PW), strength=0.6, num_inference_steps=5, **args)
    pipe.transformer.engine.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_limit_and_leave_the_engine_as_it_was(s2v):
    case, dt = "tiny-rope", torch.bfloat16
    lib, Lb = s2v.lib(), s2v._lib
    L, F, s = 7, 3, 2
    _, T, _, Hh, W = BV.CASES[case]
    inp = _long_inputs(s2v, case, L)
    coef = _plan(s2v, "ddim", dt)[0][1]
    m, eng = _engine(s2v, case, dt, 2, F)
    _condition(s2v, eng, case)
    short = inp["lat"][:, :F].to(dt).contiguous()

    def plain():
        x = short.clone()
        eng.denoise_step(x, 500.0, coef)
        torch.cuda.synchronize()
        return x

    base, bytes0 = plain(), eng.device_bytes()
    w = TW.window_weights(F, "pyramid")
    x = inp["lat"].to(dt).contiguous().clone()
    with pytest.raises(s2v.S2VError, match="s2v_denoise_step_windows: no temporal windows are set"):
        eng.denoise_step_windows(x, 500.0, coef)
    assert _same(x, inp["lat"].to(dt)) and _same(plain(), base)
    for bad, msg in (((L, s, w, 2), "B = 2 per_forward"), ((L + 1, s, w, 1), "must tile the L frames exactly"), ((L, F + 1, w, 1), "must tile the L frames exactly"),
                     ((L, 1, w, 2), "B = 2 per_forward"), ((5, 1, w, 1), None)):
        if msg is None:   # 3 windows, per_forward 1: accepted; then a plain step is refused by name
            eng.set_windows(*bad)
            continue
        with pytest.raises(s2v.S2VError, match=f"s2v_set_windows: .*{msg}"):
            eng.set_windows(*bad)
        assert eng.device_bytes() == bytes0 and _same(plain(), base)
    assert eng.device_bytes()[1] > bytes0[1], "the plane counts as workspace"
    with pytest.raises(s2v.S2VError, match="s2v_denoise_step: temporal windows are set"):
        eng.denoise_step(short.clone(), 500.0, coef)
    with pytest.raises(s2v.S2VError, match="s2v_denoise_step: temporal windows are set"):
        eng.denoise_step(short.clone(), [500.0], [coef])
    eng.clear_windows()
    assert eng.device_bytes() == bytes0 and _same(plain(), base), "after clear_windows the engine is the one it was"
    # armed features
    eng.step_cache_enable(True)
    eng._arm("capture")
    with pytest.raises(s2v.S2VError, match="s2v_set_windows: a step-cache mode is armed"):
        eng.set_windows(L, s, w)
    eng.step_cache_enable(False)   # frees the cache and takes the arm with it
    assert eng.device_bytes() == bytes0 and _same(plain(), base)
    # set_geometry clears, the same geometry included
    eng.set_windows(L, s, w)
    eng.set_geometry(2, T, F, Hh, W)
    assert eng.windows is None and eng.device_bytes() == bytes0
    eng.close()
    # a shard context
    m, sh = BV._engine(s2v, case, dt, 2)
    sh.set_shard(2, 0)
    sh.set_geometry(2, T, F, Hh, W)
    assert lib.s2v_set_windows(sh._h, L, s, 1, (ctypes.c_float * F)(*w)) != 0
    assert b"s2v_set_windows: a shard context" in lib.s2v_last_error()
    sh.close()
