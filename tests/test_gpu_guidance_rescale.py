"""Guidance rescale on the GPU (include/s2v_hip.h, "Guidance rescale": s2v_op_cfg_stats, s2v_sched_step_rescale / _masked_rescale,
s2v_set_guidance_rescale, s2v_guidance_rescale_read; S2VPipeline(guidance_rescale=...)).

The four sums are held to BITS against the restatement of their stated order (tests/guidance_rescale_ref.py).  The factor is held to one fp32
ulp of the restatement -- the device's fp64 divide and square root need not be correctly rounded -- and to exactly 1.0f where the definition
says so.  Everything downstream of the factor is held to bits WITH THE FACTOR READ BACK FROM THE DEVICE: the RESCALE step form, the engine's
armed steps and the pipeline against s2v_sched_step fed the fp32 prediction v' = v * k (flags bit1, no CFG), the kernel as it was before this
feature.  Against diffusers' rescale_noise_cfg in fp64 the bar is 4 * 2^-24 relative per element (one ulp on the factor, its rounding to
fp32, the product's rounding), on randn-scaled inputs whose std_v is well away from 0.
"""
import ctypes

import numpy as np
import pytest
import torch

import guidance_rescale_ref as GR
import test_gpu_batch_hetero as H
import test_gpu_batch_videos as BV

pytestmark = pytest.mark.gpu
DEV = BV.DEV
DT = BV.DT
GT, GS = float(np.float32(6.2831855)), float(np.float32(2.7182817))
PHI = 0.7
SLACK = 64
SIZES = [1, GR.CHUNK - 1, GR.CHUNK, GR.CHUNK + 1, 3 * GR.CHUNK + 17]
SHAPE = (3, 16, 5, 7)   # the latent of the step-form tests: 1680 elements = 6.5625 blocks of 256 threads
N = 3 * 16 * 5 * 7
SENT = 123.0


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _farr(xs):
    return (ctypes.c_float * len(xs))(*[float(x) for x in xs])


def _stats(s2v, buf, triple, np_f32, nvid, n_vid, g, gs, phi, dt):
    """s2v_op_cfg_stats on the planes at the head of `buf` -> (sums [nvid, 4] fp64, factors [nvid] fp32)"""
    lib, L = s2v.lib(), s2v._lib
    sums, factors = (ctypes.c_double * (4 * nvid))(), (ctypes.c_float * nvid)()
    flags = (L.SCHED_TRIPLE if triple else L.SCHED_CFG_PAIR) | (L.SCHED_NP_F32 if np_f32 else 0)
    L.check(lib.s2v_op_cfg_stats(L.ptr(buf), flags, nvid, n_vid, _farr(g), _farr(gs) if triple else None, _farr(phi), sums, factors, L.DTYPE_OF[dt],
                                 L.stream_ptr()))
    return np.array(sums[:], dtype=np.float64).reshape(nvid, 4), np.array(factors[:], dtype=np.float32)


_PL = {}


def _planes(p, nvid, n_vid):
    """fp32 planes [p, nvid, n_vid], randn-scaled with a mean, made once per shape"""
    key = (p, nvid, n_vid)
    if key not in _PL:
        g = torch.Generator().manual_seed(7 + 13 * p + nvid)
        scale, mean = torch.tensor([1.0, 0.8, 1.3][:p])[:, None, None], torch.tensor([0.1, -0.05, 0.2][:p])[:, None, None]
        _PL[key] = torch.randn(p, nvid, n_vid, generator=g) * scale + mean
    return _PL[key]


# ------------------------------------------------------------------------------------------------ 1. the sums and the factor
@pytest.mark.parametrize("triple", [False, True], ids=["pair", "triple"])
@pytest.mark.parametrize("inp", ["bf16", "f16", "f32", "f32-prediction"])
def test_sums_equal_the_stated_order_bitwise_and_the_factor_is_within_one_ulp(s2v, inp, triple):
    """every size at which the reduction takes another path (one element, one short of a chunk, a chunk, one over, three chunks and 17), one and
    three videos.  NaN sits behind the last plane, and with three videos the MIDDLE video of every plane is NaN: an over-read or a read of a
    neighbour turns a sum into NaN (and a finite over-read into other bits)"""
    np_f32 = inp == "f32-prediction"
    dt = torch.bfloat16 if np_f32 else DT[inp]
    p = 3 if triple else 2
    for n_vid in SIZES:
        for nvid in (1, 3):
            host = _planes(p, nvid, n_vid).clone()
            if nvid == 3:
                host[:, 1] = float("nan")
            host = host if np_f32 else host.to(dt)
            buf = torch.cat([host.flatten(), torch.full((SLACK,), float("nan"), dtype=host.dtype)]).to(DEV)
            g, gs, phi = [GT, 4.5, 3.25][:nvid], [GS, 0.75, 1.5][:nvid], [PHI, 0.5, 0.25][:nvid]
            sums, factors = _stats(s2v, buf, triple, np_f32, nvid, n_vid, g, gs, phi, dt)
            loaded = host.float()
            for k in range(nvid):
                what = f"{inp}, n_vid {n_vid}, video {k} of {nvid}"
                if nvid == 3 and k == 1:
                    assert np.isnan(sums[k]).all() and factors[k] == 1.0, f"{what}: the NaN video"
                    continue
                planes = loaded[:, k]
                v = GR.combine(planes, g[k], gs[k] if triple else None).numpy()
                f = planes[-1].numpy()
                cand = dict(sums=sums[k], std=GR.stds_from_sums(sums[k], n_vid), k=factors[k])
                assert GR.check_sums(cand, f, v) is None, f"{what}: {GR.check_sums(cand, f, v)}"
                assert GR.check_factor(cand, f, v, phi[k]) is None, f"{what}: {GR.check_factor(cand, f, v, phi[k])}"
                if n_vid == 1:
                    assert factors[k] == 1.0, f"{what}: one element has no deviation"
                else:
                    assert factors[k] != 1.0, what


@pytest.mark.parametrize("triple", [False, True], ids=["pair", "triple"])
def test_the_device_passes_every_check_of_the_restatement_including_the_references_formula(s2v, triple):
    """std_v here is > 1: well away from 0.  v' = v * k with the DEVICE's factor against rescale_noise_cfg in fp64 (REF_BAR), the deviations its
    sums give against numpy's two-pass ones (STD_BAR)"""
    p, n_vid = (3 if triple else 2), SIZES[-1]
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        planes = _planes(p, 1, n_vid)[:, 0].to(dt)
        sums, factors = _stats(s2v, planes.contiguous().to(DEV), triple, False, 1, n_vid, [GT], [GS], [PHI], dt)
        v = GR.combine(planes.float(), GT, GS if triple else None)
        cand = dict(sums=sums[0], std=GR.stds_from_sums(sums[0], n_vid), k=factors[0], vprime=(v * torch.tensor(float(factors[0]))).numpy())
        assert cand["std"][1] > 1.0
        assert GR.failures(cand, planes.float(), GT, GS if triple else None, PHI) == []


def test_the_factor_is_exactly_one_where_the_definition_says_so(s2v):
    n_vid, dt = 5000, torch.float32
    planes = _planes(2, 1, n_vid)[:, 0].contiguous()
    one = lambda pl, phi, n=n_vid: float(_stats(s2v, pl.contiguous().to(DEV), False, False, 1, n, [GT], None, [phi], dt)[1][0])
    assert one(planes, PHI) != 1.0
    assert one(planes, 0.0) == 1.0, "phi = 0"
    assert one(torch.full((2, n_vid), 1.5), PHI) == 1.0, "a constant plane (its sums are exact in fp64: std_v = 0)"
    assert one(planes[:, :1], PHI, 1) == 1.0, "n_vid = 1"
    inf = planes.clone()
    inf[1, 77] = float("inf")
    assert one(inf, PHI) == 1.0, "an inf in v: std_v is not finite"


# ------------------------------------------------------------------------------------------------ 2. the RESCALE step form
def _coefs(s2v, dt):
    """one coefficient set of every kind: DDIM (0), DPM first step (1), DPM multistep (2)"""
    d, p = H._sched(s2v, "ddim"), H._sched(s2v, "dpm")
    d.set_timesteps(4)
    p.set_timesteps(4)
    ts = p.timesteps
    out = [d.coef(d.timesteps[1], dt, GT, guidance_subject=GS), p.coef(ts[0], None, True, dt, GT, guidance_subject=GS),
           p.coef(ts[1], ts[0], False, dt, GT, guidance_subject=GS)]
    assert [c.kind for c in out] == [0, 1, 2]
    return out


_KIN = {}


def _kernel_inputs(dt):
    if dt not in _KIN:
        g = torch.Generator(device=DEV).manual_seed(173)
        r = lambda: torch.randn(SHAPE, generator=g, device=DEV)
        _KIN[dt] = dict(planes=torch.randn((3,) + SHAPE, generator=g, device=DEV), x=r().to(dt), nz=r().to(dt), x0_old=r(), z0=r().to(dt),
                        noise0=r().to(dt))
    return _KIN[dt]


def _sched(s2v, coef, npred, flags, x, nz, x0_old, dt, factor=None, masked=None):
    """one scheduler-step launch of n = x.numel() elements with sentinels behind the output and the x0 history -> (out, hist); factor: a device
    tensor -> the RESCALE entries with flags bit4; masked: (record, z0, noise0, level, (F, C, H, W))"""
    lib, L = s2v.lib(), s2v._lib
    n = x.numel()
    out = torch.full((n + SLACK,), SENT, dtype=torch.float32 if flags & 4 else dt, device=DEV)
    hist = torch.cat([x0_old.flatten().float(), torch.full((SLACK,), SENT, dtype=torch.float32, device=DEV)])
    npred, x, nz = npred.contiguous(), x.contiguous(), nz.contiguous()
    dtc, st = L.DTYPE_OF[dt], L.stream_ptr()
    if masked is None and factor is None:
        L.check(lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(npred), flags, L.ptr(x), L.ptr(out), L.ptr(hist), L.ptr(nz), n, dtc, st))
    elif masked is None:
        L.check(lib.s2v_sched_step_rescale(None, ctypes.byref(coef), L.ptr(npred), flags | L.SCHED_RESCALE, L.ptr(x), L.ptr(out), L.ptr(hist), L.ptr(nz),
                                           n, dtc, L.ptr(factor), st))
    else:
        rec, z0, noise0, level, shape = masked
        args = (None, ctypes.byref(coef), ctypes.byref(rec), L.ptr(npred), flags | (L.SCHED_RESCALE if factor is not None else 0), L.ptr(x), L.ptr(out),
                L.ptr(hist), L.ptr(nz), L.ptr(z0.contiguous()), L.ptr(noise0.contiguous()), L.ptr(level.contiguous()), *shape, dtc)
        if factor is None:
            L.check(lib.s2v_sched_step_masked(*args, st))
        else:
            L.check(lib.s2v_sched_step_masked_rescale(*args, L.ptr(factor), st))
    torch.cuda.synchronize()
    assert bool((out[n:].float() == SENT).all()) and bool((hist[n:] == SENT).all()), "a write past the last element"
    return out[:n], hist[:n]


def _levels():
    lv = (torch.arange(105) * 255 // 104).to(torch.uint8)
    lv = lv[torch.randperm(105, generator=torch.Generator().manual_seed(3))]
    return lv.reshape(3, 5, 7).contiguous().to(DEV)


@pytest.mark.parametrize("triple", [False, True], ids=["pair", "triple"])
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
def test_rescale_step_equals_the_plain_kernel_fed_v_times_k_bitwise(s2v, dt_name, triple):
    """DDIM, DPM first step and DPM multistep; model-dtype and fp32 predictions; model-dtype and fp32 output; then the masked form against the
    masked entry.  The factor is the device's own (s2v_op_cfg_stats), and v * k is one torch fp32 multiply"""
    dt = DT[dt_name]
    k = _kernel_inputs(dt)
    L = s2v._lib
    sch = H._sched(s2v, "ddim")
    level = _levels()
    cfg_flag = L.SCHED_TRIPLE if triple else L.SCHED_CFG_PAIR
    for np_f32 in (0, 1):
        planes = (k["planes"] if np_f32 else k["planes"].to(dt))[0 if triple else 1:].contiguous()
        _, factors = _stats(s2v, planes, triple, np_f32, 1, N, [GT], [GS], [PHI], dt)
        assert factors[0] != 1.0
        factor = torch.tensor([float(factors[0])], dtype=torch.float32, device=DEV)
        v = GR.combine(planes.float().flatten(1), GT, GS if triple else None)
        vprime = (v * factor).view(SHAPE)
        for coef in _coefs(s2v, dt):
            for out_f32 in (0, 1):
                what = f"kind {coef.kind}, np_f32 {np_f32}, out_f32 {out_f32}"
                got = _sched(s2v, coef, planes, cfg_flag | 2 * np_f32 | 4 * out_f32, k["x"], k["nz"], k["x0_old"], dt, factor)
                exp = _sched(s2v, coef, vprime, 2 | 4 * out_f32, k["x"], k["nz"], k["x0_old"], dt)
                plain = _sched(s2v, coef, planes, cfg_flag | 2 * np_f32 | 4 * out_f32, k["x"], k["nz"], k["x0_old"], dt)
                assert _same(got[0], exp[0]) and _same(got[1], exp[1]), what
                assert not torch.equal(got[0], plain[0]), f"{what}: the factor changed nothing"
            for t_next in (599, None):
                m = (sch.blend_record(t_next, dt, DEV, 127), k["z0"], k["noise0"], level, SHAPE)
                got = _sched(s2v, coef, planes, cfg_flag | 2 * np_f32, k["x"], k["nz"], k["x0_old"], dt, factor, masked=m)
                exp = _sched(s2v, coef, vprime, 2, k["x"], k["nz"], k["x0_old"], dt, masked=m)
                assert _same(got[0], exp[0]) and _same(got[1], exp[1]), f"masked, kind {coef.kind}, np_f32 {np_f32}, t_next {t_next}"


# ------------------------------------------------------------------------------------------------ 3. the engine
def _hand_step(s2v, eng, coefs, phi, x_in, x0_in, nz, dt, triple=False, blends=None, level=None, z0=None, noise0=None):
    """what an armed step must have left, from the pieces: the model outputs the step itself left (last_noise_pred), the restated sums and
    factor (the device's factor must be within one ulp of it and is then used, so that everything behind it is held to bits), and the
    scheduler kernel as it was before the feature on the fp32 prediction v * k -> (latents [b, ...], x0 history [b, ...])"""
    b = x_in.shape[0]
    npred = eng.last_noise_pred()
    read = eng.guidance_rescale_read()
    lats, hists = [], []
    for k in range(b):
        planes = npred[[k, b + k, 2 * b + k] if triple else [k, b + k]].float().flatten(1).cpu()
        g, gs = coefs[k].guidance, coefs[k].guidance_subject if triple else None
        v = GR.combine(planes, g, gs)
        sums = GR.sums_of(planes[-1], v)
        assert np.array(read["sums"][k]).tobytes() == sums.tobytes(), f"video {k}: the sums read back"
        want = GR.factor_of(sums, v.numel(), phi[k])
        kf = np.float32(read["factors"][k])
        assert GR.ulps32(kf, want) <= 1, f"video {k}: factor {kf!r} against {want!r}"
        assert (kf == 1.0) == (phi[k] == 0.0)
        vprime = (v * torch.tensor(float(kf))).to(DEV).view(x_in.shape[1:])
        masked = None if blends is None else (blends[k], z0[k], noise0[k], level[k], tuple(x_in.shape[1:]))
        zeros = torch.zeros_like(x_in[k], dtype=torch.float32)
        out, hist = _sched(s2v, coefs[k], vprime, 2, x_in[k], nz[k] if nz is not None else x_in[k], x0_in[k] if x0_in is not None else zeros, dt,
                           masked=masked)
        lats.append(out.view(x_in.shape[1:]))
        hists.append(hist.view(x_in.shape[1:]))
    return torch.stack(lats), torch.stack(hists)


def _plan(s2v, kind, dt, k):
    n, strength, g = [(3, None, GT), (4, 0.75, 4.5 + 2 ** -18)][k]
    steps = s2v.S2VPipeline.video_plan(H._sched(s2v, kind), n, strength, g, False, dt)["steps"]
    assert len(steps) == 3
    return [(float(st["t"]), st["coef"]) for st in steps]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_armed_steps_equal_the_hand_driven_pieces_and_new_values_capture_nothing(s2v, kind, graph):
    """two videos on their own plans, three armed steps with new phi between the second and the third (no new capture), then an un-armed step
    that must be the plain pair kernel's again"""
    case, dt, b = "tiny-rope", torch.bfloat16, 2
    inp = BV._inputs(s2v, case)
    plans = [_plan(s2v, kind, dt, k) for k in range(b)]
    m, eng = BV._engine(s2v, case, dt, 2 * b)
    eng.set_conditioning(BV._text(inp, [0, 1]), inp["ref"][:2])
    plain_bytes = eng.device_bytes()
    x = inp["lat"][:b].to(dt).contiguous().clone()
    x0, nz = torch.zeros(x.shape, dtype=torch.float32, device=DEV), torch.empty_like(x)
    phi = [PHI, 0.3]
    eng.set_guidance_rescale(phi)
    assert eng.device_bytes()[1] > plain_bytes[1], "armed: the partials and the log count as workspace"
    before = eng.lora_state["graph_captures"]
    logged = []
    for i in range(3):
        if i == 2:
            phi = [0.2, 0.9]
            eng.set_guidance_rescale(phi)
        nz.copy_(inp["noise"][i, :b].to(dt))
        x_in, x0_in = x.clone(), x0.clone()
        coefs = [p[i][1] for p in plans]
        eng.denoise_step(x, [p[i][0] for p in plans], coefs, x0, nz, use_graph=graph)
        torch.cuda.synchronize()
        lat, hist = _hand_step(s2v, eng, coefs, phi, x_in, x0_in, nz, dt)
        assert _same(x, lat) and _same(x0, hist), f"step {i}"
        logged.append(eng.guidance_rescale_read()["factors"])
    assert eng.lora_state["graph_captures"] - before == (1 if graph else 0), "one graph serves every armed step, new values included"
    read = eng.guidance_rescale_read()
    assert read["count"] == 3 and [r[:b] for r in read["log"]] == logged and all(r[b:] == [0.0] * (4 - b) for r in read["log"])
    # un-armed after armed: the plain launches, another graph
    eng.set_guidance_rescale([0.0, 0.0])
    assert eng.device_bytes() == plain_bytes
    x_in, x0_in = x.clone(), x0.clone()
    eng.denoise_step(x, [p[2][0] for p in plans], coefs, x0, nz, use_graph=graph)
    torch.cuda.synchronize()
    npred = eng.last_noise_pred()
    for k in range(b):
        out, hist = _sched(s2v, coefs[k], npred[[k, b + k]], 1, x_in[k], nz[k], x0_in[k], dt)
        assert _same(x[k].flatten(), out) and _same(x0[k].flatten(), hist), f"un-armed step, video {k}"
    assert eng.guidance_rescale_read(log_only=True)["count"] == 3, "an un-armed step logs nothing"
    eng.set_guidance_rescale(None)
    assert eng.guidance_rescale_read(log_only=True)["count"] == 0 and eng.device_bytes() == plain_bytes
    eng.close()


@pytest.mark.parametrize("case,dt_name", [("tiny-rope", "f32"), ("mid-rope", "bf16"), ("tiny-rope", "f16")])
def test_zero_phi_is_the_plain_step_and_video_0_of_phi_0_and_07_equals_its_plain_run(s2v, case, dt_name):
    """no GEMM splits K on these geometries (tests/test_gpu_batch_videos.py), so video 0's forward does not depend on its neighbour's latents"""
    dt, b = DT[dt_name], 2
    inp = BV._inputs(s2v, case)
    m, eng = BV._engine(s2v, case, dt, 2 * b)
    eng.set_conditioning(BV._text(inp, [0, 1]), inp["ref"][:2])
    plain_bytes = eng.device_bytes()
    plain = BV._steps(s2v, eng, "dpm", dt, inp["lat"][:b], inp["noise"][:, :b], True)
    eng.set_guidance_rescale(0.0)
    assert eng.device_bytes() == plain_bytes
    zero = BV._steps(s2v, eng, "dpm", dt, inp["lat"][:b], inp["noise"][:, :b], True)
    eng.set_guidance_rescale([0.0, PHI])
    mixed = BV._steps(s2v, eng, "dpm", dt, inp["lat"][:b], inp["noise"][:, :b], True)
    for i in range(BV.STEPS):
        assert _same(zero[i][0], plain[i][0]) and _same(zero[i][1], plain[i][1]), f"step {i}: all-zero phi"
        assert _same(mixed[i][0][0], plain[i][0][0]) and _same(mixed[i][1][0], plain[i][1][0]), f"step {i}: video 0 (phi = 0) beside video 1 (phi = 0.7)"
    assert not torch.equal(mixed[-1][0][1], plain[-1][0][1])
    eng.close()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_masked_triple_and_step_cache_reuse_steps_armed(s2v, graph):
    case, dt = "tiny-rope", torch.bfloat16
    _, T, F, Hh, W = BV.CASES[case]
    inp = BV._inputs(s2v, case)
    sch = H._sched(s2v, "dpm")
    sch.set_timesteps(4)
    ts = sch.timesteps
    coefs = [sch.coef(ts[0], None, True, dt, GT, guidance_subject=GS), sch.coef(ts[1], ts[0], False, dt, GT, guidance_subject=GS)]
    x = inp["lat"][:1].to(dt).contiguous().clone()
    x0, nz = torch.zeros(x.shape, dtype=torch.float32, device=DEV), inp["noise"][0, :1].to(dt).contiguous()
    # the masked step
    m, eng = BV._engine(s2v, case, dt, 2)
    eng.set_conditioning(BV._text(inp, [0]), inp["ref"][:1])
    z0, noise0 = inp["lat"][1:2].to(dt).contiguous(), inp["noise"][1, :1].to(dt).contiguous()
    level = (torch.arange(F * Hh * W, device=DEV) % 3 == 0).to(torch.uint8).view(1, F, Hh, W).contiguous()
    eng.set_blend(z0, noise0, level)
    eng.set_guidance_rescale(PHI)
    for i, coef in enumerate(coefs):
        rec = H._sched(s2v, "ddim").blend_record(int(ts[i + 1]), dt, DEV, 0)
        x_in, x0_in = x.clone(), x0.clone()
        eng.denoise_step(x, [float(ts[i])], [coef], x0, nz, use_graph=graph, blend=[rec])
        torch.cuda.synchronize()
        lat, hist = _hand_step(s2v, eng, [coef], [PHI], x_in, x0_in, nz, dt, blends=[rec], level=level, z0=z0, noise0=noise0)
        assert _same(x, lat) and _same(x0, hist), f"masked step {i}"
    eng.clear_blend()
    # the step cache: a capture step, then a reuse step, both armed
    eng.set_geometry(2, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(BV._text(inp, [0]), inp["ref"][:1])
    eng.set_guidance_rescale(None)
    eng.set_guidance_rescale(PHI)
    eng.step_cache_enable(True)
    for i, (coef, cache) in enumerate(zip(coefs, ("capture", "reuse"))):
        x_in, x0_in = x.clone(), x0.clone()
        eng.denoise_step(x, float(ts[i]), coef, x0, nz, use_graph=graph, cache=cache)
        torch.cuda.synchronize()
        lat, hist = _hand_step(s2v, eng, [coef], [PHI], x_in, x0_in, nz, dt)
        assert _same(x, lat) and _same(x0, hist), f"step-cache {cache} step"
    assert eng.step_cache_state()["valid"] and eng.guidance_rescale_read(log_only=True)["count"] == 2
    eng.step_cache_enable(False)
    eng.close()
    # the triple step: f is the triple's f
    m, eng = BV._engine(s2v, case, dt, 3)
    eng.set_conditioning_triples(BV._text(inp, [0]), inp["ref"][:1], inp["ref"][1:2] * 0.5)
    eng.set_guidance_rescale([PHI])
    for i, coef in enumerate(coefs):
        x_in, x0_in = x.clone(), x0.clone()
        eng.denoise_step(x, [float(ts[i])], [coef], x0, nz, use_graph=graph, subject=True)
        torch.cuda.synchronize()
        lat, hist = _hand_step(s2v, eng, [coef], [PHI], x_in, x0_in, nz, dt, triple=True)
        assert _same(x, lat) and _same(x0, hist), f"triple step {i}"
    eng.close()


def test_library_refusals_name_the_limit(s2v):
    case, dt = "tiny-rope", torch.bfloat16
    _, T, F, Hh, W = BV.CASES[case]
    inp = BV._inputs(s2v, case)
    lib, L = s2v.lib(), s2v._lib
    m, eng = BV._engine(s2v, case, dt, 2)
    eng.set_conditioning(BV._text(inp, [0]), inp["ref"][:1])

    def refused(call, *words):
        with pytest.raises(L.S2VError) as e:
            call()
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    for bad in (-0.5, 1.5, float("nan")):
        refused(lambda: eng.set_guidance_rescale(bad), "s2v_set_guidance_rescale", "[0, 1]")
    refused(lambda: L.check(lib.s2v_set_guidance_rescale(eng._h, _farr([0.5, 0.5]), 2)), "s2v_set_guidance_rescale", "videos of the geometry")
    x = inp["lat"][:1].to(dt).contiguous().clone()
    coef = H._sched(s2v, "ddim")
    coef.set_timesteps(3)
    coef = coef.coef(coef.timesteps[0], dt, GT)
    eng.set_guidance_rescale(PHI)
    refused(lambda: eng.denoise_step_windows(x, 500.0, coef), "s2v_denoise_step_windows", "guidance rescale is armed")
    refused(lambda: eng.set_windows(F, 1, [1.0] * F), "s2v_set_windows", "guidance rescale is armed")
    refused(lambda: eng.denoise_split_begin(x, 500.0, coef, 0), "s2v_denoise_split_begin", "guidance rescale is armed")
    eng.set_guidance_rescale(None)
    eng.set_windows(F, 1, [1.0] * F)
    refused(lambda: eng.set_guidance_rescale(PHI), "s2v_set_guidance_rescale", "temporal windows")
    eng.clear_windows()
    eng.set_geometry(1, T, F, Hh, W)
    refused(lambda: L.check(lib.s2v_set_guidance_rescale(eng._h, _farr([0.5]), 1)), "s2v_set_guidance_rescale", "B = 1")
    eng.set_geometry(2, T, F, Hh, W)
    eng.set_guidance_rescale(PHI)
    eng.set_geometry(2, T, F, Hh, W)   # the same geometry again disarms, as it clears the window plane
    refused(lambda: L.check(lib.s2v_guidance_rescale_read(eng._h, (ctypes.c_double * 4)(), None, None, None)), "s2v_guidance_rescale_read", "armed")
    eng.close()
    m, eng = BV._engine(s2v, case, dt, 2)
    eng.set_shard(2, 0)
    eng.set_geometry(2, T, F, Hh, W)
    refused(lambda: eng.set_guidance_rescale(PHI), "s2v_set_guidance_rescale", "shard")
    eng.close()
    # the kernels' own entries
    k = _kernel_inputs(dt)
    planes = k["planes"][:2].to(dt).contiguous()
    out = torch.empty(N, dtype=dt, device=DEV)
    assert lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(planes), 1 | L.SCHED_RESCALE, L.ptr(k["x"]), L.ptr(out), None, None, N, L.DTYPE_OF[dt], None) != 0
    assert b"s2v_sched_step: flags bit4" in lib.s2v_last_error() and b"s2v_sched_step_rescale" in lib.s2v_last_error()
    assert lib.s2v_sched_step_rescale(None, ctypes.byref(coef), L.ptr(planes), 1 | L.SCHED_RESCALE, L.ptr(k["x"]), L.ptr(out), None, None, N,
                                      L.DTYPE_OF[dt], None, None) != 0
    assert b"s2v_sched_step_rescale: flags bit4" in lib.s2v_last_error()
    sums, factors = (ctypes.c_double * 4)(), (ctypes.c_float * 1)()
    for flags, phi, word in ((0, 0.5, b"exactly one"), (9, 0.5, b"exactly one"), (1, 1.5, b"[0, 1]"), (8, 0.5, b"guidance_subject")):
        assert lib.s2v_op_cfg_stats(L.ptr(planes), flags, 1, N, _farr([GT]), None, _farr([phi]), sums, factors, L.DTYPE_OF[dt], None) != 0
        assert b"s2v_op_cfg_stats" in lib.s2v_last_error() and word in lib.s2v_last_error(), lib.s2v_last_error()


# ------------------------------------------------------------------------------------------------ 4. the pipeline
PH, PW, PF, PT, VF = H.PH, H.PW, H.PF, H.PT, H.VF


def _pipe_inputs(s2v, dt):
    inp = H._inputs(s2v, "tiny-rope")
    return inp["pos"][:2].to(dt), inp["neg"][:2].to(dt), inp["ref"][:2].to(dt)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_equals_the_hand_driven_armed_loop_and_reports_the_factors(s2v, kind):
    dt = torch.bfloat16
    pos, neg, ref = _pipe_inputs(s2v, dt)
    pipe = H._pipe(s2v, kind, dt)
    sch, eng = pipe.scheduler, pipe.transformer.engine
    kw = dict(prompt_embeds=pos[:1], negative_prompt_embeds=neg[:1], ref_img_states=ref[:1], height=PH, width=PW, num_frames=PF, num_inference_steps=4,
              guidance_scale=GT, use_graph=True)
    got = pipe(generator=torch.Generator().manual_seed(977), guidance_rescale=PHI, **kw)["frames"].clone()
    rep = pipe.guidance_rescale_report
    assert eng.guidance_rescale_read(log_only=True)["count"] == 0, "the call clears what it set"
    g = torch.Generator().manual_seed(977)
    lat = pipe.prepare_latents(PF, PH, PW, dt, DEV, g, None, 1).to(dt).contiguous()
    plan = s2v.S2VPipeline.video_plan(sch, 4, None, GT, False, dt)
    eng.set_geometry(2, PT, lat.shape[1], PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning(torch.cat([neg[:1], pos[:1]]), ref[:1])
    eng.set_guidance_rescale(PHI)
    x0 = torch.zeros(lat.shape, dtype=torch.float32, device=DEV) if kind == "dpm" else None
    noise, factors = None, []
    for st in plan["steps"]:
        for _ in range(st["draws"]):   # the reference discards its first draw on multistep steps
            noise = s2v.pipeline.randn_videos(lat.shape, g, DEV, dt).contiguous()
        eng.denoise_step(lat, float(st["t"]), st["coef"], x0, noise)
        factors.append([eng.guidance_rescale_read()["factors"][0]])
    assert len(factors) == 4
    eng.set_guidance_rescale(None)
    torch.cuda.synchronize()
    assert _same(got, lat)
    assert rep == {"phi": [PHI], "factors": factors} and all(f[0] != 1.0 for f in factors)
    plain = pipe(generator=torch.Generator().manual_seed(977), **kw)["frames"].clone()
    assert pipe.guidance_rescale_report is None and not torch.equal(plain, got)
    zero = pipe(generator=torch.Generator().manual_seed(977), guidance_rescale=0.0, **kw)["frames"]
    assert _same(zero, plain) and pipe.guidance_rescale_report is None, "0.0 is the call without the argument"
    eng.close()


def test_pipeline_per_video_list_on_plans_of_two_lengths_sets_the_values_again_on_the_shrink(s2v):
    dt = torch.bfloat16
    P = s2v.S2VPipeline
    pos, neg, ref = _pipe_inputs(s2v, dt)
    pipe = H._pipe(s2v, "ddim", dt)
    sch, eng = pipe.scheduler, pipe.transformer.engine
    counts, guid, phi = [2, 4], [GT, 4.5], [PHI, 0.3]
    got = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, generator=H._gens(range(2)), height=PH, width=PW, num_frames=PF,
               num_inference_steps=counts, guidance_scale=guid, guidance_rescale=phi, use_graph=True)["frames"].clone()
    rep = pipe.guidance_rescale_report
    plans = [P.video_plan(sch, counts[k], None, guid[k], False, dt) for k in range(2)]
    order = [1, 0]   # longest plan first
    lat = pipe.prepare_latents(PF, PH, PW, dt, DEV, H._gens(range(2)), None, 2).to(dt)[order].contiguous()
    factors = []
    for a, first in ((2, 0), (1, 2)):
        rows = order[:a]
        eng.set_geometry(2 * a, PT, lat.shape[1], PH // 8, PW // 8)
        eng.prepare_tables(PH, PW)
        eng.set_conditioning(torch.cat([neg[rows], pos[rows]]), ref[rows])
        eng.set_guidance_rescale([phi[k] for k in rows])
        for i in range(first, first + 2):
            steps = [plans[k]["steps"][i] for k in rows]
            eng.denoise_step(lat[:a], [float(st["t"]) for st in steps], [st["coef"] for st in steps], use_graph=True)
            f = eng.guidance_rescale_read()["factors"]
            factors.append([f[rows.index(k)] if k in rows else None for k in range(2)])
    eng.set_guidance_rescale(None)
    torch.cuda.synchronize()
    assert _same(got, lat[[1, 0]])
    assert rep == {"phi": phi, "factors": factors} and factors[-1][0] is None
    eng.close()


def test_pipeline_with_subject_guidance_and_with_a_mask_equals_the_hand_driven_armed_loops(s2v):
    dt = torch.bfloat16
    P = s2v.S2VPipeline
    pos, neg, ref = _pipe_inputs(s2v, dt)
    null = (H._inputs(s2v, "tiny-rope")["ref"][2:3] * 0.5).to(dt)
    # subject_guidance_scale=: f is the triple's f
    pipe = H._pipe(s2v, "ddim", dt, H._vae(s2v, dt))
    sch, eng = pipe.scheduler, pipe.transformer.engine
    kw = dict(prompt_embeds=pos[:1], negative_prompt_embeds=neg[:1], ref_img_states=ref[:1], height=PH, width=PW, num_inference_steps=4, guidance_scale=GT,
              guidance_rescale=PHI, use_graph=True)
    got = pipe(negative_ref_img_states=null, subject_guidance_scale=GS, num_frames=PF, generator=torch.Generator().manual_seed(977), **kw)["frames"].clone()
    assert eng.triples and all(f[0] != 1.0 for f in pipe.guidance_rescale_report["factors"])
    lat = pipe.prepare_latents(PF, PH, PW, dt, DEV, torch.Generator().manual_seed(977), None, 1).to(dt).contiguous()
    eng.set_geometry(3, PT, lat.shape[1], PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning_triples(torch.cat([neg[:1], pos[:1]]), ref[:1], null)
    eng.set_guidance_rescale([PHI])
    for st in P.video_plan(sch, 4, None, GT, False, dt, guidance_subject=GS)["steps"]:
        eng.denoise_step(lat, [float(st["t"])], [st["coef"]], subject=True)
    eng.set_guidance_rescale(None)
    torch.cuda.synchronize()
    assert _same(got, lat)
    # mask=: the statistics cover the whole video, the select runs behind the rescaled step
    video = H._videos(1)
    mask = torch.zeros(1, VF, PH, PW)
    mask[..., : PW // 2] = 1.0
    got = pipe(video=video, mask=mask, strength=0.75, generator=H._gens([0]), output_type="latent", **kw)["frames"].clone()
    factors = pipe.guidance_rescale_report["factors"]
    plan = P.video_plan(sch, 4, 0.75, GT, False, dt)
    lat, z0, noise0 = pipe.prepare_video_latents(video, dt, DEV, H._gens([0]), [plan["timesteps"][0]])
    lat, z0, noise0 = lat.to(dt).contiguous(), z0.to(dt).contiguous(), noise0.to(dt).contiguous()
    level, _ = s2v.engine.mask_to_latent(mask, DEV)
    blends = P.blend_plan(sch, plan, dt, DEV)
    eng.set_geometry(2, PT, lat.shape[1], PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning(torch.cat([neg[:1], pos[:1]]), ref[:1])
    eng.set_blend(z0, noise0, level)
    eng.set_guidance_rescale(PHI)
    seen = []
    for i, st in enumerate(plan["steps"]):
        eng.denoise_step(lat, [float(st["t"])], [st["coef"]], blend=[blends[i]], use_graph=True)
        seen.append([eng.guidance_rescale_read()["factors"][0]])
    eng.clear_blend()
    eng.set_guidance_rescale(None)
    torch.cuda.synchronize()
    assert _same(got, lat) and factors == seen and len(seen) == 3
    kept = (level == 0)[:, :, None].expand(-1, -1, 16, -1, -1)
    assert torch.equal(got[kept], z0[kept]) and kept.any() and not kept.all()
    eng.close()
