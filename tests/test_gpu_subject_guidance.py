"""Subject guidance on the GPU (include/s2v_hip.h: flags bit3 of s2v_sched_step / s2v_sched_step_masked, s2v_set_conditioning_triples,
s2v_denoise_step_guided; S2VPipeline(subject_guidance_scale=...)).  Three samples per video, u (negative text, null reference), r (negative
text, the reference), f (positive text, the reference), combined as v = (u + g_subject (r - u)) + g_text (f - r).

No tolerance appears in this file: every claim is equality of bits -- the kernel against the torch restatement (tests/subject_guidance_ref.py), the
triple engine's model outputs against pair engines', the fused step against the restatement applied to those outputs, the pipeline against
hand-driven steps -- on the shapes where tests/test_gpu_batch_videos.py already holds batches to bits (no GEMM splits K there).  The scales have
full fp32 mantissas: with 2.5 and 6.0 every product of a bf16 value is exact and a re-association or an fma would change nothing.
"""
import ctypes

import numpy as np
import pytest
import torch

import subject_guidance_ref as SG
import test_gpu_batch_hetero as H
import test_gpu_batch_videos as BV

pytestmark = pytest.mark.gpu
DEV = BV.DEV
DT = BV.DT
STEPS = 3
GS, GT = float(np.float32(2.7182817)), float(np.float32(6.2831855))
SHAPE = (3, 16, 5, 7)   # one latent [F, C, H, W]: 1680 elements = 6.5625 blocks of 256 threads
N = 3 * 16 * 5 * 7
SENT = 123.0            # a value every dtype holds
SLACK = 64


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _coefs(s2v, dt, gs=GS, gt=GT):
    """one coefficient set of every kind: DDIM (0), DPM first step (1), DPM multistep (2)"""
    d, p = H._sched(s2v, "ddim"), H._sched(s2v, "dpm")
    d.set_timesteps(4)
    p.set_timesteps(4)
    ts = p.timesteps
    out = [d.coef(d.timesteps[1], dt, gt, guidance_subject=gs), p.coef(ts[0], None, True, dt, gt, guidance_subject=gs),
           p.coef(ts[1], ts[0], False, dt, gt, guidance_subject=gs)]
    assert [c.kind for c in out] == [0, 1, 2]
    return out


_KIN = {}


def _kernel_inputs(dt):
    if dt not in _KIN:
        g = torch.Generator(device=DEV).manual_seed(171)
        _KIN[dt] = dict(planes=torch.randn((3,) + SHAPE, generator=g, device=DEV), x=torch.randn(SHAPE, generator=g, device=DEV).to(dt),
                        nz=torch.randn(SHAPE, generator=g, device=DEV).to(dt), x0_old=torch.randn(SHAPE, generator=g, device=DEV),
                        z0=torch.randn(SHAPE, generator=g, device=DEV).to(dt), noise0=torch.randn(SHAPE, generator=g, device=DEV).to(dt))
    return _KIN[dt]


def _run_sched(s2v, coef, npred, flags, x, nz, x0_old, dt, out_f32=False, masked=None):
    """one s2v_sched_step (masked: (record, z0, noise0, level) -> s2v_sched_step_masked) with sentinels behind element N of the output and of
    x0_hist -> (out [N + SLACK], hist [N + SLACK])"""
    lib, L = s2v.lib(), s2v._lib
    out = torch.full((N + SLACK,), SENT, dtype=torch.float32 if out_f32 else dt, device=DEV)
    hist = torch.cat([x0_old.flatten(), torch.full((SLACK,), SENT, dtype=torch.float32, device=DEV)])
    npred = npred.contiguous()
    if masked is None:
        L.check(lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(npred), flags, L.ptr(x), L.ptr(out), L.ptr(hist), L.ptr(nz), N, L.DTYPE_OF[dt],
                                   L.stream_ptr()))
    else:
        rec, z0, noise0, level = masked
        L.check(lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), L.ptr(npred), flags, L.ptr(x), L.ptr(out), L.ptr(hist), L.ptr(nz),
                                          L.ptr(z0), L.ptr(noise0), L.ptr(level), *SHAPE, L.DTYPE_OF[dt], L.stream_ptr()))
    torch.cuda.synchronize()
    return out, hist


def _sentinels_survive(out, hist):
    return bool((out[N:].float() == SENT).all()) and bool((hist[N:] == SENT).all())


# ------------------------------------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
def test_triple_kernel_equals_the_restatement_bitwise(s2v, dt_name):
    dt = DT[dt_name]
    k = _kernel_inputs(dt)
    for coef in _coefs(s2v, dt):
        for np_f32 in (0, 1):
            npred = k["planes"] if np_f32 else k["planes"].to(dt)
            prev, x0 = SG.triple_step(coef, npred, k["x"], k["x0_old"], k["nz"], dt)
            for out_f32 in (0, 1):
                out, hist = _run_sched(s2v, coef, npred, s2v._lib.SCHED_TRIPLE | 2 * np_f32 | 4 * out_f32, k["x"], k["nz"], k["x0_old"], dt, out_f32)
                what = f"kind {coef.kind}, np_f32 {np_f32}, out_f32 {out_f32}"
                exp = prev if out_f32 else prev.to(dt)
                assert _same(out[:N].view(SHAPE), exp), f"{what}: latents"
                assert _same(hist[:N].view(SHAPE), x0), f"{what}: x0 history"
                assert _sentinels_survive(out, hist), f"{what}: a write past element {N}"
    # the inputs tell the triple from a pair on any two of its planes
    pair = SG.pair_step(coef, k["planes"][1:], k["x"], k["x0_old"], k["nz"], dt)[0]
    assert not torch.equal(pair, prev)


def _levels():
    """[F, H, W] = 105 cells: levels spread over 0..255 in a fixed shuffle, with 0, 127, 128 and 255 present (the plane is too small for all 256)"""
    lv = (torch.arange(105) * 255 // 104).to(torch.uint8)
    lv = lv[torch.randperm(105, generator=torch.Generator().manual_seed(3))]
    lv[:4] = torch.tensor([0, 127, 128, 255], dtype=torch.uint8)
    return lv.reshape(3, 5, 7).contiguous().to(DEV)


@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
def test_masked_triple_kernel_equals_the_triple_step_then_add_noise_and_where(s2v, dt_name):
    dt = DT[dt_name]
    k = _kernel_inputs(dt)
    level = _levels()
    keep = (level <= 127)[:, None]
    assert 0 < int(keep.sum()) < level.numel()
    sch = H._sched(s2v, "ddim")
    for coef in _coefs(s2v, dt):
        for np_f32 in (0, 1):
            npred = k["planes"] if np_f32 else k["planes"].to(dt)
            flags = s2v._lib.SCHED_TRIPLE | 2 * np_f32
            plain, hist_a = _run_sched(s2v, coef, npred, flags, k["x"], k["nz"], k["x0_old"], dt)
            for t_next in (599, None):
                rec = sch.blend_record(t_next, dt, DEV, 127)
                got, hist_b = _run_sched(s2v, coef, npred, flags, k["x"], k["nz"], k["x0_old"], dt, masked=(rec, k["z0"], k["noise0"], level))
                proper = k["z0"] if t_next is None else sch.add_noise(k["z0"], k["noise0"], t_next)
                exp = torch.where(keep, proper, plain[:N].view(SHAPE))
                what = f"kind {coef.kind}, np_f32 {np_f32}, t_next {t_next}"
                assert _same(got[:N].view(SHAPE), exp), what
                assert _same(hist_a, hist_b) and _sentinels_survive(got, hist_b), what


# ------------------------------------------------------------------------------------------------ 2. the degenerate identity
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
def test_u_plane_with_the_bits_of_r_gives_the_pair_kernels_result_for_any_subject_scale(s2v, dt_name):
    dt = DT[dt_name]
    k = _kernel_inputs(dt)
    for np_f32 in (0, 1):
        planes = k["planes"] if np_f32 else k["planes"].to(dt)
        r, f = planes[1], planes[2]
        triple, pair_in = torch.stack([r, r.clone(), f]), torch.stack([r, f])
        for kind in range(3):
            pair = _run_sched(s2v, _coefs(s2v, dt)[kind], pair_in, 1 | 2 * np_f32, k["x"], k["nz"], k["x0_old"], dt)
            for gs in (0.5, 1.0, 7.5):
                got = _run_sched(s2v, _coefs(s2v, dt, gs)[kind], triple, s2v._lib.SCHED_TRIPLE | 2 * np_f32, k["x"], k["nz"], k["x0_old"], dt)
                assert _same(got[0], pair[0]) and _same(got[1], pair[1]), f"kind {kind}, np_f32 {np_f32}, g_subject {gs}"


# ------------------------------------------------------------------------------------------------ 3. the forward on triples
def _forward_bits(s2v, case, dt, cfg=None, lora=None):
    inp = BV._inputs(s2v, case)
    text, ref, null = BV._text(inp, [0]), inp["ref"][0:1], inp["ref"][1:2]
    coef = _coefs(s2v, dt)[0]
    lat = inp["lat"][:1].to(dt).contiguous()
    m3, e3 = BV._engine(s2v, case, dt, 3, cfg, lora)
    e3.set_conditioning_triples(text, ref, null)
    e3.denoise_step(lat.clone(), [500.0], [coef], subject=True)
    got = e3.last_noise_pred()
    e3.close()
    m2, e2 = BV._engine(s2v, case, dt, 2, cfg, lora)
    pairs = []
    for rr in (null, ref):
        e2.set_conditioning(text, rr)
        e2.denoise_step(lat.clone(), 500.0, coef)
        pairs.append(e2.last_noise_pred())
    e2.close()
    assert got.shape[0] == 3 and torch.isfinite(got.float()).all()
    assert _same(got[0], pairs[0][0]), "u: the negative row of a pair engine conditioned on the null reference"
    assert _same(got[1], pairs[1][0]), "r: the negative row of a pair engine conditioned on the reference"
    assert _same(got[2], pairs[1][1]), "f: the positive row of a pair engine conditioned on the reference"
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", ["tiny-rope", "mid-rope"])
def test_triple_rows_hold_the_bits_of_the_pair_engines_rows(s2v, case, dt_name):
    _forward_bits(s2v, case, DT[dt_name])


@pytest.mark.parametrize("engine", ["lora-runtime", "fp8"])
def test_triple_rows_hold_the_bits_of_the_pair_engines_rows_with_runtime_lora_and_fp8(s2v, engine):
    lora = None
    if engine == "lora-runtime":
        cfg = BV._lora_cfg(s2v, None, 8)
        lora = s2v.weights.synthetic_lora(cfg, rank=8, seed=84, std=0.05)
    else:
        cfg = BV._lora_cfg(s2v, engine)
    _forward_bits(s2v, "d256", torch.bfloat16, cfg, lora)


# ------------------------------------------------------------------------------------------------ 4. the step
def _video_plan(s2v, kind, dt, k):
    """video k's STEPS steps: [(timestep, coefficient set)].  Video 0 runs `kind` on 3 steps at (GS, GT); video 1 the OTHER scheduler on the last
    3 of 4 steps (strength 0.75) at its own scales: other timesteps, scales and kinds beside it"""
    kind_k = kind if k == 0 else ("dpm" if kind == "ddim" else "ddim")
    n, strength, gs, gt = ((3, None, GS, GT), (4, 0.75, 0.37109375 + 2 ** -20, 4.5 + 2 ** -18))[k]
    steps = s2v.S2VPipeline.video_plan(H._sched(s2v, kind_k), n, strength, gt, False, dt, guidance_subject=gs)["steps"]
    assert len(steps) == STEPS
    return [(float(st["t"]), st["coef"]) for st in steps]


def _guided_steps(s2v, eng, plans, dt, lat, noise, graph):
    """STEPS guided steps on lat [b,...]; after every step the latents and the x0 history must be the restatement applied to the model outputs
    the step itself left (last_noise_pred: [u x b | r x b | f x b]); returns ([(latents, x0_hist)], hipGraph captures made)"""
    b = lat.shape[0]
    x = lat.to(dt).contiguous().clone()
    x0, nz = torch.zeros(x.shape, dtype=torch.float32, device=DEV), torch.empty_like(x)
    before = eng.lora_state["graph_captures"]
    out = []
    for i in range(STEPS):
        nz.copy_(noise[i].to(dt))
        x_in, x0_in = x.clone(), x0.clone()
        eng.denoise_step(x, [p[i][0] for p in plans], [p[i][1] for p in plans], x0, nz, use_graph=graph, subject=True)
        torch.cuda.synchronize()
        npred = eng.last_noise_pred()
        assert npred.shape[0] == 3 * b
        for k in range(b):
            prev, e_x0 = SG.triple_step(plans[k][i][1], npred[[k, b + k, 2 * b + k]], x_in[k], x0_in[k], nz[k], dt)
            assert _same(x[k], prev.to(dt)), f"step {i}, video {k}: latents against the restatement"
            assert _same(x0[k], e_x0), f"step {i}, video {k}: x0 history against the restatement"
        out.append((x.clone(), x0.clone()))
    assert torch.isfinite(x.float()).all()
    return out, eng.lora_state["graph_captures"] - before


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("case,dt_name", [("mid-rope", "bf16"), ("tiny-rope", "f32")])
def test_guided_steps_equal_the_restatement_and_two_videos_equal_their_one_video_runs(s2v, case, dt_name, kind, graph):
    dt = DT[dt_name]
    inp = BV._inputs(s2v, case)
    null = inp["ref"][2:4] * 0.5
    plans = [_video_plan(s2v, kind, dt, k) for k in range(2)]
    assert {c.kind for p in plans for _, c in p} == {0, 1, 2} and plans[0][0][0] != plans[1][0][0]
    m, eng = BV._engine(s2v, case, dt, 6)
    eng.set_conditioning_triples(BV._text(inp, [0, 1]), inp["ref"][:2], null)
    two, captures = _guided_steps(s2v, eng, plans, dt, inp["lat"][:2], inp["noise"][:, :2], graph)
    eng.close()
    assert captures == (1 if graph else 0), f"{captures} captures over {STEPS} steps: one graph serves every step"
    m, eng = BV._engine(s2v, case, dt, 3)
    for k in range(2):
        eng.set_conditioning_triples(BV._text(inp, [k]), inp["ref"][k:k + 1], null[k:k + 1])
        one, captures = _guided_steps(s2v, eng, [plans[k]], dt, inp["lat"][k:k + 1], inp["noise"][:, k:k + 1], graph)
        # re-conditioning in the same layout keeps a captured step (it reads the same buffers): a second capture happens only when the
        # allocator hands this run other latents / history / noise addresses than the last one's
        assert captures <= (1 if graph else 0)
        for i in range(STEPS):
            assert _same(two[i][0][k:k + 1], one[i][0]) and _same(two[i][1][k:k + 1], one[i][1]), f"step {i}: video {k} of two differs from its own run"
    eng.close()
    assert not torch.equal(two[-1][0][0], two[-1][0][1])


# ------------------------------------------------------------------------------------------------ 5. the pipeline
PH, PW, PF, PT, VF = H.PH, H.PW, H.PF, H.PT, H.VF


def _pipe_inputs(s2v, dt):
    inp = H._inputs(s2v, "tiny-rope")
    return inp["pos"][:2].to(dt), inp["neg"][:2].to(dt), inp["ref"][:2].to(dt), (inp["ref"][2:4] * 0.5).to(dt)


def test_pipeline_text_to_video_equals_hand_driven_guided_steps_bitwise(s2v):
    dt = torch.bfloat16
    pos, neg, ref, null = _pipe_inputs(s2v, dt)
    pipe = H._pipe(s2v, "dpm", dt)
    sch, eng = pipe.scheduler, pipe.transformer.engine
    got = pipe(prompt_embeds=pos[:1], negative_prompt_embeds=neg[:1], ref_img_states=ref[:1], negative_ref_img_states=null[:1],
               generator=torch.Generator().manual_seed(977), height=PH, width=PW, num_frames=PF, num_inference_steps=4, guidance_scale=GT,
               subject_guidance_scale=GS, use_graph=True)["frames"].clone()
    assert eng.geometry[0] == 3 and eng.triples
    g = torch.Generator().manual_seed(977)
    lat = pipe.prepare_latents(PF, PH, PW, dt, DEV, g, None, 1).to(dt).contiguous()
    sch.set_timesteps(4)
    eng.set_geometry(3, PT, lat.shape[1], PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning_triples(torch.cat([neg[:1], pos[:1]]), ref[:1], null[:1])
    x0 = torch.zeros(lat.shape, dtype=torch.float32, device=DEV)
    for i, t in enumerate(sch.timesteps):
        coef = sch.coef(t, sch.timesteps[i - 1] if i > 0 else None, i == 0, dt, GT, guidance_subject=GS)
        for _ in range(2 if coef.kind == 2 else 1):
            noise = s2v.pipeline.randn_videos(lat.shape, g, DEV, dt).contiguous()
        eng.denoise_step(lat, [float(t)], [coef], x0, noise, subject=True)
    torch.cuda.synchronize()
    assert _same(got, lat)
    plain = pipe(prompt_embeds=pos[:1], negative_prompt_embeds=neg[:1], ref_img_states=ref[:1], generator=torch.Generator().manual_seed(977),
                 height=PH, width=PW, num_frames=PF, num_inference_steps=4, guidance_scale=GT)["frames"]
    assert eng.geometry[0] == 2 and not eng.triples and not torch.equal(plain, got)
    eng.close()


def test_pipeline_video_and_change_map_with_two_step_counts_equals_hand_driven_guided_steps_bitwise(s2v):
    dt = torch.bfloat16
    P = s2v.S2VPipeline
    pos, neg, ref, null = _pipe_inputs(s2v, dt)
    pipe = H._pipe(s2v, "ddim", dt, H._vae(s2v, dt))
    sch, eng = pipe.scheduler, pipe.transformer.engine
    video = H._videos(2)
    xs = torch.linspace(0, 1, PW)[None, None, None, :]
    cmap = (xs * torch.tensor([1.3, 1.1])[:, None, None, None] - 0.15).clamp(0, 1).expand(2, VF, PH, PW).contiguous()
    strength, scales, guid = [0.5, 1.0], [GS, 0.37109375], [GT, 4.5]
    got = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, negative_ref_img_states=null, video=video, change_map=cmap,
               strength=strength, generator=H._gens(range(2)), height=PH, width=PW, num_inference_steps=4, guidance_scale=guid,
               subject_guidance_scale=scales, use_graph=True)["frames"].clone()
    assert eng._blend is None, "the blend operands are cleared when the call ends"
    plans = [P.video_plan(sch, 4, strength[k], guid[k], False, dt, guidance_subject=scales[k]) for k in range(2)]
    assert [len(p["steps"]) for p in plans] == [2, 4]
    order = [1, 0]   # longest plan first
    lat, z0, noise0 = pipe.prepare_video_latents(video, dt, DEV, H._gens(range(2)), [p["timesteps"][0] for p in plans])
    level, _ = s2v.engine.map_to_latent(cmap, DEV)
    lat, z0, noise0, level = (t[order].contiguous() for t in (lat.to(dt), z0.to(dt), noise0.to(dt), level))
    blends = [P.blend_plan(sch, plans[k], dt, DEV, s2v.pipeline.change_map_plan(len(plans[k]["timesteps"]))) for k in order]
    for a, first in ((2, 0), (1, 2)):
        rows = order[:a]
        eng.set_geometry(3 * a, PT, lat.shape[1], PH // 8, PW // 8)
        eng.prepare_tables(PH, PW)
        eng.set_conditioning_triples(torch.cat([neg[rows], pos[rows]]), ref[rows], null[rows])
        eng.set_blend(z0[:a], noise0[:a], level[:a])
        for i in range(first, first + 2):
            steps = [plans[k]["steps"][i] for k in rows]
            eng.denoise_step(lat[:a], [float(st["t"]) for st in steps], [st["coef"] for st in steps], blend=[blends[p][i] for p in range(a)],
                             use_graph=True, subject=True)
    eng.clear_blend()
    torch.cuda.synchronize()
    exp = lat[[1, 0]]   # back to the caller's order
    assert _same(got, exp)
    kept = (level[[1, 0]] == 0)[:, :, None].expand(-1, -1, 16, -1, -1)
    assert kept.any() and _same(got[kept], z0[[1, 0]][kept]), "the final latents are z0 wherever the level is 0"
    eng.close()


def test_pipeline_with_the_reference_as_its_own_null_equals_the_plain_call_bitwise(s2v):
    """the end-to-end form of the degenerate identity: u is r, so whatever the subject scale the latents are those of the call without it"""
    dt = torch.bfloat16
    pos, neg, ref, _ = _pipe_inputs(s2v, dt)
    pipe = H._pipe(s2v, "dpm", dt)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, height=PH, width=PW, num_frames=PF, num_inference_steps=STEPS,
              guidance_scale=GT, use_graph=True)
    plain = pipe(generator=H._gens(range(2)), subject_guidance_scale=None, **kw)["frames"].clone()
    for gs in (0.5, 7.5):
        got = pipe(generator=H._gens(range(2)), subject_guidance_scale=gs, negative_ref_img_states=ref, **kw)["frames"]
        assert _same(got, plain), f"subject scale {gs}"
    assert not torch.equal(plain[0], plain[1])
    pipe.transformer.engine.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_library_refusals_are_named_and_nothing_is_launched_after_them(s2v):
    case, dt = "tiny-rope", torch.bfloat16
    _, T, F, Hh, W = BV.CASES[case]
    inp = BV._inputs(s2v, case)
    lib, L = s2v.lib(), s2v._lib
    coef = _coefs(s2v, dt)[0]
    lat = inp["lat"][:3].to(dt).contiguous()
    x = lat.clone()

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(x, lat)

    # a geometry that is no whole number of triples
    m, eng = BV._engine(s2v, case, dt, 2)
    eng.set_conditioning(BV._text(inp, [0]), inp["ref"][:1])
    with pytest.raises(s2v.S2VError, match=r"s2v_denoise_step_guided: a geometry of B = 3b samples"):
        L.check(lib.s2v_denoise_step_guided(eng._h, L.ptr(x[:1]), (ctypes.c_float * 1)(500.0), (L.SchedCoefC * 1)(coef), None, None, None, 0, None))
    t4 = BV._text(inp, [0, 1]).to(dt).contiguous()
    r1 = inp["ref"][:1].to(dt).contiguous()
    assert lib.s2v_set_conditioning_triples(eng._h, L.ptr(t4), L.ptr(r1), L.ptr(r1), 1, None) != 0
    assert b"s2v_set_conditioning_triples: a geometry of B = 3b samples" in lib.s2v_last_error()
    # B = 6 is three pairs or two triples by shape alone: the context knows which
    eng.set_geometry(6, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(BV._text(inp, [0, 1, 2]), inp["ref"][:3])
    with pytest.raises(s2v.S2VError, match=r"s2v_denoise_step_guided: the conditioning was not set by s2v_set_conditioning_triples"):
        eng.denoise_step(x[:2], [500.0] * 2, [coef] * 2, subject=True)
    assert untouched()
    eng.set_conditioning_triples(BV._text(inp, [0, 1]), inp["ref"][:2])
    with pytest.raises(s2v.S2VError, match=r"s2v_denoise_step: the context is conditioned as subject-guidance triples"):
        eng.denoise_step(x, 500.0, coef)
    with pytest.raises(s2v.S2VError, match=r"s2v_denoise_step: the context is conditioned as subject-guidance triples"):
        eng.denoise_step(x, [500.0] * 3, [coef] * 3)
    rec = H._sched(s2v, "ddim").blend_record(599, dt, DEV, 0)
    assert lib.s2v_denoise_step_masked(eng._h, L.ptr(x), (ctypes.c_float * 3)(*[500.0] * 3), (L.SchedCoefC * 3)(*[coef] * 3), (L.BlendC * 3)(*[rec] * 3),
                                       None, None, 0, None) != 0
    assert b"s2v_denoise_step_masked: the context is conditioned as subject-guidance triples" in lib.s2v_last_error()
    n_null = lib.s2v_set_conditioning_triples(eng._h, L.ptr(t4), L.ptr(inp["ref"][:2].to(dt).contiguous()), L.ptr(r1), 3, None)
    assert n_null != 0 and b"n_null must be 1" in lib.s2v_last_error()
    assert untouched()
    # an armed step-cache mode, an armed attention map: both assume pairs
    eng.set_conditioning_triples(BV._text(inp, [0, 1]), inp["ref"][:2])
    eng.step_cache_enable(True)
    with pytest.raises(s2v.S2VError, match=r"s2v_denoise_step_guided: a step-cache mode"):
        eng.denoise_step(x[:2], [500.0] * 2, [coef] * 2, cache="capture", subject=True)
    eng.step_cache_enable(False)
    eng.attn_map_enable(True)
    with pytest.raises(s2v.S2VError, match=r"s2v_denoise_step_guided: an attention map is armed"):
        eng.denoise_step(x[:2], [500.0] * 2, [coef] * 2, attn_layers=[0], subject=True)
    eng.attn_map_enable(False)
    assert untouched()
    # masked form: operands of another video count
    rec2 = (L.BlendC * 2)(rec, rec)
    assert lib.s2v_denoise_step_guided(eng._h, L.ptr(x[:2]), (ctypes.c_float * 2)(500.0, 500.0), (L.SchedCoefC * 2)(coef, coef), rec2, None, None, 0,
                                       None) != 0
    assert b"s2v_denoise_step_guided: s2v_set_blend has not set the blend operands" in lib.s2v_last_error()
    assert untouched()
    # ... and the arms were consumed: the same engine now runs the step
    eng.denoise_step(x[:2], [500.0] * 2, [coef] * 2, subject=True)
    torch.cuda.synchronize()
    assert not torch.equal(x[:2], lat[:2]) and torch.equal(x[2], lat[2]) and torch.isfinite(x.float()).all()
    x.copy_(lat)
    eng.close()
    # a pending CFG-parallel split (its geometry is B = 1)
    m, eng = BV._engine(s2v, case, dt, 1)
    eng.set_conditioning(inp["pos"][:1], inp["ref"][:1])
    eng.denoise_split_begin(x[:1], 500.0, coef, 0)
    with pytest.raises(s2v.S2VError, match=r"s2v_denoise_step_guided: a CFG-parallel split is pending"):
        L.check(lib.s2v_denoise_step_guided(eng._h, L.ptr(x[:1]), (ctypes.c_float * 1)(500.0), (L.SchedCoefC * 1)(coef), None, None, None, 0, None))
    assert untouched()
    eng.close()
    # a shard context
    m, sh = BV._engine(s2v, case, dt, 2)
    sh.set_shard(2, 0)
    sh.set_geometry(3, T, F, Hh, W)
    assert lib.s2v_set_conditioning_triples(sh._h, L.ptr(t4[:2].contiguous()), L.ptr(r1), L.ptr(r1), 1, None) != 0
    assert b"s2v_set_conditioning_triples: a shard context" in lib.s2v_last_error()
    assert lib.s2v_denoise_step_guided(sh._h, L.ptr(x[:1]), (ctypes.c_float * 1)(500.0), (L.SchedCoefC * 1)(coef), None, None, None, 0, None) != 0
    assert b"s2v_denoise_step_guided: a shard context" in lib.s2v_last_error()
    assert untouched()
    sh.close()
    # bit0 and bit3 together
    k = _kernel_inputs(dt)
    out = torch.full((N,), SENT, dtype=dt, device=DEV)
    npred = k["planes"].to(dt).contiguous()
    assert lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(npred), 1 | 8, L.ptr(k["x"]), L.ptr(out), None, None, N, L.DTYPE_OF[dt], None) != 0
    assert b"s2v_sched_step: flags bit0" in lib.s2v_last_error() and b"exclude each other" in lib.s2v_last_error()
    assert lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), L.ptr(npred), 1 | 8, L.ptr(k["x"]), L.ptr(out), None, None,
                                     L.ptr(k["z0"]), L.ptr(k["noise0"]), L.ptr(_levels()), *SHAPE, L.DTYPE_OF[dt], None) != 0
    assert b"s2v_sched_step_masked: flags bit0" in lib.s2v_last_error()
    torch.cuda.synchronize()
    assert bool((out.float() == SENT).all())
