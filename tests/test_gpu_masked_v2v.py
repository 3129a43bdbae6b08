"""Masked video-to-video on the GPU (include/s2v_hip.h: s2v_mask_to_latent, s2v_set_blend, s2v_denoise_step_masked, s2v_sched_step_masked,
s2v_vae_postprocess_masked / _u8_masked; S2VPipeline(mask=..., paste_back=...)).  Every comparison is BITWISE: the mask is exactly 0 or 1, so
the blend is a select between the step's stored result and add_noise's (or the clean latents), and both sides of every test run the same
kernels on the same values.

The engine case, weights, inputs and plans are those of tests/test_gpu_batch_hetero.py ("mid-rope": one video is 75 072 elements = 293.25
blocks, and no index of the mask plane is a power of two); so are the tiny pipeline and VAE (64 x 96 pixels, 9 frames, latents 3 x 8 x 12)."""
import ctypes

import pytest
import torch

import masked_v2v_ref as R
import test_gpu_batch_hetero as H

pytestmark = pytest.mark.gpu
DEV = H.DEV
DT = H.DT
STEPS = H.STEPS
CASE = "mid-rope"
# video k of the engine tests runs plan VID_PLANS[k] of test_gpu_batch_hetero.PLANS; (3, 1.0, 7.5) has exactly three steps, so its third step is its
# last: for b = 3 one video on its last step sits beside two that are not, every video at its own timestep
VID_PLANS = [0, 3, 2]


def _plan(s2v, kind, dt, k):
    """[(timestep, coefficient set, blend record)] of the first STEPS steps of PLANS[k]"""
    n, strength, g = H.PLANS[k]
    sch = H._sched(s2v, kind)
    plan = s2v.S2VPipeline.video_plan(sch, n, strength, g, False, dt)
    recs = s2v.S2VPipeline.blend_plan(sch, plan, dt, DEV)
    ts = plan["timesteps"]
    return [(float(st["t"]), st["coef"], recs[i], ts[i + 1] if i + 1 < len(ts) else None) for i, st in enumerate(plan["steps"][:STEPS])]


_OPER = {}


def _operands(s2v, dt_name):
    """z0, noise0 [3,...] in the model dtype and a Bernoulli(0.5) latent mask that differs per video: made once, never written"""
    if dt_name not in _OPER:
        _, T, F, Hh, W = H.CASES[CASE]
        g = torch.Generator(device=DEV).manual_seed(91)
        shape = (3, F, 16, Hh, W)
        z0 = (torch.randn(shape, generator=g, device=DEV) * 0.7).to(DT[dt_name])
        z0[:, 0, 0, 0, :4] = torch.tensor([-0.0, 0.0, -0.0, 1.0], device=DEV).to(DT[dt_name])   # signed zeros that the last step must keep
        noise0 = torch.randn(shape, generator=g, device=DEV).to(DT[dt_name])
        mask = (torch.rand((3, F, Hh, W), generator=g, device=DEV) < 0.5).to(torch.uint8)
        mask[:, 0, 0, :4] = 0
        assert not torch.equal(mask[0], mask[1]) and not torch.equal(mask[1], mask[2])
        _OPER[dt_name] = (z0.contiguous(), noise0.contiguous(), mask.contiguous())
    return _OPER[dt_name]


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
def test_masked_step_equals_the_unmasked_step_then_add_noise_and_where_bitwise(s2v, dt_name, kind, graph, b):
    dt, dpm = DT[dt_name], kind == "dpm"
    inp = H._inputs(s2v, CASE)
    z0, noise0, mask = (x[:b].contiguous() for x in _operands(s2v, dt_name))
    plans = [_plan(s2v, kind, dt, VID_PLANS[k]) for k in range(b)]
    if b == 3:
        for i in range(STEPS):
            assert len({p[i][0] for p in plans}) == 3, "every video on its own timestep"
        assert [p[STEPS - 1][2].last for p in plans] == [0, 1, 0], "one video on its last step beside two that are not"
    sch = H._sched(s2v, kind)
    m, eng = H._engine(s2v, CASE, dt, 2 * b)
    eng.set_conditioning(H._text(inp, list(range(b))), inp["ref"][:b])
    keep = (mask == 0)[:, :, None]

    def run(masked):
        x = inp["lat"][:b].to(dt).contiguous().clone()
        x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
        nz = torch.empty_like(x) if dpm else None
        out = []
        for i in range(STEPS):
            if dpm:
                nz.copy_(inp["noise"][i, :b].to(dt))
            ts, cs = [p[i][0] for p in plans], [p[i][1] for p in plans]
            if masked:
                eng.denoise_step(x, ts, cs, x0, nz, use_graph=graph, blend=[p[i][2] for p in plans])
            else:   # the unfused composition: the unmasked step, Scheduler.add_noise at t_next (the clean latents after the last step), torch.where
                eng.denoise_step(x, ts, cs, x0, nz, use_graph=False)
                for k in range(b):
                    t_next = plans[k][i][3]
                    proper = z0[k:k + 1] if t_next is None else sch.add_noise(z0[k:k + 1], noise0[k:k + 1], t_next)
                    x[k:k + 1] = torch.where(keep[k:k + 1], proper, x[k:k + 1])
            torch.cuda.synchronize()
            out.append((x.clone(), x0.clone() if dpm else None))
        return out

    exp = run(False)
    eng.set_blend(z0, noise0, mask)
    before = eng.lora_state["graph_captures"]
    got = run(True)
    captures = eng.lora_state["graph_captures"] - before
    eng.clear_blend()
    eng.close()
    assert captures == (1 if graph else 0), f"{captures} captures over {STEPS} masked steps: one graph serves every step"
    for i in range(STEPS):
        assert torch.equal(got[i][0].view(torch.uint8), exp[i][0].view(torch.uint8)), f"step {i}: latents differ"
        if dpm:
            assert torch.equal(got[i][1], exp[i][1]), f"step {i}: the x0 history must keep the unblended x0"
    full = keep.expand(-1, -1, 16, -1, -1)
    if b == 3:   # video 1 has ended: its kept cells are z0's own bits, signed zeros included
        assert torch.equal(got[-1][0][1][full[1]].view(torch.uint8), z0[1][full[1]].view(torch.uint8))
        assert torch.signbit(got[-1][0][1, 0, 0, 0, 0].float()) and not torch.signbit(got[-1][0][1, 0, 0, 0, 1].float())


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_seam_level_masked_sched_step_equals_sched_step_then_the_blend(s2v, kind):
    """s2v_sched_step_masked for one video against s2v_sched_step + add_noise + where, both blend branches"""
    dt = torch.bfloat16
    lib, L = s2v.lib(), s2v._lib
    _, T, F, Hh, W = H.CASES[CASE]
    z0, noise0, mask = (x[:1].contiguous() for x in _operands(s2v, "bf16"))
    g = torch.Generator(device=DEV).manual_seed(92)
    npred = torch.randn(2, F, 16, Hh, W, generator=g, device=DEV).to(dt)
    x = torch.randn(1, F, 16, Hh, W, generator=g, device=DEV).to(dt)
    nz = torch.randn(1, F, 16, Hh, W, generator=g, device=DEV).to(dt)
    sch = H._sched(s2v, kind)
    for t_next in (599, None):
        _, coef, _, _ = _plan(s2v, kind, dt, 1)[1]
        rec = sch.blend_record(t_next, dt, DEV)
        hist_a = torch.full(x.shape, 0.25, dtype=torch.float32, device=DEV)
        hist_b = hist_a.clone()
        plain, got = torch.empty_like(x), torch.empty_like(x)
        L.check(lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(npred), 1, L.ptr(x), L.ptr(plain), L.ptr(hist_a), L.ptr(nz), x.numel(),
                                   L.DTYPE_OF[dt], L.stream_ptr()))
        L.check(lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), L.ptr(npred), 1, L.ptr(x), L.ptr(got), L.ptr(hist_b), L.ptr(nz),
                                          L.ptr(z0), L.ptr(noise0), L.ptr(mask), F, 16, Hh, W, L.DTYPE_OF[dt], L.stream_ptr()))
        torch.cuda.synchronize()
        proper = z0 if t_next is None else sch.add_noise(z0, noise0, t_next)
        exp = torch.where((mask == 0)[:, :, None], proper, plain)
        assert torch.equal(got.view(torch.uint8), exp.view(torch.uint8)) and torch.equal(hist_a, hist_b)
    assert lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), L.ptr(npred), 1 | 4, L.ptr(x), L.ptr(got), L.ptr(hist_b), L.ptr(nz),
                                     L.ptr(z0), L.ptr(noise0), L.ptr(mask), F, 16, Hh, W, L.DTYPE_OF[dt], L.stream_ptr()) != 0
    assert b"fp32 output, is refused" in lib.s2v_last_error()


def test_masked_entry_refuses_by_name_and_an_unmasked_step_afterwards_is_a_fresh_engines(s2v):
    """the refusals of the masked entry; then (nothing else moved) an unmasked step on an engine that has made masked steps equals the same
    step on a fresh engine, eager and graph: the operands were cleared and the graph re-keyed"""
    dt, kind = torch.bfloat16, "dpm"
    inp = H._inputs(s2v, CASE)
    _, T, F, Hh, W = H.CASES[CASE]
    z0, noise0, mask = _operands(s2v, "bf16")
    plan = _plan(s2v, kind, dt, 0)
    m, eng = H._engine(s2v, CASE, dt, 2)
    eng.set_conditioning(H._text(inp, [0]), inp["ref"][:1])
    x = inp["lat"][:1].to(dt).contiguous().clone()
    x0, nz = torch.zeros(x.shape, dtype=torch.float32, device=DEV), inp["noise"][0, :1].to(dt).contiguous()
    keep = x.clone()
    with pytest.raises(s2v.S2VError, match="s2v_set_blend has not set the blend operands"):
        eng.denoise_step(x, [plan[0][0]], [plan[0][1]], x0, nz, blend=plan[0][2])
    with pytest.raises(s2v.S2VError, match=r"set_blend: z0 must be contiguous \[1, 3, 16, 34, 46\]"):
        eng.set_blend(z0[:2], noise0[:2], mask[:2])
    with pytest.raises(s2v.S2VError, match="set_blend: latent_mask must be contiguous uint8"):
        eng.set_blend(z0[:1], noise0[:1], mask[:1].float())
    eng.set_blend(z0[:1].contiguous(), noise0[:1].contiguous(), mask[:1].contiguous())
    with pytest.raises(s2v.S2VError, match="s2v_denoise_step_masked: DPM needs noise and x0_hist"):
        eng.denoise_step(x, [plan[0][0]], [plan[0][1]], None, None, blend=plan[0][2])
    with pytest.raises(s2v.S2VError, match="`blend` has 2 entries for b = 1 videos"):
        eng.denoise_step(x, [plan[0][0]], [plan[0][1]], x0, nz, blend=[plan[0][2]] * 2)
    # B = 1 (one sample of a CFG-parallel pair) and a shard context
    eng.set_geometry(1, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(inp["pos"][:1], inp["ref"][:1])
    with pytest.raises(s2v.S2VError, match=r"s2v_denoise_step_masked: a geometry with B = 1 .* the split entries .* have no masked form"):
        eng.denoise_step(x, [plan[0][0]], [plan[0][1]], x0, nz, blend=plan[0][2])
    eng.clear_blend()
    ms, sh = H._engine(s2v, "tiny-rope", dt, 2)
    sh.set_shard(2, 0)
    sh.set_geometry(2, *H.CASES["tiny-rope"][1:])
    lib, L = s2v.lib(), s2v._lib
    t_arr, c_arr, b_arr = (ctypes.c_float * 1)(plan[0][0]), (L.SchedCoefC * 1)(plan[0][1]), (L.BlendC * 1)(plan[0][2])
    assert lib.s2v_denoise_step_masked(sh._h, L.ptr(x), t_arr, c_arr, b_arr, L.ptr(x0), L.ptr(nz), 0, L.stream_ptr()) != 0
    assert b"s2v_denoise_step_masked: a shard context (s2v_set_shard) has no masked step" in lib.s2v_last_error()
    sh.close()
    torch.cuda.synchronize()
    assert torch.equal(x, keep), "a refused step touches nothing"
    # masked steps (graph), then unmasked steps on the same buffers: the bits of an engine that never saw a mask
    eng.set_geometry(2, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(H._text(inp, [0]), inp["ref"][:1])
    for graph in (True, False):
        eng.set_blend(z0[:1].contiguous(), noise0[:1].contiguous(), mask[:1].contiguous())
        y, y0 = x.clone(), x0.clone()
        eng.denoise_step(y, [plan[0][0]], [plan[0][1]], y0, nz, use_graph=graph, blend=plan[0][2])
        eng.clear_blend()
        got = H._steps(eng, [[(p[0], p[1]) for p in plan]], dt, inp["lat"][:1], inp["noise"][:, :1], graph, True, scalar=True)
        exp = H._single(s2v, CASE, "bf16", kind)[0]
        for i in range(STEPS):
            assert torch.equal(got[i][0], exp[i][0]) and torch.equal(got[i][1], exp[i][1]), f"graph={graph}, step {i}"
    eng.close()


# ------------------------------------------------------------------------------------------------ the pipeline
PH, PW, VF = H.PH, H.PW, H.VF


def _masks(n):
    """n pixel masks [n, VF, PH, PW] float in [0, 1], blobs of about a third of the frame so that kept and repainted latent cells both exist"""
    g = torch.Generator().manual_seed(78)
    coarse = torch.rand(n, VF, PH // 16, PW // 16, generator=g)
    m = torch.nn.functional.interpolate(coarse[:, None], size=(VF, PH, PW), mode="nearest")[:, 0]
    return (m < 0.35).float() * torch.rand(n, VF, PH, PW, generator=g).clamp(min=0.5)   # values in {0} and [0.5, 1): binarised at 0.5


def _call_kw(mode):
    return dict(height=PH, width=PW, num_inference_steps=4, guidance_scale=6.0, **H._mode_kw(mode))


def _z0_noise(vae, video, g, dt):
    """the two lines prepare_video_latents uses, on an identically seeded generator"""
    z0 = vae.encode(video).latent_dist.sample(g)
    z0 = vae.config.scaling_factor * z0.to(dt).permute(0, 2, 1, 3, 4).contiguous()
    noise = torch.randn(z0.shape, generator=g, device=g.device, dtype=dt).to(DEV)
    return z0.to(DEV), noise


@pytest.mark.parametrize("mode", ["fused-graph", "seams"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_masked_call_equals_the_unmasked_call_with_a_blending_callback_bitwise(s2v, kind, mode):
    inp = H._inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    args = dict(prompt_embeds=inp["pos"][:1].to(dt), negative_prompt_embeds=inp["neg"][:1].to(dt), ref_img_states=inp["ref"][:1].to(dt))
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, kind, dt, vae)
    video, mask = H._videos(1), _masks(1)
    kw = _call_kw(mode)
    seen = []
    got = pipe(video=video, mask=mask, strength=0.75, generator=H._gens([0])[0], output_type="latent",
               callback_on_step_end=lambda p, i, t, tensors: seen.append(tensors["latents"].clone()) or {}, **args, **kw)["frames"].clone()
    z0, noise0 = _z0_noise(vae, video, H._gens([0])[0], dt)
    sch = H._sched(s2v, kind)
    sch.set_timesteps(4)
    ts = sch.timesteps[1:]
    keep = (R.latent_mask(mask).to(DEV) == 0)[:, :, None]
    assert 0 < int(keep.sum()) < keep.numel()
    shown = []

    def blend(p, i, t, tensors):
        x = tensors["latents"]
        proper = z0 if i + 1 == len(ts) else sch.add_noise(z0, noise0, ts[i + 1])
        shown.append(torch.where(keep, proper, x))
        return {"latents": shown[-1]}

    exp = pipe(video=video, strength=0.75, generator=H._gens([0])[0], output_type="latent", callback_on_step_end=blend, **args, **kw)["frames"]
    assert torch.equal(got.view(torch.uint8), exp.view(torch.uint8))
    assert len(seen) == 3 and all(torch.equal(a, b) for a, b in zip(seen, shown)), "a step-end callback sees the blended latents"
    full = keep.expand(-1, -1, 16, -1, -1)
    assert torch.equal(got[full].view(torch.uint8), z0[full].view(torch.uint8)), "the final latents are z0 wherever m = 0"
    assert not torch.equal(got[~full], z0[~full])
    assert pipe.transformer.engine._blend is None, "the blend operands are cleared when the call ends"
    pipe.transformer.engine.close()


@pytest.mark.parametrize("mode", ["fused-graph", "seams"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_three_masked_videos_on_their_own_strength_equal_three_single_masked_calls_bitwise(s2v, kind, mode):
    inp = H._inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    pos, neg, ref = inp["pos"][:3].to(dt), inp["neg"][:3].to(dt), inp["ref"][:3].to(dt)
    pipe = H._pipe(s2v, kind, dt, H._vae(s2v, dt))
    vids, masks = H._videos(3), _masks(3)
    kw = dict(output_type="latent", **_call_kw(mode))
    args = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, video=vids, strength=H.STRENGTHS)
    own = pipe(mask=masks[:, None], generator=H._gens(range(3)), **args, **kw)["frames"].clone()
    shared = pipe(mask=masks[1:2], generator=H._gens(range(3)), **args, **kw)["frames"].clone()
    for k in range(3):
        one_kw = dict(prompt_embeds=pos[k:k + 1], negative_prompt_embeds=neg[k:k + 1], ref_img_states=ref[k:k + 1], video=vids[k:k + 1],
                      strength=H.STRENGTHS[k], **kw)
        one = pipe(mask=masks[k:k + 1], generator=H._gens([k])[0], **one_kw)["frames"]
        assert torch.equal(own[k:k + 1].view(torch.uint8), one.view(torch.uint8)), f"video {k} (its own mask, strength {H.STRENGTHS[k]})"
        one = pipe(mask=masks[1:2], generator=H._gens([k])[0], **one_kw)["frames"]
        assert torch.equal(shared[k:k + 1].view(torch.uint8), one.view(torch.uint8)), f"video {k} (the shared mask, strength {H.STRENGTHS[k]})"
    assert torch.equal(own[1], shared[1]) and not torch.equal(own[0], shared[0])
    pipe.transformer.engine.close()


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_the_two_ends_of_the_mask(s2v, kind):
    inp = H._inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    args = dict(prompt_embeds=inp["pos"][:1].to(dt), negative_prompt_embeds=inp["neg"][:1].to(dt), ref_img_states=inp["ref"][:1].to(dt))
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, kind, dt, vae)
    video = H._videos(1)
    kw = dict(video=video, strength=0.75, **args, **_call_kw("fused-graph"))
    ones, zeros = torch.ones(1, VF, PH, PW), torch.zeros(1, 1, VF, PH, PW)
    plain = pipe(generator=H._gens([0])[0], output_type="latent", **kw)["frames"].clone()
    assert torch.equal(pipe(mask=ones, generator=H._gens([0])[0], output_type="latent", **kw)["frames"], plain), "all ones: plain video-to-video"
    plain_np = pipe(generator=H._gens([0])[0], output_type="np", **kw)["frames"]
    got_np = pipe(mask=ones, generator=H._gens([0])[0], output_type="np", **kw)["frames"]
    assert got_np.shape == (1, VF, PH, PW, 3) and (got_np == plain_np).all(), "all ones with paste-back: the frames of plain video-to-video"
    z0, _ = _z0_noise(vae, video, H._gens([0])[0], dt)
    got = pipe(mask=zeros, generator=H._gens([0])[0], output_type="latent", **kw)["frames"]
    assert torch.equal(got.view(torch.uint8), z0.view(torch.uint8)), "all zeros: the clean input latents, bit for bit"
    seams = pipe(mask=zeros, generator=H._gens([0])[0], output_type="latent", **dict(kw, fused=False, use_graph=False))["frames"]
    assert torch.equal(seams.view(torch.uint8), z0.view(torch.uint8))
    # paste-back: with an all-zeros mask the frames are the post-processed input video; without paste-back, the decoded one
    kept = pipe(mask=zeros, generator=H._gens([0])[0], output_type="np", **kw)["frames"]
    assert (kept == vae.postprocess_video(video.to(DEV), "np")).all()
    raw = pipe(mask=zeros, paste_back=False, generator=H._gens([0])[0], output_type="np", **kw)["frames"]
    assert (raw == vae.postprocess_video(vae.decode_latents(z0), "np")).all() and not (raw == kept).all()
    pipe.transformer.engine.close()


# ------------------------------------------------------------------------------------------------ the mask kernel and the paste-back
@pytest.mark.parametrize("shape", [(VF, 64, 96), (VF, 272, 368), (1, 64, 96), (17, 64, 96)], ids=lambda s: "x".join(map(str, s)))
def test_mask_to_latent_equals_the_restatement(s2v, shape):
    F, Hh, W = shape
    g = torch.Generator().manual_seed(F + W)
    sparse = (torch.rand(2, F, Hh, W, generator=g) > 0.995).float() * 0.75
    single = torch.zeros(1, F, Hh, W)
    single[0, -1, -1, -1] = 1.0
    cases = [sparse, torch.rand(2, F, Hh, W, generator=g), sparse.to(torch.bfloat16), torch.rand(2, F, Hh, W, generator=g).to(torch.float16),
             (sparse * 255).to(torch.uint8), sparse > 0, single, sparse.double()]
    edge = torch.tensor([0.0, 0.49, 0.4999, 0.5, 0.51, 1.0, -1.0, 2.0]).repeat(F * Hh * W // 8).reshape(1, F, Hh, W)
    for mask in cases + [edge, edge.to(torch.bfloat16), edge.to(torch.float16)]:
        lat, pix = s2v.mask_to_latent(mask, DEV)
        assert lat.dtype == torch.uint8 and pix.dtype == torch.uint8
        assert torch.equal(pix.cpu(), R.binarise(mask)), f"binarised pixel mask, {mask.dtype}"
        assert torch.equal(lat.cpu(), R.latent_mask(mask)), f"latent mask, {mask.dtype}"
    lat, _ = s2v.mask_to_latent(single, DEV)
    assert int(lat.sum()) == 1 and int(lat[0, -1, -1, -1]) == 1


@pytest.mark.parametrize("keep_dt", [torch.float32, torch.bfloat16], ids=["keep-f32", "keep-bf16"])
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
def test_masked_post_processes_equal_where_over_the_two_unmasked_ones(s2v, dt_name, keep_dt):
    dt = DT[dt_name]
    vae = H._vae(s2v, torch.bfloat16)   # the post-processes are the object's own; its weights are not used
    g = torch.Generator().manual_seed(5)
    dec = (torch.randn(2, 3, VF, PH, PW, generator=g) * 0.8).to(DEV, dt)      # beyond [-1, 1] too: the clamp is part of it
    video = (torch.rand(2, 3, VF, PH, PW, generator=g) * 2 - 1).to(DEV, keep_dt)
    single = torch.zeros(1, VF, PH, PW)
    single[0, -1, -1, -1] = 1.0
    for mask in (_masks(2), single):
        _, pix = s2v.mask_to_latent(mask, DEV)
        sel = pix.bool()[..., None]   # [r,F,H,W,1] over the channels
        a, b = torch.from_numpy(vae.postprocess_video(dec, "np")), torch.from_numpy(vae.postprocess_video(video, "np"))
        got = torch.from_numpy(vae.postprocess_video(dec, "np", keep=video, pixel_mask=pix))
        exp = torch.where(sel.cpu(), a, b)
        assert torch.equal(got, exp)
        assert torch.equal(got[~sel.cpu().expand_as(got)], b[~sel.cpu().expand_as(b)]), "kept pixels are the post-processed input video, exactly"
        pt = vae.postprocess_video(dec, "pt", keep=video, pixel_mask=pix)
        assert torch.equal(pt.cpu(), exp.permute(0, 1, 4, 2, 3))
        for k in range(2):
            r = min(k, pix.shape[0] - 1)
            a8, b8 = vae.frames_uint8(dec[k:k + 1]), vae.frames_uint8(video[k:k + 1])
            got8 = vae.frames_uint8(dec[k:k + 1], keep=video[k:k + 1], pixel_mask=pix[r:r + 1])
            assert got8.dtype == torch.uint8 and torch.equal(got8, torch.where(sel[r], a8, b8))
    assert int(sel.sum()) == 1, "the single-pixel mask repaints one pixel of one frame, in all three channels"
    assert torch.equal(got[0, -1, -1, -1], a[0, -1, -1, -1]) and torch.equal(got8[-1, -1, -1], a8[-1, -1, -1])
    with pytest.raises(ValueError, match="paste-back takes"):
        vae.postprocess_video(dec, "np", keep=video)
    with pytest.raises(ValueError, match=r"`keep` must be \[1, 3, 9, 64, 96\]"):
        vae.frames_uint8(dec[:1], keep=video[:1, :, :5], pixel_mask=pix[:1])


def test_pipeline_paste_back_returns_the_input_videos_own_pixels_outside_the_mask(s2v):
    """b = 3 with a mask per video, frames out: the select of the decoded and the input video, video by video in the caller's order"""
    inp = H._inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    pos, neg, ref = inp["pos"][:3].to(dt), inp["neg"][:3].to(dt), inp["ref"][:3].to(dt)
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, "ddim", dt, vae)
    vids, masks = H._videos(3), _masks(3)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, video=vids, strength=H.STRENGTHS, mask=masks, **_call_kw("fused-graph"))
    lat = pipe(generator=H._gens(range(3)), output_type="latent", **kw)["frames"].clone()
    frames = pipe(generator=H._gens(range(3)), output_type="np", **kw)["frames"]
    assert frames.shape == (3, VF, PH, PW, 3)
    sel = R.binarise(masks).bool()[..., None].numpy()
    for k in range(3):
        dec = vae.postprocess_video(vae.decode_latents(lat[k:k + 1].contiguous()), "np")[0]
        own = vae.postprocess_video(vids[k:k + 1].to(DEV), "np")[0]
        assert (frames[k] == torch.where(torch.from_numpy(sel[k]), torch.from_numpy(dec), torch.from_numpy(own)).numpy()).all(), f"video {k}"
    raw = pipe(generator=H._gens(range(3)), output_type="np", paste_back=False, **kw)["frames"]
    assert (raw[1] == vae.postprocess_video(vae.decode_latents(lat[1:2].contiguous()), "np")[0]).all()
    pipe.transformer.engine.close()
