"""Per-video guidance, strength and step count in a batched call (include/s2v_hip.h: s2v_denoise_step_videos; engine.denoise_step with sequences;
S2VPipeline with lists and with several input videos): video k of a call equals the one-video call made with its own prompt, reference row, input
video, generator, guidance scale, step count and strength -- BITWISE, at sizes where no GEMM splits K (tests/test_gpu_batch_videos.py establishes
that a sample does not depend on how many share the call; here every video also has its own timestep and coefficient set in the same launch).

The one-video steps go through the scalar entry (s2v_denoise_step) on a B = 2 engine: they are the independent side of every comparison, computed
once per (case, dtype, scheduler) and shared by the eager and the graph runs.  The recipes (cases, seeds 81 / 82, the tiny VAE) are those of
tests/test_gpu_batch_videos.py.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
STEPS = 3
NVID = 4
# (step count, strength, guidance) of video k: four different timesteps in every launch (399 799 570 999 | 299 599 428 666 | 199 399 285 332) and,
# under DPM, video 3 on its last step (kind 1) beside three videos on multistep steps (kind 2) in the third
PLANS = [(10, 0.4, 3.0), (5, 0.8, 4.5), (7, 0.6, 6.0), (3, 1.0, 7.5)]


def _five_b(s2v):
    cfg = s2v.cogvideox_5b()
    cfg.num_layers = 2
    return cfg


CASES = {
    # name: (config factory, T, F, H, W).  mid-rope: one video is 16 * 3 * 34 * 46 = 75 072 elements = 293.25 blocks of 256 threads -- a launch
    # that lets a block run across a video boundary steps the head of video k + 1 with video k's coefficients; at tiny-rope (3 072 = 12 blocks) it would not
    "tiny-rope": (lambda s2v: s2v.tiny(use_rope=True, heads=2, layers=2, text_dim=64, temb=64), 5, 2, 8, 12),
    "mid-rope": (lambda s2v: s2v.tiny(use_rope=True, heads=6, layers=2, text_dim=128, temb=64), 7, 3, 34, 46),
    "5b-width": (_five_b, 226, 3, 60, 90),
}
_SD, _IN, _SINGLE = {}, {}, {}


def _weights(s2v, case):
    if case not in _SD:
        cfg = CASES[case][0](s2v)
        big = cfg.num_attention_heads >= 30
        _SD[case] = (cfg, s2v.weights.synthetic_state_dict(cfg, seed=81, parity=True, **({"device": DEV} if big else {})))
    return _SD[case]


def _inputs(s2v, case):
    """distinct latents, [negative | positive] text and references for NVID videos, DPM noise for every step: made once, never written"""
    if case not in _IN:
        cfg, _ = _weights(s2v, case)
        _, T, F, H, W = CASES[case]
        g = torch.Generator(device=DEV).manual_seed(82)
        C = cfg.in_channels
        _IN[case] = dict(neg=torch.randn(NVID, T, cfg.text_embed_dim, generator=g, device=DEV),
                         pos=torch.randn(NVID, T, cfg.text_embed_dim, generator=g, device=DEV),
                         ref=torch.randn(NVID, 1, C, H, W, generator=g, device=DEV) * 0.7,
                         lat=torch.randn(NVID, F, C, H, W, generator=g, device=DEV),
                         noise=torch.randn(STEPS, NVID, F, C, H, W, generator=g, device=DEV))
    return _IN[case]


def _text(inp, vids):
    return torch.cat([inp["neg"][vids], inp["pos"][vids]], dim=0)


def _engine(s2v, case, dt, B):
    cfg, sd = _weights(s2v, case)
    _, T, F, H, W = CASES[case]
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    m.load_state_dict(sd)
    eng = m.engine
    eng.set_geometry(B, T, F, H, W)
    eng.prepare_tables(H * 8, W * 8)
    return m, eng


def _sched(s2v, kind):
    return (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)


def _plan(s2v, kind, dt, k):
    """the first STEPS steps of video k's plan: [(timestep, coefficient set)]"""
    n, strength, g = PLANS[k]
    steps = s2v.S2VPipeline.video_plan(_sched(s2v, kind), n, strength, g, False, dt)["steps"][:STEPS]
    assert len(steps) == STEPS
    return [(float(st["t"]), st["coef"]) for st in steps]


def _steps(eng, plans, dt, lat, noise, graph, dpm, scalar=False):
    """STEPS denoise steps on lat [b,...] (a fresh clone is updated in place), video p on plans[p]; scalar: the one-video entry with plans[0]"""
    x = lat.to(dt).contiguous().clone()
    x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
    nz = torch.empty_like(x) if dpm else None
    out = []
    for i in range(STEPS):
        if dpm:
            nz.copy_(noise[i].to(dt))
        if scalar:
            eng.denoise_step(x, plans[0][i][0], plans[0][i][1], x0, nz, use_graph=graph)
        else:
            eng.denoise_step(x, [p[i][0] for p in plans], [p[i][1] for p in plans], x0, nz, use_graph=graph)
        torch.cuda.synchronize()
        out.append((x.clone(), x0.clone() if dpm else None))
    assert torch.isfinite(x.float()).all()
    return out


def _single(s2v, case, dt_name, kind):
    """video k alone on a B = 2 engine through the scalar entry, eagerly: [video][step] -> (latents [1,...], x0_hist)"""
    key = (case, dt_name, kind)
    if key not in _SINGLE:
        inp = _inputs(s2v, case)
        m, eng = _engine(s2v, case, DT[dt_name], 2)
        res = []
        for k in range(NVID):
            eng.set_conditioning(_text(inp, [k]), inp["ref"][k:k + 1])
            res.append(_steps(eng, [_plan(s2v, kind, DT[dt_name], k)], DT[dt_name], inp["lat"][k:k + 1], inp["noise"][:, k:k + 1], False,
                              kind == "dpm", scalar=True))
        eng.close()
        _SINGLE[key] = res
    return _SINGLE[key]


def _batched_equals_single(s2v, case, dt_name, kind, graph, b):
    inp = _inputs(s2v, case)
    dt = DT[dt_name]
    single = _single(s2v, case, dt_name, kind)
    vids = list(range(b))
    plans = [_plan(s2v, kind, dt, k) for k in vids]
    for i in range(STEPS):
        assert len({p[i][0] for p in plans}) == b and len({p[i][1].guidance for p in plans}) == b, "every video on its own timestep and guidance"
    if kind == "dpm" and b == NVID:
        assert sorted({p[STEPS - 1][1].kind for p in plans}) == [1, 2], "kinds 1 and 2 in the same launch"
    m, eng = _engine(s2v, case, dt, 2 * b)
    eng.set_conditioning(_text(inp, vids), inp["ref"][:b])
    before = eng.lora_state["graph_captures"]
    got = _steps(eng, plans, dt, inp["lat"][:b], inp["noise"][:, :b], graph, kind == "dpm")
    captures = eng.lora_state["graph_captures"] - before
    eng.close()
    assert captures == (1 if graph else 0), f"{captures} captures over {STEPS} steps: one graph serves every step, whatever the values"
    for i, (x, x0) in enumerate(got):
        for k in vids:
            assert torch.equal(x[k:k + 1], single[k][i][0]), f"b = {b}, step {i}: video {k} differs from its one-video steps"
            if x0 is not None:
                assert torch.equal(x0[k:k + 1], single[k][i][1]), f"b = {b}, step {i}: x0 history of video {k} differs"
    assert not torch.equal(got[-1][0][0], got[-1][0][1])


# ------------------------------------------------------------------------------------------------ 1. the engine step
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", ["tiny-rope", "mid-rope"])
def test_four_videos_on_their_own_timesteps_and_coefficients_equal_the_one_video_steps_bitwise(s2v, case, dt_name, kind, graph):
    _batched_equals_single(s2v, case, dt_name, kind, graph, NVID)


# ------------------------------------------------------------------------------------------------ 2. scalar compatibility
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_equal_values_give_the_bytes_of_the_scalar_call(s2v, kind):
    case, dt, b = "mid-rope", torch.bfloat16, NVID
    inp = _inputs(s2v, case)
    plan = _plan(s2v, kind, dt, 1)
    m, eng = _engine(s2v, case, dt, 2 * b)
    eng.set_conditioning(_text(inp, list(range(b))), inp["ref"][:b])
    dpm = kind == "dpm"
    scalar = _steps(eng, [plan], dt, inp["lat"][:b], inp["noise"][:, :b], False, dpm, scalar=True)
    lists = _steps(eng, [plan] * b, dt, inp["lat"][:b], inp["noise"][:, :b], False, dpm)
    # the two library entries themselves, the scalar repeated by the caller
    lib, L = s2v.lib(), s2v._lib
    x = inp["lat"][:b].to(dt).contiguous().clone()
    x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
    nz = inp["noise"][0, :b].to(dt).contiguous() if dpm else None
    t_arr = (ctypes.c_float * b)(*[plan[0][0]] * b)
    c_arr = (L.SchedCoefC * b)(*[plan[0][1]] * b)
    L.check(lib.s2v_denoise_step_videos(eng._h, L.ptr(x), t_arr, c_arr, L.ptr(x0), L.ptr(nz), 0, L.stream_ptr()))
    torch.cuda.synchronize()
    eng.close()
    for i in range(STEPS):
        assert torch.equal(scalar[i][0], lists[i][0])
        if dpm:
            assert torch.equal(scalar[i][1], lists[i][1])
    assert torch.equal(x, scalar[0][0]) and (not dpm or torch.equal(x0, scalar[0][1]))


@pytest.mark.parametrize("B", [2, 1])
def test_one_video_through_the_new_entry_equals_the_scalar_entry(s2v, B):
    """b = 1: a CFG pair (B = 2) and one sample without CFG (B = 1)"""
    case, dt = "tiny-rope", torch.bfloat16
    inp = _inputs(s2v, case)
    plan = _plan(s2v, "dpm", dt, 2)
    m, eng = _engine(s2v, case, dt, B)
    eng.set_conditioning(_text(inp, [2]) if B == 2 else inp["pos"][2:3], inp["ref"][2:3])
    scalar = _steps(eng, [plan], dt, inp["lat"][2:3], inp["noise"][:, 2:3], False, True, scalar=True)
    lists = _steps(eng, [plan], dt, inp["lat"][2:3], inp["noise"][:, 2:3], False, True)
    eng.close()
    for i in range(STEPS):
        assert torch.equal(scalar[i][0], lists[i][0]) and torch.equal(scalar[i][1], lists[i][1])
    if B == 2:
        assert torch.equal(scalar[-1][0], _single(s2v, case, "bf16", "dpm")[2][-1][0])


# ------------------------------------------------------------------------------------------------ 3. an odd count, and the 5B width
def test_three_videos_equal_the_one_video_steps_bitwise(s2v):
    _batched_equals_single(s2v, "mid-rope", "bf16", "dpm", True, 3)


def test_5b_width_four_videos_equal_the_one_video_steps_bitwise(s2v):
    """5626 tokens per sample (the four-wave attention), 45 008 rows at B = 8; one video is 259 200 elements"""
    _batched_equals_single(s2v, "5b-width", "bf16", "ddim", False, 4)
    _SINGLE.pop(("5b-width", "bf16", "ddim"), None)
    _SD.pop("5b-width", None)
    _IN.pop("5b-width", None)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 4. the pipeline, text-to-video
VAE = dict(block_out_channels=(16, 16, 32, 32), layers_per_block=1, norm_num_groups=4, latent_channels=16,
           sample_height=64, sample_width=96, scaling_factor=0.7, temporal_compression_ratio=4)
PH, PW, PF, PT = 64, 96, 5, 5   # pixels and frames of the tiny case: latents 2 x 8 x 12
VF = 9                          # frames of an input video (the encode takes 8k + 1): latents 3 x 8 x 12
GUIDANCE, COUNTS = [3.0, 4.5, 6.0, 7.5], [2, 4, 3, 3]
STRENGTHS = [0.5, 1.0, 0.75]    # at 4 steps: 2, 4 and 3 timesteps


def _vae(s2v, dt):
    vcfg = s2v.VAEConfig(**VAE)
    vae = s2v.HipAutoencoderKLCogVideoX(vcfg, dt, DEV)
    sd = dict(s2v.weights.synthetic_vae_state_dict(vcfg, seed=83))
    sd.update(s2v.weights.synthetic_vae_encoder_state_dict(vcfg, seed=84))
    vae.load_state_dict(sd)
    return vae


def _pipe(s2v, kind, dt, vae=None):
    cfg, sd = _weights(s2v, "tiny-rope")
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    m.load_state_dict(sd)
    return s2v.S2VPipeline(m, _sched(s2v, kind), vae)


def _gens(ks):
    return [torch.Generator().manual_seed(900 + k) for k in ks]


def _mode_kw(mode):
    return dict(fused=mode != "seams", use_graph=mode != "seams")


@pytest.mark.parametrize("mode,kind,dynamic", [("fused-graph", "ddim", False), ("fused-graph", "dpm", False), ("seams", "ddim", False),
                                               ("seams", "dpm", False), ("fused-graph", "dpm", True), ("seams", "ddim", True)])
def test_pipeline_four_videos_on_their_own_guidance_and_step_count_equal_four_single_calls_bitwise(s2v, mode, kind, dynamic):
    inp = _inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    pos, neg, ref = inp["pos"][:2].to(dt), inp["neg"][:2].to(dt), inp["ref"].to(dt)
    kw = dict(height=PH, width=PW, num_frames=PF, use_dynamic_cfg=dynamic, **_mode_kw(mode))
    pipe = _pipe(s2v, kind, dt)
    eng = pipe.transformer.engine
    before = eng.lora_state["graph_captures"]
    out = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, num_videos_per_prompt=2, generator=_gens(range(4)),
               guidance_scale=GUIDANCE, num_inference_steps=COUNTS, **kw)["frames"].clone()
    captures = eng.lora_state["graph_captures"] - before
    assert tuple(out.shape) == (4, 2, 16, PH // 8, PW // 8)
    assert pipe.scheduler.num_inference_steps == max(COUNTS), "the scheduler is left on the longest video's step count"
    if mode == "fused-graph":   # 4 videos for two steps, 3 for the third, 1 for the fourth
        assert 1 <= captures <= 3, f"{captures} captures: at most one per distinct active count"
    for k in range(4):
        one = pipe(prompt_embeds=pos[k // 2:k // 2 + 1], negative_prompt_embeds=neg[k // 2:k // 2 + 1], ref_img_states=ref[k:k + 1],
                   generator=_gens([k])[0], guidance_scale=GUIDANCE[k], num_inference_steps=COUNTS[k], **kw)["frames"]
        assert torch.equal(out[k:k + 1], one), f"video {k} differs from the single call at guidance {GUIDANCE[k]} and {COUNTS[k]} steps"
    eng.close()


def test_pipeline_guidance_sweep_alone_never_reorders_or_shrinks(s2v):
    """equal plan lengths: one geometry and one capture for the whole call, and a DPM call may keep its single generator"""
    inp = _inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    pos, neg, ref = inp["pos"][:1].to(dt), inp["neg"][:1].to(dt), inp["ref"][:1].to(dt)
    kw = dict(height=PH, width=PW, num_frames=PF, num_inference_steps=STEPS, use_graph=True)
    pipe = _pipe(s2v, "ddim", dt)
    eng = pipe.transformer.engine
    lat = inp["lat"][:1].to(dt).expand(4, -1, -1, -1, -1).contiguous()   # the same seed at four guidance scales
    before = eng.lora_state["graph_captures"]
    out = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, num_videos_per_prompt=4, latents=lat,
               guidance_scale=GUIDANCE, **kw)["frames"].clone()
    assert eng.lora_state["graph_captures"] - before == 1 and eng.geometry[0] == 8
    for k in range(4):
        one = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, latents=lat[:1], guidance_scale=GUIDANCE[k], **kw)["frames"]
        assert torch.equal(out[k:k + 1], one), f"guidance {GUIDANCE[k]}"
    assert not torch.equal(out[0], out[1])
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. the pipeline, video-to-video
def _videos(n):
    g = torch.Generator().manual_seed(77)
    return (torch.rand(n, 3, VF, PH, PW, generator=g) * 2 - 1)


@pytest.mark.parametrize("mode", ["fused-graph", "seams"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_video_to_video_three_videos_on_their_own_strength_equal_three_single_calls_bitwise(s2v, kind, mode):
    inp = _inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    pos, neg, ref = inp["pos"][:3].to(dt), inp["neg"][:3].to(dt), inp["ref"][:3].to(dt)
    pipe = _pipe(s2v, kind, dt, _vae(s2v, dt))
    vids = _videos(3)
    kw = dict(height=PH, width=PW, num_inference_steps=4, guidance_scale=6.0, **_mode_kw(mode))
    args = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref)
    own = pipe(video=vids, strength=STRENGTHS, generator=_gens(range(3)), **args, **kw)["frames"].clone()
    shared = pipe(video=vids[1:2], strength=STRENGTHS, generator=_gens(range(3)), **args, **kw)["frames"].clone()
    assert tuple(own.shape) == (3, 3, 16, PH // 8, PW // 8)
    for k in range(3):
        one_kw = dict(prompt_embeds=pos[k:k + 1], negative_prompt_embeds=neg[k:k + 1], ref_img_states=ref[k:k + 1], strength=STRENGTHS[k], **kw)
        one = pipe(video=vids[k:k + 1], generator=_gens([k])[0], **one_kw)["frames"]
        assert torch.equal(own[k:k + 1], one), f"video {k} (its own input video, strength {STRENGTHS[k]}) differs from the single call"
        one = pipe(video=vids[1:2], generator=_gens([k])[0], **one_kw)["frames"]
        assert torch.equal(shared[k:k + 1], one), f"video {k} (the shared input video, strength {STRENGTHS[k]}) differs from the single call"
    assert not torch.equal(own[0], shared[0]) and torch.equal(own[1], shared[1])
    pipe.transformer.engine.close()


def test_pipeline_video_to_video_one_generator_draws_in_the_reference_order(s2v):
    """pipeline_cogvideox_video2video.py:384-388 with one generator: the rows' posterior samples in turn, then ONE noise draw of b.  DDIM (nothing
    is drawn in the loop): the start latents are built here draw by draw and stepped through the scalar entry; DPM: the fused and the seam path,
    which both draw the noise of all videos at once, agree"""
    inp = _inputs(s2v, "tiny-rope")
    dt, b = torch.bfloat16, 3
    pos, neg, ref = inp["pos"][:b].to(dt), inp["neg"][:b].to(dt), inp["ref"][:b].to(dt)
    vae = _vae(s2v, dt)
    vids = _videos(b)
    pipe = _pipe(s2v, "ddim", dt, vae)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, height=PH, width=PW, num_inference_steps=4, guidance_scale=6.0,
              video=vids, strength=0.75)
    got = pipe(generator=torch.Generator().manual_seed(31), **kw)["frames"].clone()
    g = torch.Generator().manual_seed(31)
    z0 = torch.cat([vae.encode(vids[r:r + 1]).latent_dist.sample(g) for r in range(b)], dim=0)
    z0 = vae.config.scaling_factor * z0.to(dt).permute(0, 2, 1, 3, 4).contiguous()
    noise = torch.randn(z0.shape, generator=g, dtype=dt).to(DEV)
    sch = _sched(s2v, "ddim")
    sch.set_timesteps(4)
    ts = sch.timesteps[1:]
    x = torch.cat([sch.add_noise(z0[r:r + 1], noise[r:r + 1], ts[:1]) for r in range(b)], dim=0).contiguous()
    eng = pipe.transformer.engine
    eng.set_geometry(2 * b, PT, x.shape[1], PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning(torch.cat([neg, pos]), ref)
    for t in ts:
        eng.denoise_step(x, float(t), sch.coef(t, dt, 6.0))
    torch.cuda.synchronize()
    assert torch.equal(got, x)
    eng.close()
    dpm = _pipe(s2v, "dpm", dt, vae)
    fused = dpm(generator=torch.Generator().manual_seed(32), use_graph=True, **kw)["frames"].clone()
    seams = dpm(generator=torch.Generator().manual_seed(32), fused=False, **kw)["frames"]
    assert torch.equal(fused, seams)
    dpm.transformer.engine.close()


# ------------------------------------------------------------------------------------------------ 6. the callback
def test_callback_sees_the_callers_order_and_an_edit_of_one_video_leaves_the_others_alone(s2v):
    inp = _inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    pos, neg, ref = inp["pos"][:2].to(dt), inp["neg"][:2].to(dt), inp["ref"].to(dt)
    pipe = _pipe(s2v, "ddim", dt)
    kw = dict(height=PH, width=PW, num_frames=PF, use_graph=True)
    args = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, num_videos_per_prompt=2, guidance_scale=GUIDANCE,
                num_inference_steps=COUNTS)
    seen = {}

    def look(p, i, t, tensors):
        seen[i] = (t.clone(), tensors["latents"].clone(), tuple(tensors["prompt_embeds"].shape))
        return {}

    base = pipe(generator=_gens(range(4)), callback_on_step_end=look, callback_on_step_end_tensor_inputs=("latents", "prompt_embeds"),
                **args, **kw)["frames"].clone()
    assert sorted(seen) == [0, 1, 2, 3] and all(tuple(s[1].shape) == tuple(base.shape) and s[2] == (8, PT, 64) for s in seen.values())
    sch = _sched(s2v, "ddim")
    ts = [sch.timesteps_for(n) for n in COUNTS]
    assert seen[0][0].ndim == 0 and int(seen[0][0]) == 999, "every plan starts at 999: the 0-dim timestep of a scalar call"
    for i in (1, 2):   # the plans differ: [b] timesteps in the caller's order, a finished video keeps its last one
        assert seen[i][0].tolist() == [int(ts[k][min(i, COUNTS[k] - 1)]) for k in range(4)]
    assert seen[3][0].ndim == 0 and int(seen[3][0]) == int(ts[1][3]), "only video 1 is left"
    firsts = {}
    for k in range(4):   # the latents the callback saw after the first step are the single calls', video by video
        def one_look(p, i, t, tensors, k=k):
            if i == 0:
                firsts[k] = tensors["latents"].clone()
            return {}

        pipe(prompt_embeds=pos[k // 2:k // 2 + 1], negative_prompt_embeds=neg[k // 2:k // 2 + 1], ref_img_states=ref[k:k + 1],
             generator=_gens([k])[0], guidance_scale=GUIDANCE[k], num_inference_steps=COUNTS[k], callback_on_step_end=one_look, **kw)
        assert torch.equal(seen[0][1][k:k + 1], firsts[k]), f"the callback's row {k} is not the caller's video {k}"
    assert torch.equal(seen[3][1], base), "finished videos keep their latents"

    def edit(p, i, t, tensors):
        if i != 0:
            return {}
        x = tensors["latents"].clone()
        x[2] += 0.5
        return {"latents": x}

    got = pipe(generator=_gens(range(4)), callback_on_step_end=edit, **args, **kw)["frames"]
    for k in (0, 1, 3):
        assert torch.equal(got[k], base[k]), f"the edit of video 2 changed video {k}"
    assert not torch.equal(got[2], base[2])
    pipe.transformer.engine.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_the_limit_and_the_engine_still_runs_a_scalar_one_video_call(s2v):
    case = "tiny-rope"
    _, T, F, H, W = CASES[case]
    inp = _inputs(s2v, case)
    dt = torch.bfloat16
    m, eng = _engine(s2v, case, dt, 2 * NVID)
    eng.set_conditioning(_text(inp, list(range(NVID))), inp["ref"])
    plans = [_plan(s2v, "dpm", dt, k) for k in range(NVID)]
    x = inp["lat"].to(dt).contiguous().clone()
    keep = x.clone()
    with pytest.raises(s2v.S2VError, match=r"`timestep` has 3 entries for b = 4 videos"):
        eng.denoise_step(x, [p[0][0] for p in plans[:3]], [p[0][1] for p in plans])
    with pytest.raises(s2v.S2VError, match=r"`coef` has 2 entries for b = 4 videos"):
        eng.denoise_step(x, [p[0][0] for p in plans], [p[0][1] for p in plans[:2]])
    with pytest.raises(s2v.S2VError, match="DPM needs noise and x0_hist"):   # one DPM kind among the sets is enough
        eng.denoise_step(x, [p[0][0] for p in plans], [p[0][1] for p in plans])
    lib, L = s2v.lib(), s2v._lib
    assert lib.s2v_denoise_step_videos(eng._h, L.ptr(x), None, None, None, None, 0, L.stream_ptr()) != 0
    assert b"s2v_denoise_step_videos: null argument" in lib.s2v_last_error()
    # a shard context is refused with the wording of s2v_denoise_step
    ms, sh = _engine(s2v, case, dt, 2)
    sh.set_shard(2, 0)
    sh.set_geometry(2, T, F, H, W)
    sh.prepare_tables(H * 8, W * 8)
    sh.set_conditioning(_text(inp, [0]), inp["ref"][:1])
    ddim = _plan(s2v, "ddim", dt, 0)
    msgs = []
    for ts, cs in (([ddim[0][0]], [ddim[0][1]]), (ddim[0][0], ddim[0][1])):   # the new entry, then the scalar one
        with pytest.raises(s2v.S2VError, match=r"a shard context \(s2v_set_shard\) runs the staged step") as e:
            sh.denoise_step(x[:1].clone(), ts, cs)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    sh.close()
    torch.cuda.synchronize()
    assert torch.equal(x, keep), "a refused step touches nothing"
    pipe = s2v.S2VPipeline(m, _sched(s2v, "dpm"))
    pos, neg, ref = inp["pos"][:2].to(dt), inp["neg"][:2].to(dt), inp["ref"].to(dt)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, num_videos_per_prompt=2, height=PH, width=PW, num_frames=PF)
    with pytest.raises(ValueError, match=r"`guidance_scale` is a list of 2 entries for b = 4 videos"):
        pipe(guidance_scale=[3.0, 4.0], **kw)
    with pytest.raises(ValueError, match=r"guidance_scale\[0\] = 0.5: every guidance scale must be > 1"):
        pipe(guidance_scale=[0.5, 4.0, 5.0, 6.0], **kw)
    with pytest.raises(ValueError, match=r"`strength` as a list applies only together with `video`"):
        pipe(strength=[0.5, 0.6, 0.7, 0.8], **kw)
    with pytest.raises(ValueError, match=r"under the DPM scheduler with a single generator.*list of 4 generators"):
        pipe(num_inference_steps=COUNTS, generator=torch.Generator().manual_seed(5), **kw)
    with pytest.raises(ValueError, match=r"`video` must be \[v, 3, F, H, W\] with v = 1 .* or v = b = 4"):
        pipe(video=torch.zeros(2, 3, VF, PH, PW), **kw)
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=rf"as a list together with `{name}`"):
            pipe(**dict(kw, prompt_embeds=pos[:1], negative_prompt_embeds=neg[:1], ref_img_states=ref[:1], num_videos_per_prompt=1),
                 guidance_scale=[6.0], **{name: object()})
    assert eng.geometry == (2 * NVID, T, F, H, W), "no refusal reached the engine"
    # ... and the engine still runs a scalar one-video step, with the bits of an engine that was never refused anything
    eng.set_geometry(2, T, F, H, W)
    eng.prepare_tables(H * 8, W * 8)
    eng.set_conditioning(_text(inp, [0]), inp["ref"][:1])
    got = _steps(eng, [plans[0]], dt, inp["lat"][:1], inp["noise"][:, :1], False, True, scalar=True)
    exp = _single(s2v, case, "bf16", "dpm")
    assert torch.equal(got[-1][0], exp[0][-1][0]) and torch.equal(got[-1][1], exp[0][-1][1])
    eng.close()
