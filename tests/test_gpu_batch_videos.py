"""Several videos per call (include/s2v_hip.h: S2V_MAX_BATCH, s2v_set_conditioning_refs, s2v_denoise_step on [b] latents; engine, transformer seam,
S2VPipeline): b <= 4 videos run as ONE step on the batch [negative x b | positive x b] (custom_cogvideox_pipe.py:196,246-248), sample j taking
video j mod b and reference j mod n_ref (cogvideox_transformer_3d.py:503-504).

Per sample nothing may depend on how many videos share the call: at sizes where no GEMM of either engine splits K (K < 2048, or the geometry has no
split-K workspace) every claim is BITWISE -- the batched step against b one-video engines, DDIM and DPM, eager and hipGraph, three dtypes, the runtime
LoRA and fp8 engines, the pipeline with one generator per video.  At configs[0]'s geometry (2B width) the one-video engine splits K and the two-video
engine does not: fp32 stays bitwise (gemm_f32m sums in k order), bf16 is held to 2 x the one-video engine's own error against the fp32 run.

The one-video results are computed once per (case, dtype, scheduler) and shared by the eager and the graph comparison.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import transformer_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
F32_BAR = 4e-5   # tests/test_gpu_parity.py: max-abs of the fp32 path against the CPU oracle
STEPS = 3
NVID = 4


def _five_b(s2v):
    cfg = s2v.cogvideox_5b()
    cfg.num_layers = 2
    return cfg


def _lora_cfg(s2v, fmt=None, rank=0):
    cfg = s2v.tiny(use_rope=True, heads=4, layers=2, text_dim=128, temb=64)   # D = 256: the fp8 formats need D % 128 == 0
    cfg.max_text_seq_length = 7
    cfg.weight_format = fmt
    cfg.lora_runtime_rank = rank
    return cfg


CASES = {
    # name: (config factory, T, F, H, W).  tiny / mid: tests/test_gpu_cfg_parallel.py (mid: 1571 tokens per sample, ragged against every tile at
    # B = 4 and B = 8); 5b-width: 5626 tokens per sample, over the 4608-token switch to the four-wave attention, B = 8 is 45 008 rows
    "tiny-rope": (lambda s2v: s2v.tiny(use_rope=True, heads=2, layers=2, text_dim=64, temb=64), 5, 2, 8, 12),
    "tiny-sincos": (lambda s2v: s2v.tiny(use_rope=False, heads=2, layers=2, text_dim=64, temb=64), 5, 2, 8, 12),
    "mid-rope": (lambda s2v: s2v.tiny(use_rope=True, heads=6, layers=2, text_dim=128, temb=64), 7, 3, 34, 46),
    "5b-width": (_five_b, 226, 3, 60, 90),
    "d256": (_lora_cfg, 7, 3, 16, 24),
    "2b-c1": (None, 226, 3, 32, 32),   # configs[0]: 9 x 256 x 256 at 2B width, two layers (test 7)
}
_SD, _IN, _SINGLE = {}, {}, {}


def _weights(s2v, case):
    if case not in _SD:
        if case == "2b-c1":
            cfg = s2v.cogvideox_2b()
            cfg.num_layers = 2
        else:
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


def _engine(s2v, case, dt, B, cfg=None, lora=None):
    cfg0, sd = _weights(s2v, case)
    _, T, F, H, W = CASES[case]
    m = s2v.HipCogVideoXTransformer3DModel(cfg or cfg0, dt, DEV)
    m.load_state_dict(sd, lora=lora, lora_scale=0.5)
    eng = m.engine
    eng.set_geometry(B, T, F, H, W)
    eng.prepare_tables(H * 8, W * 8)
    return m, eng


def _sched(s2v, kind):
    sch = (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)
    sch.set_timesteps(STEPS)
    return sch


def _steps(s2v, eng, kind, dt, lat, noise, graph, after=None):
    """STEPS denoise steps on lat [b,...] (a fresh clone is updated in place); noise [STEPS, b, ...]; returns [(latents, x0_hist)] after every step"""
    sch = _sched(s2v, kind)
    ts = sch.timesteps
    dpm = kind == "dpm"
    x = lat.to(dt).contiguous().clone()
    x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
    nz = torch.empty_like(x) if dpm else None
    out = []
    for i, t in enumerate(ts):
        if dpm:
            nz.copy_(noise[i].to(dt))
            coef = sch.coef(t, ts[i - 1] if i > 0 else None, i == 0, dt, 6.0)
        else:
            coef = sch.coef(t, dt, 6.0)
        eng.denoise_step(x, float(t), coef, x0, nz, use_graph=graph)
        torch.cuda.synchronize()
        out.append((x.clone(), x0.clone() if dpm else None))
    assert torch.isfinite(x.float()).all()
    return out


def _single(s2v, case, dt_name, kind, cfg=None, lora=None, key=None, nvid=NVID):
    """video k alone on a B = 2 engine (re-conditioned per video), eagerly: [video][step] -> (latents [1,...], x0_hist)"""
    key = key or (case, dt_name, kind)
    if key not in _SINGLE:
        inp = _inputs(s2v, case)
        m, eng = _engine(s2v, case, DT[dt_name], 2, cfg, lora)
        res = []
        for k in range(nvid):
            eng.set_conditioning(_text(inp, [k]), inp["ref"][k:k + 1])
            res.append(_steps(s2v, eng, kind, DT[dt_name], inp["lat"][k:k + 1], inp["noise"][:, k:k + 1], False))
        eng.close()
        _SINGLE[key] = res
    return _SINGLE[key]


def _batched_equals_single(s2v, case, dt_name, kind, graph, b, cfg=None, lora=None, key=None, nvid=NVID):
    inp = _inputs(s2v, case)
    single = _single(s2v, case, dt_name, kind, cfg, lora, key, nvid)
    vids = list(range(b))
    m, eng = _engine(s2v, case, DT[dt_name], 2 * b, cfg, lora)
    eng.set_conditioning(_text(inp, vids), inp["ref"][:b])
    got = _steps(s2v, eng, kind, DT[dt_name], inp["lat"][:b], inp["noise"][:, :b], graph)
    eng.close()
    for i, (x, x0) in enumerate(got):
        for k in vids:
            assert torch.equal(x[k:k + 1], single[k][i][0]), f"b = {b}, step {i}: video {k} differs from its one-video run"
            if x0 is not None:
                assert torch.equal(x0[k:k + 1], single[k][i][1]), f"b = {b}, step {i}: x0 history of video {k} differs"
    assert not torch.equal(got[-1][0][0], got[-1][0][1]), "two videos of the batch must differ"
    assert not torch.equal(got[-1][0], inp["lat"][:b].to(DT[dt_name]))


# ------------------------------------------------------------------------------------------------ 1. batched equals separate, bitwise
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", ["tiny-rope", "tiny-sincos", "mid-rope"])
def test_batched_step_equals_the_one_video_steps_bitwise(s2v, case, dt_name, kind, graph):
    for b in (2, 4):
        _batched_equals_single(s2v, case, dt_name, kind, graph, b)


def test_three_videos_equal_the_one_video_steps_bitwise(s2v):
    _batched_equals_single(s2v, "mid-rope", "bf16", "dpm", True, 3)


def test_5b_width_four_videos_equal_the_one_video_steps_bitwise(s2v):
    """5626 tokens per sample (the four-wave attention), 45 008 rows at B = 8 against 11 252 at B = 2"""
    _batched_equals_single(s2v, "5b-width", "bf16", "ddim", False, 4)
    _SINGLE.pop(("5b-width", "bf16", "ddim"), None)
    _SD.pop("5b-width", None)
    _IN.pop("5b-width", None)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 2. the reference mapping is the reference's
def test_reference_mapping_is_j_mod_b_as_in_the_reference(s2v):
    case, b = "tiny-rope", 2
    cfg, sd = _weights(s2v, case)
    _, T, F, H, W = CASES[case]
    inp = {k: v.cpu() for k, v in _inputs(s2v, case).items()}
    text = torch.cat([inp["neg"][:b], inp["pos"][:b]])
    lat, ref = inp["lat"][:b], inp["ref"][:b]
    ts = torch.tensor([500.0] * (2 * b))
    ref_rope, rope = tr.pipeline_rope(H * 8, W * 8, F)
    ocfg = dict(num_heads=2, num_layers=2, use_rope=True, norm_eps=1e-5)
    with torch.no_grad():   # B rows of references: the oracle takes them as given, which is what :503-504 builds from b rows
        exp = tr.transformer_forward(sd, ocfg, torch.cat([lat, lat]), text, torch.cat([ref, ref]), ts.long(), rope, ref_rope)
    m, eng = _engine(s2v, case, torch.float32, 2 * b)
    eng.set_conditioning(text, ref)
    y = eng.forward(lat, ts, shared_latent=True).clone()
    torch.cuda.synchronize()
    err = (y.cpu() - exp).abs().max().item()
    print(f"MEASURED f32 batched forward vs oracle: max-abs {err:.3e}")
    assert err <= F32_BAR, err
    eng.set_conditioning(text, ref.flip(0))
    y2 = eng.forward(lat, ts, shared_latent=True)
    torch.cuda.synchronize()
    assert not torch.equal(y2[0], y[0]) and not torch.equal(y2[b], y[b]), "swapping the references must change video 0 (both of its samples)"
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. the n_ref forms
def test_one_shared_reference_equals_identical_rows_and_the_eval_false_seam(s2v):
    case, b = "tiny-rope", 2
    _, T, F, H, W = CASES[case]
    inp = _inputs(s2v, case)
    dt = torch.bfloat16
    text = _text(inp, [0, 1])
    lat = inp["lat"][:b].to(dt)
    ts = torch.tensor([400.0] * (2 * b))
    m, eng = _engine(s2v, case, dt, 2 * b)
    ys = []
    for rows in (1, b, 2 * b):
        eng.set_conditioning(text, inp["ref"][:1].expand(rows, -1, -1, -1, -1))
        ys.append(eng.forward(lat, ts, shared_latent=True).clone())
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2]), "one shared reference row must equal b (and B) identical rows"
    # the seam: eval=True duplicates b rows over the 2b samples; eval=False takes one row per sample
    ref_rope, rope = tr.pipeline_rope(H * 8, W * 8, F)
    kw = dict(image_rotary_emb=tuple(x.to(DEV) for x in rope), ref_image_rotary_emb=tuple(x.to(DEV) for x in ref_rope))
    x = torch.cat([lat, lat])
    ref = inp["ref"][:b].to(dt)
    y_true = m(hidden_states=x, encoder_hidden_states=text.to(dt), ref_img_states=ref, timestep=ts.to(DEV), return_dict=False, eval=True, **kw)[0].clone()
    y_false = m(hidden_states=x, encoder_hidden_states=text.to(dt), ref_img_states=torch.cat([ref, ref]), timestep=ts.to(DEV), return_dict=False,
                eval=False, **kw)[0].clone()
    torch.cuda.synchronize()
    assert torch.equal(y_true, y_false)
    eng.set_conditioning(text, ref)
    assert torch.equal(y_true, eng.forward(lat, ts, shared_latent=True))
    with pytest.raises(RuntimeError, match="eval=True duplicates"):   # the reference's own failure at its concat stays
        m(hidden_states=x, encoder_hidden_states=text.to(dt), ref_img_states=inp["ref"][:3].to(dt), timestep=ts.to(DEV), eval=True, **kw)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. the pipeline
VAE = dict(block_out_channels=(16, 16, 32, 32), layers_per_block=1, norm_num_groups=4, latent_channels=16,
           sample_height=64, sample_width=96, scaling_factor=0.7, temporal_compression_ratio=4)
PH, PW, PF, PT = 64, 96, 5, 5   # pixels and frames of the tiny case: latents 2 x 8 x 12


def _pipe(s2v, kind, dt, vae=None):
    cfg, sd = _weights(s2v, "tiny-rope")
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    m.load_state_dict(sd)
    sch = (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)
    return s2v.S2VPipeline(m, sch, vae)


def _pipe_inputs(s2v):
    inp = _inputs(s2v, "tiny-rope")
    return inp["pos"][:2].to(torch.bfloat16), inp["neg"][:2].to(torch.bfloat16), inp["ref"].to(torch.bfloat16)


def _gens(ks):
    return [torch.Generator().manual_seed(900 + k) for k in ks]


@pytest.mark.parametrize("mode", ["fused-graph", "seams"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_two_prompts_two_videos_each_equal_four_single_calls_bitwise(s2v, kind, mode):
    pos, neg, ref = _pipe_inputs(s2v)
    kw = dict(height=PH, width=PW, num_frames=PF, num_inference_steps=STEPS, guidance_scale=6.0, fused=mode != "seams", use_graph=mode != "seams")
    pipe = _pipe(s2v, kind, torch.bfloat16)
    seen = {}

    def cb(p, i, t, tensors):
        seen[i] = (tuple(tensors["latents"].shape), tuple(tensors["prompt_embeds"].shape))
        return {}

    out = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, num_videos_per_prompt=2, generator=_gens(range(4)),
               callback_on_step_end=cb, callback_on_step_end_tensor_inputs=("latents", "prompt_embeds"), **kw)["frames"].clone()
    assert tuple(out.shape) == (4, 2, 16, PH // 8, PW // 8)
    assert seen[STEPS - 1] == (tuple(out.shape), (8, PT, 64)), "the callback sees [b] latents and the [2b] text"
    for k in range(4):
        one = pipe(prompt_embeds=pos[k // 2:k // 2 + 1], negative_prompt_embeds=neg[k // 2:k // 2 + 1], ref_img_states=ref[k:k + 1],
                   generator=_gens([k])[0], **kw)["frames"]
        assert torch.equal(out[k:k + 1], one), f"video {k} differs from the single call with prompt {k // 2} and generator {k}"
    assert not torch.equal(out[0], out[1]) and not torch.equal(out[1], out[2])
    pipe.transformer.engine.close()


_LOOP = {}


def _two_videos_one_stream_written_out(s2v):
    """what a call with scalars, two videos, the DPM scheduler and ONE generator does, written out: prepare_latents once for both videos, then
    per step the coefficients, as many draws of the whole [2,...] noise as the step's kind says (the last one counts) and one scalar step"""
    if not _LOOP:
        pos, neg, ref = _pipe_inputs(s2v)
        dt = torch.bfloat16
        pipe = _pipe(s2v, "dpm", dt)
        sch, eng = pipe.scheduler, pipe.transformer.engine
        g = torch.Generator().manual_seed(977)
        lat = pipe.prepare_latents(PF, PH, PW, dt, DEV, g, None, 2).to(dt).contiguous()
        sch.set_timesteps(4)
        eng.set_geometry(4, PT, lat.shape[1], PH // 8, PW // 8)
        eng.prepare_tables(PH, PW)
        eng.set_conditioning(torch.cat([neg, pos]), ref[:2])
        x0, kinds = torch.zeros(lat.shape, dtype=torch.float32, device=DEV), []
        for i, t in enumerate(sch.timesteps):
            coef = sch.coef(t, sch.timesteps[i - 1] if i > 0 else None, i == 0, dt, 6.0)
            kinds.append(coef.kind)
            for _ in range(2 if coef.kind == 2 else 1):
                noise = s2v.pipeline.randn_videos(lat.shape, g, DEV, dt).contiguous()
            eng.denoise_step(lat, float(t), coef, x0, noise, use_graph=False)
        torch.cuda.synchronize()
        assert kinds == [1, 2, 2, 1], "the two multistep steps draw twice and discard the first draw"
        eng.close()
        _LOOP["latents"] = lat.clone()
    return _LOOP["latents"]


@pytest.mark.parametrize("mode", ["fused-graph", "seams"])
def test_pipeline_two_videos_with_scalars_and_one_dpm_stream_equal_the_written_out_loop_bitwise(s2v, mode):
    pos, neg, ref = _pipe_inputs(s2v)
    exp = _two_videos_one_stream_written_out(s2v)
    pipe = _pipe(s2v, "dpm", torch.bfloat16)
    out = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref[:2], generator=torch.Generator().manual_seed(977), height=PH,
               width=PW, num_frames=PF, num_inference_steps=4, guidance_scale=6.0, fused=mode != "seams", use_graph=mode != "seams")["frames"]
    assert pipe.guidance_scale == 6.0 and isinstance(pipe.guidance_scale, float)
    assert tuple(out.shape) == (2, 2, 16, PH // 8, PW // 8) and torch.equal(out, exp)
    assert not torch.equal(out[0], out[1])
    pipe.transformer.engine.close()


def test_pipeline_callback_on_one_video_leaves_the_others_alone_and_frames_are_decoded_per_video(s2v):
    pos, neg, ref = _pipe_inputs(s2v)
    dt = torch.bfloat16
    vcfg = s2v.VAEConfig(**VAE)
    vae = s2v.HipAutoencoderKLCogVideoX(vcfg, dt, DEV)
    vae.load_state_dict(dict(s2v.weights.synthetic_vae_state_dict(vcfg, seed=83)))
    pipe = _pipe(s2v, "ddim", dt, vae)
    kw = dict(height=PH, width=PW, num_frames=PF, num_inference_steps=STEPS, guidance_scale=6.0, use_graph=True)
    args = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, num_videos_per_prompt=2)
    base = pipe(generator=_gens(range(4)), **args, **kw)["frames"].clone()

    def edit(p, i, t, tensors):
        if i != 0:
            return {}
        x = tensors["latents"].clone()
        x[1] += 0.5
        return {"latents": x}

    got = pipe(generator=_gens(range(4)), callback_on_step_end=edit, **args, **kw)["frames"]
    for k in (0, 2, 3):
        assert torch.equal(got[k], base[k]), f"the edit of video 1 changed video {k}"
    assert not torch.equal(got[1], base[1])
    # frames: b videos, each the decode of the single call
    frames = pipe(generator=_gens(range(4)), output_type="np", **args, **kw)["frames"]
    assert frames.shape[0] == 4 and frames.shape[2:] == (PH, PW, 3)
    for k in (0, 3):
        one = pipe(prompt_embeds=pos[k // 2:k // 2 + 1], negative_prompt_embeds=neg[k // 2:k // 2 + 1], ref_img_states=ref[k:k + 1],
                   generator=_gens([k])[0], output_type="np", **kw)["frames"]
        assert np.array_equal(frames[k], one[0]), f"frames of video {k} differ from the single call's decode"
    pipe.transformer.engine.close()


# ------------------------------------------------------------------------------------------------ 5. the other engines
@pytest.mark.parametrize("engine", ["lora-runtime", "fp8", "fp8-qk"])
def test_other_engines_batched_step_equals_the_one_video_steps_bitwise(s2v, engine):
    """per-row activation quantisation, MX block scales and the adapter's down-projection are per sample"""
    lora = None
    if engine == "lora-runtime":
        cfg = _lora_cfg(s2v, None, 8)
        lora = s2v.weights.synthetic_lora(cfg, rank=8, seed=84, std=0.05)
    else:
        cfg = _lora_cfg(s2v, engine)
    _batched_equals_single(s2v, "d256", "bf16", "ddim", False, 2, cfg=cfg, lora=lora, key=("d256", engine), nvid=2)
    if lora is not None:   # re-conditioning after a rescale (engine._cond_args) keeps the per-video references
        inp = _inputs(s2v, "d256")
        m, eng = _engine(s2v, "d256", torch.bfloat16, 4, cfg, lora)
        eng.set_conditioning(_text(inp, [0, 1]), inp["ref"][:2])
        ts = torch.tensor([300.0] * 4)
        y = eng.forward(inp["lat"][:2], ts, shared_latent=True).clone()
        eng.set_lora_scale(0.25)
        y2 = eng.forward(inp["lat"][:2], ts, shared_latent=True).clone()
        eng.set_lora_scale(0.5)
        y3 = eng.forward(inp["lat"][:2], ts, shared_latent=True)
        torch.cuda.synchronize()
        assert torch.equal(y, y3) and not torch.equal(y, y2)
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_limit_and_the_engine_still_runs_one_video(s2v):
    case = "tiny-rope"
    _, T, F, H, W = CASES[case]
    inp = _inputs(s2v, case)
    dt = torch.bfloat16
    m, eng = _engine(s2v, case, dt, 4)
    with pytest.raises(s2v.S2VError, match="S2V_MAX_BATCH"):
        eng.set_geometry(10, T, F, H, W)
    assert eng.geometry == (4, T, F, H, W)
    with pytest.raises(s2v.S2VError, match="n_ref"):
        eng.set_conditioning(_text(inp, [0, 1]), inp["ref"][:3])
    lib = s2v.lib()
    t4, r3 = _text(inp, [0, 1]).to(dt).contiguous(), inp["ref"][:3].to(dt).contiguous()
    assert lib.s2v_set_conditioning_refs(eng._h, ctypes.c_void_p(t4.data_ptr()), ctypes.c_void_p(r3.data_ptr()), 3, None) < 0
    assert b"n_ref" in lib.s2v_last_error()
    # the one-video-per-call paths say that a batched call runs on one GPU
    sch = _sched(s2v, "ddim")
    coef = sch.coef(sch.timesteps[0], dt, 6.0)
    x = inp["lat"][:2].to(dt).contiguous()
    with pytest.raises(s2v.S2VError, match="batched call"):
        eng.denoise_split_begin(x, 999.0, coef, 0)
    with pytest.raises(s2v.S2VError, match="batched call"):
        eng.denoise_split_end(x)
    # a Ulysses shard with the samples of two videos: s2v_shard_step_begin, the first thing s2v_denoise_step_ulysses runs, refuses it by name
    ms, sh = _engine(s2v, case, dt, 2)
    sh.set_shard(2, 0)
    sh.set_geometry(4, T, F, H, W)
    sh.prepare_tables(H * 8, W * 8)
    sh.set_conditioning(_text(inp, [0, 1]), inp["ref"][:1])
    with pytest.raises(s2v.S2VError, match="batched call"):
        sh.shard_step_begin(x, 999.0, coef)
    sh.close()
    pos, neg, ref = _pipe_inputs(s2v)
    pipe = s2v.S2VPipeline(m, s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0))
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, height=PH, width=PW, num_frames=PF, num_inference_steps=STEPS)
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match="one video per call"):
            pipe(ref_img_states=ref[:2], **{name: object()}, **kw)
    with pytest.raises(ValueError, match="one video per call"):
        pipe(ref_img_states=ref[:2], video=torch.zeros(1, 3, PF, PH, PW), **kw)
    with pytest.raises(ValueError, match="one row per video"):
        pipe(ref_img_states=ref[:3], num_videos_per_prompt=2, **kw)
    with pytest.raises(ValueError, match="at most 4 videos"):
        pipe(ref_img_states=ref[:1], num_videos_per_prompt=3, **kw)
    # ... and the engine still runs a one-video step, with the bits of an engine that was never refused anything
    eng.set_geometry(2, T, F, H, W)
    eng.prepare_tables(H * 8, W * 8)
    eng.set_conditioning(_text(inp, [0]), inp["ref"][:1])
    got = _steps(s2v, eng, "ddim", dt, inp["lat"][:1], None, False)
    exp = _single(s2v, case, "bf16", "ddim")
    assert torch.equal(got[-1][0], exp[0][-1][0])
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. a size where split K makes bits differ
def _rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm()).item()


def test_configs0_geometry_where_one_video_splits_k_and_two_do_not(s2v):
    """2B width, two layers, 9 x 256 x 256 (1250 tokens per sample): M = 2500 rows split K on the out-projection / FF2, M = 5000 do not.
    fp32: bitwise (gemm_f32m is a k-ordered chain whatever the plan).  bf16, after three steps, rel-L2 against the fp32 run of the same video:
    batched <= 2 x the one-video engine's, measured here (the project's 2 x measured convention; the yardstick is the existing engine)."""
    case, b = "2b-c1", 2
    _batched_equals_single(s2v, case, "f32", "ddim", False, b, nvid=b)
    f32 = _single(s2v, case, "f32", "ddim", nvid=b)
    one = _single(s2v, case, "bf16", "ddim", nvid=b)
    inp = _inputs(s2v, case)
    m, eng = _engine(s2v, case, torch.bfloat16, 2 * b)
    eng.set_conditioning(_text(inp, [0, 1]), inp["ref"][:b])
    got = _steps(s2v, eng, "ddim", torch.bfloat16, inp["lat"][:b], None, False)
    eng.close()
    errs = []
    for k in range(b):
        e_b, e_1 = _rel_l2(got[-1][0][k], f32[k][-1][0][0]), _rel_l2(one[k][-1][0][0], f32[k][-1][0][0])
        print(f"MEASURED configs[0] bf16 video {k} after {STEPS} steps, rel-L2 vs fp32: batched {e_b:.3e}, one-video {e_1:.3e}")
        errs.append((e_b, e_1))
    for e_b, e_1 in errs:
        assert e_b <= 2 * e_1, errs
    for key in [k for k in _SINGLE if k[0] == case]:
        _SINGLE.pop(key)
    _SD.pop(case, None)
    _IN.pop(case, None)
    torch.cuda.empty_cache()
