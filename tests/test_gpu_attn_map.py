"""Attention map on the GPU at engine and pipeline level (include/s2v_hip.h: s2v_attn_map_*; engine.attn_map_* and attn_layers=;
S2VPipeline with attention_map=).  Engines, weights and inputs are those of tests/test_gpu_step_cache.py, imported: "mid-rope" (6 heads,
T / R / V = 7 / 391 / 1173: ten query tiles, the last ragged, and 25 key tiles, the last ragged) and "sincos" (no RoPE, 3 heads, V = 30).

Bars of the per-head sums of ONE armed layer against the fp32 CPU oracle's recorded q and k (tests/attn_map_ref.py), 2 x the largest
absolute error measured on an MI355X over both cases, both layers and three ranges:
    engine dtype   measured      bar
    f32            2.464e-07     4.928e-07     (mid-rope 1.779e-07, sincos 2.464e-07)
    bf16           3.807e-03     7.614e-03     (mid-rope 1.055e-03, sincos 3.807e-03)
    f16            6.036e-04     1.207e-03     (mid-rope 1.339e-04, sincos 6.036e-04)
The fp32 engine's figure is the kernel's own (tests/test_gpu_attn_mass.py); the 16-bit engines' is the error of their q and k, i.e. of the
block stack in that dtype up to the armed layer, against an fp32 oracle.
"""
import ctypes

import pytest
import torch

import attn_map_ref as R
import test_gpu_batch_hetero as H
import test_gpu_step_cache as S

pytestmark = pytest.mark.gpu
DEV = S.DEV
MEASURED = {"f32": 2.464e-07, "bf16": 3.807e-03, "f16": 6.036e-04}
BARS = {k: (None if v is None else 2 * v) for k, v in MEASURED.items()}
SPANS = [(0, 2), (3, 5)]
_ORACLE = {}


def _ranges(T, Rr):
    return [(T, T + Rr)] + SPANS


def _oracle(s2v, case):
    """the fp32 oracle's q and k of every block on the B = 2 forward of _forward_inputs, once per case"""
    if case not in _ORACLE:
        from oracle import transformer_ref as tr

        cfg, sd = S._weights(s2v, case)
        _, T, F, Hh, W = S.CASES[case]
        inp = S._inputs(s2v, case)
        lat, _ = S._forward_inputs(s2v, case, 2, torch.float32)
        rope = cfg.use_rotary_positional_embeddings
        ocfg = dict(num_heads=cfg.num_attention_heads, num_layers=cfg.num_layers, use_rope=rope, norm_eps=cfg.norm_eps,
                    spatial_scale=cfg.spatial_interpolation_scale, temporal_scale=cfg.temporal_interpolation_scale)
        ref_rope, rp = tr.pipeline_rope(Hh * 8, W * 8, F) if rope else (None, None)
        _, calls = R.recorded_forward(sd, ocfg, lat.cpu(), H._text(inp, [0]).cpu(), inp["ref"][:1].cpu(), torch.tensor([799, 799]), rp, ref_rope)
        Rr = (Hh // 2) * (W // 2)
        V = F * Rr
        assert len(calls) == cfg.num_layers and tuple(calls[0][0].shape) == (2, cfg.num_attention_heads, T + Rr + V, 64)
        _ORACLE[case] = [R.oracle_mass(q, k, _ranges(T, Rr), T + Rr, V) for q, k in calls]
    return _ORACLE[case]


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("dt_name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", list(S.CASES))
def test_per_head_sums_of_one_armed_forward_against_the_recording_oracle(s2v, case, dt_name):
    dt = S.DT[dt_name]
    want = _oracle(s2v, case)
    cfg, _ = S._weights(s2v, case)
    m, eng = S._engine(s2v, case, dt, 2)
    lat, _ = S._forward_inputs(s2v, case, 2, dt)
    t = torch.tensor([799.0, 799.0])
    base = eng.forward(lat, t)
    eng.attn_map_enable(True, SPANS)
    worst = 0.0
    for l in range(cfg.num_layers):
        eng.attn_map_reset()
        out = eng.forward(lat, t, attn_layers=[l])
        assert S._bits(out, base), "an armed forward returns the un-armed forward's bits"
        got, count = eng.attn_map_read(per_head=True)
        assert count == 1 and tuple(got.shape) == tuple(want[l].shape)
        assert torch.isfinite(got).all()
        worst = max(worst, (got.cpu().double() - want[l]).abs().max().item())
    if cfg.num_layers > 1:
        assert (want[0] - want[1]).abs().max().item() > 1e-3, "the layers must differ, or a wrong layer would pass"
    eng.close()
    print(f"attention map {case} {dt_name}: largest absolute error of the per-head sums against the fp32 oracle {worst:.3e}")
    assert BARS[dt_name] is not None, f"no bar recorded for {dt_name}: measured {worst:.3e} here"
    assert worst <= BARS[dt_name], f"{worst:.3e} > {BARS[dt_name]:.3e}"


# ------------------------------------------------------------------------------------------------ 2. armed steps, eager and graph
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", list(S.CASES))
def test_armed_steps_return_the_unarmed_bits_and_the_sums_add_up(s2v, case, dt_name, kind):
    dt, B = S.DT[dt_name], 4
    inp = S._inputs(s2v, case)
    m, eng = S._engine(s2v, case, dt, B)
    plan = S._plan(s2v, kind, dt)
    bufs = S._Bufs(inp["lat"][:2], dt, kind == "dpm")
    tail = (inp["lat"][:2], inp["noise"][:, :2])
    bytes0 = eng.device_bytes()
    eng.attn_map_enable(True, SPANS)
    _, T, F, Hh, W = S.CASES[case]
    V, nh = F * (Hh // 2) * (W // 2), eng.cfg.num_attention_heads
    assert eng.device_bytes() == (bytes0[0], bytes0[1] + 3 * B * nh * V * 4), "the sums count as workspace while on"

    def run(idx, layers, graph):
        """the steps idx from the start latents, step j armed with layers[j] -> the step outputs"""
        bufs.load(tail[0], None, tail[1][0] if bufs.dpm else None)
        out = []
        for j, i in enumerate(idx):
            if bufs.dpm:
                bufs.nz.copy_(tail[1][j % tail[1].shape[0]].to(bufs.x.dtype))
            eng.denoise_step(bufs.x, plan[i][0], plan[i][1], bufs.x0, bufs.nz, use_graph=graph, attn_layers=layers[j])
            torch.cuda.synchronize()
            out.append((bufs.x.clone(), bufs.x0.clone() if bufs.dpm else None, eng.last_noise_pred()))
        return out

    sums = {}
    for graph in (False, True):
        base = run([0, 1], [None, None], graph)
        got, count = eng.attn_map_read(per_head=True)
        assert count == 0 and not got.any(), "un-armed steps add nothing"
        caps = eng.lora_state["graph_captures"]
        armed = run([0, 1], [[0, 1], [1]], graph)
        for i in range(2):
            for k in range(3):
                assert S._bits(armed[i][k], base[i][k]), f"graph {graph} step {i}: an armed step differs from the un-armed step"
        both, count = eng.attn_map_read(per_head=True)
        assert count == 3, "one per armed layer launch"
        if graph:
            assert eng.lora_state["graph_captures"] - caps == 2, "one executable per layer mask"
        # an un-armed step after an armed one: the un-armed executable, nothing collected (arm is one-shot)
        again = run([0, 1], [None, None], graph)
        assert all(S._bits(again[i][k], base[i][k]) for i in range(2) for k in range(3))
        same, count = eng.attn_map_read(per_head=True)
        assert count == 3 and torch.equal(same, both)
        if graph:
            assert eng.lora_state["graph_captures"] - caps == 2, "the un-armed executable was still held"
            run([0, 1], [[0, 1], [1]], graph)
            assert eng.lora_state["graph_captures"] - caps == 2, "the armed executables are replayed"
            twice, count = eng.attn_map_read(per_head=True)
            assert count == 6 and torch.allclose(twice, both + both, rtol=1e-5, atol=1e-6), "the same three launches again, on top"
        # each armed step alone, then their fp32 sum
        eng.attn_map_reset()
        zero, count = eng.attn_map_read(per_head=True)
        assert count == 0 and not zero.any(), "reset zeroes the sums and the count"
        run([0, 1], [[0, 1], None], graph)
        first, c1 = eng.attn_map_read(per_head=True)
        eng.attn_map_reset()
        run([0, 1], [None, [1]], graph)
        second, c2 = eng.attn_map_read(per_head=True)
        assert (c1, c2) == (2, 1) and first.any() and second.any()
        # step 0 armed with two layers adds layer 0 then layer 1 to zeros; step 1 adds layer 1 on top: ((l0 + l1) + l1')
        assert torch.equal(both.view(torch.int32), (first + second).view(torch.int32)), "two armed steps are not the fp32 sum of each alone"
        mean, c = eng.attn_map_read(per_head=False)
        assert c == 1 and torch.equal(mean.view(torch.int32), R.mean_reference(second, 1).view(torch.int32))
        sums[graph] = both
        eng.attn_map_reset()
    assert torch.equal(sums[False].view(torch.int32), sums[True].view(torch.int32)), "graph and eager sums differ"
    # the positive halves see other text than the negative ones, and the ranges are masses: in (0, 1], the reference stream not all of it
    assert (sums[True] >= 0).all() and sums[True].any() and (sums[True] <= 3.0 + 1e-3).all()
    assert not torch.equal(sums[True][:, :2], sums[True][:, 2:])
    eng.attn_map_enable(False)
    assert eng.device_bytes() == bytes0, "off: device_bytes is what it was"
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. geometry
def test_a_new_geometry_resizes_and_zeroes_and_off_means_off(s2v):
    case, dt = "sincos", torch.bfloat16
    inp = S._inputs(s2v, case)
    m, eng = S._engine(s2v, case, dt, 2)
    _, T, F, Hh, W = S.CASES[case]
    nh = eng.cfg.num_attention_heads
    eng.attn_map_enable(True)
    lat = inp["lat"][:2].to(dt).contiguous()
    eng.forward(lat, torch.tensor([500.0, 500.0]), attn_layers=[0])
    got, count = eng.attn_map_read(per_head=True)
    assert count == 1 and tuple(got.shape) == (1, 2, nh, F * (Hh // 2) * (W // 2)) and got.any()
    ws = eng.device_bytes()[1]
    eng.set_geometry(4, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(H._text(inp, [0, 1]), inp["ref"][:2])
    got, count = eng.attn_map_read(per_head=True)
    assert count == 0 and tuple(got.shape) == (1, 4, nh, F * (Hh // 2) * (W // 2)) and not got.any()
    assert eng.device_bytes()[1] > ws
    eng.forward(inp["lat"][:4].to(dt).contiguous(), torch.tensor([500.0] * 4), attn_layers=[1])
    got, count = eng.attn_map_read(per_head=True)
    assert count == 1 and (got >= 0).all() and got[:, 3].any(), "the fourth sample collects too"
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def _refused(s2v, fn, match):
    with pytest.raises(s2v._lib.S2VError, match=match):
        fn()


def test_every_refusal_of_the_context_state_refuses_by_name(s2v):
    case, dt = "sincos", torch.bfloat16
    inp = S._inputs(s2v, case)
    m, eng = S._engine(s2v, case, dt, 2)
    lat = inp["lat"][:2].to(dt).contiguous()
    t = torch.tensor([500.0, 500.0])
    _refused(s2v, lambda: eng.forward(lat, t, attn_layers=[0]), r"s2v_attn_map_arm: the attention map is not enabled")
    _refused(s2v, lambda: eng.attn_map_read(), r"s2v_attn_map_read: the attention map is not enabled")
    _refused(s2v, lambda: eng.attn_map_reset(), r"s2v_attn_map_reset: the attention map is not enabled")
    _refused(s2v, lambda: eng.attn_map_enable(True, [(0, 1)] * 4), r"0\.\.3 text spans")
    _refused(s2v, lambda: eng.attn_map_enable(True, [(2, 6)]), r"a text span must be a token range inside \[0, T\)")
    _refused(s2v, lambda: eng.attn_map_enable(True, [(3, 2)]), r"a text span must be a token range inside \[0, T\)")
    eng.attn_map_enable(True, [(0, 5)])
    _refused(s2v, lambda: eng.attn_map_read(), r"the head mean needs at least one armed layer launch")
    _refused(s2v, lambda: eng.forward(lat, t, attn_layers=[2]), r"a layer bit at or beyond num_layers is set")
    # together with S2V_STEP_REUSE, in either order of the two arms
    eng.step_cache_enable(True)
    eng.forward(lat, t, cache="capture", attn_layers=[0])
    assert eng.attn_map_read(per_head=True)[1] == 1, "a CAPTURE step runs the block stack: it collects"
    L = s2v._lib
    L.check(L.lib().s2v_step_cache_arm(eng._h, L.STEP_REUSE))
    assert L.lib().s2v_attn_map_arm(eng._h, 1) != 0 and b"S2V_STEP_REUSE is armed for the next forward" in L.lib().s2v_last_error()
    L.check(L.lib().s2v_step_cache_arm(eng._h, L.STEP_FULL))
    L.check(L.lib().s2v_attn_map_arm(eng._h, 1))
    assert L.lib().s2v_step_cache_arm(eng._h, L.STEP_REUSE) != 0 and b"S2V_STEP_REUSE while an attention map is armed" in L.lib().s2v_last_error()
    L.check(L.lib().s2v_attn_map_arm(eng._h, 0))
    # a CFG-parallel split finds a mask armed
    eng.set_geometry(1, *S.CASES[case][1:])
    eng.prepare_tables(S.CASES[case][3] * 8, S.CASES[case][4] * 8)
    eng.set_conditioning(inp["pos"][:1], inp["ref"][:1])
    L.check(L.lib().s2v_attn_map_arm(eng._h, 1))
    x = inp["lat"][:1].to(dt).contiguous().clone()
    sch = H._sched(s2v, "ddim")
    sch.set_timesteps(10)
    _refused(s2v, lambda: eng.denoise_split_begin(x, 500.0, sch.coef(sch.timesteps[1], dt, 6.0), 1), r"s2v_denoise_split_begin: an attention map is armed")
    eng.close()
    # a shard context
    m, eng = S._engine(s2v, case, dt, 2)
    eng.set_shard(1, 0)
    eng.set_geometry(2, *S.CASES[case][1:])
    _refused(s2v, lambda: eng.attn_map_enable(True), r"s2v_attn_map_enable: a shard context")
    L.check(L.lib().s2v_attn_map_arm(eng._h, 0))
    assert L.lib().s2v_attn_map_arm(eng._h, 1) != 0 and b"s2v_attn_map_arm: a shard context" in L.lib().s2v_last_error()
    eng.close()


def test_arm_is_refused_while_fp8_qk_is_active_and_allowed_with_the_plain_fp8_format(s2v):
    T, F, Hh, W = 7, 3, 16, 24   # D = 256: whole fp8 tiles (tests/test_gpu_fp8.py)
    g = torch.Generator(device=DEV).manual_seed(85)
    text = torch.randn(2, T, 128, generator=g, device=DEV)
    ref = torch.randn(1, 1, 16, Hh, W, generator=g, device=DEV) * 0.7
    lat = torch.randn(2, F, 16, Hh, W, generator=g, device=DEV).to(torch.bfloat16).contiguous()
    for fmt in ("fp8-qk", "fp8"):
        c = s2v.tiny(use_rope=True, heads=4, layers=2, text_dim=128, temb=64)
        sd = s2v.weights.synthetic_state_dict(c, seed=81, parity=True)
        c.weight_format = fmt
        m = s2v.HipCogVideoXTransformer3DModel(c, torch.bfloat16, DEV)
        m.load_state_dict(sd)
        eng = m.engine
        eng.set_geometry(2, T, F, Hh, W)
        eng.prepare_tables(Hh * 8, W * 8)
        eng.set_conditioning(text, ref)
        eng.attn_map_enable(True)
        t = torch.tensor([500.0, 500.0])
        if fmt == "fp8-qk":
            _refused(s2v, lambda: eng.forward(lat, t, attn_layers=[0]), r"s2v_attn_map_arm: fp8 QK\^T is active")
        else:
            base = eng.forward(lat, t)
            assert S._bits(eng.forward(lat, t, attn_layers=[0, 1]), base)
            got, count = eng.attn_map_read(per_head=True)
            assert count == 2 and (got >= 0).all() and got.any() and (got <= 2.0 + 1e-3).all()
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. the pipeline
PH, PW, PF, PT = S.PH, S.PW, S.PF, S.PT


def _hand_driven(s2v, pipe, kind, dt, kw, n, armed, layers, spans, modes=None, vids=(0,)):
    """the call's steps by hand through engine.denoise_step: step i armed with `layers` where i is in `armed` -> (latents, head mean, count)"""
    eng, sch = pipe.transformer.engine, pipe.scheduler
    b = len(vids)
    g = torch.Generator().manual_seed(44)
    x = (kw["latents"].to(DEV) * sch.init_noise_sigma).to(dt).contiguous().clone()
    eng.set_geometry(2 * b, PT, x.shape[1], PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning(torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]]), kw["ref_img_states"])
    if modes is not None:
        eng.step_cache_enable(True)
    eng.attn_map_enable(True, spans)
    steps = s2v.S2VPipeline.video_plan(H._sched(s2v, kind), n, None, 6.0, False, dt)["steps"]
    dpm = kind == "dpm"
    x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
    nz = torch.empty_like(x) if dpm else None
    for i, st in enumerate(steps):
        for _ in range(st["draws"]):
            nz.copy_(torch.randn(nz.shape, generator=g, dtype=dt))
        eng.denoise_step(x, float(st["t"]), st["coef"], x0, nz, cache=None if modes is None else modes[i], attn_layers=layers if i in armed else None)
    mean, count = eng.attn_map_read(per_head=False)
    eng.attn_map_enable(False)
    if modes is not None:
        eng.step_cache_enable(False)
    torch.cuda.synchronize()
    return x, mean, count


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_maps_are_the_hand_driven_armed_steps_in_bits(s2v, kind):
    dt = torch.bfloat16
    pipe = H._pipe(s2v, kind, dt)
    eng = pipe.transformer.engine
    inp = H._inputs(s2v, "tiny-rope")
    kw = dict(height=PH, width=PW, num_frames=PF, num_inference_steps=6, guidance_scale=6.0, latents=inp["lat"][:1].to(dt), **S._args(s2v, dt))
    gen = lambda: torch.Generator().manual_seed(44)
    base = pipe(generator=gen(), use_graph=True, **kw)["frames"].clone()
    assert pipe.attention_maps is None
    bytes0 = eng.device_bytes()
    am = s2v.AttentionMap([1, 0], steps=[1, 4, 5], text_spans=[(0, 2), (2, 5)])
    got = pipe(generator=gen(), use_graph=True, attention_map=am, **kw)["frames"].clone()
    assert S._bits(got, base), "the latents are those of the call without attention_map"
    maps = pipe.attention_maps
    Fl, h, w = got.shape[1], PH // 16, PW // 16
    assert maps["count"] == 6 and maps["layers"] == [1, 0] and maps["steps"] == [1, 4, 5] and maps["skipped_steps"] == []
    assert tuple(maps["subject"].shape) == (1, Fl, h, w) and tuple(maps["text"].shape) == (2, 1, Fl, h, w)
    assert maps["subject"].dtype == torch.float32 and (maps["subject"] > 0).all() and (maps["subject"] < 1).all()
    assert eng.device_bytes() == bytes0, "the map is disabled when the call ends"
    eager = pipe(generator=gen(), use_graph=False, attention_map=am, **kw)["frames"]
    assert S._bits(eager, base) and torch.equal(pipe.attention_maps["subject"], maps["subject"]) and torch.equal(pipe.attention_maps["text"], maps["text"])
    x, mean, count = _hand_driven(s2v, pipe, kind, dt, kw, 6, {1, 4, 5}, [0, 1], [(0, 2), (2, 5)])
    assert count == 6 and S._bits(x, base)
    assert torch.equal(mean[0, 1:2].reshape(1, Fl, h, w), maps["subject"]), "the positive half, head mean, mean over the launches"
    assert torch.equal(mean[1:, 1:2].reshape(2, 1, Fl, h, w), maps["text"])
    assert not torch.equal(mean[0, 0], mean[0, 1]), "the negative half is another map"
    eng.close()


def test_pipeline_with_a_step_cache_plan_collects_on_full_steps_only_and_reports_it(s2v):
    dt, kind = torch.bfloat16, "ddim"
    pipe = H._pipe(s2v, kind, dt)
    inp = H._inputs(s2v, "tiny-rope")
    kw = dict(height=PH, width=PW, num_frames=PF, num_inference_steps=6, guidance_scale=6.0, latents=inp["lat"][:1].to(dt), **S._args(s2v, dt))
    plan = S.PLAN   # F R R F R F
    base = pipe(step_cache=plan, use_graph=True, **kw)["frames"].clone()
    got = pipe(step_cache=plan, use_graph=True, attention_map=s2v.AttentionMap([1]), **kw)["frames"].clone()
    assert S._bits(got, base)
    maps = pipe.attention_maps
    assert maps["steps"] == [0, 3, 5] and maps["skipped_steps"] == [1, 2, 4] and maps["count"] == 3
    assert pipe.step_cache_report == {"plan": plan, "full": 3, "reused": 3, "ran_full": []}
    modes = ["capture", "reuse", "reuse", "capture", "reuse", None]
    x, mean, count = _hand_driven(s2v, pipe, kind, dt, kw, 6, {0, 3, 5}, [1], [], modes)
    assert count == 3 and S._bits(x, base)
    assert torch.equal(mean[0, 1:2].reshape(maps["subject"].shape), maps["subject"])
    pipe(step_cache=plan, attention_map=s2v.AttentionMap([1], steps=[1, 2]), **kw)
    assert pipe.attention_maps["count"] == 0 and pipe.attention_maps["steps"] == [] and not pipe.attention_maps["subject"].any()
    pipe.transformer.engine.close()


def test_pipeline_two_videos_with_scalars_and_a_second_call_with_the_map_as_change_map(s2v):
    dt, kind = torch.bfloat16, "ddim"
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, kind, dt, vae)
    kw = dict(height=PH, width=PW, num_frames=H.VF, num_inference_steps=4, guidance_scale=6.0, use_graph=True)   # 9 frames: the input video's
    am = s2v.AttentionMap([0, 1], steps=[2, 3])
    both = pipe(generator=H._gens(range(2)), attention_map=am, **S._args(s2v, dt, (0, 1)), **kw)["frames"].clone()
    maps = pipe.attention_maps
    assert tuple(maps["subject"].shape)[0] == 2 and maps["count"] == 4
    for k in range(2):
        one = pipe(generator=H._gens([k])[0], attention_map=am, **S._args(s2v, dt, (k,)), **kw)["frames"]
        # tiny-rope runs no split-K GEMM at either batch size (tests/test_gpu_step_cache.py holds the latents of such calls to bits)
        assert S._bits(both[k:k + 1], one), f"video {k} differs from its one-video call"
        assert torch.equal(maps["subject"][k:k + 1], pipe.attention_maps["subject"]), f"row {k} of the map is not the one-video call's map"
    assert not torch.equal(maps["subject"][0], maps["subject"][1])
    # generate, then repaint only the subject: two calls
    m = maps["subject"][:1]
    cm = s2v.attention_map_to_change_map(m, float(m.min()), float(m.max()), H.VF)
    assert cm.dtype == torch.uint8 and tuple(cm.shape) == (1, H.VF, PH, PW) and cm.min() == 0 and cm.max() == 255
    lat, _ = s2v.engine.map_to_latent(cm, DEV)
    level = torch.floor(((m - m.min()) / (m.max() - m.min())).clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)
    assert torch.equal(lat, level.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)), "every latent cell has the level of its own patch"
    out = pipe(video=H._videos(1), change_map=cm, strength=0.75, generator=H._gens([0])[0], output_type="latent",
               **kw, **S._args(s2v, dt, (0,)))["frames"]
    assert torch.isfinite(out.float()).all()
    pipe.transformer.engine.close()
