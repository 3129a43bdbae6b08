"""Attention steering on the GPU at engine and pipeline level (include/s2v_hip.h: s2v_attn_steer_*; engine.attn_steer_* and steer_layers=;
S2VPipeline with attention_steer=).  Engines, weights and inputs are those of tests/test_gpu_step_cache.py, imported: "mid-rope" (6 heads,
T / R / V = 7 / 391 / 1173) and "sincos" (no RoPE, 3 heads, T / R / V = 5 / 15 / 30).

Against the steered fp32 CPU oracle (tests/attn_steer_ref.py: the bias as an additive mask of scaled_dot_product_attention on one block) the
error of a forward with ONE layer steered may be at most 2 x the error of the un-steered forward against the un-steered oracle at the same
case and dtype, measured in the same run; the figure is the relative L2 error of the noise prediction.

The oracle test runs the weights variant "out16": attn1.to_out.0 (weight and bias) of every block times 16.  With the plain weights the
attention branch is a small part of the residual stream and the test is vacuous in bf16: steering one block moves the fp32 oracle's output
by 5.3e-3 (mid-rope, block 0) and 2.8e-2 (sincos), against a bf16 error of 6.7e-3 / 7.3e-3 -- a forward that ignored the arm would pass.
Times 16 the oracle moves by 8.2e-2 / 9.8e-2 (mid-rope, block 0 / 1) and 3.6e-1 / 2.6e-1 (sincos), against a bf16 error of 7.4e-3 (chosen
before a GPU run from the CPU oracle in bf16 against itself in fp32 over the factors 1 .. 32).  The test asks for 4 bars = 8 x the
un-steered error between any two of the three oracles: a forward that ignores the arm, or steers the other block, then ends at least three
bars beyond the bar.

Measured on an MI355X (rel-l2 against the oracle, un-steered forward -> one block steered, blocks 0 / 1; profiles/r20_attn_steer.txt):
    mid-rope f32   2.424e-06 -> 2.552e-06 / 2.588e-06      the oracles 8.2e-02 / 9.8e-02 apart
    mid-rope bf16  7.439e-03 -> 7.552e-03 / 7.650e-03
    sincos   f32   1.038e-06 -> 1.008e-06 / 1.175e-06      the oracles 3.6e-01 / 2.6e-01 apart
    sincos   bf16  7.443e-03 -> 7.251e-03 / 7.192e-03"""
import pytest
import torch

import attn_steer_ref as R
import test_gpu_batch_hetero as H
import test_gpu_step_cache as S

pytestmark = pytest.mark.gpu
DEV = S.DEV
_ORACLE, _SD = {}, {}


def _dims(case):
    _, T, F, Hh, W = S.CASES[case]
    Rr = (Hh // 2) * (W // 2)
    return T, Rr, F * Rr


def _ranges(case, b=1, subject=64.0, span=2.0 ** -6):
    """a text span on the positive halves, the reference keys on every sample"""
    T, Rr, V = _dims(case)
    return [(0, 3, span, ((1 << b) - 1) << b), (T, T + Rr, subject, (1 << (2 * b)) - 1)]


def _weights(s2v, case):
    """S._weights' plain variant with the attention out-projection of every block times 16 (see the module docstring)"""
    if case not in _SD:
        cfg, sd = S._weights(s2v, case)
        sd = dict(sd)
        for l in range(cfg.num_layers):
            for k in ("weight", "bias"):
                n = f"transformer_blocks.{l}.attn1.to_out.0.{k}"
                sd[n] = sd[n] * 16.0
        _SD[case] = (cfg, sd)
    return _SD[case]


def _engine16(s2v, case, dt, B):
    """S._engine on the out16 weights"""
    cfg, sd = _weights(s2v, case)
    _, T, F, Hh, W = S.CASES[case]
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    m.load_state_dict(sd)
    eng = m.engine
    eng.set_geometry(B, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    inp = S._inputs(s2v, case)
    eng.set_conditioning(H._text(inp, list(range(B // 2))), inp["ref"][:B // 2])
    return m, eng


def _oracle(s2v, case, layers):
    """the fp32 oracle's noise prediction on the B = 2 forward of S._forward_inputs with the blocks `layers` steered by _ranges(case)"""
    key = (case, tuple(layers))
    if key not in _ORACLE:
        from oracle import transformer_ref as tr

        cfg, sd = _weights(s2v, case)
        _, T, F, Hh, W = S.CASES[case]
        inp = S._inputs(s2v, case)
        lat, _ = S._forward_inputs(s2v, case, 2, torch.float32)
        rope = cfg.use_rotary_positional_embeddings
        ocfg = dict(num_heads=cfg.num_attention_heads, num_layers=cfg.num_layers, use_rope=rope, norm_eps=cfg.norm_eps,
                    spatial_scale=cfg.spatial_interpolation_scale, temporal_scale=cfg.temporal_interpolation_scale)
        ref_rope, rp = tr.pipeline_rope(Hh * 8, W * 8, F) if rope else (None, None)
        T_, Rr, V = _dims(case)
        rec = R.Record(_ranges(case), T_ + Rr, T_ + Rr + V)
        _ORACLE[key] = R.steered_forward(layers, rec, 2, T_ + Rr + V, sd, ocfg, lat.cpu(), H._text(inp, [0]).cpu(), inp["ref"][:1].cpu(),
                                         torch.tensor([799, 799]), rp, ref_rope).double()
    return _ORACLE[key]


def _refused(s2v, fn, match):
    with pytest.raises(s2v.S2VError, match=match):
        fn()


# ------------------------------------------------------------------------------------------------ 1. against the steered oracle
@pytest.mark.parametrize("dt_name", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(S.CASES))
def test_one_steered_layer_against_the_steered_oracle_within_twice_the_unsteered_error(s2v, case, dt_name):
    dt = S.DT[dt_name]
    cfg, _ = _weights(s2v, case)
    m, eng = _engine16(s2v, case, dt, 2)
    lat, _ = S._forward_inputs(s2v, case, 2, dt)
    t = torch.tensor([799.0, 799.0])
    plain = _oracle(s2v, case, [])
    base = eng.forward(lat, t)
    err_u = R.rel_l2(base, plain)
    bar = 2 * err_u
    eng.attn_steer_enable(True)
    empty = eng.forward(lat, t, steer_layers=[0])   # enabled and armed, no range set: the record steers nothing
    if dt == torch.bfloat16:   # attn_pp<STEER> beside attn_pp; the fp32 engine's steered layer is the generic kernel beside attn_f32m: other bits
        assert S._bits(empty, base)
    assert R.rel_l2(empty, plain) <= bar
    eng.attn_steer_set(_ranges(case))
    assert S._bits(eng.forward(lat, t), base), "an un-armed forward runs today's launches"
    want = [_oracle(s2v, case, [l]) for l in range(cfg.num_layers)]
    for l in range(cfg.num_layers):
        got = eng.forward(lat, t, steer_layers=[l])
        assert torch.isfinite(got.float()).all()
        err = R.rel_l2(got, want[l])
        apart = R.rel_l2(plain, want[l])
        print(f"MEASURED steer {case} {dt_name} layer {l}: un-steered {err_u:.3e} steered {err:.3e} (ratio {err / err_u:.2f}); the oracles are {apart:.3e} apart")
        assert apart >= 4 * bar, f"layer {l}: the steered oracle is only {apart:.3e} from the un-steered one: a forward that ignores the arm would pass"
        assert err <= bar, f"layer {l}: {err:.3e} > 2 x {err_u:.3e}"
        assert S._bits(eng.forward(lat, t), base), "an un-armed forward after an armed one returns the un-armed bits"
    d = R.rel_l2(want[0], want[1])
    assert d >= 4 * bar, f"steering layer 0 and layer 1 must differ by far more than the bar ({d:.3e}), or a wrong layer would pass"
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. launch sequences
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_armed_steps_eager_captured_and_new_weights_without_a_new_capture(s2v, dt_name, kind):
    case, dt, B = "sincos", S.DT[dt_name], 4
    b = B // 2
    inp = S._inputs(s2v, case)
    m, eng = S._engine(s2v, case, dt, B)
    plan = S._plan(s2v, kind, dt)
    dpm = kind == "dpm"
    bufs = S._Bufs(inp["lat"][:b], dt, dpm)

    def step(i, graph, layers):
        bufs.load(inp["lat"][:b], None, inp["noise"][0, :b] if dpm else None)
        eng.denoise_step(bufs.x, plan[i][0], plan[i][1], bufs.x0, bufs.nz, use_graph=graph, steer_layers=layers)
        torch.cuda.synchronize()
        return bufs.x.clone()

    bytes0 = eng.device_bytes()
    plain = step(1, False, None)
    eng.attn_steer_enable(True)
    assert eng.device_bytes()[1] > bytes0[1] and eng.device_bytes()[0] == bytes0[0]
    w1, w2 = _ranges(case, b), _ranges(case, b, subject=2.0 ** -5, span=16.0)
    eng.attn_steer_set(w1)
    eager1 = step(1, False, [1])
    assert not S._bits(eager1, plain)
    assert S._bits(step(1, False, None), plain), "un-armed after armed: the un-armed bits"
    cap0 = eng.lora_state["graph_captures"]
    assert S._bits(step(1, True, [1]), eager1), "an armed captured step equals the armed eager step"
    assert S._bits(step(1, True, None), plain), "an un-armed step never replays an armed executable"
    assert S._bits(step(1, True, [1]), eager1), "... nor the reverse"
    cap1 = eng.lora_state["graph_captures"]
    assert cap1 == cap0 + 2, "one executable per layer mask: armed and un-armed, each captured once"
    assert not S._bits(step(1, True, [0]), eager1) and eng.lora_state["graph_captures"] == cap1 + 1, "another layer mask is another executable"
    eng.attn_steer_set(w2)   # the table is data: the replay reads the new record
    replay2 = step(1, True, [1])
    assert eng.lora_state["graph_captures"] == cap1 + 1, "new weights re-capture nothing"
    assert not S._bits(replay2, eager1)
    assert S._bits(replay2, step(1, False, [1])), "the replay at the new weights equals the eager step at the new weights"
    assert S._bits(step(1, True, None), plain)
    eng.attn_steer_enable(False)
    assert eng.device_bytes() == bytes0, "disabling restores s2v_device_bytes"
    assert S._bits(step(1, True, None), plain) and S._bits(step(1, False, None), plain)
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. the library's refusals
def test_every_refusal_of_the_library_refuses_by_name(s2v):
    case, dt = "sincos", torch.bfloat16
    inp = S._inputs(s2v, case)
    m, eng = S._engine(s2v, case, dt, 2)
    lat, _ = S._forward_inputs(s2v, case, 2, dt)
    t = torch.tensor([500.0, 500.0])
    T, Rr, V = _dims(case)
    N = T + Rr + V
    _refused(s2v, lambda: eng.attn_steer_set(_ranges(case)), r"s2v_attn_steer_set: attention steering is not enabled")
    _refused(s2v, lambda: eng.forward(lat, t, steer_layers=[0]), r"s2v_attn_steer_arm: attention steering is not enabled")
    eng.attn_steer_enable(True)
    _refused(s2v, lambda: eng.attn_steer_set([(0, 3, 2.0, 3), (2, 5, 2.0, 3)]), r"s2v_attn_steer_set: key range 1 = \[2, 5\) overlaps or precedes range 0")
    _refused(s2v, lambda: eng.attn_steer_set([(0, N + 1, 2.0, 3)]), rf"s2v_attn_steer_set: key range 0 = \[0, {N + 1}\) must be non-empty and inside \[0, Ntok = {N}\)")
    _refused(s2v, lambda: eng.attn_steer_set([(0, 3, 0.0, 3)]), r"s2v_attn_steer_set: weight 0 = 0 must be finite and inside \[2\^-16, 2\^16\]")
    _refused(s2v, lambda: eng.attn_steer_set([(0, 3, 2.0 ** 17, 3)]), r"weight 0 = 131072")
    eng.attn_steer_set(_ranges(case))
    _refused(s2v, lambda: eng.forward(lat, t, steer_layers=[2]), r"s2v_attn_steer_arm: a layer bit at or beyond num_layers is set")
    # an armed attention map or S2V_STEP_REUSE together with an armed steer, in either order of the two arms
    L = s2v._lib
    eng.attn_map_enable(True)
    _refused(s2v, lambda: eng.forward(lat, t, attn_layers=[0], steer_layers=[0]), r"s2v_attn_steer_arm: an attention map is armed")
    base = eng.forward(lat, t)   # the refused call left the map's arm behind: this forward takes it
    L.check(L.lib().s2v_attn_steer_arm(eng._h, 1))
    _refused(s2v, lambda: L.check(L.lib().s2v_attn_map_arm(eng._h, 1)), r"s2v_attn_map_arm: attention steering is armed")
    L.check(L.lib().s2v_attn_steer_arm(eng._h, 0))
    eng.attn_map_enable(False)
    eng.step_cache_enable(True)
    eng.forward(lat, t, cache="capture")
    _refused(s2v, lambda: eng.forward(lat, t, cache="reuse", steer_layers=[0]), r"s2v_attn_steer_arm: S2V_STEP_REUSE is armed")
    eng.forward(lat, t)
    eng.forward(lat, t, cache="capture")
    L.check(L.lib().s2v_attn_steer_arm(eng._h, 1))
    _refused(s2v, lambda: L.check(L.lib().s2v_step_cache_arm(eng._h, L.STEP_REUSE)), r"s2v_step_cache_arm: S2V_STEP_REUSE while attention steering is armed")
    L.check(L.lib().s2v_attn_steer_arm(eng._h, 0))
    eng.step_cache_enable(False)
    # the seams
    hid = torch.zeros(2, V, eng.D, dtype=dt, device=DEV)
    enc = torch.zeros(2, T + Rr, eng.D, dtype=dt, device=DEV)
    L.check(L.lib().s2v_attn_steer_arm(eng._h, 1))
    _refused(s2v, lambda: eng.attn_forward(0, hid, enc), r"s2v_attn_forward: attention steering is armed")
    assert S._bits(eng.forward(lat, t), base), "a refusing entry takes the arm with it"
    # attn_p_format 1, then a geometry the ranges no longer fit
    eng.set_attn_p_format("f16")
    _refused(s2v, lambda: eng.forward(lat, t, steer_layers=[0]), r"s2v_attn_steer_arm: attn_p_format 1 keeps V\^T in fp16")
    eng.set_attn_p_format("bf16")
    _, T0, F0, Hh, W = S.CASES[case]
    bytes_on = eng.device_bytes()
    _refused(s2v, lambda: eng.set_geometry(2, T0, F0, 2, 2), r"s2v_set_geometry \(attention steering\): key range 1")
    _refused(s2v, lambda: eng.attn_steer_set([]), r"attention steering is not enabled")   # ... and steering is left off
    assert eng.device_bytes()[1] < bytes_on[1]
    eng.close()
    # engines the steered kernels do not serve
    m16, e16 = S._engine(s2v, case, torch.float16, 2)
    _refused(s2v, lambda: e16.attn_steer_enable(True), r"s2v_attn_steer_enable: an fp16 engine has no steered attention kernel")
    e16.close()


def test_split_windows_and_triples_are_refused_by_name_at_the_arm_and_at_the_step(s2v):
    """an arm on a context the feature does not serve refuses (st_check); an arm taken BEFORE the context became one is found by the step
    entry, which refuses by name and takes the arm with it"""
    import ctypes
    case, dt = "sincos", torch.bfloat16
    _, T, F, Hh, W = S.CASES[case]
    inp = S._inputs(s2v, case)
    m, eng = S._engine(s2v, case, dt, 2)
    eng.attn_steer_enable(True)
    eng.attn_steer_set(_ranges(case))
    L = s2v._lib
    arm = lambda mask=1: L.check(L.lib().s2v_attn_steer_arm(eng._h, mask))
    plan = S._plan(s2v, "ddim", dt)
    # a CFG-parallel split on a B = 1 geometry
    eng.set_geometry(1, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(inp["pos"][:1].to(dt), inp["ref"][:1].to(dt))
    eng.attn_steer_set([(0, 3, 2.0, 1)])
    x = inp["lat"][:1].to(dt).contiguous().clone()
    arm()
    rc = L.lib().s2v_denoise_split_begin(eng._h, L.ptr(x), plan[0][0], ctypes.byref(plan[0][1]), 1, 0, L.stream_ptr())
    assert rc != 0 and b"s2v_denoise_split_begin: attention steering is armed" in L.lib().s2v_last_error()
    # temporal windows: the arm on a context that has them, and the windowed step that finds an earlier arm
    eng.set_geometry(2, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(H._text(inp, [0]).to(dt), inp["ref"][:1].to(dt))
    arm()
    eng.set_windows(F + 2, 2, [1.0] * F)
    long = torch.cat([inp["lat"][:1], inp["lat"][1:2]], dim=1)[:, :F + 2].to(dt).contiguous().clone()
    _refused(s2v, lambda: eng.denoise_step_windows(long, plan[0][0], plan[0][1]), r"s2v_denoise_step_windows: attention steering is armed")
    _refused(s2v, arm, r"s2v_attn_steer_arm: temporal windows are set")
    _refused(s2v, lambda: eng.attn_steer_enable(True), r"s2v_attn_steer_enable: temporal windows are set")
    eng.clear_windows()
    # triples: B = 6 is three pairs or two triples; the arm is taken on the pairs, the guided step finds it
    eng.set_geometry(6, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(H._text(inp, [0, 1, 2]).to(dt), inp["ref"][:3].to(dt))
    eng.attn_steer_set(_ranges(case, 3))
    arm()
    eng.set_conditioning_triples(H._text(inp, [0, 1]).to(dt), inp["ref"][:2].to(dt))
    x2 = inp["lat"][:2].to(dt).contiguous().clone()
    _refused(s2v, lambda: eng.denoise_step(x2, plan[0][0], plan[0][1], subject=True), r"s2v_denoise_step_guided: attention steering is armed")
    _refused(s2v, arm, r"s2v_attn_steer_arm: the context is conditioned as subject-guidance triples")
    _refused(s2v, lambda: eng.attn_steer_enable(True), r"s2v_attn_steer_enable: the context is conditioned as subject-guidance triples")
    eng.close()


def test_shard_attention_only_and_fp8_contexts_and_the_seams_are_refused_by_name(s2v):
    case, dt = "sincos", torch.bfloat16
    _, T, F, Hh, W = S.CASES[case]
    Tt, Rr, V = _dims(case)
    L = s2v._lib
    # the block and AttnProcessor seams while a steer is armed: each refuses and takes the arm with it
    m, eng = S._engine(s2v, case, dt, 2)
    eng.attn_steer_enable(True)
    eng.attn_steer_set(_ranges(case))
    arm = lambda: L.check(L.lib().s2v_attn_steer_arm(eng._h, 1))
    hid = torch.zeros(2, V, eng.D, dtype=dt, device=DEV)
    enc = torch.zeros(2, Tt + Rr, eng.D, dtype=dt, device=DEV)
    temb = torch.zeros(2, eng.cfg.time_embed_dim, dtype=dt, device=DEV)
    arm()
    _refused(s2v, lambda: eng.block_forward(0, hid, enc[:, :Tt].contiguous(), enc[:, Tt:].contiguous(), temb), r"s2v_block_forward: attention steering is armed")
    eng.block_forward(0, hid, enc[:, :Tt].contiguous(), enc[:, Tt:].contiguous(), temb)   # the arm is gone
    arm()
    _refused(s2v, lambda: eng.attn_forward(0, hid, enc), r"s2v_attn_forward: attention steering is armed")
    arm()
    _refused(s2v, lambda: eng.attn_forward_with(eng, 0, hid, enc), r"s2v_attn_forward_with: attention steering is armed")
    eng.attn_forward_with(eng, 0, hid, enc)
    # a shard context: making one switches steering off, and it cannot be switched on
    eng.set_shard(1, 0)
    eng.set_geometry(2, T, F, Hh, W)
    _refused(s2v, lambda: eng.attn_steer_set([]), r"s2v_attn_steer_set: attention steering is not enabled")
    _refused(s2v, lambda: eng.attn_steer_enable(True), r"s2v_attn_steer_enable: a shard context")
    _refused(s2v, arm, r"s2v_attn_steer_arm: attention steering is not enabled")
    eng.close()
    # attention-only contexts
    acfg = s2v.TransformerConfig(num_layers=1, num_attention_heads=2, time_embed_dim=8, text_embed_dim=64, use_rotary_positional_embeddings=True)
    ws = s2v.S2VEngine(acfg, dt, DEV, kind=L.CTX_ATTN_WORKSPACE)
    ws.set_geometry(1, 3, 1, 4, 4)
    _refused(s2v, lambda: ws.attn_steer_enable(True), r"s2v_attn_steer_enable: attention-only contexts")
    ws.close()
    aw = s2v.S2VEngine(acfg, dt, DEV, kind=L.CTX_ATTN_WEIGHTS)
    _refused(s2v, lambda: aw.attn_steer_enable(True), r"s2v_attn_steer_enable: attention-only contexts")
    aw.close()
    # every fp8 weight format
    for fmt in ("fp8", "fp8-qk", "fp8-auto"):
        c8 = s2v.tiny(use_rope=True, heads=4, layers=2, text_dim=128, temb=64)
        c8.weight_format = fmt
        e8 = s2v.S2VEngine(c8, dt, DEV)
        e8.set_geometry(2, 7, 3, 16, 24)
        _refused(s2v, lambda: e8.attn_steer_enable(True), r"s2v_attn_steer_enable: fp8 weight formats have no steered attention")
        e8.close()


# ------------------------------------------------------------------------------------------------ 4. the pipeline
PH, PW, PF, PT = S.PH, S.PW, S.PF, S.PT


def _hand_driven(s2v, pipe, kind, dt, kw, n, armed, steer, vids=(0,), blend=None):
    """the call's steps by hand through engine.denoise_step: step i steered on steer.layers where i is in `armed`"""
    eng, sch = pipe.transformer.engine, pipe.scheduler
    b = len(vids)
    g = torch.Generator().manual_seed(44)
    x = (kw["latents"].to(DEV) * sch.init_noise_sigma).to(dt).contiguous().clone()
    eng.set_geometry(2 * b, PT, x.shape[1], PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning(torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]]), kw["ref_img_states"])
    eng.attn_steer_enable(True)
    eng.attn_steer_set(s2v.attention_steer_ranges(steer, PT, (PH // 16) * (PW // 16), b))
    steps = s2v.S2VPipeline.video_plan(H._sched(s2v, kind), n, None, 6.0, False, dt)["steps"]
    dpm = kind == "dpm"
    x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
    nz = torch.empty_like(x) if dpm else None
    for i, st in enumerate(steps):
        for _ in range(st["draws"]):
            nz.copy_(torch.randn(nz.shape, generator=g, dtype=dt))
        eng.denoise_step(x, float(st["t"]), st["coef"], x0, nz, steer_layers=steer.layers if i in armed else None)
    eng.attn_steer_enable(False)
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_equals_the_hand_driven_armed_steps_in_bits(s2v, kind):
    dt = torch.bfloat16
    pipe = H._pipe(s2v, kind, dt)
    eng = pipe.transformer.engine
    inp = H._inputs(s2v, "tiny-rope")
    kw = dict(height=PH, width=PW, num_frames=PF, num_inference_steps=6, guidance_scale=6.0, latents=inp["lat"][:1].to(dt), **S._args(s2v, dt))
    gen = lambda: torch.Generator().manual_seed(44)
    base = pipe(generator=gen(), use_graph=True, **kw)["frames"].clone()
    bytes0 = eng.device_bytes()
    ones = s2v.AttentionSteer([0, 1], subject=1.0, text_spans=[(0, 2, 1.0)])
    assert S._bits(pipe(generator=gen(), use_graph=True, attention_steer=ones, **kw)["frames"], base), "subject = 1, spans of 1: the plain call's bits"
    assert pipe.attention_steer_report == {"steps": [], "layers": [], "ranges": []}
    st = s2v.AttentionSteer([1, 0], steps=[1, 4, 5], subject=8.0, text_spans=[(0, 2, 0.125), (2, 5, 4.0)])
    got = pipe(generator=gen(), use_graph=True, attention_steer=st, **kw)["frames"].clone()
    assert not S._bits(got, base) and torch.isfinite(got.float()).all()
    rep = pipe.attention_steer_report
    assert rep["steps"] == [1, 4, 5] and rep["layers"] == [1, 0] and len(rep["ranges"]) == 3 and rep["ranges"][2] == (PT, PT + 24, 8.0, 0b11)
    assert eng.device_bytes() == bytes0, "steering is disabled when the call ends"
    assert S._bits(pipe(generator=gen(), use_graph=False, attention_steer=st, **kw)["frames"], got), "captured == eager"
    assert S._bits(_hand_driven(s2v, pipe, kind, dt, kw, 6, {1, 4, 5}, st), got), "the pipeline is the hand-driven armed steps"
    every = s2v.AttentionSteer([0], subject=8.0)
    got_all = pipe(generator=gen(), use_graph=True, attention_steer=every, **kw)["frames"].clone()
    assert pipe.attention_steer_report["steps"] == list(range(6))
    assert S._bits(_hand_driven(s2v, pipe, kind, dt, kw, 6, set(range(6)), every), got_all)
    assert S._bits(pipe(generator=gen(), use_graph=True, **kw)["frames"], base), "the plain call afterwards"
    eng.close()


def test_pipeline_two_videos_with_scalars_and_a_mask_together_with_steering(s2v):
    dt, kind = torch.bfloat16, "ddim"
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, kind, dt, vae)
    kw = dict(height=PH, width=PW, num_frames=H.VF, num_inference_steps=4, guidance_scale=6.0, use_graph=True, output_type="latent")
    st = s2v.AttentionSteer([0, 1], steps=[0, 2, 3], subject=8.0, text_spans=[(1, 4, 0.25)])
    both = pipe(generator=H._gens(range(2)), attention_steer=st, **S._args(s2v, dt, (0, 1)), **kw)["frames"].clone()
    assert pipe.attention_steer_report["ranges"] == [(1, 4, 0.25, 0b1100), (PT, PT + 24, 8.0, 0b1111)]
    plain = pipe(generator=H._gens(range(2)), **S._args(s2v, dt, (0, 1)), **kw)["frames"]
    assert not S._bits(both, plain)
    for k in range(2):
        one = pipe(generator=H._gens([k])[0], attention_steer=st, **S._args(s2v, dt, (k,)), **kw)["frames"]
        # tiny-rope runs no split-K GEMM at either batch size (tests/test_gpu_step_cache.py holds the latents of such calls to bits)
        assert S._bits(both[k:k + 1], one), f"video {k} differs from its one-video call: the sample masks cover [negative x b | positive x b]"
    # mask= together with steering: the kept cells are the input's, the repainted ones differ from the un-steered call's
    mask = torch.zeros(1, H.VF, PH, PW)
    mask[:, :, :, PW // 2:] = 1.0
    mk = dict(video=H._videos(1), mask=mask, strength=0.75, **kw)
    st = s2v.AttentionSteer([0, 1], steps=[0, 2], subject=8.0, text_spans=[(1, 4, 0.25)])   # strength 0.75 of 4 steps runs 3
    a = pipe(generator=H._gens([0])[0], attention_steer=st, **mk, **S._args(s2v, dt, (0,)))["frames"].clone()
    b = pipe(generator=H._gens([0])[0], **mk, **S._args(s2v, dt, (0,)))["frames"]
    w = a.shape[-1]
    assert S._bits(a[..., : w // 2], b[..., : w // 2]), "kept cells: the clean input latents in both calls"
    assert not S._bits(a[..., w // 2:], b[..., w // 2:]) and torch.isfinite(a.float()).all()
    pipe.transformer.engine.close()
