"""Local attention in time on the GPU at engine and pipeline level (include/s2v_hip.h: s2v_attn_local_*; engine.attn_local_* and
local_layers=; S2VPipeline with local_attention=).  Engines, weights and inputs are those of tests/test_gpu_step_cache.py, imported: "mid-rope"
(6 heads, T / R / V = 7 / 391 / 1173, three latent frames) and "sincos" (no RoPE, 3 heads, T / R / V = 5 / 15 / 30, two frames).

Against the windowed fp32 CPU oracle (tests/attn_local_ref.py: vis(i) as a boolean mask of scaled_dot_product_attention on one block, frames =
0) the error of a forward with ONE local layer may be at most 2 x the error of the un-windowed forward against the plain oracle at the same
case and dtype, measured in the same run; the figure is the relative L2 error of the noise prediction.

The oracle test runs the weights variant "out16q4": attn1.to_out.0 (weight and bias) of every block times 16, as the steering test does, and
attn1.norm_q (weight and bias) times 4.  With the plain weights the test is vacuous in bf16: windowing one block moves the fp32 oracle's
output by 2.9e-3 / 3.6e-3 (mid-rope, block 0 / 1) and 8.4e-3 (sincos) against a bf16 error of 6.7e-3 / 7.1e-3.  The out-projection alone does
not mend it: the synthetic weights give nearly uniform softmax rows, and a window then replaces one average of V rows by another -- at times
16 the oracles are 4.1e-2 / 4.5e-2 apart (mid-rope), at times 32 and 64 no further (5.3e-2 / 3.9e-2, 5.3e-2 / 2.4e-2), under four bars = 8 x
the bf16 error = 5.9e-2.  Scores times 4 (the q-norm's affine) make the rows peaked: times 16 and 4 the oracles are 4.1e-1 / 3.1e-1 (mid-rope)
and 2.3e-1 / 2.2e-1 (sincos) apart and blocks 0 and 1 4.7e-1 / 3.1e-1, against a bf16 error of 1.6e-2 / 1.5e-2, i.e. four bars of 1.3e-1 /
1.2e-1.  Chosen before a GPU run from the CPU oracle in bf16 against itself in fp32, over out-projection factors 1 .. 64 and score factors
1 .. 8, on CPU draws of the same input recipe.

Measured on an MI355X (rel-l2 against the oracle, un-windowed forward -> one block local, blocks 0 / 1; profiles/r21_attn_local.txt):
    mid-rope f32   3.803e-06 -> 3.837e-06 / 3.946e-06      the oracles 4.1e-01 / 3.0e-01 apart
    mid-rope bf16  1.664e-02 -> 1.711e-02 / 1.721e-02
    sincos   f32   1.458e-06 -> 1.476e-06 / 1.458e-06      the oracles 2.9e-01 / 2.0e-01 apart
    sincos   bf16  1.476e-02 -> 1.480e-02 / 1.462e-02"""
import ctypes

import pytest
import torch

import attn_local_ref as R
import test_gpu_batch_hetero as H
import test_gpu_step_cache as S

pytestmark = pytest.mark.gpu
DEV = S.DEV
_ORACLE, _SD = {}, {}


def _dims(case):
    """T, S (rows of a latent frame = rows of the reference image), F"""
    _, T, F, Hh, W = S.CASES[case]
    return T, (Hh // 2) * (W // 2), F


def _table(case, frames=0):
    T, Sr, F = _dims(case)
    return R.frames_table(T, Sr, F, Sr, frames)


def _weights(s2v, case):
    """S._weights' plain variant, the attention out-projection of every block times 16 and its q-norm times 4 (see the module docstring)"""
    if case not in _SD:
        cfg, sd = S._weights(s2v, case)
        sd = dict(sd)
        for l in range(cfg.num_layers):
            for k in ("weight", "bias"):
                n = f"transformer_blocks.{l}.attn1.to_out.0.{k}"
                sd[n] = sd[n] * 16.0
                n = f"transformer_blocks.{l}.attn1.norm_q.{k}"
                sd[n] = sd[n] * 4.0
        _SD[case] = (cfg, sd)
    return _SD[case]


def _engine164(s2v, case, dt, B):
    """S._engine on the out16q4 weights"""
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
    """the fp32 oracle's noise prediction on the B = 2 forward of S._forward_inputs with the blocks `layers` windowed by _table(case)"""
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
        _ORACLE[key] = R.local_forward(layers, _table(case), sd, ocfg, lat.cpu(), H._text(inp, [0]).cpu(), inp["ref"][:1].cpu(),
                                       torch.tensor([799, 799]), rp, ref_rope).double()
    return _ORACLE[key]


def _refused(s2v, fn, match):
    with pytest.raises(s2v.S2VError, match=match):
        fn()


def _set(eng, tab):
    eng.attn_local_set(tab.P, tab.lo, tab.hi)


# ------------------------------------------------------------------------------------------------ 1. against the windowed oracle
@pytest.mark.parametrize("dt_name", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(S.CASES))
def test_one_local_layer_against_the_windowed_oracle_within_twice_the_unwindowed_error(s2v, case, dt_name):
    dt = S.DT[dt_name]
    cfg, _ = _weights(s2v, case)
    m, eng = _engine164(s2v, case, dt, 2)
    lat, _ = S._forward_inputs(s2v, case, 2, dt)
    t = torch.tensor([799.0, 799.0])
    plain = _oracle(s2v, case, [])
    base = eng.forward(lat, t)
    err_u = R.rel_l2(base, plain)
    bar = 2 * err_u
    eng.attn_local_enable(True)
    dense = eng.forward(lat, t, local_layers=[0, 1])   # enabled and armed, no table set: the table windows nothing
    if dt == torch.bfloat16:   # attn_pp<LOCAL> beside attn_pp; the fp32 engine's local layer is the generic kernel beside attn_f32m: other bits
        assert S._bits(dense, base), "an all-dense table, armed: the plain bits"
    assert R.rel_l2(dense, plain) <= bar
    tab = _table(case)
    _set(eng, tab)
    assert S._bits(eng.forward(lat, t), base), "an un-armed forward runs today's launches"
    want = [_oracle(s2v, case, [l]) for l in range(cfg.num_layers)]
    for l in range(cfg.num_layers):
        got = eng.forward(lat, t, local_layers=[l])
        assert torch.isfinite(got.float()).all()
        err = R.rel_l2(got, want[l])
        apart = R.rel_l2(plain, want[l])
        print(f"MEASURED local {case} {dt_name} layer {l}: un-windowed {err_u:.3e} local {err:.3e} (ratio {err / err_u:.2f}); the oracles are {apart:.3e} apart")
        assert apart >= 4 * bar, f"layer {l}: the windowed oracle is only {apart:.3e} from the plain one: a forward that ignores the arm would pass"
        assert err <= bar, f"layer {l}: {err:.3e} > 2 x {err_u:.3e}"
        assert S._bits(eng.forward(lat, t), base), "an un-armed forward after an armed one returns the un-armed bits"
    d = R.rel_l2(want[0], want[1])
    assert d >= 4 * bar, f"windowing layer 0 and layer 1 must differ by far more than the bar ({d:.3e}), or a wrong layer would pass"
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. launch sequences
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_armed_steps_eager_captured_and_a_new_table_without_a_new_capture(s2v, dt_name, kind):
    case, dt, B = "sincos", S.DT[dt_name], 4
    b = B // 2
    inp = S._inputs(s2v, case)
    m, eng = S._engine(s2v, case, dt, B)
    plan = S._plan(s2v, kind, dt)
    dpm = kind == "dpm"
    bufs = S._Bufs(inp["lat"][:b], dt, dpm)

    def step(i, graph, layers):
        bufs.load(inp["lat"][:b], None, inp["noise"][0, :b] if dpm else None)
        eng.denoise_step(bufs.x, plan[i][0], plan[i][1], bufs.x0, bufs.nz, use_graph=graph, local_layers=layers)
        torch.cuda.synchronize()
        return bufs.x.clone()

    bytes0 = eng.device_bytes()
    plain = step(1, False, None)
    eng.attn_local_enable(True)
    assert eng.device_bytes()[1] > bytes0[1] and eng.device_bytes()[0] == bytes0[0]
    if dt == torch.bfloat16:
        assert S._bits(step(1, False, [0, 1]), plain), "enabled with the all-dense table and armed: the plain bits"
    t1 = _table(case)
    T, Sr, F = _dims(case)
    t2 = R.Table(t1.P, [min(a + 3, c) for a, c in zip(t1.lo, t1.hi)], t1.hi)   # another table: every window three keys shorter
    _set(eng, t1)
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
    _set(eng, t2)   # the table is data: the replay reads the new one
    replay2 = step(1, True, [1])
    assert eng.lora_state["graph_captures"] == cap1 + 1, "a new table re-captures nothing"
    assert not S._bits(replay2, eager1)
    assert S._bits(replay2, step(1, False, [1])), "the replay at the new table equals the eager step at the new table"
    assert S._bits(step(1, True, None), plain)
    eng.attn_local_enable(False)
    assert eng.device_bytes() == bytes0, "disabling restores s2v_device_bytes"
    assert S._bits(step(1, True, None), plain) and S._bits(step(1, False, None), plain)
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. the library's refusals
def test_every_refusal_of_the_library_refuses_by_name(s2v):
    case, dt = "sincos", torch.bfloat16
    m, eng = S._engine(s2v, case, dt, 2)
    lat, _ = S._forward_inputs(s2v, case, 2, dt)
    t = torch.tensor([500.0, 500.0])
    T, Sr, F = _dims(case)
    N = T + (F + 1) * Sr
    tab = _table(case)
    _refused(s2v, lambda: _set(eng, tab), r"s2v_attn_local_set: local attention is not enabled")
    _refused(s2v, lambda: eng.forward(lat, t, local_layers=[0]), r"s2v_attn_local_arm: local attention is not enabled")
    eng.attn_local_enable(True)
    _refused(s2v, lambda: eng.attn_local_set(0, tab.lo, tab.hi), rf"s2v_attn_local_set: the prefix P = 0 must lie inside \[1, Ntok = {N}\]")
    _refused(s2v, lambda: eng.attn_local_set(N + 1, tab.lo, tab.hi), rf"s2v_attn_local_set: the prefix P = {N + 1} must lie inside")
    lo = list(tab.lo)
    lo[30] = tab.P - 1
    _refused(s2v, lambda: eng.attn_local_set(tab.P, lo, tab.hi), rf"s2v_attn_local_set: row 30 has the window \[{tab.P - 1}, {tab.hi[30]}\)")
    hi = list(tab.hi)
    hi[N - 1] = N + 1
    _refused(s2v, lambda: eng.attn_local_set(tab.P, tab.lo, hi), rf"row {N - 1} has the window \[{tab.lo[N - 1]}, {N + 1}\)")
    lo = list(tab.lo)
    lo[25] = tab.hi[25] + 1
    _refused(s2v, lambda: eng.attn_local_set(tab.P, lo, tab.hi), r"row 25 has the window")
    _refused(s2v, lambda: eng.attn_local_set(tab.P, tab.lo[:-1], tab.hi[:-1]), rf"attn_local_set: the row table has {N - 1} rows, the geometry {N} tokens")
    _set(eng, tab)
    _refused(s2v, lambda: eng.forward(lat, t, local_layers=[2]), r"s2v_attn_local_arm: a layer bit at or beyond num_layers is set")
    # an armed attention map, an armed steer or S2V_STEP_REUSE together with an armed local mask, in either order of the two arms
    L = s2v._lib
    arm = lambda mask=1: L.check(L.lib().s2v_attn_local_arm(eng._h, mask))
    eng.attn_map_enable(True)
    _refused(s2v, lambda: eng.forward(lat, t, attn_layers=[0], local_layers=[0]), r"s2v_attn_local_arm: an attention map is armed")
    base = eng.forward(lat, t)   # the refused call left the map's arm behind: this forward takes it
    arm()
    _refused(s2v, lambda: L.check(L.lib().s2v_attn_map_arm(eng._h, 1)), r"s2v_attn_map_arm: local attention is armed")
    arm(0)
    eng.attn_map_enable(False)
    eng.attn_steer_enable(True)
    eng.attn_steer_set([(0, 3, 2.0, 3)])
    _refused(s2v, lambda: eng.forward(lat, t, steer_layers=[0], local_layers=[0]), r"s2v_attn_local_arm: attention steering is armed")
    eng.forward(lat, t)
    arm()
    _refused(s2v, lambda: L.check(L.lib().s2v_attn_steer_arm(eng._h, 1)), r"s2v_attn_steer_arm: local attention is armed")
    arm(0)
    eng.attn_steer_enable(False)
    eng.step_cache_enable(True)
    eng.forward(lat, t, cache="capture")
    _refused(s2v, lambda: eng.forward(lat, t, cache="reuse", local_layers=[0]), r"s2v_attn_local_arm: S2V_STEP_REUSE is armed")
    eng.forward(lat, t)
    eng.forward(lat, t, cache="capture")
    arm()
    _refused(s2v, lambda: L.check(L.lib().s2v_step_cache_arm(eng._h, L.STEP_REUSE)), r"s2v_step_cache_arm: S2V_STEP_REUSE while local attention is armed")
    arm(0)
    eng.step_cache_enable(False)
    # the seams: each refuses and takes the arm with it
    V = F * Sr
    hid = torch.zeros(2, V, eng.D, dtype=dt, device=DEV)
    enc = torch.zeros(2, T + Sr, eng.D, dtype=dt, device=DEV)
    temb = torch.zeros(2, eng.cfg.time_embed_dim, dtype=dt, device=DEV)
    arm()
    _refused(s2v, lambda: eng.block_forward(0, hid, enc[:, :T].contiguous(), enc[:, T:].contiguous(), temb), r"s2v_block_forward: local attention is armed")
    eng.block_forward(0, hid, enc[:, :T].contiguous(), enc[:, T:].contiguous(), temb)   # the arm is gone
    arm()
    _refused(s2v, lambda: eng.attn_forward(0, hid, enc), r"s2v_attn_forward: local attention is armed")
    arm()
    _refused(s2v, lambda: eng.attn_forward_with(eng, 0, hid, enc), r"s2v_attn_forward_with: local attention is armed")
    assert S._bits(eng.forward(lat, t), base), "a refusing entry takes the arm with it"
    # attn_p_format 1, then a geometry of another Ntok: the feature is switched off
    eng.set_attn_p_format("f16")
    _refused(s2v, lambda: eng.forward(lat, t, local_layers=[0]), r"s2v_attn_local_arm: attn_p_format 1 keeps V\^T in fp16")
    eng.set_attn_p_format("bf16")
    _, T0, F0, Hh, W = S.CASES[case]
    bytes_on = eng.device_bytes()
    eng.set_geometry(2, T0, F0, 2, 2)
    _refused(s2v, lambda: eng.attn_local_set(1, [1] * (T0 + F0 + 1), [T0 + F0 + 1] * (T0 + F0 + 1)), r"local attention is not enabled")
    assert eng.device_bytes()[1] < bytes_on[1]
    eng.close()
    # engines the local kernels do not serve
    m16, e16 = S._engine(s2v, case, torch.float16, 2)
    _refused(s2v, lambda: e16.attn_local_enable(True), r"s2v_attn_local_enable: an fp16 engine has no local attention kernel")
    e16.close()


def test_split_windows_and_triples_are_refused_by_name_at_the_arm_and_at_the_step(s2v):
    """an arm on a context the feature does not serve refuses (la_check); an arm taken BEFORE the context became one is found by the step
    entry, which refuses by name and takes the arm with it"""
    case, dt = "sincos", torch.bfloat16
    _, T, F, Hh, W = S.CASES[case]
    inp = S._inputs(s2v, case)
    m, eng = S._engine(s2v, case, dt, 2)
    eng.attn_local_enable(True)
    _set(eng, _table(case))
    L = s2v._lib
    arm = lambda mask=1: L.check(L.lib().s2v_attn_local_arm(eng._h, mask))
    plan = S._plan(s2v, "ddim", dt)
    # a CFG-parallel split on a B = 1 geometry (the same Ntok: the table stays)
    eng.set_geometry(1, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(inp["pos"][:1].to(dt), inp["ref"][:1].to(dt))
    x = inp["lat"][:1].to(dt).contiguous().clone()
    arm()
    rc = L.lib().s2v_denoise_split_begin(eng._h, L.ptr(x), plan[0][0], ctypes.byref(plan[0][1]), 1, 0, L.stream_ptr())
    assert rc != 0 and b"s2v_denoise_split_begin: local attention is armed" in L.lib().s2v_last_error()
    # temporal windows: the arm on a context that has them, and the windowed step that finds an earlier arm
    eng.set_geometry(2, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(H._text(inp, [0]).to(dt), inp["ref"][:1].to(dt))
    arm()
    eng.set_windows(F + 2, 2, [1.0] * F)
    long = torch.cat([inp["lat"][:1], inp["lat"][1:2]], dim=1)[:, :F + 2].to(dt).contiguous().clone()
    _refused(s2v, lambda: eng.denoise_step_windows(long, plan[0][0], plan[0][1]), r"s2v_denoise_step_windows: local attention is armed")
    _refused(s2v, arm, r"s2v_attn_local_arm: temporal windows are set")
    _refused(s2v, lambda: eng.attn_local_enable(True), r"s2v_attn_local_enable: temporal windows are set")
    eng.clear_windows()
    # triples: B = 6 is three pairs or two triples; the arm is taken on the pairs, the guided step finds it
    eng.set_geometry(6, T, F, Hh, W)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(H._text(inp, [0, 1, 2]).to(dt), inp["ref"][:3].to(dt))
    arm()
    eng.set_conditioning_triples(H._text(inp, [0, 1]).to(dt), inp["ref"][:2].to(dt))
    x2 = inp["lat"][:2].to(dt).contiguous().clone()
    _refused(s2v, lambda: eng.denoise_step(x2, plan[0][0], plan[0][1], subject=True), r"s2v_denoise_step_guided: local attention is armed")
    _refused(s2v, arm, r"s2v_attn_local_arm: the context is conditioned as subject-guidance triples")
    _refused(s2v, lambda: eng.attn_local_enable(True), r"s2v_attn_local_enable: the context is conditioned as subject-guidance triples")
    eng.close()


def test_shard_attention_only_and_fp8_contexts_are_refused_by_name(s2v):
    case, dt = "sincos", torch.bfloat16
    _, T, F, Hh, W = S.CASES[case]
    L = s2v._lib
    m, eng = S._engine(s2v, case, dt, 2)
    eng.attn_local_enable(True)
    tab = _table(case)
    # a shard context: making one switches the feature off, and it cannot be switched on
    eng.set_shard(1, 0)
    eng.set_geometry(2, T, F, Hh, W)
    _refused(s2v, lambda: _set(eng, tab), r"s2v_attn_local_set: local attention is not enabled")
    _refused(s2v, lambda: eng.attn_local_enable(True), r"s2v_attn_local_enable: a shard context")
    _refused(s2v, lambda: L.check(L.lib().s2v_attn_local_arm(eng._h, 1)), r"s2v_attn_local_arm: local attention is not enabled")
    eng.close()
    # attention-only contexts
    acfg = s2v.TransformerConfig(num_layers=1, num_attention_heads=2, time_embed_dim=8, text_embed_dim=64, use_rotary_positional_embeddings=True)
    ws = s2v.S2VEngine(acfg, dt, DEV, kind=L.CTX_ATTN_WORKSPACE)
    ws.set_geometry(1, 3, 1, 4, 4)
    _refused(s2v, lambda: ws.attn_local_enable(True), r"s2v_attn_local_enable: attention-only contexts")
    ws.close()
    aw = s2v.S2VEngine(acfg, dt, DEV, kind=L.CTX_ATTN_WEIGHTS)
    _refused(s2v, lambda: aw.attn_local_enable(True), r"s2v_attn_local_enable: attention-only contexts")
    aw.close()
    # every fp8 weight format
    for fmt in ("fp8", "fp8-qk", "fp8-auto"):
        c8 = s2v.tiny(use_rope=True, heads=4, layers=2, text_dim=128, temb=64)
        c8.weight_format = fmt
        e8 = s2v.S2VEngine(c8, dt, DEV)
        e8.set_geometry(2, 7, 3, 16, 24)
        _refused(s2v, lambda: e8.attn_local_enable(True), r"s2v_attn_local_enable: fp8 weight formats have no local attention")
        e8.close()


# ------------------------------------------------------------------------------------------------ 4. the pipeline
PH, PW, PF, PT = S.PH, S.PW, S.PF, S.PT


def _hand_driven(s2v, pipe, kind, dt, kw, n, armed, layers, frames):
    """the call's steps by hand through engine.denoise_step: step i local on `layers` where i is in `armed`"""
    eng, sch = pipe.transformer.engine, pipe.scheduler
    g = torch.Generator().manual_seed(44)
    x = (kw["latents"].to(DEV) * sch.init_noise_sigma).to(dt).contiguous().clone()
    eng.set_geometry(2, PT, x.shape[1], PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning(torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]]), kw["ref_img_states"])
    Sr = (PH // 16) * (PW // 16)
    eng.attn_local_enable(True)
    _set(eng, R.frames_table(PT, Sr, x.shape[1], Sr, frames))
    steps = s2v.S2VPipeline.video_plan(H._sched(s2v, kind), n, None, 6.0, False, dt)["steps"]
    dpm = kind == "dpm"
    x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
    nz = torch.empty_like(x) if dpm else None
    for i, st in enumerate(steps):
        for _ in range(st["draws"]):
            nz.copy_(torch.randn(nz.shape, generator=g, dtype=dt))
        eng.denoise_step(x, float(st["t"]), st["coef"], x0, nz, local_layers=layers if i in armed else None)
    eng.attn_local_enable(False)
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
    for frames in (1, 7):   # two latent frames: frames >= F - 1 covers every frame
        assert S._bits(pipe(generator=gen(), use_graph=True, local_attention=s2v.LocalAttention("all", frames), **kw)["frames"], base), "the plain call's bits"
        assert pipe.local_attention_report == {"steps": [], "layers": [], "frames": frames, "visited_tile_share": 1.0}
    la = s2v.LocalAttention([1, 0], 0, steps=[1, 4, 5])
    got = pipe(generator=gen(), use_graph=True, local_attention=la, **kw)["frames"].clone()
    assert not S._bits(got, base) and torch.isfinite(got.float()).all()
    Sr = (PH // 16) * (PW // 16)
    tab = R.frames_table(PT, Sr, 2, Sr, 0)
    assert pipe.local_attention_report == {"steps": [1, 4, 5], "layers": [1, 0], "frames": 0, "visited_tile_share": R.share(tab)}
    assert eng.device_bytes() == bytes0, "local attention is disabled when the call ends"
    assert S._bits(pipe(generator=gen(), use_graph=False, local_attention=la, **kw)["frames"], got), "captured == eager"
    assert S._bits(_hand_driven(s2v, pipe, kind, dt, kw, 6, {1, 4, 5}, [1, 0], 0), got), "the pipeline is the hand-driven armed steps"
    every = s2v.LocalAttention("all", 0)
    got_all = pipe(generator=gen(), use_graph=True, local_attention=every, **kw)["frames"].clone()
    assert pipe.local_attention_report["steps"] == list(range(6)) and pipe.local_attention_report["layers"] == [0, 1]
    assert S._bits(_hand_driven(s2v, pipe, kind, dt, kw, 6, set(range(6)), [0, 1], 0), got_all)
    assert S._bits(pipe(generator=gen(), use_graph=True, **kw)["frames"], base), "the plain call afterwards"
    eng.close()


def test_pipeline_two_videos_with_scalars_and_a_mask_together_with_local_attention(s2v):
    dt, kind = torch.bfloat16, "ddim"
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, kind, dt, vae)
    kw = dict(height=PH, width=PW, num_frames=H.VF, num_inference_steps=4, guidance_scale=6.0, use_graph=True, output_type="latent")
    la = s2v.LocalAttention([0, 1], 1, steps=[0, 2, 3])   # three latent frames: frames = 1 windows the first and the last
    both = pipe(generator=H._gens(range(2)), local_attention=la, **S._args(s2v, dt, (0, 1)), **kw)["frames"].clone()
    assert pipe.local_attention_report["steps"] == [0, 2, 3] and pipe.local_attention_report["frames"] == 1
    plain = pipe(generator=H._gens(range(2)), **S._args(s2v, dt, (0, 1)), **kw)["frames"]
    assert not S._bits(both, plain)
    for k in range(2):
        one = pipe(generator=H._gens([k])[0], local_attention=la, **S._args(s2v, dt, (k,)), **kw)["frames"]
        # tiny-rope runs no split-K GEMM at either batch size (tests/test_gpu_step_cache.py holds the latents of such calls to bits)
        assert S._bits(both[k:k + 1], one), f"video {k} differs from its one-video call: one table serves every sample"
    # mask= together with local attention: the kept cells are the input's, the repainted ones differ from the un-windowed call's
    mask = torch.zeros(1, H.VF, PH, PW)
    mask[:, :, :, PW // 2:] = 1.0
    mk = dict(video=H._videos(1), mask=mask, strength=0.75, **kw)
    la = s2v.LocalAttention("all", 0, steps=[0, 2])   # strength 0.75 of 4 steps runs 3
    a = pipe(generator=H._gens([0])[0], local_attention=la, **mk, **S._args(s2v, dt, (0,)))["frames"].clone()
    b = pipe(generator=H._gens([0])[0], **mk, **S._args(s2v, dt, (0,)))["frames"]
    w = a.shape[-1]
    assert S._bits(a[..., : w // 2], b[..., : w // 2]), "kept cells: the clean input latents in both calls"
    assert not S._bits(a[..., w // 2:], b[..., w // 2:]) and torch.isfinite(a.float()).all()
    pipe.transformer.engine.close()
