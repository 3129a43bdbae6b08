"""Local attention in space and time on the GPU at engine and pipeline level (include/s2v_hip.h: s2v_attn_local_set_box beside s2v_attn_local_*;
engine.attn_local_set_box and local_layers=; S2VPipeline with local_attention=LocalAttention(..., rows=)).  Engines, weights and inputs are
those of tests/test_gpu_attn_local_engine.py, imported: "mid-rope" (6 heads, T / R / V = 7 / 391 / 1173, three latent frames of 17 patch rows of
23 cells) on the weights variant "out16q4" described there.  The pipeline runs the "tiny-rope" weights at 128 x 192 pixels: latent frames of 8
patch rows of 12 cells, S = 96 -- the 64 x 96 pixels of the other pipeline tests give frames of 24 cells, under the 64 the box form needs.

Against the boxed fp32 CPU oracle (vis(i) of tests/attn_box_ref.py passed to scaled_dot_product_attention through attn_local_ref._LocalF, one
block at a time, frames = 0, rows = 2) the error of a forward with ONE box layer may be at most 2 x the error of the un-windowed forward against
the plain oracle at the same dtype, measured in the same run; the figure is the relative L2 error of the noise prediction.  The guard: the
boxed oracle must lie at least 4 bars from the plain one and from the oracle windowed in time only (the same lo / hi).

Measured on an MI355X (rel-l2 against the oracle, un-windowed forward -> one block boxed, blocks 0 / 1):
    mid-rope f32   3.803e-06 -> 3.884e-06 / 4.061e-06      the boxed oracle 5.0e-01 / 3.9e-01 from the plain, 3.8e-01 / 2.9e-01 from the temporal one
    mid-rope bf16  1.664e-02 -> 1.721e-02 / 1.780e-02      four bars are 1.3e-01"""
import pytest
import torch

import attn_box_ref as X
import attn_local_ref as R
import test_gpu_attn_local_engine as E
import test_gpu_batch_hetero as H
import test_gpu_step_cache as S

pytestmark = pytest.mark.gpu
DEV = S.DEV
CASE = "mid-rope"
_ORACLE = {}


def _geom(case=CASE):
    """T, Hp, Wp, F"""
    _, T, F, Hh, W = S.CASES[case]
    return T, Hh // 2, W // 2, F


def _table(frames=0, rows=2, case=CASE):
    T, Hp, Wp, F = _geom(case)
    return X.box_table(T, Hp * Wp, F, Hp, Wp, frames, rows)


def _set(eng, tab):
    if isinstance(tab, X.BoxTable):
        eng.attn_local_set_box(tab.P, tab.S, tab.lo, tab.hi, tab.olo, tab.ohi)
    else:
        eng.attn_local_set(tab.P, tab.lo, tab.hi)


def _oracle(s2v, layers, vis_name):
    """the fp32 oracle's noise prediction on the B = 2 forward of S._forward_inputs with the blocks `layers` masked by the box table ("box"), by
    the window table of the same lo / hi ("temporal"), or not at all (layers empty)"""
    key = (tuple(layers), vis_name)
    if key not in _ORACLE:
        from oracle import transformer_ref as tr

        case = CASE
        cfg, sd = E._weights(s2v, case)
        _, T, F, Hh, W = S.CASES[case]
        inp = S._inputs(s2v, case)
        lat, _ = S._forward_inputs(s2v, case, 2, torch.float32)
        rope = cfg.use_rotary_positional_embeddings
        ocfg = dict(num_heads=cfg.num_attention_heads, num_layers=cfg.num_layers, use_rope=rope, norm_eps=cfg.norm_eps,
                    spatial_scale=cfg.spatial_interpolation_scale, temporal_scale=cfg.temporal_interpolation_scale)
        ref_rope, rp = tr.pipeline_rope(Hh * 8, W * 8, F) if rope else (None, None)
        tab = _table()
        vis = X.visible(tab) if vis_name == "box" else R.visible(tab.temporal())
        real = tr.F
        tr.F = R._LocalF(real, layers, vis)
        try:
            with torch.no_grad():
                _ORACLE[key] = tr.transformer_forward(sd, ocfg, lat.cpu(), H._text(inp, [0]).cpu(), inp["ref"][:1].cpu(), torch.tensor([799, 799]), rp,
                                                      ref_rope).double()
        finally:
            tr.F = real
    return _ORACLE[key]


# ------------------------------------------------------------------------------------------------ 1. against the boxed oracle
@pytest.mark.parametrize("dt_name", ["f32", "bf16"])
def test_one_box_layer_against_the_boxed_oracle_within_twice_the_unwindowed_error(s2v, dt_name):
    dt = S.DT[dt_name]
    cfg, _ = E._weights(s2v, CASE)
    m, eng = E._engine164(s2v, CASE, dt, 2)
    lat, _ = S._forward_inputs(s2v, CASE, 2, dt)
    t = torch.tensor([799.0, 799.0])
    plain = _oracle(s2v, [], "box")
    base = eng.forward(lat, t)
    err_u = X.rel_l2(base, plain)
    bar = 2 * err_u
    eng.attn_local_enable(True)
    tab = _table()
    _set(eng, X.from_local(R.dense_table(tab.N, tab.P), tab.S))
    dense = eng.forward(lat, t, local_layers=[0, 1])
    if dt == torch.bfloat16:   # attn_pp<BOX> beside attn_pp; the fp32 engine's box layer is the generic kernel beside attn_f32m: other bits
        assert S._bits(dense, base), "an all-dense box table, armed: the plain bits"
    assert X.rel_l2(dense, plain) <= bar
    _set(eng, tab)
    assert S._bits(eng.forward(lat, t), base), "an un-armed forward runs today's launches"
    for l in range(cfg.num_layers):
        want, temporal = _oracle(s2v, [l], "box"), _oracle(s2v, [l], "temporal")
        got = eng.forward(lat, t, local_layers=[l])
        assert torch.isfinite(got.float()).all()
        err = X.rel_l2(got, want)
        apart, apart_t = X.rel_l2(plain, want), X.rel_l2(temporal, want)
        print(f"MEASURED box {CASE} {dt_name} layer {l}: un-windowed {err_u:.3e} box {err:.3e} (ratio {err / err_u:.2f}); the boxed oracle is "
              f"{apart:.3e} from the plain and {apart_t:.3e} from the temporal one")
        assert apart >= 4 * bar, f"layer {l}: the boxed oracle is only {apart:.3e} from the plain one: a forward that ignores the arm would pass"
        assert apart_t >= 4 * bar, f"layer {l}: the boxed oracle is only {apart_t:.3e} from the temporal one: a kernel that ignores the offsets would pass"
        assert err <= bar, f"layer {l}: {err:.3e} > 2 x {err_u:.3e}"
        assert S._bits(eng.forward(lat, t), base), "an un-armed forward after an armed one returns the un-armed bits"
    d = X.rel_l2(_oracle(s2v, [0], "box"), _oracle(s2v, [1], "box"))
    assert d >= 4 * bar, f"boxing layer 0 and layer 1 must differ by far more than the bar ({d:.3e}), or a wrong layer would pass"
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. launch sequences
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_armed_steps_eager_captured_new_tables_and_the_other_kind(s2v, dt_name, kind):
    case, dt, B = CASE, S.DT[dt_name], 4
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

    caps = lambda: eng.lora_state["graph_captures"]
    bytes0 = eng.device_bytes()
    plain = step(1, False, None)
    eng.attn_local_enable(True)
    bytes_on = eng.device_bytes()
    b1, b2, win = _table(0, 2), _table(0, 1), _table().temporal()
    _set(eng, b1)
    assert eng.device_bytes()[1] > bytes_on[1] > bytes0[1] and eng.device_bytes()[0] == bytes0[0], "the box table counts as workspace"
    eager_b1 = step(1, False, [1])
    assert not S._bits(eager_b1, plain)
    assert S._bits(step(1, False, None), plain), "un-armed after armed: the un-armed bits"
    cap0 = caps()
    assert S._bits(step(1, True, [1]), eager_b1), "an armed captured step equals the armed eager step"
    assert S._bits(step(1, True, None), plain), "an un-armed step never replays an armed executable"
    assert S._bits(step(1, True, [1]), eager_b1), "... nor the reverse"
    assert caps() == cap0 + 2, "one executable per layer mask: armed and un-armed, each captured once"
    _set(eng, b2)   # a new box table: data
    replay_b2 = step(1, True, [1])
    assert caps() == cap0 + 2, "a new box table between two replays re-captures nothing"
    assert not S._bits(replay_b2, eager_b1)
    assert S._bits(replay_b2, step(1, False, [1])), "the replay at the new table equals the eager step at the new table"
    # a window table after a box table: the other kernel, so the captured steps are dropped; the bits are those of the window launch
    _set(eng, win)
    eager_win = step(1, False, [1])
    assert not S._bits(eager_win, replay_b2) and not S._bits(eager_win, plain)
    got = step(1, True, [1])
    assert caps() == cap0 + 3 and S._bits(got, eager_win), "a window table after a box table: a new capture, the window launch's bits"
    _set(eng, X.from_local(win, b1.S))   # the same rows as a box table with full offsets: the box kernel, the window launch's bits (bf16)
    got = step(1, True, [1])
    assert caps() == cap0 + 4, "a box table after a window table drops the captured steps as well"
    if dt == torch.bfloat16:
        assert S._bits(got, eager_win), "full offsets: the window launch's bits"
    _set(eng, b1)
    assert S._bits(step(1, True, [1]), eager_b1) and caps() == cap0 + 4, "and the first table again, replayed"
    assert S._bits(step(1, True, None), plain)
    eng.attn_local_enable(False)
    assert eng.device_bytes() == bytes0, "disabling restores s2v_device_bytes"
    assert S._bits(step(1, True, None), plain) and S._bits(step(1, False, None), plain)
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. the library's refusals
def test_every_refusal_of_the_library_refuses_by_name(s2v):
    case, dt = CASE, torch.bfloat16
    m, eng = S._engine(s2v, case, dt, 2)
    lat, _ = S._forward_inputs(s2v, case, 2, dt)
    t = torch.tensor([500.0, 500.0])
    tab = _table()
    N, P, Sr = tab.N, tab.P, tab.S
    refused = lambda fn, match: E._refused(s2v, fn, match)
    refused(lambda: _set(eng, tab), r"s2v_attn_local_set_box: local attention is not enabled")
    eng.attn_local_enable(True)
    sb = eng.attn_local_set_box
    refused(lambda: sb(0, Sr, tab.lo, tab.hi, tab.olo, tab.ohi), rf"s2v_attn_local_set_box: the prefix P = 0 must lie inside \[1, Ntok = {N}\]")
    refused(lambda: sb(N + 1, Sr, tab.lo, tab.hi, tab.olo, tab.ohi), rf"s2v_attn_local_set_box: the prefix P = {N + 1} must lie inside")
    refused(lambda: sb(P, 63, tab.lo, tab.hi, [0] * N, [63] * N), r"s2v_attn_local_set_box: the period S = 63 must be at least 64")
    lo = list(tab.lo)
    lo[30] = P - 1
    refused(lambda: sb(P, Sr, lo, tab.hi, tab.olo, tab.ohi), rf"s2v_attn_local_set_box: row 30 has the window \[{P - 1}, {tab.hi[30]}\)")
    hi = list(tab.hi)
    hi[N - 1] = N + 1
    refused(lambda: sb(P, Sr, tab.lo, hi, tab.olo, tab.ohi), rf"row {N - 1} has the window \[{tab.lo[N - 1]}, {N + 1}\)")
    ohi = list(tab.ohi)
    ohi[N - 1] = Sr + 1
    refused(lambda: sb(P, Sr, tab.lo, tab.hi, tab.olo, ohi), rf"row {N - 1} has the offsets \[{tab.olo[N - 1]}, {Sr + 1}\): 0 <= olo <= ohi <= S = {Sr}")
    olo = list(tab.olo)
    olo[P + 5] = -1
    refused(lambda: sb(P, Sr, tab.lo, tab.hi, olo, tab.ohi), rf"row {P + 5} has the offsets \[-1, ")
    olo[P + 5] = tab.ohi[P + 5] + 1
    refused(lambda: sb(P, Sr, tab.lo, tab.hi, olo, tab.ohi), rf"row {P + 5} has the offsets")
    refused(lambda: sb(P, Sr, tab.lo, tab.hi, tab.olo[:-1], tab.ohi), rf"attn_local_set_box: offs_lo has {N - 1} rows, the geometry {N} tokens")
    base = eng.forward(lat, t)
    assert S._bits(eng.forward(lat, t, local_layers=[0]), base), "every refused table left the all-dense one in place"
    _set(eng, tab)
    refused(lambda: eng.forward(lat, t, local_layers=[2]), r"s2v_attn_local_arm: a layer bit at or beyond num_layers is set")
    # the compositions: the arm is the existing entry, so the names are its names
    L = s2v._lib
    arm = lambda mask=1: L.check(L.lib().s2v_attn_local_arm(eng._h, mask))
    eng.attn_map_enable(True)
    refused(lambda: eng.forward(lat, t, attn_layers=[0], local_layers=[0]), r"s2v_attn_local_arm: an attention map is armed")
    eng.forward(lat, t)
    eng.attn_map_enable(False)
    eng.attn_steer_enable(True)
    eng.attn_steer_set([(0, 3, 2.0, 3)])
    refused(lambda: eng.forward(lat, t, steer_layers=[0], local_layers=[0]), r"s2v_attn_local_arm: attention steering is armed")
    eng.forward(lat, t)
    eng.attn_steer_enable(False)
    eng.step_cache_enable(True)
    eng.forward(lat, t, cache="capture")
    refused(lambda: eng.forward(lat, t, cache="reuse", local_layers=[0]), r"s2v_attn_local_arm: S2V_STEP_REUSE is armed")
    eng.forward(lat, t)
    eng.step_cache_enable(False)
    T, Hp, Wp, F = _geom()
    hid = torch.zeros(2, F * Sr, eng.D, dtype=dt, device=DEV)
    enc = torch.zeros(2, T + Sr, eng.D, dtype=dt, device=DEV)
    arm()
    refused(lambda: eng.attn_forward(0, hid, enc), r"s2v_attn_forward: local attention is armed")
    arm()
    refused(lambda: eng.attn_forward_with(eng, 0, hid, enc), r"s2v_attn_forward_with: local attention is armed")
    assert S._bits(eng.forward(lat, t), base), "a refusing entry takes the arm with it"
    # attn_p_format 1, temporal windows, triples: set_box names them as the other entries do
    eng.set_attn_p_format("f16")
    refused(lambda: _set(eng, tab), r"s2v_attn_local_set_box: attn_p_format 1 keeps V\^T in fp16")
    eng.set_attn_p_format("bf16")
    eng.set_windows(F + 2, 2, [1.0] * F)
    refused(lambda: _set(eng, tab), r"s2v_attn_local_set_box: temporal windows are set")
    eng.clear_windows()
    inp = S._inputs(s2v, case)
    eng.set_geometry(6, T, F, 2 * Hp, 2 * Wp)
    eng.prepare_tables(16 * Hp, 16 * Wp)
    eng.set_conditioning_triples(H._text(inp, [0, 1]).to(dt), inp["ref"][:2].to(dt))
    refused(lambda: _set(eng, tab), r"s2v_attn_local_set_box: the context is conditioned as subject-guidance triples")
    # a geometry of another Ntok: the feature is switched off, both tables freed
    bytes_on = eng.device_bytes()
    eng.set_geometry(2, T, F, 4, 4)
    refused(lambda: sb(1, 64, [1] * 3, [3] * 3, [0] * 3, [64] * 3), r"local attention is not enabled|has 3 rows")
    assert eng.device_bytes()[1] < bytes_on[1]
    eng.close()
    # engines and contexts the local kernels do not serve: by name, through la_check
    m16, e16 = S._engine(s2v, case, torch.float16, 2)
    refused(lambda: _set(e16, tab), r"s2v_attn_local_set_box: an fp16 engine has no local attention kernel")
    e16.close()
    m2, e2 = S._engine(s2v, case, dt, 2)
    e2.set_shard(1, 0)
    _, T0, F0, Hh, W = S.CASES[case]
    e2.set_geometry(2, T0, F0, Hh, W)
    refused(lambda: _set(e2, tab), r"s2v_attn_local_set_box: a shard context")
    e2.close()
    acfg = s2v.TransformerConfig(num_layers=1, num_attention_heads=2, time_embed_dim=8, text_embed_dim=64, use_rotary_positional_embeddings=True)
    ws = s2v.S2VEngine(acfg, dt, DEV, kind=L.CTX_ATTN_WORKSPACE)
    ws.set_geometry(1, 3, 1, 16, 16)
    n = 3 + 2 * 64
    refused(lambda: ws.attn_local_set_box(1, 64, [1] * n, [n] * n, [0] * n, [64] * n), r"s2v_attn_local_set_box: attention-only contexts")
    ws.close()
    for fmt in ("fp8", "fp8-qk", "fp8-auto"):
        c8 = s2v.tiny(use_rope=True, heads=4, layers=2, text_dim=128, temb=64)
        c8.weight_format = fmt
        e8 = s2v.S2VEngine(c8, dt, DEV)
        e8.set_geometry(2, 7, 3, 16, 24)
        n = 7 + 4 * 96
        refused(lambda: e8.attn_local_set_box(7 + 96, 96, [103] * n, [n] * n, [0] * n, [96] * n), r"s2v_attn_local_set_box: fp8 weight formats have no local attention")
        e8.close()


# ------------------------------------------------------------------------------------------------ 4. the pipeline
PH, PW, PT = 128, 192, S.PT   # latents 16 x 24: 8 patch rows of 12 cells
HP, WP = PH // 16, PW // 16
_PIN = {}


def _pin(s2v, dt, vids=(0,), frames=2):
    """prompt, reference and initial latents for the videos `vids` at 128 x 192 (made once, never written)"""
    if "x" not in _PIN:
        cfg, _ = H._weights(s2v, "tiny-rope")
        g = torch.Generator(device=DEV).manual_seed(91)
        _PIN["x"] = dict(neg=torch.randn(2, PT, cfg.text_embed_dim, generator=g, device=DEV),
                         pos=torch.randn(2, PT, cfg.text_embed_dim, generator=g, device=DEV),
                         ref=torch.randn(2, 1, cfg.in_channels, PH // 8, PW // 8, generator=g, device=DEV) * 0.7,
                         lat=torch.randn(2, 3, cfg.in_channels, PH // 8, PW // 8, generator=g, device=DEV))
    p, v = _PIN["x"], list(vids)
    return dict(prompt_embeds=p["pos"][v].to(dt), negative_prompt_embeds=p["neg"][v].to(dt), ref_img_states=p["ref"][v].to(dt),
                latents=p["lat"][v][:, :frames].to(dt))


def _hand_driven(s2v, pipe, kind, dt, kw, n, armed, layers, frames, rows):
    """the call's steps by hand through engine.denoise_step: step i boxed on `layers` where i is in `armed`"""
    eng, sch = pipe.transformer.engine, pipe.scheduler
    g = torch.Generator().manual_seed(44)
    x = (kw["latents"].to(DEV) * sch.init_noise_sigma).to(dt).contiguous().clone()
    F = x.shape[1]
    eng.set_geometry(2, PT, F, PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning(torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]]), kw["ref_img_states"])
    eng.attn_local_enable(True)
    _set(eng, X.box_table(PT, HP * WP, F, HP, WP, frames, rows))
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
    kw = dict(height=PH, width=PW, num_frames=5, num_inference_steps=6, guidance_scale=6.0, **_pin(s2v, dt))
    gen = lambda: torch.Generator().manual_seed(44)
    base = pipe(generator=gen(), use_graph=True, **kw)["frames"].clone()
    bytes0 = eng.device_bytes()
    today = pipe(generator=gen(), use_graph=True, local_attention=s2v.LocalAttention("all", 0), **kw)["frames"].clone()
    for rows in (HP - 1, HP, 50):
        got = pipe(generator=gen(), use_graph=True, local_attention=s2v.LocalAttention("all", 0, rows=rows), **kw)["frames"]
        assert S._bits(got, today), f"rows = {rows} >= Hp - 1: the bits of the call with rows=None"
        assert pipe.local_attention_report["rows"] == rows and pipe.local_attention_report["visited_tile_share"] == \
            R.share(R.frames_table(PT, HP * WP, 2, HP * WP, 0))
        got = pipe(generator=gen(), use_graph=True, local_attention=s2v.LocalAttention("all", 1, rows=rows), **kw)["frames"]
        assert S._bits(got, base), "... and over every frame as well: the plain call's bits"
    la = s2v.LocalAttention([1, 0], 0, steps=[1, 4, 5], rows=1)
    got = pipe(generator=gen(), use_graph=True, local_attention=la, **kw)["frames"].clone()
    assert not S._bits(got, base) and not S._bits(got, today) and torch.isfinite(got.float()).all()
    tab = X.box_table(PT, HP * WP, 2, HP, WP, 0, 1)
    assert pipe.local_attention_report == {"steps": [1, 4, 5], "layers": [1, 0], "frames": 0, "rows": 1, "visited_tile_share": X.share(tab)}
    assert eng.device_bytes() == bytes0, "local attention is disabled when the call ends"
    assert S._bits(pipe(generator=gen(), use_graph=False, local_attention=la, **kw)["frames"], got), "captured == eager"
    assert S._bits(_hand_driven(s2v, pipe, kind, dt, kw, 6, {1, 4, 5}, [1, 0], 0, 1), got), "the pipeline is the hand-driven armed steps"
    spatial = s2v.LocalAttention("all", 5, rows=2)   # frames >= F - 1 with a real rows: the purely spatial window
    got_sp = pipe(generator=gen(), use_graph=True, local_attention=spatial, **kw)["frames"].clone()
    assert pipe.local_attention_report["steps"] == list(range(6)) and pipe.local_attention_report["layers"] == [0, 1]
    assert S._bits(_hand_driven(s2v, pipe, kind, dt, kw, 6, set(range(6)), [0, 1], 2, 2), got_sp)
    assert S._bits(pipe(generator=gen(), use_graph=True, **kw)["frames"], base), "the plain call afterwards"
    eng.close()


def test_pipeline_two_videos_with_scalars_and_a_mask_together_with_a_box(s2v):
    dt, kind = torch.bfloat16, "ddim"
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, kind, dt, vae)
    kw = dict(height=PH, width=PW, num_frames=9, num_inference_steps=4, guidance_scale=6.0, use_graph=True, output_type="latent")
    la = s2v.LocalAttention([0, 1], 1, steps=[0, 2, 3], rows=1)   # three latent frames
    both = pipe(generator=H._gens(range(2)), local_attention=la, **_pin(s2v, dt, (0, 1), 3), **kw)["frames"].clone()
    assert pipe.local_attention_report["steps"] == [0, 2, 3] and pipe.local_attention_report["rows"] == 1
    plain = pipe(generator=H._gens(range(2)), **_pin(s2v, dt, (0, 1), 3), **kw)["frames"]
    assert not S._bits(both, plain)
    for k in range(2):
        one = pipe(generator=H._gens([k])[0], local_attention=la, **_pin(s2v, dt, (k,), 3), **kw)["frames"]
        assert S._bits(both[k:k + 1], one), f"video {k} differs from its one-video call: one table serves every sample"
    # mask= together with a box: the kept cells are the input's, the repainted ones differ from the un-windowed call's
    mask = torch.zeros(1, 9, PH, PW)
    mask[:, :, :, PW // 2:] = 1.0
    video = torch.rand(1, 3, 9, PH, PW, generator=torch.Generator().manual_seed(92)) * 2 - 1
    args = {k: v for k, v in _pin(s2v, dt, (0,), 3).items() if k != "latents"}
    mk = dict(video=video, mask=mask, strength=0.75, **kw)
    la = s2v.LocalAttention("all", 0, steps=[0, 2], rows=1)   # strength 0.75 of 4 steps runs 3
    a = pipe(generator=H._gens([0])[0], local_attention=la, **mk, **args)["frames"].clone()
    b = pipe(generator=H._gens([0])[0], **mk, **args)["frames"]
    w = a.shape[-1]
    assert S._bits(a[..., : w // 2], b[..., : w // 2]), "kept cells: the clean input latents in both calls"
    assert not S._bits(a[..., w // 2:], b[..., w // 2:]) and torch.isfinite(a.float()).all()
    pipe.transformer.engine.close()
