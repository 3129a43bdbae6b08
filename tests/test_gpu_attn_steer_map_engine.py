"""Steering maps on the GPU at engine and pipeline level (include/s2v_hip.h: s2v_attn_steer_set_maps; engine.attn_steer_set_maps and
steer_layers=; S2VPipeline with attention_steer=AttentionSteer(..., subject_map=)).  Engines, weights and inputs are those of
tests/test_gpu_step_cache.py ("mid-rope": T / R / V = 7 / 391 / 1173, a frame of 17 x 23 cells; "sincos": 5 / 15 / 30, 3 x 5 cells) with the out16
weights of tests/test_gpu_attn_steer_engine.py (its docstring says why).

Against the mapped fp32 CPU oracle (tests/attn_steer_map_ref.py mapped_forward: the bias as an additive mask of scaled_dot_product_attention on
one block) the error of a forward with ONE layer mapped may be at most 2 x the error of the un-steered forward against the un-steered oracle,
measured in the same run; the figure is the relative L2 error of the noise prediction.  The map is a box that moves by frame on the reference
keys, inside 64, outside 2^-6; its size is the first of HEIGHTS whose oracles meet the condition (the planes change, never the bar).  Condition,
asserted from the oracles alone before a mapped forward runs: the mapped oracle lies at least four
bars from the un-steered oracle, from the constant-weight oracle (the plane's geometric-mean weight) and from the oracle with the other layer
mapped.  The constant-weight oracle is taken on block 1: steering block 0 of mid-rope with 64 on EVERY cell moves the oracle by 8.2e-02
(tests/test_gpu_attn_steer_engine.py), 5.5 bars of the bf16 engine, so no box on block 0 can lie four bars from both the un-steered and a constant
oracle there; block 1 moves it by 9.8e-02 and more per cell.

MEASURED on an MI355X (profiles/r23_attn_steer_map.txt):
    mid-rope f32: box height 0.95, un-steered 2.424e-06; the oracles are 6.649e-02 / 8.679e-02 (mapped, layers 0 / 1, from un-steered), 5.778e-02 (layer 1 from constant-weight), 1.058e-01 (layer 0 from layer 1) apart
    mid-rope f32 layer 0: un-steered 2.424e-06 mapped 2.503e-06 (ratio 1.03)
    mid-rope f32 layer 1: un-steered 2.424e-06 mapped 2.534e-06 (ratio 1.05)
    mid-rope bf16: the box of height 0.95 is not taken, its oracles are 6.649e-02 / 8.679e-02 / 5.778e-02 / 1.058e-01 apart, the bar is 1.488e-02
    mid-rope bf16: box height 0.875, un-steered 7.439e-03; the oracles are 6.375e-02 / 8.456e-02 (mapped, layers 0 / 1, from un-steered), 6.109e-02 (layer 1 from constant-weight), 1.033e-01 (layer 0 from layer 1) apart
    mid-rope bf16 layer 0: un-steered 7.439e-03 mapped 7.520e-03 (ratio 1.01)
    mid-rope bf16 layer 1: un-steered 7.439e-03 mapped 7.572e-03 (ratio 1.02)
    sincos f32: box height 0.95, un-steered 1.038e-06; the oracles are 3.278e-01 / 2.283e-01 (mapped, layers 0 / 1, from un-steered), 1.242e-01 (layer 1 from constant-weight), 3.968e-01 (layer 0 from layer 1) apart
    sincos f32 layer 0: un-steered 1.038e-06 mapped 1.023e-06 (ratio 0.98)
    sincos f32 layer 1: un-steered 1.038e-06 mapped 1.140e-06 (ratio 1.10)
    sincos bf16: box height 0.95, un-steered 7.443e-03; the oracles are 3.278e-01 / 2.283e-01 (mapped, layers 0 / 1, from un-steered), 1.242e-01 (layer 1 from constant-weight), 3.968e-01 (layer 0 from layer 1) apart
    sincos bf16 layer 0: un-steered 7.443e-03 mapped 7.356e-03 (ratio 0.99)
    sincos bf16 layer 1: un-steered 7.443e-03 mapped 7.270e-03 (ratio 0.98)
"""
import numpy as np
import pytest
import torch

import attn_steer_map_ref as M
import attn_steer_ref as R
import test_gpu_attn_steer_engine as E
import test_gpu_batch_hetero as H
import test_gpu_step_cache as S

pytestmark = pytest.mark.gpu
DEV = S.DEV
_ORACLE = {}
INSIDE, OUTSIDE = 64.0, 2.0 ** -6


def _grid(case):
    _, T, F, Hh, W = S.CASES[case]
    return F, Hh // 2, W // 2


# the heights of the box the oracle test may take, tried in this order: the box is 80 % of the width, so 0.75, 0.70, 0.80, 0.65 and 0.85 of the cells
# of mid-rope lie inside.  Which one is taken is decided from the fp32 oracles alone (the planes change, the bar does not): with a box of 0.24 of
# the cells the mapped oracle of mid-rope lay only 3.8e-02 from the un-steered one, under four bars of the bf16 engine; that distance grows with
# the square root of the share, while the distance from the constant-weight oracle falls as the share nears 1
HEIGHTS = (0.95, 0.875, 1.0, 0.82, 1.0625)


def _box_map(s2v, case, shift=0, inside=INSIDE, outside=OUTSIDE, height=HEIGHTS[0]):
    """a box 80 % of the width and `height` of the height (beyond 1: the whole height and 85 % of the width) that moves right by frame"""
    F, Hp, Wp = _grid(case)
    wide = 0.8 if height <= 1.0 else 0.85
    boxes = [((1 - wide) * ((f + shift) % F) / max(F - 1, 1), 0.0, (1 - wide) * ((f + shift) % F) / max(F - 1, 1) + wide, min(height, 1.0)) for f in range(F)]
    return s2v.box_weight_map(boxes, F, Hp, Wp, inside, outside)


def _map_ranges(case, b=1):
    """the reference keys on every sample with plane 0, as engine.attn_steer_set_maps takes them"""
    T, Rr, V = E._dims(case)
    return [(T, T + Rr, [0] * (2 * b))]


def _oracle(s2v, case, layers, kind, height=HEIGHTS[0]):
    """the fp32 oracle on the B = 2 forward of S._forward_inputs with the blocks `layers` steered: kind "map" by the box map, "const" by its
    geometric-mean weight on every cell"""
    key = (case, tuple(layers), kind, height)
    if key not in _ORACLE:
        from oracle import transformer_ref as tr

        cfg, sd = E._weights(s2v, case)
        _, T, F, Hh, W = S.CASES[case]
        inp = S._inputs(s2v, case)
        lat, _ = S._forward_inputs(s2v, case, 2, torch.float32)
        rope = cfg.use_rotary_positional_embeddings
        ocfg = dict(num_heads=cfg.num_attention_heads, num_layers=cfg.num_layers, use_rope=rope, norm_eps=cfg.norm_eps,
                    spatial_scale=cfg.spatial_interpolation_scale, temporal_scale=cfg.temporal_interpolation_scale)
        ref_rope, rp = tr.pipeline_rope(Hh * 8, W * 8, F) if rope else (None, None)
        T_, Rr, V = E._dims(case)
        plane = _box_map(s2v, case, height=height).reshape(-1)
        if kind == "const":
            plane = torch.full_like(plane, M.geometric_mean_weight(plane))
        rec = M.MapRecord([(T_, T_ + Rr, [0, 0])], plane, T_ + Rr, T_ + Rr + V)
        _ORACLE[key] = M.mapped_forward(layers, rec, 2, T_ + Rr + V, sd, ocfg, lat.cpu(), H._text(inp, [0]).cpu(), inp["ref"][:1].cpu(),
                                        torch.tensor([799, 799]), rp, ref_rope).double()
    return _ORACLE[key]


# ------------------------------------------------------------------------------------------------ 1. against the mapped oracle
@pytest.mark.parametrize("dt_name", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(S.CASES))
def test_one_mapped_layer_against_the_mapped_oracle_within_twice_the_unsteered_error(s2v, case, dt_name):
    dt = S.DT[dt_name]
    cfg, _ = E._weights(s2v, case)
    plain = E._oracle(s2v, case, [])
    m, eng = E._engine16(s2v, case, dt, 2)
    lat, _ = S._forward_inputs(s2v, case, 2, dt)
    t = torch.tensor([799.0, 799.0])
    base = eng.forward(lat, t)
    err_u = R.rel_l2(base, plain)
    bar = 2 * err_u
    for height in HEIGHTS:   # the first box whose oracles lie four bars apart: chosen from the oracles, before a mapped forward runs
        want = [_oracle(s2v, case, [l], "map", height) for l in range(cfg.num_layers)]
        const1 = _oracle(s2v, case, [1], "const", height)   # on block 1: see the module docstring
        apart = [R.rel_l2(plain, want[0]), R.rel_l2(plain, want[1]), R.rel_l2(const1, want[1]), R.rel_l2(want[0], want[1])]
        if min(apart) >= 4 * bar:
            break
        print(f"MEASURED map {case} {dt_name}: the box of height {height} is not taken, its oracles are {apart[0]:.3e} / {apart[1]:.3e} / {apart[2]:.3e} / "
              f"{apart[3]:.3e} apart, the bar is {bar:.3e}")
    print(f"MEASURED map {case} {dt_name}: box height {height}, un-steered {err_u:.3e}; the oracles are {apart[0]:.3e} / {apart[1]:.3e} (mapped, layers 0 / 1, from un-steered), "
          f"{apart[2]:.3e} (layer 1 from constant-weight), {apart[3]:.3e} (layer 0 from layer 1) apart")
    assert min(apart) >= 4 * bar, f"vacuous: the oracles are {apart} apart, under 4 x the bar {bar:.3e}"
    eng.attn_steer_enable(True)
    plane = _box_map(s2v, case, height=height).reshape(1, -1)
    eng.attn_steer_set_maps(_map_ranges(case), plane)
    assert S._bits(eng.forward(lat, t), base), "an un-armed forward runs today's launches"
    for l in range(cfg.num_layers):
        got = eng.forward(lat, t, steer_layers=[l])
        assert torch.isfinite(got.float()).all()
        err = R.rel_l2(got, want[l])
        print(f"MEASURED map {case} {dt_name} layer {l}: un-steered {err_u:.3e} mapped {err:.3e} (ratio {err / err_u:.2f})")
        assert err <= bar, f"layer {l}: {err:.3e} > 2 x {err_u:.3e}"
        assert S._bits(eng.forward(lat, t), base), "an un-armed forward after an armed one returns the plain bits"
    if dt == torch.bfloat16:
        # constant maps armed equal the scalar-steered armed forward bit for bit (the ranges of the steer engine test: a span on the positive sample,
        # the reference keys on both)
        T, Rr, V = E._dims(case)
        eng.attn_steer_set(E._ranges(case))
        scalar = eng.forward(lat, t, steer_layers=[0])
        assert not S._bits(scalar, base)
        eng.attn_steer_set_maps([(0, 3, [-1, 0]), (T, T + Rr, [1, 1])], torch.stack([torch.full((V,), 2.0 ** -6), torch.full((V,), 64.0)]))
        assert S._bits(eng.forward(lat, t, steer_layers=[0]), scalar), "constant planes: the scalar record's bits"
        ones = torch.ones(1, V)
        eng.attn_steer_set_maps(_map_ranges(case), ones)
        assert S._bits(eng.forward(lat, t, steer_layers=[0, 1]), base), "planes of ones: no wave is live, the un-steered bits (attn_pp beside attn_pp)"
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. launch sequences
@pytest.mark.parametrize("kind,dt_name", [("ddim", "bf16"), ("dpm", "bf16"), ("ddim", "f32")])
def test_armed_steps_eager_captured_new_maps_without_a_new_capture_and_a_change_of_kind(s2v, dt_name, kind):
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

    T, Rr, V = E._dims(case)
    bytes0 = eng.device_bytes()
    plain = step(1, False, None)
    eng.attn_steer_enable(True)
    bytes_on = eng.device_bytes()
    # two videos with a map each (planes 0 and 1 on [negative x 2 | positive x 2])
    ranges = [(T, T + Rr, [0, 1, 0, 1])]
    m1 = torch.stack([_box_map(s2v, case).reshape(-1), _box_map(s2v, case, 1).reshape(-1)])
    m2 = torch.stack([_box_map(s2v, case, 1, 2.0 ** -5, 16.0).reshape(-1), _box_map(s2v, case, 0, 8.0, 0.5).reshape(-1)])
    eng.attn_steer_set_maps(ranges, m1)
    assert eng.device_bytes()[1] > bytes_on[1] and eng.device_bytes()[0] == bytes0[0], "the map table counts as workspace while held"
    eager1 = step(1, False, [1])
    assert not S._bits(eager1, plain)
    assert S._bits(step(1, False, None), plain), "un-armed after armed: the plain bits"
    cap0 = eng.lora_state["graph_captures"]
    assert S._bits(step(1, True, [1]), eager1), "an armed captured step equals the armed eager step"
    assert S._bits(step(1, True, None), plain), "an un-armed step never replays an armed executable"
    assert S._bits(step(1, True, [1]), eager1), "... nor the reverse"
    cap1 = eng.lora_state["graph_captures"]
    assert cap1 == cap0 + 2, "one executable per layer mask: armed and un-armed, each captured once"
    eng.attn_steer_set_maps(ranges, m2)   # the table is data: the replay reads the new maps
    replay2 = step(1, True, [1])
    assert eng.lora_state["graph_captures"] == cap1, "new maps re-capture nothing"
    assert not S._bits(replay2, eager1)
    assert S._bits(replay2, step(1, False, [1])), "the replay at the new maps equals the eager step at the new maps"
    eng.attn_steer_set_maps([(T, T + Rr, [0, 0, 0, 0])], m1[:1])   # fewer planes than the allocation holds: kept in place
    one_plane = step(1, True, [1])
    assert eng.lora_state["graph_captures"] == cap1 and S._bits(one_plane, step(1, False, [1]))
    # a scalar record after maps: the captured steps go, the bits are the scalar record's
    w = E._ranges(case, b)
    eng.attn_steer_set(w)
    scalar_cap = step(1, True, [1])
    assert eng.lora_state["graph_captures"] == cap1 + 1, "the other kind of record drops the captured steps"
    assert S._bits(scalar_cap, step(1, False, [1])) and not S._bits(scalar_cap, one_plane)
    assert eng.device_bytes() == bytes_on, "the map table is freed when a scalar record replaces it"
    # ... and the reverse
    eng.attn_steer_set_maps(ranges, m1)
    again = step(1, True, [1])
    assert eng.lora_state["graph_captures"] == cap1 + 2 and S._bits(again, eager1), "maps after a scalar record: a new capture, the first maps' bits"
    assert S._bits(step(1, True, None), plain)
    eng.attn_steer_enable(False)
    assert eng.device_bytes() == bytes0, "disabling restores s2v_device_bytes"
    assert S._bits(step(1, True, None), plain) and S._bits(step(1, False, None), plain)
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. the library's refusals
def test_every_refusal_of_the_library_refuses_by_name(s2v):
    case, dt = "sincos", torch.bfloat16
    m, eng = S._engine(s2v, case, dt, 2)
    lat, _ = S._forward_inputs(s2v, case, 2, dt)
    t = torch.tensor([500.0, 500.0])
    T, Rr, V = E._dims(case)
    N = T + Rr + V
    two = torch.full((2, V), 2.0)
    ok = [(T, T + Rr, [0, 1])]
    rf = lambda fn, match: E._refused(s2v, fn, match)
    rf(lambda: eng.attn_steer_set_maps(ok, two), r"s2v_attn_steer_set_maps: attention steering is not enabled")
    eng.attn_steer_enable(True)
    rf(lambda: eng.attn_steer_set_maps([(0, 3, [0, 0]), (2, 5, [0, 0])], two), r"s2v_attn_steer_set_maps: key range 1 = \[2, 5\) overlaps or precedes range 0")
    rf(lambda: eng.attn_steer_set_maps([(0, N + 1, [0, 0])], two), rf"s2v_attn_steer_set_maps: key range 0 = \[0, {N + 1}\) must be non-empty and inside \[0, Ntok = {N}\)")
    rf(lambda: eng.attn_steer_set_maps(ok, torch.ones(0, V)), r"1\.\.16 planes are accepted \(n_planes = 0\)")
    rf(lambda: eng.attn_steer_set_maps(ok, torch.ones(17, V)), r"1\.\.16 planes are accepted \(n_planes = 17\)")
    rf(lambda: eng.attn_steer_set_maps([(T, T + Rr, [0, 2])], two), r"plane index 2 of range 0, sample 1 lies outside \[-1, n_planes = 2\)")
    rf(lambda: eng.attn_steer_set_maps([(T, T + Rr, [0, 0, 1])], two), r"range 0 names plane 1 on sample 2, at or beyond B = 2")
    for w, shown in ((float("nan"), "nan"), (0.0, "0"), (2.0 ** 17, "131072"), (2.0 ** -17, r"7\.62939e-06")):
        bad = two.clone()
        bad[1, 7] = w
        rf(lambda: eng.attn_steer_set_maps(ok, bad), rf"s2v_attn_steer_set_maps: plane 1, cell 7: weight {shown} must be finite and inside \[2\^-16, 2\^16\]")
    rf(lambda: eng.attn_steer_set_maps(ok, torch.ones(2, V + 1)), rf"planes must be \[n_planes, V = {V}\]")
    # a refused call replaced nothing: the context still holds the record that steers nothing
    base = eng.forward(lat, t)
    assert S._bits(eng.forward(lat, t, steer_layers=[0]), base)
    eng.attn_steer_set_maps(ok, two)
    rf(lambda: eng.forward(lat, t, steer_layers=[2]), r"s2v_attn_steer_arm: a layer bit at or beyond num_layers is set")
    # what the scalar record is refused with is refused with maps held, by the same entries
    L = s2v._lib
    eng.attn_map_enable(True)
    rf(lambda: eng.forward(lat, t, attn_layers=[0], steer_layers=[0]), r"s2v_attn_steer_arm: an attention map is armed")
    eng.forward(lat, t)   # the refused call left the map's arm behind: this forward takes it
    eng.attn_map_enable(False)
    eng.step_cache_enable(True)
    eng.forward(lat, t, cache="capture")
    rf(lambda: eng.forward(lat, t, cache="reuse", steer_layers=[0]), r"s2v_attn_steer_arm: S2V_STEP_REUSE is armed")
    eng.forward(lat, t)
    eng.step_cache_enable(False)
    hid = torch.zeros(2, V, eng.D, dtype=dt, device=DEV)
    enc = torch.zeros(2, T + Rr, eng.D, dtype=dt, device=DEV)
    L.check(L.lib().s2v_attn_steer_arm(eng._h, 1))
    rf(lambda: eng.attn_forward(0, hid, enc), r"s2v_attn_forward: attention steering is armed")
    assert S._bits(eng.forward(lat, t), base), "a refusing entry takes the arm with it"
    eng.set_attn_p_format("f16")
    rf(lambda: eng.forward(lat, t, steer_layers=[0]), r"s2v_attn_steer_arm: attn_p_format 1 keeps V\^T in fp16")
    eng.set_attn_p_format("bf16")
    # another V: refused by name, steering is left off and its memory freed
    _, T0, F0, Hh, W = S.CASES[case]
    bytes_on = eng.device_bytes()
    rf(lambda: eng.set_geometry(2, T0, F0, 2, 2), rf"s2v_set_geometry \(steering maps\): the held planes have {V} cells, the new geometry has V = {F0} video rows")
    rf(lambda: eng.attn_steer_set_maps(ok, two), r"attention steering is not enabled")
    assert eng.device_bytes()[1] < bytes_on[1]
    eng.close()
    m16, e16 = S._engine(s2v, case, torch.float16, 2)
    rf(lambda: e16.attn_steer_enable(True), r"s2v_attn_steer_enable: an fp16 engine has no steered attention kernel")
    rf(lambda: e16.attn_steer_set_maps(ok, two), r"s2v_attn_steer_set_maps: attention steering is not enabled")
    e16.close()


def test_triples_and_windows_are_refused_by_name_with_maps_held(s2v):
    case, dt = "sincos", torch.bfloat16
    _, T, F, Hh, W = S.CASES[case]
    inp = S._inputs(s2v, case)
    m, eng = S._engine(s2v, case, dt, 2)
    Tt, Rr, V = E._dims(case)
    eng.attn_steer_enable(True)
    eng.attn_steer_set_maps(_map_ranges(case), _box_map(s2v, case).reshape(1, -1))
    L = s2v._lib
    arm = lambda: L.check(L.lib().s2v_attn_steer_arm(eng._h, 1))
    plan = S._plan(s2v, "ddim", dt)
    arm()
    eng.set_windows(F + 2, 2, [1.0] * F)
    long = torch.cat([inp["lat"][:1], inp["lat"][1:2]], dim=1)[:, :F + 2].to(dt).contiguous().clone()
    E._refused(s2v, lambda: eng.denoise_step_windows(long, plan[0][0], plan[0][1]), r"s2v_denoise_step_windows: attention steering is armed")
    E._refused(s2v, arm, r"s2v_attn_steer_arm: temporal windows are set")
    eng.clear_windows()
    eng.set_geometry(6, T, F, Hh, W)   # the same V: the maps are re-made at the new geometry (plane 0 on samples 0 and 1 only)
    eng.prepare_tables(Hh * 8, W * 8)
    eng.set_conditioning(H._text(inp, [0, 1, 2]).to(dt), inp["ref"][:3].to(dt))
    arm()
    eng.set_conditioning_triples(H._text(inp, [0, 1]).to(dt), inp["ref"][:2].to(dt))
    x2 = inp["lat"][:2].to(dt).contiguous().clone()
    E._refused(s2v, lambda: eng.denoise_step(x2, plan[0][0], plan[0][1], subject=True), r"s2v_denoise_step_guided: attention steering is armed")
    E._refused(s2v, arm, r"s2v_attn_steer_arm: the context is conditioned as subject-guidance triples")
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. the pipeline
PH, PW, PF, PT = S.PH, S.PW, S.PF, S.PT
PHp, PWp = PH // 16, PW // 16


def _pipe_map(s2v, F, shift=0, inside=8.0, outside=0.25):
    boxes = [(0.5 * ((f + shift) % 2), 0.0, 0.5 * ((f + shift) % 2) + 0.5, 0.75) for f in range(F)]
    return s2v.box_weight_map(boxes, F, PHp, PWp, inside, outside)


def _hand_driven(s2v, pipe, kind, dt, kw, n, armed, steer):
    """the call's steps by hand through engine.denoise_step: step i steered on steer.layers where i is in `armed`"""
    eng, sch = pipe.transformer.engine, pipe.scheduler
    g = torch.Generator().manual_seed(44)
    x = (kw["latents"].to(DEV) * sch.init_noise_sigma).to(dt).contiguous().clone()
    F = x.shape[1]
    eng.set_geometry(2, PT, F, PH // 8, PW // 8)
    eng.prepare_tables(PH, PW)
    eng.set_conditioning(torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]]), kw["ref_img_states"])
    eng.attn_steer_enable(True)
    ranges, planes, _ = s2v.attention_steer_map_ranges(steer, PT, PHp * PWp, 1, F, PHp, PWp)
    eng.attn_steer_set_maps(ranges, planes)
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
    lat = inp["lat"][:1].to(dt)
    F = lat.shape[1]
    kw = dict(height=PH, width=PW, num_frames=PF, num_inference_steps=6, guidance_scale=6.0, latents=lat, **S._args(s2v, dt))
    gen = lambda: torch.Generator().manual_seed(44)
    base = pipe(generator=gen(), use_graph=True, **kw)["frames"].clone()
    bytes0 = eng.device_bytes()
    ones = s2v.AttentionSteer([0, 1], subject_map=torch.ones(F, PHp, PWp), text_spans=[(0, 2, 1.0)], text_span_maps=[np.ones((F, PHp, PWp), dtype=np.float32)])
    assert S._bits(pipe(generator=gen(), use_graph=True, attention_steer=ones, **kw)["frames"], base), "maps of ones: the plain call's bits"
    assert pipe.attention_steer_report["steps"] == [] and pipe.attention_steer_report["planes"] == 0
    st = s2v.AttentionSteer([1, 0], steps=[1, 4, 5], subject_map=_pipe_map(s2v, F), text_spans=[(0, 2, 0.125), (2, 5, 1.0)],
                            text_span_maps=[None, _pipe_map(s2v, F, 1, 4.0, 1.0)])
    got = pipe(generator=gen(), use_graph=True, attention_steer=st, **kw)["frames"].clone()
    assert not S._bits(got, base) and torch.isfinite(got.float()).all()
    rep = pipe.attention_steer_report
    assert rep["steps"] == [1, 4, 5] and rep["layers"] == [1, 0] and rep["planes"] == 3 and rep["mapped"] == [False, True, True]
    assert rep["ranges"] == [(0, 2, [-1, 0]), (2, 5, [-1, 1]), (PT, PT + 24, [2, 2])] and 0.0 < rep["live_wave_share"] <= 1.0
    assert eng.device_bytes() == bytes0, "steering is disabled when the call ends"
    assert S._bits(pipe(generator=gen(), use_graph=False, attention_steer=st, **kw)["frames"], got), "captured == eager"
    assert S._bits(_hand_driven(s2v, pipe, kind, dt, kw, 6, {1, 4, 5}, st), got), "the pipeline is the hand-driven armed steps"
    assert S._bits(pipe(generator=gen(), use_graph=True, **kw)["frames"], base), "the plain call afterwards"
    eng.close()


def test_pipeline_two_videos_with_their_own_maps_and_a_mask_together_with_maps(s2v):
    dt, kind = torch.bfloat16, "ddim"
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, kind, dt, vae)
    F = (H.VF - 1) // 4 + 1
    kw = dict(height=PH, width=PW, num_frames=H.VF, num_inference_steps=4, guidance_scale=6.0, use_graph=True, output_type="latent")
    maps = [_pipe_map(s2v, F), _pipe_map(s2v, F, 1, 0.125, 16.0)]
    steer = lambda m: s2v.AttentionSteer([0, 1], steps=[0, 2, 3], subject_map=m, text_spans=[(1, 4, 0.25)])
    both = pipe(generator=H._gens(range(2)), attention_steer=steer(torch.stack(maps)), **S._args(s2v, dt, (0, 1)), **kw)["frames"].clone()
    assert pipe.attention_steer_report["ranges"] == [(1, 4, [-1, -1, 0, 0]), (PT, PT + 24, [1, 2, 1, 2])] and pipe.attention_steer_report["planes"] == 3
    plain = pipe(generator=H._gens(range(2)), **S._args(s2v, dt, (0, 1)), **kw)["frames"]
    assert not S._bits(both, plain)
    for k in range(2):
        one = pipe(generator=H._gens([k])[0], attention_steer=steer(maps[k]), **S._args(s2v, dt, (k,)), **kw)["frames"]
        # tiny-rope runs no split-K GEMM at either batch size (tests/test_gpu_step_cache.py holds the latents of such calls to bits)
        assert S._bits(both[k:k + 1], one), f"video {k} differs from its one-video call with its own map"
    swapped = pipe(generator=H._gens(range(2)), attention_steer=steer(torch.stack(maps[::-1])), **S._args(s2v, dt, (0, 1)), **kw)["frames"]
    assert not S._bits(swapped[:1], both[:1]), "the map of the other video gives other bits"
    # mask= together with maps: the kept cells are the input's, the repainted ones differ from the un-steered call's
    mask = torch.zeros(1, H.VF, PH, PW)
    mask[:, :, :, PW // 2:] = 1.0
    mk = dict(video=H._videos(1), mask=mask, strength=0.75, **kw)
    st = s2v.AttentionSteer([0, 1], steps=[0, 2], subject_map=maps[0])   # strength 0.75 of 4 steps runs 3
    a = pipe(generator=H._gens([0])[0], attention_steer=st, **mk, **S._args(s2v, dt, (0,)))["frames"].clone()
    b = pipe(generator=H._gens([0])[0], **mk, **S._args(s2v, dt, (0,)))["frames"]
    w = a.shape[-1]
    assert S._bits(a[..., : w // 2], b[..., : w // 2]), "kept cells: the clean input latents in both calls"
    assert not S._bits(a[..., w // 2:], b[..., w // 2:]) and torch.isfinite(a.float()).all()
    pipe.transformer.engine.close()
