"""Steering maps, the parts that need no GPU: the CPU emulation of attn_pp<MAP> (per-lane addends, liveness skipping) against the fp64
restatement, six mutated emulations that must fail it, the library's liveness table against brute force, box_weight_map against a hand-written
grid, the plane layout and every refusal of the pipeline, the loop with a recording engine, "all ones arms nothing", and the new symbols with
their host-side refusals."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_steer_map_ref as M
import attn_steer_ref as R
from test_attn_steer_cpu import _Engine, _args, _pipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECS = M.map_records()
# the un-steered launch's own error at this shape (tests/test_gpu_attn_steer.py, measured): impl 0 2.3e-03, so a bar of 2 x is 4.6e-03 and "four
# bars apart" 1.9e-02.  The CPU check asks for 5e-02, so the GPU test's condition holds with room
APART = 5e-2


def _bar(ref):
    return R.EMU_BAR * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
@pytest.mark.parametrize("name", sorted(RECS))
def test_the_emulation_with_per_lane_addends_and_liveness_skipping_equals_the_restatement(name):
    c, rec = R.case("randn"), RECS[name]
    ref = M.map_reference(c, "bf16", rec)
    err = (M.emulate_maps(c, "bf16", rec).double() - ref).abs().max().item()
    assert err <= _bar(ref), f"{name}: {err:.3e} > {_bar(ref):.3e}"


def test_the_restatement_is_the_brute_force_loop():
    c = R.case("randn", "bf16", (2, 2, 31))
    rec = M.MapRecord([(0, 3, [0, -1]), (7, 20, [1, 0])], torch.stack([M.pow2_plane(24, 1), M.pow2_plane(24, 2)]), 5, 29)
    ref = M.map_reference(c, "natural", rec).reshape(2, 31, 2, 64)
    q, k, v = (c.heads(p) for p in range(3))
    for b in range(2):
        for i in (0, 5, 17, 28, 30):
            s = (q[b, 0, i] * 0.125) @ k[b, 0].T
            for r, (k0, k1, _) in enumerate(rec.ranges):
                p = rec.plane(r, b)
                if p >= 0 and 5 <= i < 29:
                    s[k0:k1] += float(torch.log(rec.planes[p, i - 5].double()))
            want = torch.softmax(s, dim=-1) @ v[b, 0]
            assert (ref[b, i, 0] - want).abs().max().item() < 1e-12
    got = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=M.beta_maps(rec, 2, 31)[:, None])
    assert (got.transpose(1, 2).reshape(62, 128) - M.map_reference(c, "natural", rec)).abs().max().item() < 1e-12


def test_a_constant_plane_restates_the_scalar_record():
    c = R.case("randn")
    for name, srec in R.range_sets().items():
        assert torch.equal(M.map_reference(c, "bf16", M.constant_record(srec)), R.steered_reference(c, "bf16", srec)), name


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_every_mutation_of_the_emulation_fails_a_check_the_emulation_passes(mutation):
    c = R.case("randn")
    failed = []
    for name, rec in RECS.items():
        ref = M.map_reference(c, "bf16", rec)
        if (M.emulate_maps(c, "bf16", rec, mutation).double() - ref).abs().max().item() > _bar(ref):
            failed.append(name)
    print(f"{mutation}: caught on {failed}")
    expect = {"other_sample_plane": "plane_per_sample", "row_off_by_one": "inside_one_tile", "plane_from_row_0": "query_range",
              "live_from_first_row": "liveness", "natural_log": "first_tile", "planes_swapped": "four_ranges_four_planes"}[mutation]
    assert expect in failed, f"{mutation} must fail on the record built for it ({expect}); it failed on {failed}"
    if mutation == "other_sample_plane":
        assert "sample_1_off" in failed
    if mutation in ("plane_from_row_0", "live_from_first_row", "planes_swapped", "other_sample_plane"):
        assert "inside_one_tile" not in failed, "a mutation that a one-plane, whole-range record cannot see"


def test_the_mapped_answers_are_far_from_the_unsteered_and_the_constant_plane_answers():
    """the condition of the GPU test, on the CPU: a kernel that ignores the cell (no bias, or one weight for every row) cannot pass"""
    c = R.case("randn")
    plain = R.steered_reference(c, "bf16", None)
    for name, rec in RECS.items():
        if name == "liveness":
            continue
        rows = rec.steered_rows(c.B, c.N).reshape(-1)
        ref = M.map_reference(c, "bf16", rec)
        gm = M.MapRecord(rec.ranges, torch.stack([torch.full_like(p, M.geometric_mean_weight(p)) for p in rec.planes]), rec.q0, rec.q1)
        d_plain, d_const = R.rel_l2(plain, ref, rows), R.rel_l2(M.map_reference(c, "bf16", gm), ref, rows)
        print(f"{name}: {d_plain:.3e} from the un-steered answer, {d_const:.3e} from the constant plane at the geometric mean")
        assert d_plain >= APART and d_const >= APART, name


# ------------------------------------------------------------------------------------------------ the liveness table
def _lib_flags(L, rec, N):
    nqb = (N + 255) // 256
    pl = (ctypes.c_int8 * 32)(*[rec.plane(r, b) if r < len(rec.ranges) else -1 for r in range(4) for b in range(8)])
    w = np.ascontiguousarray(rec.planes.numpy())
    out = np.full((8, 8 * nqb), -1, dtype=np.int32)
    L.check(L.lib().s2v_attn_steer_map_wave_flags(len(rec.ranges), rec.q0, rec.q1, N, pl, w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return torch.from_numpy(out)


def test_the_librarys_liveness_table_equals_brute_force(s2v):
    L = s2v._lib
    recs = dict(RECS)
    recs.update({f"constant {k}": M.constant_record(v) for k, v in R.range_sets().items()})
    ones = M.MapRecord([(60, 200, [0, 0])], torch.ones(330), 0, 330)
    recs["all ones"] = ones
    for name, rec in recs.items():
        assert torch.equal(_lib_flags(L, rec, 330), M.wave_flags_bruteforce(rec, 330)), name
    assert int(_lib_flags(L, ones, 330).abs().sum()) == 0
    f = _lib_flags(L, RECS["liveness"], 330)
    assert f[0, 2] == 0 and f[0, 1] == 1 and (f[:2, 8:] == 0).all() and (f[2:] == 0).all(), "rows [64, 96) and item 1 are dead; wave 1 lives by its other rows"
    q = _lib_flags(L, RECS["query_range"], 330)
    assert q[0, 0] == 0 and q[0, 1] == 1 and q[0, 9] == 1 and q[0, 10] == 0, "waves outside [37, 300)"
    # a long record: the ragged last wave and several items
    big = M.MapRecord([(3, 9, [-1, 0]), (226, 1576, [1, 1])], torch.stack([M.pow2_plane(3124, 3), torch.cat([torch.ones(1500), M.pow2_plane(1624, 4)])]), 1576, 4700)
    assert torch.equal(_lib_flags(L, big, 4700), M.wave_flags_bruteforce(big, 4700))


# ------------------------------------------------------------------------------------------------ box_weight_map
def test_box_weight_map_against_a_hand_written_grid(s2v):
    box = s2v.box_weight_map
    # 4 x 4 cells, centres at .125 .375 .625 .875: x in [.375, .75) takes the centres .375 (an edge ON a centre: inside) and .625; y in [.125, .625)
    # takes .125 and .375 -- .625 is the open end, outside
    got = box((0.375, 0.125, 0.75, 0.625), 2, 4, 4, 8.0, 0.5)
    want = torch.tensor([[.5, 8, 8, .5], [.5, 8, 8, .5], [.5, .5, .5, .5], [.5, .5, .5, .5]])
    assert got.dtype == torch.float32 and got.shape == (2, 4, 4) and torch.equal(got[0], want) and torch.equal(got[1], want)
    moving = box([(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 1.0, 1.0)], 2, 2, 4, 64.0)
    assert torch.equal(moving[0], torch.tensor([[64., 64, 1, 1]] * 2)) and torch.equal(moving[1], torch.tensor([[1., 1, 64, 64]] * 2))
    assert torch.equal(box((0, 0, 1, 1), 1, 3, 5, 2.0), torch.full((1, 3, 5), 2.0))
    for bad in ((0.5, 0.0, 0.5, 1.0), (0.6, 0.0, 0.5, 1.0), (-0.1, 0.0, 0.5, 1.0), (0.0, 0.0, 0.5, 1.1)):
        with pytest.raises(ValueError, match=r"0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1"):
            box(bad, 2, 4, 4, 8.0)
    with pytest.raises(ValueError, match=r"3 boxes for 2 latent frames"):
        box([(0, 0, 1, 1)] * 3, 2, 4, 4, 8.0)


# ------------------------------------------------------------------------------------------------ the plane layout of a call
def test_the_planes_and_ranges_of_a_call(s2v):
    A, ranges = s2v.AttentionSteer, s2v.attention_steer_map_ranges
    T, F, Hp, Wp = 7, 2, 2, 3
    Rr, V = Hp * Wp, F * Hp * Wp
    m1 = torch.arange(1, V + 1, dtype=torch.float32).reshape(F, Hp, Wp)
    r, p, mp = ranges(A([0], subject_map=m1), T, Rr, 1, F, Hp, Wp)
    assert r == [(7, 13, [0, 0])] and mp == [True] and p.shape == (1, V) and p[0].tolist() == list(range(1, V + 1)), "cell (f Hp + y) Wp + x"
    # two videos with their own subject maps; a scalar span rides along as a constant plane on the positive samples; a span map on them as well
    m2 = torch.stack([m1, 2 * m1])
    sm = torch.full((F, Hp, Wp), 4.0)
    r, p, mp = ranges(A([0], subject_map=m2, text_spans=[(3, 5, 1.0), (0, 2, 0.25)], text_span_maps=[sm, None]), T, Rr, 2, F, Hp, Wp)
    assert r == [(0, 2, [-1, -1, 0, 0]), (3, 5, [-1, -1, 1, 1]), (7, 13, [2, 3, 2, 3])] and mp == [False, True, True]
    assert p.shape == (4, V) and (p[0] == 0.25).all() and (p[1] == 4).all() and np.array_equal(p[3], 2 * p[2])
    # ranges whose weights are all 1 are left out; all of them: nothing
    r, p, mp = ranges(A([0], subject_map=torch.ones(F, Hp, Wp), text_spans=[(0, 2, 3.0)]), T, Rr, 1, F, Hp, Wp)
    assert r == [(0, 2, [-1, 0])] and mp == [False]
    assert ranges(A([0], subject_map=torch.ones(F, Hp, Wp), text_spans=[(0, 2, 1.0)], text_span_maps=[np.ones((F, Hp, Wp))]), T, Rr, 1, F, Hp, Wp) == ([], None, [])
    with pytest.raises(ValueError, match=r"`subject_map` together with a scalar weight 2.0 on the same keys: one or the other"):
        ranges(A([0], subject=2.0, subject_map=m1), T, Rr, 1, F, Hp, Wp)
    with pytest.raises(ValueError, match=r"the map of text span \(0, 2\) together with a scalar weight"):
        ranges(A([0], text_spans=[(0, 2, 3.0)], text_span_maps=[sm]), T, Rr, 1, F, Hp, Wp)
    with pytest.raises(ValueError, match=r"`text_span_maps` has 2 entries for 1 text spans"):
        ranges(A([0], text_spans=[(0, 2, 1.0)], text_span_maps=[sm, sm]), T, Rr, 1, F, Hp, Wp)
    with pytest.raises(ValueError, match=r"`subject_map` has the shape \(2, 2, 2, 3\); a map is \[F_lat, Hp, Wp\] = \(2, 2, 3\) or one per video"):
        ranges(A([0], subject_map=m2), T, Rr, 3, F, Hp, Wp)
    for bad in (0.0, 2.0 ** 17, 2.0 ** -17, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"the weights of `subject_map` must be finite and inside \[2\^-16, 2\^16\]"):
            ranges(A([0], subject_map=torch.full((F, Hp, Wp), bad)), T, Rr, 1, F, Hp, Wp)
    with pytest.raises(ValueError, match=r"reaches beyond the 7 prompt tokens"):
        ranges(A([0], text_spans=[(5, 8, 1.0)], text_span_maps=[sm]), T, Rr, 1, F, Hp, Wp)
    with pytest.raises(ValueError, match=r"`attention_steer` with maps in a call of 5 videos: a plane index is held for 8 samples"):
        ranges(A([0], subject_map=m1), T, Rr, 5, F, Hp, Wp)
    with pytest.raises(ValueError, match=r"attention_steer_live_share: at most four ranges, each with a plane index for at most 8 samples"):
        s2v.attention_steer_live_share([(7, 13, [0] * 10)], np.ones((1, V), dtype=np.float32), T + Rr, T + Rr + V, 8)
    with pytest.raises(ValueError, match=r"overlap"):
        ranges(A([0], text_spans=[(0, 4, 1.0), (3, 5, 2.0)], text_span_maps=[sm, None]), T, Rr, 1, F, Hp, Wp)


def test_every_refusal_of_a_mapped_call_names_its_argument_and_leaves_the_engine_alone(s2v):
    """what `attention_steer=` refuses stays refused by name when the object carries maps"""
    eng = _Engine()
    pipe = _pipe(s2v, eng)
    four, one = _args()
    st = s2v.AttentionSteer([0, 2], subject_map=s2v.box_weight_map((0, 0, 0.5, 0.5), 2, 4, 6, 8.0))
    for name, val in (("attention_map", s2v.AttentionMap([0])), ("step_cache", 0.1), ("subject_guidance_scale", 2.0),
                      ("temporal_windows", s2v.TemporalWindows(13, 8))):
        with pytest.raises(ValueError, match=rf"`attention_steer` together with `{name}`"):
            pipe(attention_steer=st, **{name: val}, **one)
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=rf"`attention_steer` together with `{name}`"):
            pipe(attention_steer=st, **{name: object()}, **one)
    with pytest.raises(ValueError, match=r"`attention_steer` together with fused=False"):
        pipe(attention_steer=st, fused=False, **one)
    for lists in (dict(guidance_scale=[3.0, 4.0, 5.0, 6.0]), dict(num_inference_steps=[3, 3, 3, 3]), dict(strength=[0.5] * 4)):
        with pytest.raises(ValueError, match=r"`attention_steer` together with per-video lists"):
            pipe(attention_steer=st, **lists, **four)
    with pytest.raises(ValueError, match=r"`attention_steer` with an fp16 engine"):
        _pipe(s2v, eng, torch.float16)(attention_steer=st, **one)
    for wf in ("fp8", "fp8-qk", "fp8-auto"):
        with pytest.raises(ValueError, match=rf"`attention_steer` with weight_format '{wf}'"):
            _pipe(s2v, eng, weight_format=wf)(attention_steer=st, **one)
    with pytest.raises(ValueError, match=r"`local_attention` together with `attention_steer`: a layer runs one attention kernel, the steered or the local one"):
        pipe(attention_steer=st, local_attention=s2v.LocalAttention([1], 0), **one)
    assert pipe.attention_steer_report is None


class _Recording:
    """an engine that records the steer entries and the armed layers of every step of a fused DDIM call"""

    def __init__(self):
        self.calls, self.sets, self.geometry, self.fp8_qk_active = [], [], None, False
        self.cfg, self.attn_p_format = SimpleNamespace(attn_p_format="bf16"), "bf16"

    def set_geometry(self, B, T, F, H, W):
        self.geometry = (B, T, F, H, W)

    def prepare_tables(self, *a):
        pass

    def set_conditioning(self, *a):
        pass

    def attn_steer_enable(self, on=True):
        self.sets.append(("enable", bool(on)))

    def attn_steer_set_maps(self, ranges, planes):
        self.sets.append(("maps", list(ranges), np.array(planes)))

    def denoise_step(self, latents, *a, **kw):
        self.calls.append(kw.get("steer_layers"))

    def __getattr__(self, name):
        raise AssertionError(f"the call reached the engine entry {name}")


def _recorded(s2v, steer, videos=1):
    eng = _Recording()
    pipe = _pipe(s2v, eng)
    pipe.transformer.config.in_channels = 16
    pipe.transformer.config.use_rotary_positional_embeddings = False
    four, one = _args()
    kw = dict(one if videos == 1 else four, num_inference_steps=4, latents=torch.zeros(videos, 2, 16, 8, 12), output_type="latent")
    pipe(attention_steer=steer, **kw)
    return eng, pipe


def test_the_loop_sets_and_arms_exactly_the_planned_steps_and_layers(s2v):
    m = s2v.box_weight_map([(0, 0, 0.5, 0.5), (0.5, 0.5, 1, 1)], 2, 4, 6, 8.0)
    eng, pipe = _recorded(s2v, s2v.AttentionSteer([1, 3], steps=[0, 2], subject_map=m, text_spans=[(0, 2, 3.0)]))
    assert eng.calls == [[1, 3], None, [1, 3], None]
    assert [s[0] for s in eng.sets] == ["enable", "maps", "enable"] and eng.sets[0][1] is True and eng.sets[-1][1] is False
    _, ranges, planes = eng.sets[1]
    T, Rr = 5, 24
    assert ranges == [(0, 2, [-1, 0]), (T, T + Rr, [1, 1])] and planes.shape == (2, 48) and (planes[0] == 3.0).all()
    assert np.array_equal(planes[1], m.reshape(-1).numpy())
    rep = pipe.attention_steer_report
    assert rep["steps"] == [0, 2] and rep["layers"] == [1, 3] and rep["planes"] == 2 and rep["mapped"] == [False, True] and rep["ranges"] == ranges
    # Ntok = 5 + 24 * 3 = 77: three waves a sample; the video rows [29, 77) touch all of them, and the constant span plane is live wherever a row is
    assert rep["live_wave_share"] == 1.0
    # the map alone, ones outside a box in frame 0: wave 0 (rows 0 .. 31) holds the video rows 29, 30, 31 = cells 0, 1, 2 (inside the box), wave 1
    # the cells 3 .. 34 (cell 6 is inside), wave 2 the cells 35 .. 47, all of frame 1 and all 1: two of three waves a sample are live
    only = s2v.box_weight_map([(0, 0, 0.5, 0.5), (0, 0, 0.5, 0.5)], 2, 4, 6, 8.0)
    only[1] = 1.0
    eng, pipe = _recorded(s2v, s2v.AttentionSteer([0], subject_map=only))
    assert pipe.attention_steer_report["live_wave_share"] == pytest.approx(2 / 3) and eng.calls == [[0]] * 4


def test_per_video_maps_in_a_batched_call_with_scalars(s2v):
    m = torch.stack([s2v.box_weight_map((0, 0, 0.5, 1), 2, 4, 6, 8.0), s2v.box_weight_map((0.5, 0, 1, 1), 2, 4, 6, 0.25)] * 2)
    eng, pipe = _recorded(s2v, s2v.AttentionSteer([2], subject_map=m), videos=4)
    _, ranges, planes = eng.sets[1]
    assert ranges == [(5, 29, [0, 1, 2, 3, 0, 1, 2, 3])] and planes.shape == (4, 48) and eng.geometry[0] == 8
    assert pipe.attention_steer_report["planes"] == 4


def test_all_ones_maps_arm_nothing(s2v):
    eng, pipe = _recorded(s2v, s2v.AttentionSteer([0, 1], subject_map=torch.ones(2, 4, 6), text_spans=[(0, 2, 1.0)], text_span_maps=[torch.ones(2, 4, 6)]))
    assert eng.calls == [None] * 4 and eng.sets == [], "no steer entry, no steer_layers: the launches of the call without the argument"
    assert pipe.attention_steer_report == {"steps": [], "layers": [], "ranges": [], "planes": 0, "mapped": [], "live_wave_share": 0.0}


def test_an_object_without_maps_takes_the_scalar_path(s2v):
    class _Scalar(_Recording):
        def attn_steer_set(self, ranges):
            self.sets.append(("scalar", list(ranges)))

        def attn_steer_set_maps(self, *a):
            raise AssertionError("a call without maps reached attn_steer_set_maps")

    eng = _Scalar()
    pipe = _pipe(s2v, eng)
    pipe.transformer.config.in_channels = 16
    pipe.transformer.config.use_rotary_positional_embeddings = False
    _, one = _args()
    pipe(attention_steer=s2v.AttentionSteer([0], subject=2.0), num_inference_steps=2, latents=torch.zeros(1, 2, 16, 8, 12), output_type="latent", **one)
    assert eng.sets[1] == ("scalar", [(5, 29, 2.0, 0b11)]) and pipe.attention_steer_report == {"steps": [0, 1], "layers": [0], "ranges": [(5, 29, 2.0, 3)]}


# ------------------------------------------------------------------------------------------------ symbols and host-side refusals
NEW = ["s2v_attn_steer_set_maps", "s2v_op_attention_steer_map", "s2v_attn_steer_map_wave_flags"]


def test_the_new_entries_are_declared_bound_and_exported_and_refuse_by_name(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib, L = s2v.lib(), s2v._lib
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert name in L._SIGS, f"{name} is not bound"
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.s2v_attn_steer_set_maps(None, 0, None, 1, None) != 0 and b"s2v_attn_steer_set_maps: null context" in lib.s2v_last_error()
    assert lib.s2v_op_attention_steer_map(None, None, None, 1, 1, 1, 1, 0, None, None, None) != 0
    assert b"s2v_op_attention_steer_map: null argument" in lib.s2v_last_error()
    assert ctypes.sizeof(L.SteerMapRangeC) == 16 and ctypes.sizeof(L.SteerMapRecordC) == 80
    for name in ("box_weight_map", "attention_steer_map_ranges", "attention_steer_live_share"):
        assert hasattr(s2v, name)
    assert hasattr(s2v.S2VEngine, "attn_steer_set_maps")


def test_the_operator_entry_refuses_a_bad_record_by_name_before_it_touches_the_device(s2v):
    lib, L = s2v.lib(), s2v._lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(rec, match, N=330, B=2, dtype=L.DTYPE_BF16, impl=0, n_planes=None, planes=True):
        r, pp, keep = rec.c(L, n_planes)
        assert lib.s2v_op_attention_steer_map(p, p, p, B, 2, N, dtype, impl, ctypes.byref(r), pp if planes else None, None) != 0
        msg = lib.s2v_last_error().decode()
        assert re.search(match, msg), msg

    two = torch.full((2, 330), 2.0)
    ok = M.MapRecord([(70, 100, [0, 1])], two, 0, 330)
    refused(ok, r"1\.\.16 planes are accepted \(n_planes = 0\)", n_planes=0)
    refused(ok, r"1\.\.16 planes are accepted \(n_planes = 17\)", n_planes=17)
    refused(M.MapRecord([(70, 100, [0, 2])], two, 0, 330), r"plane index 2 of range 0, sample 1 lies outside \[-1, n_planes = 2\)")
    refused(M.MapRecord([(70, 100, [-2, 0])], two, 0, 330), r"plane index -2 of range 0, sample 0 lies outside")
    refused(M.MapRecord([(70, 100, [0, 0, 1])], two, 0, 330), r"range 0 names plane 1 on sample 2, at or beyond B = 2")
    refused(ok, r"null plane pointer", planes=False)
    for w, shown in ((float("nan"), "nan"), (0.0, "0"), (2.0 ** -17, r"7\.62939e-06"), (2.0 ** 17, "131072"), (float("inf"), "inf"), (-2.0, "-2")):
        bad = two.clone()
        bad[1, 217] = w
        refused(M.MapRecord([(70, 100, [0, 1])], bad, 0, 330), rf"plane 1, cell 217: weight {shown} must be finite and inside \[2\^-16, 2\^16\] \(no w = 0\)")
    refused(M.MapRecord([(70, 100, [0, 0]), (90, 120, [0, 0])], two, 0, 330), r"key range 1 = \[90, 120\) overlaps or precedes range 0")
    refused(M.MapRecord([(300, 331, [0, 0])], two, 0, 330), r"key range 0 = \[300, 331\) must be non-empty and inside \[0, Ntok = 330\)")
    refused(M.MapRecord([(70, 100, [0, 0])], torch.full((2, 331), 2.0), 0, 331), r"the query range \[0, 331\) must be non-empty and lie inside \[0, Ntok = 330\)")
    refused(ok, r"impl 0 is bf16 and needs vt_scratch", dtype=L.DTYPE_F32)
    refused(ok, r"1 <= B <= 8", B=9)
    refused(ok, r"impl 0 \(MFMA, bf16\), 1 \(generic\) or 2 \(MFMA, bf16, the persistent launch\)", impl=3)
    refused(ok, r"impl 0 is bf16 and needs vt_scratch \(and so is impl 2\)", dtype=L.DTYPE_F32, impl=2)
    r, pp, keep = ok.c(L)
    r.n = 5
    assert lib.s2v_op_attention_steer_map(p, p, p, 2, 2, 330, L.DTYPE_BF16, 0, ctypes.byref(r), pp, None) != 0
    assert b"0..4 key ranges are accepted (n = 5)" in lib.s2v_last_error()
