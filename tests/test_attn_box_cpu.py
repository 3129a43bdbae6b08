"""Local attention in space and time, the parts that need no GPU: the restatement against F.scaled_dot_product_attention with a boolean mask, the
table and the plan (the package's and the restatement's, against each other and against a brute-force count from the visibility matrix), a CPU
emulation of attn_pp<BOX>'s visit-list + whole-bit + per-lane-mask algorithm that meets the restatement (and seven mutated emulations that must
not), validation of LocalAttention(rows=), the refusals of the pipeline with an engine that must not be reached, the loop with a recording
engine, "rows=None and rows >= Hp - 1 take today's path", and the new symbols of the built library with the table refusals of the operator
entry."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

import attn_box_ref as X
import attn_local_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = X.tables()


def _bar(ref):
    return X.EMU_BAR * max(1.0, ref.abs().max().item())


def _package_plan(s2v, tab):
    """the package's visit lists for the table: what the tests below hold the restatement's and the emulation's against, so that each of them
    goes through the package"""
    return s2v.local_attention_box_items(tab.P, tab.S, tab.lo, tab.hi, tab.olo, tab.ohi)


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_is_sdpa_with_a_boolean_mask_and_full_offsets_are_the_window_table(s2v):
    c = X.case("randn")
    q, k, v = (c.heads(p) for p in range(3))
    for name in ("f1r1", "hidden_end_seen_start", "empty_boxes", "P100"):
        tab = TABLES[name]
        # the package's plan visits a tile exactly when the restatement's mask shows some row of the item a key of it (or it is a prefix tile)
        assert _package_plan(s2v, tab) == X.brute_visits(tab), name
        got = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=X.visible(tab)[None, None], dropout_p=0.0, is_causal=False)
        assert (got.transpose(1, 2).reshape(2 * X.N0, 128) - X.box_reference(c, "natural", tab)).abs().max().item() < 1e-12, name
    for w in (0, 1, 4):
        loc = R.frames_table(R.T_, R.R_, R.F_, R.S_, w)
        assert torch.equal(X.visible(X.from_local(loc, X.S_)), R.visible(loc))
        assert torch.equal(X.visible(X.box_table(X.T_, X.R_, X.F_, X.HP_, X.WP_, w, X.HP_ - 1)), R.visible(loc)), "rows = Hp - 1 sees every patch row"
    # the definition, key by key, on one row of the pipeline's family: frame 2, patch row 4 -> frames 1 .. 3, patch rows 3 .. 5
    tab, i = TABLES["f1r1"], X.P0 + 2 * X.S_ + 4 * X.WP_ + 7
    want = set(range(X.P0)) | {X.P0 + f * X.S_ + y * X.WP_ + x for f in (1, 2, 3) for y in (3, 4, 5) for x in range(X.WP_)}
    assert set(torch.nonzero(X.visible(tab)[i]).flatten().tolist()) == want


# ------------------------------------------------------------------------------------------------ the table and the plan
def test_the_table_and_the_plan_of_the_package_equal_the_restatement_and_a_brute_force_count(s2v):
    for w, r in ((0, 0), (1, 1), (1, 3), (X.F_, 1), (2, 9), (9, 20)):
        tab = X.box_table(X.T_, X.R_, X.F_, X.HP_, X.WP_, w, r)
        got = s2v.local_attention_box_table(X.T_, X.R_, X.F_, X.HP_, X.WP_, w, r)
        assert got == (tab.P, tab.S, tab.lo, tab.hi, tab.olo, tab.ohi)
        assert s2v.local_attention_box_items(*got) == X.visits(tab) == X.brute_visits(tab)
        assert s2v.local_attention_box_share(*got) == X.share(tab) == X.brute_share(tab)
    for name, tab in TABLES.items():
        v = X.visits(tab)
        assert v == X.brute_visits(tab), name
        assert s2v.local_attention_box_items(tab.P, tab.S, tab.lo, tab.hi, tab.olo, tab.ohi) == v, name
        assert all(x[0] == 0 and x == sorted(set(x)) for x in v), "iteration 0 is tile 0; ascending"
    # one run per frame: the last item (rows 768, 769: patch row 9) sees the offsets [120, 150) of each of the five frames
    assert X.visits(TABLES["allframes_r1"])[3] == [0, 2, 4, 6, 7, 9, 11, 12]
    # full offsets: the two visit lists coincide on every window table of the pipeline's family
    for w in range(5):
        loc = R.frames_table(R.T_, R.R_, R.F_, R.S_, w)
        assert X.visits(X.from_local(loc, X.S_)) == R.visits(loc), f"frames = {w}"
    # the headline geometry, T / R / F / S = 226 / 1350 / 13 / 1350 with 30 patch rows of 45 cells
    for w, shares in ((1, (0.253, 0.272, 0.293)), (2, (0.302, 0.333, 0.366)), (13, (0.546, 0.639, 0.725))):
        for r, want in zip((3, 5, 7), shares):
            assert round(s2v.local_attention_box_share(*s2v.local_attention_box_table(226, 1350, 13, 30, 45, w, r)), 3) == want
    for bad in (dict(T=0, R=0), dict(F=0), dict(Hp=0), dict(Wp=0), dict(frames=-1), dict(rows=-1)):
        kw = dict(dict(T=5, R=15, F=5, Hp=10, Wp=15, frames=1, rows=1), **bad)
        with pytest.raises(ValueError, match=r"local attention: T \+ R >= 1, F >= 1, Hp >= 1, Wp >= 1, frames >= 0 and rows >= 0 are required"):
            s2v.local_attention_box_table(**kw)


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
@pytest.mark.parametrize("family", ["randn", "sharp"])
def test_the_emulation_of_the_visit_list_algorithm_meets_the_restatement(s2v, family):
    c = X.case(family)
    for name, tab in TABLES.items():
        assert _package_plan(s2v, tab) == X.visits(tab), f"{name}: the emulation walks the package's visit lists"
        ref = X.box_reference(c, "bf16", tab)
        err = (X.emulate(c, "bf16", tab).double() - ref).abs().max().item()
        assert err <= _bar(ref), f"{family} {name}: {err:.3e} > {_bar(ref):.3e}"


def test_with_full_offsets_the_emulation_is_the_window_emulation_bit_for_bit(s2v):
    c = X.case("randn")
    for w in (0, 1):
        loc = R.frames_table(R.T_, R.R_, R.F_, R.S_, w)
        assert _package_plan(s2v, X.from_local(loc, X.S_)) == R.visits(loc), f"frames = {w}: the package's box plan is the window plan"
        assert torch.equal(X.emulate(c, "bf16", X.from_local(loc, X.S_)), R.emulate(c, "bf16", loc)), f"frames = {w}"


def test_the_box_answer_is_far_from_the_dense_and_from_the_temporal_one(s2v):
    c = X.case("randn")
    f1r1 = s2v.local_attention_box_table(X.T_, X.R_, X.F_, X.HP_, X.WP_, 1, 1)
    assert X.BoxTable(*f1r1).key() == TABLES["f1r1"].key(), "the tables compared below are the pipeline's family, as the package builds it"
    for name, tab in TABLES.items():
        box = X.box_reference(c, "bf16", tab)
        d = X.rel_l2(R.local_reference(c, "bf16", None), box, tab.windowed_rows().repeat(c.B))
        t = X.rel_l2(R.local_reference(c, "bf16", tab.temporal()), box, tab.narrowed_rows().repeat(c.B))
        print(f"randn {name}: the box restatement is {d:.3e} from the dense and {t:.3e} from the temporal one")
        assert d >= 0.2 and t >= 0.2, "four bars of the GPU test are about 4 x 2 x 2.3e-3 = 1.8e-2: the guard there must have room"


CAUGHT_ON = {"offset_edge_off_by_one": "offsets_inside_one_tile", "no_wrap_in_tile": "hidden_end_seen_start", "whole_ignores_offsets": "allframes_r1",
             "frame_window_ignored": "f0r0", "prefix_ignored": "P100", "ring_by_tile": "f0r0", "mask_after_sum": "ends_in_ragged_tile"}


@pytest.mark.parametrize("mutation", X.MUTATIONS)
def test_every_mutation_of_the_emulation_misses_the_restatement(s2v, mutation):
    c = X.case("randn")
    tab = TABLES[CAUGHT_ON[mutation]]
    assert _package_plan(s2v, tab) == X.visits(tab), "the un-mutated emulation walks the package's visit lists on the table built for the mutation"
    failed = []
    for name, tab in TABLES.items():
        ref = X.box_reference(c, "bf16", tab)
        err = (X.emulate(c, "bf16", tab, mutation).double() - ref).abs().max().item()
        if not err <= _bar(ref):   # a NaN (a row left without a key) misses it as well
            failed.append(name)
    print(f"{mutation}: caught on {failed}")
    assert CAUGHT_ON[mutation] in failed, f"{mutation} must miss on the table built for it ({CAUGHT_ON[mutation]})"


# ------------------------------------------------------------------------------------------------ validation and refusals of the pipeline
class _Engine:
    """stands where the engine would: any attribute access beyond `geometry` is a refusal that came too late"""
    geometry = (8, 5, 3, 8, 12)

    def __getattr__(self, name):
        raise AssertionError(f"a refused call reached the engine ({name})")


def _pipe(s2v, eng, dtype=torch.bfloat16, weight_format=None):
    tr = SimpleNamespace(dtype=dtype, device=torch.device("cpu"), engine=eng, config=SimpleNamespace(num_layers=4, weight_format=weight_format))
    return s2v.S2VPipeline(tr, s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0), object())


def _args(h=8, w=12):
    T, D = 5, 8
    four = dict(prompt_embeds=torch.zeros(2, T, D), negative_prompt_embeds=torch.zeros(2, T, D), ref_img_states=torch.zeros(4, 1, 16, h, w),
                num_videos_per_prompt=2, height=8 * h, width=8 * w, num_frames=5)
    one = dict(four, prompt_embeds=torch.zeros(1, T, D), negative_prompt_embeds=torch.zeros(1, T, D), ref_img_states=torch.zeros(1, 1, 16, h, w),
               num_videos_per_prompt=1)
    return four, one


def test_every_refusal_names_its_argument_and_leaves_the_engine_alone(s2v):
    A = s2v.LocalAttention
    eng = _Engine()
    pipe = _pipe(s2v, eng)
    four, one = _args()
    la = A([0, 2], 0, rows=1)
    for name, val in (("attention_map", s2v.AttentionMap([0])), ("attention_steer", s2v.AttentionSteer([0], subject=2.0)), ("step_cache", 0.1),
                      ("subject_guidance_scale", 2.0), ("temporal_windows", s2v.TemporalWindows(13, 8))):
        with pytest.raises(ValueError, match=rf"`local_attention` together with `{name}`"):
            pipe(local_attention=la, **{name: val}, **one)
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=rf"`local_attention` together with `{name}`: the local attention kernel runs on one GPU"):
            pipe(local_attention=la, **{name: object()}, **one)
    with pytest.raises(ValueError, match=r"`local_attention` together with fused=False"):
        pipe(local_attention=la, fused=False, **one)
    for lists in (dict(guidance_scale=[3.0, 4.0, 5.0, 6.0]), dict(num_inference_steps=[3, 3, 3, 3]), dict(strength=[0.5] * 4)):
        with pytest.raises(ValueError, match=r"`local_attention` together with per-video lists"):
            pipe(local_attention=la, **lists, **four)
    with pytest.raises(ValueError, match=r"`local_attention` with an fp16 engine"):
        _pipe(s2v, eng, torch.float16)(local_attention=la, **one)
    for wf in ("fp8", "fp8-qk", "fp8-auto"):
        with pytest.raises(ValueError, match=rf"`local_attention` with weight_format '{wf}'"):
            _pipe(s2v, eng, weight_format=wf)(local_attention=la, **one)
    for rows in (-1, 1.0, "2", True):
        with pytest.raises(ValueError, match=r"`rows` counts patch rows either side of the row's own, an integer >= 0 or None"):
            pipe(local_attention=A([1], 1, rows=rows), **one)
    assert eng.geometry == (8, 5, 3, 8, 12) and pipe.local_attention_report is None
    assert A([0], 1).rows is None and A([0], 1, None, 2).rows == 2 and A([0], 1, rows=0).rows == 0


class _Recording:
    """an engine that records the local-attention entries and the steps a fused DDIM call reaches"""

    def __init__(self):
        self.calls, self.geometry, self.fp8_qk_active = [], None, False
        self.cfg, self.attn_p_format = SimpleNamespace(attn_p_format="bf16"), "bf16"

    def set_geometry(self, B, T, F, H, W):
        self.geometry = (B, T, F, H, W)

    def prepare_tables(self, *a):
        pass

    def set_conditioning(self, *a):
        pass

    def attn_local_enable(self, on=True):
        self.calls.append(("enable", bool(on)))

    def attn_local_set(self, *a):
        self.calls.append(("set",) + a)

    def attn_local_set_box(self, *a):
        self.calls.append(("set_box",) + a)

    def denoise_step(self, latents, *a, **kw):
        self.calls.append(("step", kw.get("local_layers")))

    def __getattr__(self, name):
        raise AssertionError(f"the call reached the engine entry {name}")


def _recorded(s2v, la, h=16, w=24, steps=3, F=3):
    eng = _Recording()
    pipe = _pipe(s2v, eng)
    pipe.transformer.config.in_channels = 16
    pipe.transformer.config.use_rotary_positional_embeddings = False
    _, one = _args(h, w)
    kw = dict(one, num_frames=4 * (F - 1) + 1, num_inference_steps=steps, latents=torch.zeros(1, F, 16, h, w), output_type="latent")
    pipe(**kw) if la is None else pipe(local_attention=la, **kw)
    return eng.calls, pipe.local_attention_report


def test_the_loop_sets_the_box_table_once_and_arms_the_listed_steps(s2v):
    """latent 16 x 24 -> 8 patch rows of 12 cells, S = 96, F = 3, T = 5"""
    A = s2v.LocalAttention
    calls, rep = _recorded(s2v, A([2, 0], 1, steps=[0, 2], rows=2))
    table = s2v.local_attention_box_table(5, 96, 3, 8, 12, 1, 2)
    assert calls == [("enable", True), ("set_box",) + table, ("step", [2, 0]), ("step", None), ("step", [2, 0]), ("enable", False)]
    assert rep == {"steps": [0, 2], "layers": [2, 0], "frames": 1, "rows": 2, "visited_tile_share": s2v.local_attention_box_share(*table)}
    # frames >= F - 1 with a real rows: the purely spatial window -- every frame, and still the box table
    calls, rep = _recorded(s2v, A("all", 7, rows=0))
    table = s2v.local_attention_box_table(5, 96, 3, 8, 12, 3, 0)
    assert calls[1] == ("set_box",) + table and table[2][5 + 96:] == [5 + 96] * (3 * 96) and rep["rows"] == 0 and rep["layers"] == [0, 1, 2, 3]
    assert [c for c in calls if c[0] == "step"] == [("step", [0, 1, 2, 3])] * 3


def test_rows_none_and_rows_over_every_patch_row_take_todays_path(s2v):
    A = s2v.LocalAttention
    plain, _ = _recorded(s2v, None)
    assert plain == [("step", None)] * 3
    today, rep0 = _recorded(s2v, A("all", 0))
    assert today[1] == ("set",) + s2v.local_attention_table(5, 96, 3, 96, 0) and "rows" not in rep0
    for rows in (7, 8, 100):   # Hp - 1 and beyond
        calls, rep = _recorded(s2v, A("all", 0, rows=rows))
        assert calls == today, f"rows = {rows}: the entries and the table of the call without it"
        assert rep == dict(rep0, rows=rows)
        calls, rep = _recorded(s2v, A("all", 2, rows=rows))   # ... and a window over every frame as well: nothing is armed
        assert calls == plain and rep == {"steps": [], "layers": [], "frames": 2, "rows": rows, "visited_tile_share": 1.0}
    calls, _ = _recorded(s2v, A("all", 0, rows=6))
    assert calls[1][0] == "set_box"


def test_a_frame_shorter_than_a_key_tile_is_refused_by_name(s2v):
    with pytest.raises(ValueError, match=r"`local_attention` with `rows`: a latent frame of 24 cells is shorter than a 64-key tile"):
        _recorded(s2v, s2v.LocalAttention("all", 0, rows=1), h=8, w=12)
    eng = _Engine()   # ... and before the engine is touched, as every other refusal
    _, one = _args()
    with pytest.raises(ValueError, match=r"a latent frame of 24 cells is shorter than a 64-key tile"):
        _pipe(s2v, eng)(local_attention=s2v.LocalAttention([0], 0, rows=1), **one)


# ------------------------------------------------------------------------------------------------ symbols and host-side refusals
NEW = ["s2v_attn_local_set_box", "s2v_op_attention_box"]


def test_the_new_entries_are_declared_bound_and_exported_and_refuse_by_name(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib, L = s2v.lib(), s2v._lib
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert name in L._SIGS, f"{name} is not bound"
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.s2v_attn_local_set_box(None, 1, 64, None, None, None, None) != 0 and b"s2v_attn_local_set_box: null context" in lib.s2v_last_error()
    assert lib.s2v_op_attention_box(None, None, None, 1, 1, 1, 1, 0, 1, 64, None, None, None, None, None) != 0
    assert b"s2v_op_attention_box: null argument" in lib.s2v_last_error()
    for name in ("local_attention_box_table", "local_attention_box_items", "local_attention_box_share"):
        assert hasattr(s2v, name)
    assert hasattr(s2v.S2VEngine, "attn_local_set_box")


def test_the_operator_entry_refuses_a_bad_table_by_name_before_it_touches_the_device(s2v):
    lib, L = s2v.lib(), s2v._lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(tab, match, N=X.N0, B=2, dtype=L.DTYPE_BF16, impl=0):
        assert lib.s2v_op_attention_box(p, p, p, B, 2, N, dtype, impl, *tab.c(), None) != 0
        msg = lib.s2v_last_error().decode()
        assert re.search(match, msg), msg

    for tab, match in X.bad_tables():
        refused(tab, "s2v_op_attention_box: " + match)
    ok = TABLES["f1r1"]
    assert lib.s2v_op_attention_box(p, p, p, 2, 2, X.N0, L.DTYPE_BF16, 0, ok.P, ok.S, None, None, None, None, None) != 0
    assert b"null row table" in lib.s2v_last_error()
    refused(ok, r"impl 0 is bf16 and needs vt_scratch", dtype=L.DTYPE_F32)
    refused(ok, r"B >= 1, H >= 1, Ntok >= 1", B=0)
    refused(ok, r"impl 0 \(MFMA, bf16\) or 1 \(generic\)", impl=2)
