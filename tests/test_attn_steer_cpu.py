"""Attention steering, the parts that need no GPU: the restatement against a brute-force loop and against F.scaled_dot_product_attention with
an additive mask, a CPU emulation of attn_pp<STEER>'s tile-classified algorithm that passes the check the GPU tests apply (and six mutated
emulations that must not), the range layout and step plan of the pipeline, validation of AttentionSteer, every refusal of the pipeline with
an engine that must not be reached, "all weights 1 arms nothing", and the new symbols of the built library."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import attn_steer_ref as R
from oracle import attn_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["onehot", "sharp", "sharp2", "randn"]
SETS = R.range_sets()


def _bar(ref):
    return R.EMU_BAR * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_is_the_brute_force_loop_and_sdpa_with_an_additive_mask():
    c = R.case("randn", "bf16", (2, 2, 31))
    rec = R.Record([(0, 3, 2.0 ** 16, 0b01), (7, 20, 2.0 ** -16, 0b11), (30, 31, 8.0, 0b10)], 5, 29)
    for qmode in ("bf16", "natural"):
        ref = R.steered_reference(c, qmode, rec).reshape(2, 31, 2, 64)
        qs, base = R.scaled_q(c.heads(0), qmode)
        k, v = c.heads(1), c.heads(2)
        for b in range(2):
            for h in range(2):
                for i in (0, 5, 17, 28, 30):
                    s = [sum(float(qs[b, h, i, d]) * float(k[b, h, j, d]) for d in range(64)) * math.log(base) for j in range(31)]
                    for k0, k1, w, m in rec.ranges:
                        if (m >> b) & 1 and 5 <= i < 29:
                            for j in range(k0, k1):
                                s[j] += math.log(w)
                    mx = max(s)
                    e = [math.exp(x - mx) for x in s]
                    want = sum(e[j] * v[b, h, j] for j in range(31)) / sum(e)
                    assert (ref[b, i, h] - want).abs().max().item() < 1e-12
    # the oracle's own operator with the bias as an additive float mask: what tests/test_gpu_attn_steer_engine.py steers the CPU oracle with
    q, k, v = (c.heads(p) for p in range(3))
    got = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=R.beta(rec, 2, 31)[:, None], dropout_p=0.0, is_causal=False)
    assert (got.transpose(1, 2).reshape(62, 128) - R.steered_reference(c, "natural", rec)).abs().max().item() < 1e-12
    assert torch.equal(R.steered_reference(c, "bf16", R.Record([], 0, 31)), R.steered_reference(c, "bf16", None))


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
@pytest.mark.parametrize("family", FAMILIES)
def test_the_emulation_of_the_tile_classified_algorithm_equals_the_restatement(family):
    c = R.case(family)
    for name, rec in SETS.items():
        ref = R.steered_reference(c, "bf16", rec)
        err = (R.emulate(c, "bf16", rec).double() - ref).abs().max().item()
        assert err <= _bar(ref), f"{family} {name}: {err:.3e} > {_bar(ref):.3e}"


def test_the_inputs_are_far_from_their_unsteered_answer_and_the_threshold_case_crosses_it():
    c = R.case("randn")
    plain = R.steered_reference(c, "bf16", None)
    for name, rec in SETS.items():
        rows = rec.steered_rows(c.B, c.N).reshape(-1)
        d = R.rel_l2(plain, R.steered_reference(c, "bf16", rec), rows)
        assert d >= 0.7, f"randn {name}: the steered answer is only {d:.3e} (rel-l2) from the un-steered one"
    # a large weight on sharp scores: the row sum passes the deferred-maximum threshold inside a biased tile, and would not without the bias
    with_bias, without = R.crossings(R.case("sharp2"), SETS["straddle_interior_straddle"])
    print(f"sharp2, w = 2^16 on [60, 200): {with_bias} (sample, head, row) cross 2^64 inside the range, {without} without the bias")
    assert with_bias > without and with_bias >= 8
    # one-hot margins (>= 36 natural units) exceed ln 2^16 = 11.1: no allowed weight changes a one-hot winner
    assert R.case("onehot").margin > math.log(R.W_HI) + 20


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_of_the_emulation_fails_the_same_check(mutation):
    failed = []
    for family in ("sharp", "randn"):
        c = R.case(family)
        for name, rec in SETS.items():
            ref = R.steered_reference(c, "bf16", rec)
            if (R.emulate(c, "bf16", rec, mutation).double() - ref).abs().max().item() > _bar(ref):
                failed.append((family, name))
    print(f"{mutation}: caught on {failed}")
    assert failed, f"the mutation {mutation} passes every check"
    expect = {"edge_off_by_one": "inside_one_tile", "bias_outside_query": "query_range", "span_on_every_sample": "one_sample",
              "natural_log": "tile_aligned", "bias_after_sum": "first_tile", "straddle_as_interior": "straddle_interior_straddle"}[mutation]
    assert ("randn", expect) in failed, f"{mutation} must fail on the set built for it ({expect})"


# ------------------------------------------------------------------------------------------------ ranges, plan, validation
def test_the_ranges_cover_the_cfg_layout_and_weights_of_one_are_left_out(s2v):
    A, ranges = s2v.AttentionSteer, s2v.attention_steer_ranges
    T, Rr = 7, 391
    assert ranges(A([0], subject=2.0), T, Rr, 1) == [(7, 398, 2.0, 0b11)]
    assert ranges(A([0], subject=0.5, text_spans=[(3, 5, 4.0), (0, 2, 0.25)]), T, Rr, 2) == [(0, 2, 0.25, 0b1100), (3, 5, 4.0, 0b1100), (7, 398, 0.5, 0b1111)]
    assert ranges(A([0], subject=1.0, text_spans=[(0, 2, 1.0)]), T, Rr, 1) == [], "all weights 1: nothing to steer"
    assert ranges(A([0], subject=1.0, text_spans=[(0, 2, 1.0), (2, 7, 3.0)]), T, Rr, 1) == [(2, 7, 3.0, 0b10)]
    with pytest.raises(ValueError, match=r"reaches beyond the 7 prompt tokens"):
        ranges(A([0], text_spans=[(5, 8, 2.0)]), T, Rr, 1)
    with pytest.raises(ValueError, match=r"overlap"):
        ranges(A([0], text_spans=[(0, 4, 2.0), (3, 5, 2.0)]), T, Rr, 1)
    plan = s2v.attention_steer_plan
    assert plan(A([0]), 4) == [0, 1, 2, 3] and plan(A([0], steps=[3, 1, 3]), 4) == [1, 3] and plan(A([0], steps=[]), 4) == []
    for bad in ([4], [-1]):
        with pytest.raises(ValueError, match="is outside the 4 steps this call runs"):
            plan(A([0], steps=bad), 4)


class _Engine:
    """stands where the engine would: any attribute access beyond `geometry` is a refusal that came too late"""
    geometry = (8, 5, 3, 8, 12)

    def __getattr__(self, name):
        raise AssertionError(f"a refused call reached the engine ({name})")


def _pipe(s2v, eng, dtype=torch.bfloat16, weight_format=None):
    tr = SimpleNamespace(dtype=dtype, device=torch.device("cpu"), engine=eng, config=SimpleNamespace(num_layers=4, weight_format=weight_format))
    return s2v.S2VPipeline(tr, s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0), object())


def _args():
    T, D = 5, 8
    four = dict(prompt_embeds=torch.zeros(2, T, D), negative_prompt_embeds=torch.zeros(2, T, D), ref_img_states=torch.zeros(4, 1, 16, 8, 12),
                num_videos_per_prompt=2, height=64, width=96, num_frames=5)
    one = dict(four, prompt_embeds=torch.zeros(1, T, D), negative_prompt_embeds=torch.zeros(1, T, D), ref_img_states=torch.zeros(1, 1, 16, 8, 12),
               num_videos_per_prompt=1)
    return four, one


def test_every_refusal_names_its_argument_and_leaves_the_engine_alone(s2v):
    A = s2v.AttentionSteer
    eng = _Engine()
    pipe = _pipe(s2v, eng)
    four, one = _args()
    st = A([0, 2], subject=2.0)
    for name, val in (("attention_map", s2v.AttentionMap([0])), ("step_cache", 0.1), ("subject_guidance_scale", 2.0),
                      ("temporal_windows", s2v.TemporalWindows(13, 8))):
        with pytest.raises(ValueError, match=rf"`attention_steer` together with `{name}`"):
            pipe(attention_steer=st, **{name: val}, **one)
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=rf"`attention_steer` together with `{name}`: the steered attention runs on one GPU"):
            pipe(attention_steer=st, **{name: object()}, **one)
    with pytest.raises(ValueError, match=r"`attention_steer` together with fused=False"):
        pipe(attention_steer=st, fused=False, **one)
    for lists in (dict(guidance_scale=[3.0, 4.0, 5.0, 6.0]), dict(num_inference_steps=[3, 3, 3, 3]), dict(strength=[0.5] * 4)):
        with pytest.raises(ValueError, match=r"`attention_steer` together with per-video lists"):
            pipe(attention_steer=st, **lists, **four)
    with pytest.raises(ValueError, match=r"`attention_steer` together with per-video lists \(or several input videos"):
        pipe(attention_steer=st, video=torch.zeros(4, 3, 9, 64, 96), **dict(four, num_frames=9))
    with pytest.raises(ValueError, match=r"`attention_steer` with an fp16 engine"):
        _pipe(s2v, eng, torch.float16)(attention_steer=st, **one)
    for wf in ("fp8", "fp8-qk", "fp8-auto"):
        with pytest.raises(ValueError, match=rf"`attention_steer` with weight_format '{wf}'"):
            _pipe(s2v, eng, weight_format=wf)(attention_steer=st, **one)
    assert eng.geometry == (8, 5, 3, 8, 12) and pipe.attention_steer_report is None


def test_validation_of_attention_steer(s2v):
    A = s2v.AttentionSteer
    pipe = _pipe(s2v, _Engine())
    _, one = _args()
    with pytest.raises(ValueError, match=r"must be an AttentionSteer"):
        pipe(attention_steer=[0, 1], **one)
    for layers in (None, [], 3):
        with pytest.raises(ValueError, match=r"`layers` is an explicit, non-empty list"):
            pipe(attention_steer=A(layers), **one)
    for layers in ([4], [-1], [0.5]):
        with pytest.raises(ValueError, match=r"is no block index of a model of 4 blocks"):
            pipe(attention_steer=A(layers), **one)
    with pytest.raises(ValueError, match=r"a layer is listed twice"):
        pipe(attention_steer=A([1, 1]), **one)
    with pytest.raises(ValueError, match=r"`steps` is a list of step indices"):
        pipe(attention_steer=A([1], steps=3), **one)
    with pytest.raises(ValueError, match=r"at most three text spans"):
        pipe(attention_steer=A([1], text_spans=[(0, 1, 2.0)] * 4), **one)
    for sp in ((3, 2, 2.0), (2, 2, 2.0), (-1, 2, 2.0)):
        with pytest.raises(ValueError, match=r"a text span is \(k0, k1, w\)"):
            pipe(attention_steer=A([1], text_spans=[sp]), **one)
    for w in (0.0, -1.0, 2.0 ** 17, 2.0 ** -17, float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError, match=r"the weight of subject must be finite and inside \[2\^-16, 2\^16\]"):
            pipe(attention_steer=A([1], subject=w), **one)
        with pytest.raises(ValueError, match=r"the weight of text span \(0, 2\) must be finite"):
            pipe(attention_steer=A([1], text_spans=[(0, 2, w)]), **one)


class _Recording:
    """an engine that records the entries a fused DDIM call reaches and refuses every steer entry"""

    def __init__(self):
        self.calls, self.geometry, self.fp8_qk_active = [], None, False
        self.cfg, self.attn_p_format = SimpleNamespace(attn_p_format="bf16"), "bf16"

    def set_geometry(self, B, T, F, H, W):
        self.geometry = (B, T, F, H, W)

    def prepare_tables(self, *a):
        pass

    def set_conditioning(self, *a):
        pass

    def denoise_step(self, latents, *a, **kw):
        self.calls.append(sorted(k for k in kw if k not in ("blend", "cache", "attn_layers")))

    def __getattr__(self, name):
        raise AssertionError(f"the call reached the engine entry {name}")


def test_all_weights_one_arms_nothing(s2v):
    eng = _Recording()
    pipe = _pipe(s2v, eng)
    pipe.transformer.config.in_channels = 16
    pipe.transformer.config.use_rotary_positional_embeddings = False
    _, one = _args()
    kw = dict(one, num_inference_steps=3, latents=torch.zeros(1, 2, 16, 8, 12), output_type="latent")
    pipe(**kw)
    plain, eng.calls = eng.calls, []
    pipe(attention_steer=s2v.AttentionSteer([0, 1], subject=1.0, text_spans=[(0, 2, 1.0)]), **kw)
    assert eng.calls == plain == [[]] * 3, "no steer entry, no steer_layers: the launches of the call without the argument"
    assert pipe.attention_steer_report == {"steps": [], "layers": [], "ranges": []}


# ------------------------------------------------------------------------------------------------ symbols and host-side refusals
NEW = ["s2v_attn_steer_enable", "s2v_attn_steer_set", "s2v_attn_steer_arm", "s2v_op_attention_steer"]


def test_the_new_entries_are_declared_bound_and_exported_and_refuse_by_name(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib, L = s2v.lib(), s2v._lib
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert name in L._SIGS, f"{name} is not bound"
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.s2v_attn_steer_enable(None, 1) != 0 and b"s2v_attn_steer_enable: null context" in lib.s2v_last_error()
    assert lib.s2v_attn_steer_set(None, 0, None) != 0 and b"s2v_attn_steer_set: null context" in lib.s2v_last_error()
    assert lib.s2v_attn_steer_arm(None, 1) != 0 and b"s2v_attn_steer_arm: null context" in lib.s2v_last_error()
    assert lib.s2v_op_attention_steer(None, None, None, 1, 1, 1, 1, 0, None, None) != 0 and b"s2v_op_attention_steer: null argument" in lib.s2v_last_error()
    assert ctypes.sizeof(L.SteerRangeC) == 16 and ctypes.sizeof(L.SteerRecordC) == 80
    for name in ("AttentionSteer", "attention_steer_ranges", "attention_steer_plan"):
        assert hasattr(s2v, name)


def test_the_operator_entry_refuses_a_bad_record_by_name_before_it_touches_the_device(s2v):
    lib, L = s2v.lib(), s2v._lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(rec, match, N=330, B=2, dtype=L.DTYPE_BF16, impl=0):
        assert lib.s2v_op_attention_steer(p, p, p, B, 2, N, dtype, impl, ctypes.byref(rec.c(L)), None) != 0
        msg = lib.s2v_last_error().decode()
        assert re.search(match, msg), msg

    ok = [(70, 100, 2.0, 3)]
    refused(R.Record([(70, 100, 2.0, 3), (90, 120, 2.0, 3)], 0, 330), r"key range 1 = \[90, 120\) overlaps or precedes range 0")
    refused(R.Record([(200, 220, 2.0, 3), (70, 100, 2.0, 3)], 0, 330), r"key range 1 = \[70, 100\) overlaps or precedes range 0")
    refused(R.Record([(300, 331, 2.0, 3)], 0, 330), r"key range 0 = \[300, 331\) must be non-empty and inside \[0, Ntok = 330\)")
    refused(R.Record([(-1, 5, 2.0, 3)], 0, 330), r"key range 0 = \[-1, 5\) must be non-empty")
    refused(R.Record([(5, 5, 2.0, 3)], 0, 330), r"key range 0 = \[5, 5\) must be non-empty")
    for w in (0.0, 2.0 ** 17, 2.0 ** -17, float("nan"), float("inf"), -2.0):
        refused(R.Record([(70, 100, w, 3)], 0, 330), r"weight 0 = \S+ must be finite and inside \[2\^-16, 2\^16\] \(no w = 0\)")
    refused(R.Record(ok, 0, 331), r"the query range \[0, 331\) must lie inside \[0, Ntok = 330\)")
    refused(R.Record(ok, 200, 100), r"the query range \[200, 100\)")
    rec = R.Record(ok, 0, 330).c(L)
    rec.n = 5
    assert lib.s2v_op_attention_steer(p, p, p, 2, 2, 330, L.DTYPE_BF16, 0, ctypes.byref(rec), None) != 0
    assert b"0..4 key ranges are accepted (n = 5)" in lib.s2v_last_error()
    refused(R.Record(ok, 0, 330), r"impl 0 is bf16 and needs vt_scratch", dtype=L.DTYPE_F32)
    refused(R.Record(ok, 0, 330), r"1 <= B <= 32", B=33)
    refused(R.Record(ok, 0, 330), r"impl 0 \(MFMA, bf16\) or 1 \(generic\)", impl=2)
