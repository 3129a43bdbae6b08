"""Local attention in time, the parts that need no GPU: the restatement against a brute-force loop and against F.scaled_dot_product_attention
with a boolean mask, the table and the plan (the package's and the restatement's, against each other and against a brute-force count), a CPU
emulation of attn_pp<LOCAL>'s visit-list + wave-classification + per-lane-mask algorithm that meets the restatement (and six mutated
emulations that must not), validation of LocalAttention, every refusal of the pipeline with an engine that must not be reached, "a window over
every frame arms nothing", and the new symbols of the built library with the table refusals of the operator entry."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import attn_local_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = R.tables()


def _bar(ref):
    return R.EMU_BAR * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_is_the_brute_force_loop_and_sdpa_with_a_boolean_mask():
    c = R.case("randn", "bf16", (2, 2, 31))
    lo = [3] * 3 + [min(28, 3 + i) for i in range(28)]
    hi = [31] * 3 + [min(31, 3 + i + (i % 4)) for i in range(28)]   # i % 4 == 0: an empty window
    tab = R.Table(3, lo, hi)
    for qmode in ("bf16", "natural"):
        ref = R.local_reference(c, qmode, tab).reshape(2, 31, 2, 64)
        qs, base = R.SR.scaled_q(c.heads(0), qmode)
        k, v = c.heads(1), c.heads(2)
        for b in range(2):
            for h in range(2):
                for i in (0, 3, 4, 17, 30):
                    see = [j for j in range(31) if j < 3 or lo[i] <= j < hi[i]]
                    s = {j: sum(float(qs[b, h, i, d]) * float(k[b, h, j, d]) for d in range(64)) * math.log(base) for j in see}
                    mx = max(s.values())
                    e = {j: math.exp(x - mx) for j, x in s.items()}
                    want = sum(e[j] * v[b, h, j] for j in see) / sum(e.values())
                    assert (ref[b, i, h] - want).abs().max().item() < 1e-12
    q, k, v = (c.heads(p) for p in range(3))
    got = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=R.visible(tab)[None, None], dropout_p=0.0, is_causal=False)
    assert (got.transpose(1, 2).reshape(62, 128) - R.local_reference(c, "natural", tab)).abs().max().item() < 1e-12
    assert torch.equal(R.local_reference(c, "bf16", R.dense_table(31)), R.local_reference(c, "bf16", None))


# ------------------------------------------------------------------------------------------------ the table and the plan
def test_the_table_and_the_plan_of_the_package_equal_the_restatement_and_a_brute_force_count(s2v):
    for w in (0, 1, 2, 4, 9):
        tab = R.frames_table(R.T_, R.R_, R.F_, R.S_, w)
        P, lo, hi = s2v.local_attention_table(R.T_, R.R_, R.F_, R.S_, w)
        assert (P, lo, hi) == (tab.P, tab.lo, tab.hi)
        assert s2v.local_attention_items(P, lo, hi) == R.items(tab)
        assert s2v.local_attention_share(P, lo, hi) == R.share(tab)
    assert R.visits(TABLES["frames0"]) == R.VISITS_FRAMES0
    assert round(R.share(TABLES["frames0"]), 3) == 0.654 and round(R.share(TABLES["frames1"]), 3) == 0.808
    assert R.share(R.frames_table(R.T_, R.R_, R.F_, R.S_, 4)) == 1.0
    for name, tab in TABLES.items():
        assert R.share(tab) == R.brute_share(tab), name
        assert s2v.local_attention_items(tab.P, tab.lo, tab.hi) == R.items(tab), name
    # the headline geometry: P = 226 + 1350, S = 1350, F = 13
    for w, want in ((1, 0.364), (2, 0.472), (3, 0.570)):
        assert round(R.share(R.frames_table(226, 1350, 13, 1350, w)), 3) == want
    for bad in (dict(T=0, R=0), dict(F=0), dict(S=0), dict(frames=-1)):
        kw = dict(dict(T=5, R=15, F=5, S=150, frames=1), **bad)
        with pytest.raises(ValueError, match=r"local attention: T \+ R >= 1, F >= 1, S >= 1 and frames >= 0 are required"):
            s2v.local_attention_table(**kw)
    plan, A = s2v.local_attention_plan, s2v.LocalAttention
    assert plan(A([0], 1), 4) == [0, 1, 2, 3] and plan(A([0], 1, steps=[3, 1, 3]), 4) == [1, 3] and plan(A([0], 1, steps=[]), 4) == []
    for bad in ([4], [-1]):
        with pytest.raises(ValueError, match="is outside the 4 steps this call runs"):
            plan(A([0], 1, steps=bad), 4)


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
@pytest.mark.parametrize("family", ["randn", "sharp"])
def test_the_emulation_of_the_visit_list_algorithm_meets_the_restatement(family):
    c = R.case(family)
    for name, tab in TABLES.items():
        ref = R.local_reference(c, "bf16", tab)
        err = (R.emulate(c, "bf16", tab).double() - ref).abs().max().item()
        assert err <= _bar(ref), f"{family} {name}: {err:.3e} > {_bar(ref):.3e}"


def test_the_windowed_answer_is_far_from_the_dense_one():
    c = R.case("randn")
    tab = TABLES["frames0"]
    d = R.rel_l2(R.local_reference(c, "bf16", None), R.local_reference(c, "bf16", tab), tab.windowed_rows().repeat(c.B))
    print(f"randn frames = 0: the dense and local restatements are {d:.3e} apart (rel-l2 over the video rows)")
    assert d >= 0.5, "four bars of the GPU test are about 4 x 2 x 2.3e-3 = 1.8e-2: the guard there must have room"


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_of_the_emulation_misses_the_restatement(mutation):
    c = R.case("randn")
    failed = []
    for name, tab in TABLES.items():
        ref = R.local_reference(c, "bf16", tab)
        err = (R.emulate(c, "bf16", tab, mutation).double() - ref).abs().max().item()
        if not err <= _bar(ref):   # a NaN (a row left without a key) misses it as well
            failed.append(name)
    print(f"{mutation}: caught on {failed}")
    expect = {"edge_off_by_one": "inside_one_tile", "prefix_ignored": "P100", "wave_envelope_on_edge": "lo_is_P", "straddle_as_interior": "frames0",
              "ring_by_tile": "frames0", "mask_after_sum": "ends_in_ragged_tile"}[mutation]
    assert expect in failed, f"{mutation} must miss on the table built for it ({expect})"


# ------------------------------------------------------------------------------------------------ validation and refusals of the pipeline
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
    A = s2v.LocalAttention
    eng = _Engine()
    pipe = _pipe(s2v, eng)
    four, one = _args()
    la = A([0, 2], 0)
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
    with pytest.raises(ValueError, match=r"`local_attention` together with per-video lists \(or several input videos"):
        pipe(local_attention=la, video=torch.zeros(4, 3, 9, 64, 96), **dict(four, num_frames=9))
    with pytest.raises(ValueError, match=r"`local_attention` with an fp16 engine"):
        _pipe(s2v, eng, torch.float16)(local_attention=la, **one)
    for wf in ("fp8", "fp8-qk", "fp8-auto"):
        with pytest.raises(ValueError, match=rf"`local_attention` with weight_format '{wf}'"):
            _pipe(s2v, eng, weight_format=wf)(local_attention=la, **one)
    assert eng.geometry == (8, 5, 3, 8, 12) and pipe.local_attention_report is None


def test_validation_of_local_attention(s2v):
    A = s2v.LocalAttention
    pipe = _pipe(s2v, _Engine())
    _, one = _args()
    with pytest.raises(ValueError, match=r"must be a LocalAttention"):
        pipe(local_attention=[0, 1], **one)
    for layers in (None, [], 3, "every"):
        with pytest.raises(ValueError, match=r"`layers` is an explicit, non-empty list of block indices or the string \"all\""):
            pipe(local_attention=A(layers, 1), **one)
    for layers in ([4], [-1], [0.5], [True]):
        with pytest.raises(ValueError, match=r"is no block index of a model of 4 blocks"):
            pipe(local_attention=A(layers, 1), **one)
    with pytest.raises(ValueError, match=r"a layer is listed twice"):
        pipe(local_attention=A([1, 1], 1), **one)
    for frames in (-1, 1.0, None, "2", True):
        with pytest.raises(ValueError, match=r"`frames` counts latent frames either side of the row's own, an integer >= 0"):
            pipe(local_attention=A([1], frames), **one)
    with pytest.raises(ValueError, match=r"`steps` is a list of step indices"):
        pipe(local_attention=A([1], 1, steps=3), **one)
    assert s2v.S2VPipeline.check_local_attention(A("all", 0), 4) == [0, 1, 2, 3]


class _Recording:
    """an engine that records the entries a fused DDIM call reaches and refuses every local-attention entry"""

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


def test_a_window_over_every_frame_arms_nothing(s2v):
    eng = _Recording()
    pipe = _pipe(s2v, eng)
    pipe.transformer.config.in_channels = 16
    pipe.transformer.config.use_rotary_positional_embeddings = False
    _, one = _args()
    kw = dict(one, num_inference_steps=3, latents=torch.zeros(1, 2, 16, 8, 12), output_type="latent")   # F = 2 latent frames
    pipe(**kw)
    plain, eng.calls = eng.calls, []
    for frames in (1, 5):
        pipe(local_attention=s2v.LocalAttention("all", frames), **kw)
        assert eng.calls == plain == [[]] * 3, "no local entry, no local_layers: the launches of the call without the argument"
        assert pipe.local_attention_report == {"steps": [], "layers": [], "frames": frames, "visited_tile_share": 1.0}
        eng.calls = []


# ------------------------------------------------------------------------------------------------ symbols and host-side refusals
NEW = ["s2v_attn_local_enable", "s2v_attn_local_set", "s2v_attn_local_arm", "s2v_op_attention_local"]


def test_the_new_entries_are_declared_bound_and_exported_and_refuse_by_name(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib, L = s2v.lib(), s2v._lib
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert name in L._SIGS, f"{name} is not bound"
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.s2v_attn_local_enable(None, 1) != 0 and b"s2v_attn_local_enable: null context" in lib.s2v_last_error()
    assert lib.s2v_attn_local_set(None, 1, None, None) != 0 and b"s2v_attn_local_set: null context" in lib.s2v_last_error()
    assert lib.s2v_attn_local_arm(None, 1) != 0 and b"s2v_attn_local_arm: null context" in lib.s2v_last_error()
    assert lib.s2v_op_attention_local(None, None, None, 1, 1, 1, 1, 0, 1, None, None, None) != 0 and b"s2v_op_attention_local: null argument" in lib.s2v_last_error()
    for name in ("LocalAttention", "local_attention_table", "local_attention_items", "local_attention_share", "local_attention_plan"):
        assert hasattr(s2v, name)


def test_the_operator_entry_refuses_a_bad_table_by_name_before_it_touches_the_device(s2v):
    lib, L = s2v.lib(), s2v._lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(tab, match, N=R.N0, B=2, dtype=L.DTYPE_BF16, impl=0):
        P, lo, hi = tab.c()
        assert lib.s2v_op_attention_local(p, p, p, B, 2, N, dtype, impl, P, lo, hi, None) != 0
        msg = lib.s2v_last_error().decode()
        assert re.search(match, msg), msg

    for tab, match in R.bad_tables():
        refused(tab, "s2v_op_attention_local: " + match)
    ok = R.frames_table(R.T_, R.R_, R.F_, R.S_, 0)
    assert lib.s2v_op_attention_local(p, p, p, 2, 2, R.N0, L.DTYPE_BF16, 0, ok.P, None, None, None) != 0 and b"null row table" in lib.s2v_last_error()
    refused(ok, r"impl 0 is bf16 and needs vt_scratch", dtype=L.DTYPE_F32)
    refused(ok, r"B >= 1, H >= 1, Ntok >= 1", B=0)
    refused(ok, r"impl 0 \(MFMA, bf16\) or 1 \(generic\)", impl=2)
