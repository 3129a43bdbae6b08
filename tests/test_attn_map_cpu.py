"""Attention map, the parts that need no GPU: the restatement against a brute-force loop, a CPU emulation of the kernel's tiled online
algorithm that passes the checks the GPU tests apply (and mutated emulations that must not), attention_map_to_change_map, the pipeline's
refusals and step plan, and the new symbols of the built library."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import attn_map_ref as R
import change_map_ref as CR
from oracle import attn_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 2, 31), (1, 2, 65), (1, 2, 257)]
_CASES = {}


def _case(family, perm, shape, dt="bf16"):
    key = (family, perm, shape, dt)
    if key not in _CASES:
        _CASES[key] = R.randn_case(dt, *shape) if family == "randn" else AC.build(family, perm, dt, *shape)
    return _CASES[key]


FAMILIES = [("onehot", p) for p in AC.PERMS] + [("sharp", "random"), ("randn", "none")]


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_is_the_brute_force_loop_at_31_keys():
    for family, perm in (("sharp", "random"), ("randn", "none")):
        case = _case(family, perm, (2, 2, 31))
        for qmode in ("bf16", "natural"):
            ranges = [(0, 11), (11, 31), (5, 5), (30, 31)]
            ref = R.mass_reference(case, qmode, ranges, 3, 28)
            assert (ref - R.brute_force(case, qmode, ranges, 3, 28)).abs().max().item() < 1e-13
            assert (ref[0] + ref[1] - 1.0).abs().max().item() < 1e-13 and (ref[2] == 0).all()


def test_traps_and_slack_rows_do_not_count_in_the_restatement():
    case = _case("onehot", "identity", (2, 2, 31))
    ref = R.mass_reference(case, "bf16", [(0, 31)], 0, 31)
    assert (ref - 1.0).abs().max().item() < 1e-13, "trap rows spread their weight over the sample's own keys: still 1"


# ------------------------------------------------------------------------------------------------ the emulation passes
@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{b}H{h}N{n}" for b, h, n in SHAPES])
def test_the_emulated_tiled_algorithm_passes_every_check(shape):
    N = shape[2]
    for family, perm in FAMILIES:
        case = _case(family, perm, shape)
        for ranges in R.range_sets(N):
            for q0, nq in R.query_sets(N):
                got = R.emulate(case, "bf16", ranges, q0, nq)
                assert R.checks(case, got, "bf16", ranges, q0, nq, R.EMU_BAR) == [], (family, perm, ranges, q0)


# ------------------------------------------------------------------------------------------------ the mutations do not
def _failures(mutation, shape):
    N = shape[2]
    out = []
    for family, perm in FAMILIES:
        case = _case(family, perm, shape)
        for ranges in R.range_sets(N):
            for q0, nq in R.query_sets(N):
                bad = R.checks(case, R.emulate(case, "bf16", ranges, q0, nq, mutation), "bf16", ranges, q0, nq, R.EMU_BAR)
                out += [(family, perm, tuple(ranges), q0, b[0]) for b in bad]
    return out


@pytest.mark.parametrize("mutation,shape", [("tile_index", (1, 2, 65)), ("tile_index", (1, 2, 257)), ("no_tail_mask", (2, 2, 31)),
                                            ("no_tail_mask", (1, 2, 65)), ("no_tail_mask", (1, 2, 257)), ("next_sample", (2, 2, 31)),
                                            ("q0_ignored", (2, 2, 31)), ("q0_ignored", (1, 2, 257)), ("no_rescale", (1, 2, 257))])
def test_a_mutated_emulation_fails_the_checks(mutation, shape):
    bad = _failures(mutation, shape)
    assert bad, f"{mutation} at {shape} passes every check"
    if mutation == "q0_ignored":
        assert all(f[3] != 0 for f in bad), "with q0 = 0 the mutation is no mutation"
    if mutation in ("no_tail_mask", "next_sample"):
        assert any(f[0] == "onehot" for f in bad), "the trap rows of the one-hot family ask for exactly the keys that must not count"


def test_mutations_that_cannot_show_at_a_shape_do_not():
    assert _failures("tile_index", (2, 2, 31)) == [], "one tile: the tile-local index is the key index"
    assert _failures("next_sample", (1, 2, 64)) == [], "one sample of whole tiles has no neighbour to leak"


# ------------------------------------------------------------------------------------------------ attention_map_to_change_map
def test_change_map_levels_ties_and_frames(s2v):
    f = s2v.attention_map_to_change_map
    lo, hi = 0.25, 0.75
    vals = torch.tensor([-1.0, 0.25, 0.75, 2.0, float("nan"), 0.5, 0.25 + 0.5 * (0.5 / 255), 0.25 + 0.5 * (1.5 / 255), 0.25 + 0.5 * (254.5 / 255)])
    m = vals.reshape(1, 1, 3, 3)
    out = f(m, lo, hi, 1)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 1, 48, 48)
    x = (vals.float() - lo) / (hi - lo)
    want = torch.floor(torch.nan_to_num(x, nan=0.0).clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)
    assert want[:6].tolist() == [0, 0, 255, 255, 0, 128], "clamp below and above, NaN -> 0, 0.5 * 255 + 0.5 = 128 exactly"
    got = out[0, 0].reshape(3, 16, 3, 16)
    for i in range(3):
        for j in range(3):
            assert (got[i, :, j, :] == want[3 * i + j]).all(), "every patch is one 16 x 16 block of its level"
    # frames: latent 0 -> frame 0, latent f >= 1 -> frames 4f - 3 .. 4f
    m = torch.arange(3, dtype=torch.float32).reshape(1, 3, 1, 1) / 2.0
    out = f(m, 0.0, 1.0, 9)
    assert tuple(out.shape) == (1, 9, 16, 16)
    assert out[0, :, 0, 0].tolist() == [0] + [128] * 4 + [255] * 4
    with pytest.raises(ValueError, match="3 latent frames are 9 frames, not num_frames = 8"):
        f(m, 0.0, 1.0, 8)
    with pytest.raises(ValueError, match="need lo < hi"):
        f(m, 1.0, 1.0, 9)
    with pytest.raises(ValueError, match=r"must be \[b, F_lat, h, w\]"):
        f(m[0], 0.0, 1.0, 9)


def test_change_map_round_trip_gives_every_latent_cell_its_own_patch_level(s2v):
    g = torch.Generator().manual_seed(5)
    m = torch.rand(2, 3, 3, 5, generator=g) * 0.02
    lo, hi = 0.004, 0.013
    cm = s2v.attention_map_to_change_map(m, lo, hi, 9)
    assert tuple(cm.shape) == (2, 9, 48, 80)
    lat = CR.latent_level(cm)                      # [2, 3, 6, 10]: the CPU restatement of s2v_map_to_latent
    level = torch.floor(((m - lo) / (hi - lo)).clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)
    assert torch.equal(lat, level.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3))
    assert len(level.unique()) > 20, "the map spans the levels"


# ------------------------------------------------------------------------------------------------ refusals and the plan
class _Engine:
    """stands where the engine would: any attribute access beyond `geometry` is a refusal that came too late"""
    geometry = (8, 5, 3, 8, 12)

    def __getattr__(self, name):
        raise AssertionError(f"a refused call reached the engine ({name})")


def test_every_refusal_names_its_cause_and_leaves_the_engine_alone(s2v):
    P, A = s2v.S2VPipeline, s2v.AttentionMap
    eng = _Engine()

    def pipe_for(weight_format=None):
        tr = SimpleNamespace(dtype=torch.bfloat16, device=torch.device("cpu"), engine=eng, config=SimpleNamespace(num_layers=4, weight_format=weight_format))
        return P(tr, s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0), object())

    pipe = pipe_for()
    T, D = 5, 8
    four = dict(prompt_embeds=torch.zeros(2, T, D), negative_prompt_embeds=torch.zeros(2, T, D), ref_img_states=torch.zeros(4, 1, 16, 8, 12),
                num_videos_per_prompt=2, height=64, width=96, num_frames=5)
    one = dict(four, prompt_embeds=torch.zeros(1, T, D), negative_prompt_embeds=torch.zeros(1, T, D), ref_img_states=torch.zeros(1, 1, 16, 8, 12),
               num_videos_per_prompt=1)
    am = A([0, 2])
    for lists in (dict(guidance_scale=[3.0, 4.0, 5.0, 6.0]), dict(num_inference_steps=[3, 3, 3, 3])):
        with pytest.raises(ValueError, match=r"`attention_map` together with per-video lists"):
            pipe(attention_map=am, **lists, **four)
    with pytest.raises(ValueError, match=r"`attention_map` together with per-video lists \(or several input videos"):
        pipe(attention_map=am, video=torch.zeros(4, 3, 9, 64, 96), **dict(four, num_frames=9))
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=rf"`attention_map` together with `{name}`: the map is collected on one GPU"):
            pipe(attention_map=am, **{name: object()}, **one)
    with pytest.raises(ValueError, match=r"`attention_map` together with fused=False"):
        pipe(attention_map=am, fused=False, **one)
    with pytest.raises(ValueError, match=r"`attention_map` with weight_format 'fp8-qk'"):
        pipe_for("fp8-qk")(attention_map=am, **one)
    with pytest.raises(ValueError, match=r"must be an AttentionMap"):
        pipe(attention_map=[0, 1], **one)
    for layers in (None, [], 3):
        with pytest.raises(ValueError, match=r"`layers` is an explicit, non-empty list"):
            pipe(attention_map=A(layers), **one)
    for layers in ([4], [-1], [0.5]):
        with pytest.raises(ValueError, match=r"is no block index of a model of 4 blocks"):
            pipe(attention_map=A(layers), **one)
    with pytest.raises(ValueError, match=r"a layer is listed twice"):
        pipe(attention_map=A([1, 1]), **one)
    with pytest.raises(ValueError, match=r"`steps` is a list of step indices"):
        pipe(attention_map=A([1], steps=3), **one)
    with pytest.raises(ValueError, match=r"at most three text spans"):
        pipe(attention_map=A([1], text_spans=[(0, 1)] * 4), **one)
    with pytest.raises(ValueError, match=r"a text span is a token range"):
        pipe(attention_map=A([1], text_spans=[(3, 2)]), **one)
    assert eng.geometry == (8, 5, 3, 8, 12), "no refusal reached the engine"
    assert pipe.attention_maps is None


def test_the_step_plan_with_and_without_a_step_cache_plan(s2v):
    A, plan = s2v.AttentionMap, s2v.attention_map_plan
    assert plan(A([0]), 5) == ([0, 1, 2, 3, 4], [])
    assert plan(A([0], steps=[3, 1, 3]), 5) == ([1, 3], [])
    sc = [True, False, True, False, True]
    assert plan(A([0]), 5, sc) == ([0, 2, 4], [1, 3]), "planned reuse steps are skipped and reported"
    assert plan(A([0], steps=[1, 2]), 5, sc) == ([2], [1])
    assert plan(A([0], steps=[]), 5, sc) == ([], [])
    for bad in ([5], [-1]):
        with pytest.raises(ValueError, match="is outside the 5 steps this call runs"):
            plan(A([0], steps=bad), 5)


# ------------------------------------------------------------------------------------------------ symbols
NEW = ["s2v_attn_map_enable", "s2v_attn_map_arm", "s2v_attn_map_read", "s2v_attn_map_reset", "s2v_op_attn_mass", "s2v_op_attn_mass_mean"]


def test_the_new_entries_are_declared_bound_and_exported_and_refuse_a_null_context_by_name(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib, L = s2v.lib(), s2v._lib
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert name in L._SIGS, f"{name} is not bound"
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.s2v_attn_map_enable(None, 1, None, 0) != 0 and b"s2v_attn_map_enable: null context" in lib.s2v_last_error()
    assert lib.s2v_attn_map_arm(None, 1) != 0 and b"s2v_attn_map_arm: null context" in lib.s2v_last_error()
    assert lib.s2v_attn_map_read(None, 0, None, None, None) != 0 and b"s2v_attn_map_read: null argument" in lib.s2v_last_error()
    assert lib.s2v_attn_map_reset(None) != 0 and b"s2v_attn_map_reset" in lib.s2v_last_error()
    assert lib.s2v_op_attn_mass(None, 1, 1, 1, 0, 1, None, 1, None, 0, 1, 0, None) != 0 and b"s2v_op_attn_mass: null argument" in lib.s2v_last_error()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, f"{name} is missing from INTEGRATION.md"
    for name in ("AttentionMap", "attention_map_to_change_map", "attention_map_plan"):
        assert hasattr(s2v, name)
