"""Attention steering at kernel level (pytest -m gpu): s2v_op_attention_steer impl 0 (attn_pp<STEER>, bf16) and impl 1 (the steered generic
kernel) against the fp64 restatement of tests/attn_steer_ref.py.

Shapes: B = 2, H = 2, N = 330 -- six key tiles of 64 with a ragged last one, two 256-row query blocks with a ragged last one -- and
B = 2, H = 1, N = 4700 beyond ATTN_PP_MAX_TOKENS (74 tiles: the long loop; the un-steered launch there is attn_q4).  Range sets: R.range_sets().

The bar is not fixed here.  Every randn case measures, in the same test and on the same q, k, v, the error of today's un-steered launch
(s2v_op_attention impl 0, or impl 1 for the generic form) against its own fp64 restatement; the steered launch may err at most 2 x that figure.
The figure is the relative L2 error over the steered rows (R.rel_l2: the kernels' roundings are relative to what they round, so it does not move
with the magnitude of the output as max-abs does).  Condition on the inputs, asserted: the fp64 steered and un-steered answers differ by at
least 100 x the bar over those rows, so a kernel that ignores the bias cannot pass.  The sign-code families keep their dominant key under any
allowed weight, so the condition cannot hold for them; they are held to the restatement by the project's own bars (oracle.attn_cases.SOFT_BARS
on trap and sharp rows, one ulp + leak on one-hot rows) and carry the bit-for-bit and threshold checks.

Deviations from the issue's wording, on purpose:
  * the issue asks for the 2 x bar on every input together with the condition that the fp64 answers lie 100 bars apart.  Both hold on randn
    inputs.  On the sharp sign-code inputs (sharp, sharp2) the 2 x bar is applied as well, but WITHOUT the condition: their answers move by
    0.04 .. 0.19 only (tests/attn_steer_ref.py range_sets), so there the bar shows that steering costs no accuracy, not that the bias is applied
    -- the randn cases and the mutation tests show that.  There the bar also has a floor, twice the error of the fp64 steered answer rounded
    once to the storage type: an un-steered sharp answer is nearly a stored V row (error 1.4e-04 for the generic kernel, a tenth of bf16
    rounding), a row whose dominant key is weighted down is not, and the ideal kernel itself goes from 1.442e-04 to 4.559e-04 on four_ranges.
    For the MFMA kernel the floor also holds the bf16 rounding of P (2^-9 / sqrt 3 where one key carries a row), which the deferred maximum
    hides or shows depending on which tile raised the maximum last.  Measured: sharp impl 0 1.52e-03 -> 0.88e-03 .. 1.58e-03 (ratio 0.59 ..
    1.04); sharp impl 1 1.44e-04 -> 1.79e-04 .. 4.56e-04, each equal to the ideal kernel's figure; sharp2 impl 0 2.17e-04 -> 7.28e-04 on
    inside_one_tile, where biased keys raise the maximum before the row's own key arrives.  One-hot rows have an un-steered error of zero
    (the output is V[pi(i)] itself), so twice it is no bar: they are held to one ulp + leak.
  * "the biased winner where it does [change]" has no one-hot case: with 2^-16 <= w <= 2^16 the bias is at most 11.1 natural units and a
    one-hot margin is at least 36, so no allowed weight moves a one-hot winner, and a winner that a bias did move would not be one-hot to one
    ulp.  The test asserts that precondition instead; winners that do move are the sharp inputs' (own key 32 against <= 21), held to the
    restatement.
  * rows outside [q0, q1) that share a 32-row wave with steered rows equal today's launch bit for bit only while no row of the wave passes the
    deferred-maximum threshold past the first tile in either launch (asserted where R.crossings says so); where rows do pass it (onehot, sharp2)
    those rows are held to a rounding bound instead, derived at mixed_wave_bound below.

Measured on an MI355X (rel-l2 over the steered rows; un-steered launch -> steered launch, the worst of the range sets; profiles/r20_attn_steer.txt):
    impl 0 bf16  N 330    2.298e-03 -> 2.383e-03  (ratio 0.82 .. 1.04; the fp64 answers 0.75 .. 0.995 apart, the bar 4.6e-03)
    impl 1 bf16  N 330    1.653e-03 -> 1.667e-03  (ratio 1.00 .. 1.01)
    impl 1 f32   N 330    4.281e-07 -> 5.291e-07  (ratio 0.81 .. 1.24)
    impl 1 f16   N 330    2.075e-04 -> 2.093e-04  (ratio 1.00 .. 1.01)
    impl 0 bf16  N 4700   2.329e-03 (attn_q4) -> 2.318e-03 (attn_pp<STEER>), ratio 1.00, the fp64 answers 0.985 apart
    impl 1 bf16  N 4700   1.655e-03 -> 1.660e-03
"""
import ctypes

import pytest
import torch

import attn_steer_ref as R
from oracle import attn_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SETS = R.range_sets()
LONG = (2, 1, 4700)
LONG_REC = R.Record([(3, 9, R.W_HI, R.S1), (226, 1576, 4.0, R.BOTH), (2000, 2100, R.W_LO, R.S0), (4600, 4700, R.W_HI, R.BOTH)], 1576, 4700)
_OUT = {}


def run(s2v, case, impl, rec=None):
    """rec None: today's un-steered launch (s2v_op_attention); else the steered one.  -> [B * N, H * 64] on the device, memoised (inputs are never written)"""
    key = (id(case), impl, None if rec is None else (tuple(rec.ranges), rec.q0, rec.q1))
    if key not in _OUT:
        _OUT[key] = launch(s2v, case, impl, rec)
    return _OUT[key]


def launch(s2v, case, impl, rec):
    L = s2v._lib
    B, H, N = case.B, case.H, case.N
    dt = L.DTYPE_OF[case.qkv.dtype]
    qd = case.qkv.to(DEV)
    out = torch.full((B * N, H * 64), float("nan"), dtype=case.qkv.dtype, device=DEV)
    vt = torch.zeros(B * H * 64 * ((N + 63) // 64 * 64), dtype=torch.bfloat16, device=DEV) if impl == 0 else None
    if rec is None:
        L.check(L.lib().s2v_op_attention(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, dt, impl, L.stream_ptr()))
    else:
        L.check(L.lib().s2v_op_attention_steer(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, dt, impl, ctypes.byref(rec.c(L)), L.stream_ptr()))
    torch.cuda.synchronize()
    return out


def qmode(impl, case):
    return "bf16" if impl == 0 else "natural"


def twice_the_unsteered_error(s2v, case, impl, rec, what, device="cpu", need_apart=True):
    qm = qmode(impl, case)
    rows = rec.steered_rows(case.B, case.N).reshape(-1)
    ref_u, ref_s = R.steered_reference(case, qm, None, device), R.steered_reference(case, qm, rec, device)
    got_s = run(s2v, case, impl, rec)
    assert torch.isfinite(got_s.float()).all(), f"{what}: non-finite output"
    err_u, err_s = R.rel_l2(run(s2v, case, impl), ref_u, rows), R.rel_l2(got_s, ref_s, rows)
    bar = 2 * err_u
    if not need_apart:
        # sign-code inputs: the un-steered answer is (nearly) a stored V row, so the un-steered error is far below what rounding a general answer
        # to the storage type costs, and a bias that takes a row's dominance away makes its answer general.  No kernel can beat the fp64 answer
        # rounded once to the storage type: twice THAT error is the floor of the bar (it comes from the references alone).  On the sharp case
        # with four ranges it is 1.442e-04 un-steered against 4.559e-04 steered -- the very figures the generic kernel measures
        # The MFMA kernel also rounds P to bf16 before P.V while its row sum keeps the fp32 p: where one key carries a row, the row comes out
        # times bf16(p) / p, a relative error uniform in +-2^-9 (rms 2^-9 / sqrt 3) -- unless p is a power of two, which it is exactly when the
        # row's own key set the running maximum.  Under the deferred maximum that depends on which tile raised the maximum last, and a biased
        # key can raise it before the row's own key arrives (sharp2, inside_one_tile: 2.17e-04 un-steered, 7.28e-04 steered).  Today's launch
        # rounds P the same way (randn: 2.3e-03 against an ideal 1.65e-03), so the format's own figure joins the floor for impl 0
        ideal = R.rel_l2(ref_s.to(case.qkv.dtype), ref_s, rows)
        p_round = 2.0 ** -9 / 3.0 ** 0.5 if impl == 0 else 0.0
        bar = max(bar, 2 * (ideal ** 2 + p_round ** 2) ** 0.5)
    apart = R.rel_l2(ref_u, ref_s, rows)
    print(f"MEASURED {what}: un-steered {err_u:.3e} steered {err_s:.3e} (ratio {err_s / err_u:.2f}, bar {bar:.3e}); fp64 answers {apart:.3e} apart")
    assert not need_apart or apart >= 100 * bar, f"{what}: vacuous -- the fp64 steered and un-steered answers are {apart:.3e} apart, under 100 x the bar {bar:.3e}"
    assert err_s <= bar, f"{what}: steered rel-l2 {err_s:.3e} > 2 x the un-steered launch's {err_u:.3e}"


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("impl,dt_name", [(0, "bf16"), (1, "bf16"), (1, "f32"), (1, "f16")])
def test_both_implementations_against_the_restatement_within_twice_the_unsteered_error(s2v, impl, dt_name):
    case = R.case("randn", dt_name)
    for name, rec in SETS.items():
        twice_the_unsteered_error(s2v, case, impl, rec, f"impl {impl} {dt_name} N 330 randn {name}")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("family", ["sharp", "sharp2"])
def test_sharp_inputs_within_twice_the_unsteered_error(s2v, family, impl):
    """the same 2 x bar where the un-steered error is not zero; the 100-bars condition cannot hold on these inputs (module docstring)"""
    case = R.case(family)
    for name, rec in SETS.items():
        twice_the_unsteered_error(s2v, case, impl, rec, f"impl {impl} bf16 N 330 {family} {name}", need_apart=False)


@pytest.mark.parametrize("impl", [0, 1])
def test_the_long_loop_beyond_the_attn_pp_switch(s2v, impl):
    case = R.case("randn", "bf16", LONG)
    twice_the_unsteered_error(s2v, case, impl, LONG_REC, f"impl {impl} bf16 N 4700 randn four ranges", DEV)


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("family", ["onehot", "sharp", "sharp2"])
def test_sign_code_inputs_one_hot_rows_trap_rows_and_sharp_rows(s2v, family, impl):
    """one-hot rows return V[pi(i)] to one ulp (no allowed weight changes a one-hot winner: margin >= 36 > ln 2^16); trap rows -- queries for a
    code of the 64 rows that follow their sample in memory, V = 1e4 there -- and sharp rows follow the steered restatement; a leak of a pad key
    or of the next sample takes a whole row"""
    case = R.case(family)
    qm = qmode(impl, case)
    B, H, N = case.B, case.H, case.N
    for name, rec in SETS.items():
        got = run(s2v, case, impl, rec).double().cpu()
        assert torch.isfinite(got).all(), f"{family} {name}: non-finite"
        ref = R.steered_reference(case, qm, rec)
        g4, r4 = got.reshape(B, N, H, 64), ref.reshape(B, N, H, 64)
        soft = case.trap if family == "onehot" else torch.ones(N, dtype=torch.bool)
        scale = torch.clamp(r4.abs().amax(dim=(1, 3), keepdim=True), min=1.0)
        err = ((g4 - r4).abs() / scale)[:, soft].max().item()
        assert err <= AC.SOFT_BARS["bf16"], f"{family} {name} impl {impl}: soft rows {err:.3e} of the sample-and-head scale"
        if family == "onehot":
            wmax = max(w for _, _, w, _ in rec.ranges)
            leak = case.leak(AC.SHRINK[qm]) * wmax
            assert leak <= 2.0 ** -14
            v = case.heads(2).transpose(1, 2)   # [B, N, H, 64]
            want = v[:, case.pi[~case.trap]]
            over = (g4[:, ~case.trap] - want).abs() - (AC.ulp_at(want, "bf16") + leak * v.abs().max())
            assert over.max().item() <= 0, f"{family} {name} impl {impl}: {int((over > 0).sum())} elements beyond one ulp of V[pi(i)]"


def test_a_large_weight_on_sharp_scores_crosses_the_deferred_maximum_threshold_inside_a_biased_tile(s2v):
    """the precondition, on the CPU: with w = 2^16 on [60, 200) more rows of the sharp2 case pass 2^64 above their first tile's maximum inside
    the range than without the bias -- the slow path runs on biased scores.  The result is held to the restatement above (sharp2 runs every set)"""
    with_bias, without = R.crossings(R.case("sharp2"), SETS["straddle_interior_straddle"])
    assert with_bias > without and with_bias >= 8
    case, rec = R.case("sharp2"), SETS["straddle_interior_straddle"]
    got, ref = run(s2v, case, 0, rec), R.steered_reference(case, "bf16", rec)
    assert R.rel_l2(got, ref) <= 6.3e-3, "the project's operator-level rel-l2 bar for bf16 attention (tests/test_gpu_parity.py)"


# ------------------------------------------------------------------------------------------------ 2. bit for bit
def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def mixed_wave_bound(case, got, plain):
    """un-steered rows of a wave whose vote a steered row changed: the same scores and the same softmax, but the running maximum moved at another
    tile, so every p is rounded to bf16 at another scale (2^-9 relative each, in both launches: 2^-8 of sum |p v| <= max|V| of the sample and
    head) and the output is rounded once more (one ulp).  got, plain [B, n, H * 64] -> elements beyond 2^-8 max|V| + one ulp"""
    B, H = case.B, case.H
    g, p = got.double().cpu().reshape(B, -1, H, 64), plain.double().cpu().reshape(B, -1, H, 64)
    vmax = case.heads(2).abs().amax(dim=(2, 3)).reshape(B, 1, H, 1)
    return int(((g - p).abs() > 2.0 ** -8 * vmax + AC.ulp_at(p, "bf16")).sum().item())


@pytest.mark.parametrize("family", ["randn", "onehot", "sharp", "sharp2"])
def test_unsteered_rows_equal_todays_launch_bit_for_bit(s2v, family):
    """N = 330 <= ATTN_PP_MAX_TOKENS: s2v_op_attention impl 0 runs attn_pp as well"""
    case = R.case(family)
    B, H, N = case.B, case.H, case.N
    plain = run(s2v, case, 0).reshape(B, N, H * 64)
    ones = R.Record([(k0, k1, 1.0, m) for k0, k1, _, m in SETS["four_ranges"].ranges], 37, 300)
    assert _bits(run(s2v, case, 0, ones).reshape(B, N, -1), plain), "a record of weights all 1"
    assert _bits(run(s2v, case, 0, R.Record([], 0, N)).reshape(B, N, -1), plain), "a record of no ranges"
    got = run(s2v, case, 0, SETS["one_sample"]).reshape(B, N, -1)
    assert _bits(got[1], plain[1]), "a sample outside every mask"
    assert not _bits(got[0], plain[0])
    rec = SETS["query_range"]   # rows [37, 300): waves 0 (rows 0 .. 31) and 10 (rows 320 .. 329) hold no steered row
    got = run(s2v, case, 0, rec).reshape(B, N, -1)
    assert _bits(got[:, :32], plain[:, :32]) and _bits(got[:, 320:], plain[:, 320:]), "the waves outside the query range"
    assert not _bits(got[:, 37:300], plain[:, 37:300])
    if R.crossings(case, R.Record(rec.ranges, 0, N)) == (0, 0):
        # no row of either launch takes a slow path past the first tile: the rows outside [37, 300) of the two mixed waves are equal as well
        assert _bits(got[:, :37], plain[:, :37]) and _bits(got[:, 300:], plain[:, 300:]), "rows outside the query range inside a steered wave"
    else:   # rows of either launch pass the threshold: within rounding of today's launch (mixed_wave_bound), not its bits
        assert family in ("onehot", "sharp2")
        for lo, hi in ((32, 37), (300, 320)):
            assert mixed_wave_bound(case, got[:, lo:hi], plain[:, lo:hi]) == 0, f"rows [{lo}, {hi}) outside the query range inside a steered wave"
    # the generic form: every un-steered row, always
    g1, p1 = run(s2v, case, 1, rec).reshape(B, N, -1), run(s2v, case, 1).reshape(B, N, -1)
    assert _bits(g1[:, :37], p1[:, :37]) and _bits(g1[:, 300:], p1[:, 300:]) and not _bits(g1[:, 37:300], p1[:, 37:300])


def test_two_runs_give_the_same_bits(s2v):
    for family, shape in (("randn", R.SHAPE), ("sharp2", R.SHAPE), ("randn", LONG)):
        case = R.case(family, "bf16", shape)
        rec = LONG_REC if shape == LONG else SETS["four_ranges"]
        for impl in (0, 1):
            assert _bits(launch(s2v, case, impl, rec), launch(s2v, case, impl, rec)), f"{family} N {shape[2]} impl {impl}"


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_bad_records_are_refused_by_name(s2v):
    L = s2v._lib
    case = R.case("randn")
    qd = case.qkv.to(DEV)
    out = torch.zeros(660, 128, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(2 * 2 * 64 * 384, dtype=torch.bfloat16, device=DEV)

    def refused(rec, match, impl=0, dt=L.DTYPE_BF16, B=2):
        with pytest.raises(s2v.S2VError, match=match):
            L.check(L.lib().s2v_op_attention_steer(L.ptr(qd), L.ptr(vt), L.ptr(out), B, 2, 330, dt, impl, ctypes.byref(rec.c(L)), L.stream_ptr()))

    refused(R.Record([(70, 100, 2.0, 3), (90, 120, 2.0, 3)], 0, 330), r"key range 1 = \[90, 120\) overlaps or precedes range 0")
    refused(R.Record([(200, 220, 2.0, 3), (70, 100, 2.0, 3)], 0, 330), r"overlaps or precedes")
    refused(R.Record([(300, 331, 2.0, 3)], 0, 330), r"must be non-empty and inside \[0, Ntok = 330\)")
    refused(R.Record([(70, 100, 0.0, 3)], 0, 330), r"weight 0 = 0 must be finite and inside \[2\^-16, 2\^16\] \(no w = 0\)")
    refused(R.Record([(70, 100, 2.0 ** 17, 3)], 0, 330), r"weight 0 = 131072 must be finite")
    refused(R.Record([(70, 100, float("nan"), 3)], 0, 330), r"must be finite")
    refused(R.Record([(70, 100, 2.0, 3)], 0, 331), r"the query range \[0, 331\) must lie inside")
    refused(R.Record([(70, 100, 2.0, 3)], 0, 330), r"impl 0 is bf16", dt=L.DTYPE_F32)
    refused(R.Record([(70, 100, 2.0, 3)], 0, 330), r"1 <= B <= 32", B=33)
    # the process-wide record table is ordered on the stream of the first call: another stream is refused
    run(s2v, case, 0, SETS["tile_aligned"])
    side = torch.cuda.Stream()
    rec = R.Record([(70, 100, 2.0, 3)], 0, 330).c(L)
    with pytest.raises(s2v.S2VError, match=r"s2v_op_attention_steer: another stream than the first call's"):
        L.check(L.lib().s2v_op_attention_steer(L.ptr(qd), L.ptr(vt), L.ptr(out), 2, 2, 330, L.DTYPE_BF16, 0, ctypes.byref(rec), ctypes.c_void_p(side.cuda_stream)))
    torch.cuda.synchronize()
    assert (out == 0).all(), "a refused call launches nothing"
