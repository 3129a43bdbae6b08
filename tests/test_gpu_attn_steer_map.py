"""Steering maps at kernel level (pytest -m gpu): s2v_op_attention_steer_map impl 0 (attn_pp<MAP>, bf16) and impl 1 (the mapped generic kernel)
against the scalar entry (constant planes, bit for bit), the fp64 restatement of tests/attn_steer_map_ref.py (per-row planes) and the
un-steered launch (dead waves, bit for bit).

Shapes: attn_steer_ref.SHAPE = B 2, H 2, N 330 -- six key tiles with a ragged last one, two query items with a ragged last one -- and
B 2, H 1, N 4700 for the long loop and the persistent form: impl 0 runs attn_pp_steer_map_k, one workgroup per item; impl 2 runs the persistent
twin attn_pp_steer_map_persist_k (the engine's launch beyond two rounds of items) on a queue of the process, at any item count.

The bar of the per-row records is not fixed here: the relative L2 error over the steered rows may be at most twice the error of today's
un-steered launch against its own restatement, both measured in the same run on the same inputs.  Condition on the inputs, asserted on the CPU
before the launch: the mapped restatement lies at least four such bars from the un-steered restatement and from the constant-plane restatement
at each plane's geometric-mean weight, so a kernel that ignores the cell cannot pass.

MEASURED on an MI355X (rel-l2 over the steered rows; un-steered launch -> mapped launch, best .. worst of the nine per-row records;
profiles/r23_attn_steer_map.txt keeps every line):
    impl 0 bf16  N 330    2.298e-03 -> 1.905e-03 .. 2.373e-03  (ratio 0.83 .. 1.03; the bar 4.6e-03; the restatements 0.67 .. 0.96 apart)
    impl 1 bf16  N 330    1.653e-03 -> 1.649e-03 .. 1.672e-03  (ratio 1.00 .. 1.01)
    impl 1 f32   N 330    4.281e-07 -> 3.457e-07 .. 4.989e-07  (ratio 0.81 .. 1.17)
    impl 0 bf16  N 4700   2.329e-03 (attn_q4) -> 2.129e-03 (attn_pp<MAP>), ratio 0.91, the restatements 0.98 apart
    impl 1 bf16  N 4700   1.655e-03 -> 1.664e-03
"""
import ctypes

import pytest
import torch

import attn_steer_map_ref as M
import attn_steer_ref as R
from oracle import attn_cases as AC
from test_gpu_attn_steer import DEV, LONG, SETS, _bits, mixed_wave_bound, qmode
from test_gpu_attn_steer import run as run_scalar

pytestmark = pytest.mark.gpu
RECS = M.map_records()
PER_ROW = [n for n in RECS if n != "liveness"]
_OUT = {}


def launch(s2v, case, impl, rec):
    L = s2v._lib
    B, H, N = case.B, case.H, case.N
    dt = L.DTYPE_OF[case.qkv.dtype]
    qd = case.qkv.to(DEV)
    out = torch.full((B * N, H * 64), float("nan"), dtype=case.qkv.dtype, device=DEV)
    vt = torch.zeros(B * H * 64 * ((N + 63) // 64 * 64), dtype=torch.bfloat16, device=DEV) if impl != 1 else None
    r, planes, keep = rec.c(L)
    L.check(L.lib().s2v_op_attention_steer_map(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, dt, impl, ctypes.byref(r), planes, L.stream_ptr()))
    torch.cuda.synchronize()
    return out


def run(s2v, case, impl, rec):
    key = (id(case), impl, rec.key())
    if key not in _OUT:
        _OUT[key] = launch(s2v, case, impl, rec)
    return _OUT[key]


def twice_the_unsteered_error(s2v, case, impl, rec, what, device="cpu"):
    plain_impl = 0 if impl == 2 else impl   # the persistent form (impl 2) is held against the same un-steered launch as impl 0
    qm = qmode(plain_impl, case)
    rows = rec.steered_rows(case.B, case.N).reshape(-1)
    ref_u, ref_s = M.map_reference(case, qm, None, device), M.map_reference(case, qm, rec, device)
    gm = M.MapRecord(rec.ranges, torch.stack([torch.full_like(p, M.geometric_mean_weight(p)) for p in rec.planes]), rec.q0, rec.q1)
    ref_c = M.map_reference(case, qm, gm, device)
    err_u = R.rel_l2(run_scalar(s2v, case, plain_impl), ref_u, rows)
    bar = 2 * err_u   # the same floor as test_gpu_attn_steer.twice_the_unsteered_error on inputs that must lie apart: none
    apart_u, apart_c = R.rel_l2(ref_u, ref_s, rows), R.rel_l2(ref_c, ref_s, rows)
    assert apart_u >= 4 * bar and apart_c >= 4 * bar, (f"{what}: vacuous -- the mapped restatement is {apart_u:.3e} from the un-steered one and {apart_c:.3e} from the "
                                                       f"constant plane, under 4 x the bar {bar:.3e}")
    got = run(s2v, case, impl, rec)
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    err_s = R.rel_l2(got, ref_s, rows)
    print(f"MEASURED {what}: un-steered {err_u:.3e} mapped {err_s:.3e} (ratio {err_s / err_u:.2f}, bar {bar:.3e}); restatements {apart_u:.3e} / {apart_c:.3e} apart")
    assert err_s <= bar, f"{what}: mapped rel-l2 {err_s:.3e} > 2 x the un-steered launch's {err_u:.3e}"


# ------------------------------------------------------------------------------------------------ 1. constant planes: the scalar entry's bits
@pytest.mark.parametrize("impl,dt_name", [(0, "bf16"), (1, "bf16"), (1, "f32")])
def test_constant_planes_equal_the_scalar_entry_bit_for_bit(s2v, impl, dt_name):
    case = R.case("randn", dt_name)
    for name, srec in SETS.items():
        assert _bits(run(s2v, case, impl, M.constant_record(srec)), run_scalar(s2v, case, impl, srec)), f"impl {impl} {dt_name} {name}"
    sharp = R.case("sharp2")
    if dt_name == "bf16":
        for name in ("straddle_interior_straddle", "four_ranges"):
            assert _bits(run(s2v, sharp, impl, M.constant_record(SETS[name])), run_scalar(s2v, sharp, impl, SETS[name])), f"sharp2 impl {impl} {name}"


# ------------------------------------------------------------------------------------------------ 2. per-row planes against the restatement
@pytest.mark.parametrize("impl,dt_name", [(0, "bf16"), (1, "bf16"), (1, "f32")])
def test_per_row_planes_against_the_restatement_within_twice_the_unsteered_error(s2v, impl, dt_name):
    case = R.case("randn", dt_name)
    for name in PER_ROW:
        twice_the_unsteered_error(s2v, case, impl, RECS[name], f"impl {impl} {dt_name} N 330 randn {name}")


LONG_MAP = M.MapRecord([(3, 9, [-1, 0]), (226, 1576, [1, 1]), (2000, 2100, [2, -1]), (4600, 4700, [3, 3])],
                       torch.stack([M.pow2_plane(3124, s) for s in (31, 32, 33, 34)]), 1576, 4700)


@pytest.mark.parametrize("impl", [0, 1, 2])
def test_the_long_loop_with_four_mapped_ranges(s2v, impl):
    """impl 2 is attn_pp_steer_map_persist_k: the persistent launch the engine takes beyond two rounds of items, here on 38 items"""
    case = R.case("randn", "bf16", LONG)
    twice_the_unsteered_error(s2v, case, impl, LONG_MAP, f"impl {impl} bf16 N 4700 randn four mapped ranges", DEV)


def test_the_persistent_launch_returns_the_bits_of_the_launch_per_item(s2v):
    """the same work items pulled from a queue: N 4700 (38 items, most workgroups find none), N 330 with every record (edge tiles, dead waves, a
    sample without planes), and twice in a row -- the last workgroup to leave must have zeroed the queue for the next launch"""
    long = R.case("randn", "bf16", LONG)
    assert _bits(run(s2v, long, 2, LONG_MAP), run(s2v, long, 0, LONG_MAP))
    assert _bits(launch(s2v, long, 2, LONG_MAP), run(s2v, long, 0, LONG_MAP)), "a second persistent launch"
    for family in ("randn", "sharp2"):
        case = R.case(family)
        for name, rec in RECS.items():
            assert _bits(run(s2v, case, 2, rec), run(s2v, case, 0, rec)), f"{family} {name}"


# ------------------------------------------------------------------------------------------------ 3. liveness
@pytest.mark.parametrize("family", ["randn", "sharp2"])
def test_dead_waves_equal_the_unsteered_launch_bit_for_bit(s2v, family):
    """N = 330 <= ATTN_PP_MAX_TOKENS: s2v_op_attention impl 0 runs attn_pp.  The liveness record is 1 on the rows [64, 96), [32, 40) and on all of
    item 1, random elsewhere"""
    case = R.case(family)
    B, H, N = case.B, case.H, case.N
    plain = run_scalar(s2v, case, 0).reshape(B, N, H * 64)
    got = run(s2v, case, 0, RECS["liveness"]).reshape(B, N, -1)
    assert _bits(got[:, 64:96], plain[:, 64:96]), "a wave whose weights are all 1"
    assert _bits(got[:, 256:], plain[:, 256:]), "an item whose weights are all 1"
    assert not _bits(got[:, :64], plain[:, :64]) and not _bits(got[:, 96:256], plain[:, 96:256])
    off = run(s2v, case, 0, RECS["sample_1_off"]).reshape(B, N, -1)
    assert _bits(off[1], plain[1]) and not _bits(off[0], plain[0]), "a sample whose planes are all -1"
    ones = M.MapRecord(RECS["four_ranges_four_planes"].ranges, torch.ones(4, N), 0, N)
    assert _bits(run(s2v, case, 0, ones).reshape(B, N, -1), plain), "planes of ones"
    # every row of weight 1 inside a live wave (the rows [32, 40) and those whose random weight came out as 2^0, found from the record itself): 0.0f is added to its scores, and it is
    # held to the rounding bound of the scalar test (mixed_wave_bound); its bits are the un-steered launch's as well when, by the record under
    # test, no row of either launch passes the deferred-maximum threshold past the first tile
    rec = RECS["liveness"]
    flags = M.wave_flags_bruteforce(rec, N)
    mixed = torch.tensor([bool(flags[0, i // 32]) and float(rec.planes[0, i]) == 1.0 for i in range(N)])
    assert set(range(32, 40)) <= set(mixed.nonzero().flatten().tolist()), "and the rows whose random weight is 2^0"
    assert mixed_wave_bound(case, got[:, mixed], plain[:, mixed]) == 0, "rows of weight 1 inside a live wave"
    if M.map_crossings(case, rec) == (0, 0):
        assert _bits(got[:, mixed], plain[:, mixed]), "rows of weight 1 inside a live wave, no slow path past the first tile in either launch"
    assert family != "randn" or M.map_crossings(case, rec) == (0, 0), "randn scores stay far below the threshold: the bit check above must have run"
    # the generic form reads no table: ln 1 = 0.0f is added, the same bits on every row of weight 1
    g1, p1 = run(s2v, case, 1, RECS["liveness"]).reshape(B, N, -1), run_scalar(s2v, case, 1).reshape(B, N, -1)
    assert _bits(g1[:, 64:96], p1[:, 64:96]) and _bits(g1[:, 256:], p1[:, 256:]) and _bits(g1[:, 32:40], p1[:, 32:40]) and not _bits(g1[:, :32], p1[:, :32])


# ------------------------------------------------------------------------------------------------ 4. sign-code inputs
@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("family", ["onehot", "sharp", "sharp2"])
def test_sign_code_inputs_under_random_planes(s2v, family, impl):
    """one-hot rows return V[pi(i)] to one ulp (margin >= 36 natural units > ln 2^16 under any plane); soft rows follow the mapped restatement
    within oracle.attn_cases.SOFT_BARS; a leak of a pad key, a trap row or the next sample takes a whole row"""
    case = R.case(family)
    qm = qmode(impl, case)
    B, H, N = case.B, case.H, case.N
    for name in ("four_ranges_four_planes", "plane_per_sample", "ragged_tile", "query_range"):
        rec = RECS[name]
        got = run(s2v, case, impl, rec).double().cpu()
        assert torch.isfinite(got).all(), f"{family} {name}: non-finite"
        ref = M.map_reference(case, qm, rec)
        g4, r4 = got.reshape(B, N, H, 64), ref.reshape(B, N, H, 64)
        soft = case.trap if family == "onehot" else torch.ones(N, dtype=torch.bool)
        scale = torch.clamp(r4.abs().amax(dim=(1, 3), keepdim=True), min=1.0)
        err = ((g4 - r4).abs() / scale)[:, soft].max().item()
        assert err <= AC.SOFT_BARS["bf16"], f"{family} {name} impl {impl}: soft rows {err:.3e} of the sample-and-head scale"
        if family == "onehot":
            leak = case.leak(AC.SHRINK[qm]) * float(rec.planes.max())
            assert leak <= 2.0 ** -14
            v = case.heads(2).transpose(1, 2)   # [B, N, H, 64]
            want = v[:, case.pi[~case.trap]]
            over = (g4[:, ~case.trap] - want).abs() - (AC.ulp_at(want, "bf16") + leak * v.abs().max())
            assert over.max().item() <= 0, f"{family} {name} impl {impl}: {int((over > 0).sum())} elements beyond one ulp of V[pi(i)]"


# ------------------------------------------------------------------------------------------------ 5. determinism and refusals
def test_two_runs_give_the_same_bits(s2v):
    for family, shape, rec in (("randn", R.SHAPE, RECS["four_ranges_four_planes"]), ("sharp2", R.SHAPE, RECS["plane_per_sample"]), ("randn", LONG, LONG_MAP)):
        case = R.case(family, "bf16", shape)
        for impl in (0, 1):
            assert _bits(launch(s2v, case, impl, rec), launch(s2v, case, impl, rec)), f"{family} N {shape[2]} impl {impl}"


def test_bad_records_are_refused_by_name(s2v):
    L = s2v._lib
    case = R.case("randn")
    qd = case.qkv.to(DEV)
    out = torch.zeros(660, 128, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(2 * 2 * 64 * 384, dtype=torch.bfloat16, device=DEV)
    two = torch.full((2, 330), 2.0)
    ok = M.MapRecord([(70, 100, [0, 1])], two, 0, 330)

    def refused(rec, match, impl=0, dt=L.DTYPE_BF16, n_planes=None, planes=True):
        r, pp, keep = rec.c(L, n_planes)
        with pytest.raises(s2v.S2VError, match=match):
            L.check(L.lib().s2v_op_attention_steer_map(L.ptr(qd), L.ptr(vt), L.ptr(out), 2, 2, 330, dt, impl, ctypes.byref(r), pp if planes else None, L.stream_ptr()))

    refused(ok, r"1\.\.16 planes are accepted \(n_planes = 0\)", n_planes=0)
    refused(ok, r"1\.\.16 planes are accepted \(n_planes = 17\)", n_planes=17)
    refused(M.MapRecord([(70, 100, [0, 2])], two, 0, 330), r"plane index 2 of range 0, sample 1 lies outside \[-1, n_planes = 2\)")
    refused(ok, r"null plane pointer", planes=False)
    for w, shown in ((float("nan"), "nan"), (0.0, "0"), (2.0 ** -17, r"7\.62939e-06"), (2.0 ** 17, "131072")):
        bad = two.clone()
        bad[1, 217] = w
        refused(M.MapRecord([(70, 100, [0, 1])], bad, 0, 330), rf"plane 1, cell 217: weight {shown} must be finite and inside \[2\^-16, 2\^16\] \(no w = 0\)")
    refused(M.MapRecord([(70, 100, [0, 0]), (90, 120, [0, 0])], two, 0, 330), r"key range 1 = \[90, 120\) overlaps or precedes range 0")
    refused(ok, r"impl 0 is bf16", dt=L.DTYPE_F32)
    # the process-wide record table is ordered on the stream of the first call: another stream is refused
    run(s2v, case, 0, RECS["inside_one_tile"])
    side = torch.cuda.Stream()
    r, pp, keep = ok.c(L)
    with pytest.raises(s2v.S2VError, match=r"s2v_op_attention_steer_map: another stream than the first call's"):
        L.check(L.lib().s2v_op_attention_steer_map(L.ptr(qd), L.ptr(vt), L.ptr(out), 2, 2, 330, L.DTYPE_BF16, 0, ctypes.byref(r), pp, ctypes.c_void_p(side.cuda_stream)))
    torch.cuda.synchronize()
    assert (out == 0).all(), "a refused call launches nothing"
