"""Local attention in time on the GPU, kernel level: s2v_op_attention_local impl 0 (attn_pp<LOCAL>, bf16) and impl 1 (the local generic kernel)
against the fp64 restatement of tests/attn_local_ref.py.

Shape B = 2, H = 2, P = 20, S = 150, F = 5 (Ntok = 770: 13 key tiles with a ragged last one of 2 keys, 4 work items with a ragged last one of 2
rows) with the tables of attn_local_ref.tables(); one longer launch, B = 2, H = 14, Ntok = 4693 (P = 226 + 247, S = 422, F = 10, frames = 1: 74
key tiles, 19 x 28 = 532 work items, more than two per CU, so impl 0 runs the persistent form there as a context does).

The error bar is the project's "2 x measured": the local launch's rel-l2 against the local restatement may be at most twice the rel-l2 of
today's un-windowed launch (s2v_op_attention) against the dense restatement on the same inputs, measured in the same run over the same rows.
The guard: the two restatements must lie at least 4 bars apart over the windowed rows, or the test fails as vacuous.

Measured on an MI355X (rel-l2 over the windowed rows, un-windowed -> local; profiles/r21_attn_local.txt):
    impl 0 bf16  N 770    2.318e-03 -> 2.042e-03 .. 2.328e-03 over the ten tables (ratio 0.88 .. 1.00), the fp64 answers 0.70 .. 0.97 apart
    impl 1 bf16  N 770    1.660e-03 -> 1.649e-03 .. 1.661e-03
    impl 1 f32   N 770    5.765e-07 -> 2.184e-07 .. 4.494e-07 (fewer keys, fewer roundings)
    impl 0 bf16  N 4693   2.331e-03 (attn_q4) -> 2.339e-03 (attn_pp<LOCAL>, persistent), the fp64 answers 0.81 apart
    impl 1 bf16  N 4693   1.656e-03 -> 1.659e-03
"""
import pytest
import torch

import attn_local_ref as R
from oracle import attn_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLES = R.tables()
LONG = (2, 14, 4693)
LONG_TAB = R.frames_table(226, 247, 10, 422, 1)
_OUT = {}


def launch(s2v, case, impl, tab):
    """tab None: today's un-windowed launch (s2v_op_attention); else the local one.  -> [B * N, H * 64] on the device"""
    L = s2v._lib
    B, H, N = case.B, case.H, case.N
    dt = L.DTYPE_OF[case.qkv.dtype]
    qd = case.qkv.to(DEV)
    out = torch.full((B * N, H * 64), float("nan"), dtype=case.qkv.dtype, device=DEV)
    vt = torch.zeros(B * H * 64 * ((N + 63) // 64 * 64), dtype=torch.bfloat16, device=DEV) if impl == 0 else None
    if tab is None:
        L.check(L.lib().s2v_op_attention(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, dt, impl, L.stream_ptr()))
    else:
        P, lo, hi = tab.c()
        L.check(L.lib().s2v_op_attention_local(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, dt, impl, P, lo, hi, L.stream_ptr()))
    torch.cuda.synchronize()
    return out


def run(s2v, case, impl, tab=None):
    """memoised (inputs are never written)"""
    key = (id(case), impl, None if tab is None else tab.key())
    if key not in _OUT:
        _OUT[key] = launch(s2v, case, impl, tab)
    return _OUT[key]


def qmode(impl):
    return "bf16" if impl == 0 else "natural"


_REFS = {}


def ref(case, qm, tab, device="cpu"):
    key = (id(case), qm, None if tab is None else tab.key())
    if key not in _REFS:
        _REFS[key] = R.local_reference(case, qm, tab, device)
    return _REFS[key]


def twice_the_unwindowed_error(s2v, case, impl, tab, what, device="cpu"):
    qm = qmode(impl)
    rows = tab.windowed_rows().repeat(case.B)
    ref_d, ref_l = ref(case, qm, None, device), ref(case, qm, tab, device)
    got = run(s2v, case, impl, tab)
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    err_d, err_l = R.rel_l2(run(s2v, case, impl), ref_d, rows), R.rel_l2(got, ref_l, rows)
    err_all = R.rel_l2(got, ref_l)
    bar = 2 * err_d
    apart = R.rel_l2(ref_d, ref_l, rows)
    print(f"MEASURED {what}: un-windowed {err_d:.3e} local {err_l:.3e} (ratio {err_l / err_d:.2f}, bar {bar:.3e}; every row {err_all:.3e}); "
          f"fp64 answers {apart:.3e} apart")
    assert apart >= 4 * bar, f"{what}: vacuous -- the fp64 local and dense answers are {apart:.3e} apart, under 4 x the bar {bar:.3e}"
    assert err_l <= bar, f"{what}: local rel-l2 {err_l:.3e} > 2 x the un-windowed launch's {err_d:.3e}"
    assert err_all <= 2 * R.rel_l2(run(s2v, case, impl), ref_d), f"{what}: every row, dense ones included"


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("impl,dt_name", [(0, "bf16"), (1, "bf16"), (1, "f32")])
def test_both_implementations_against_the_restatement_within_twice_the_unwindowed_error(s2v, impl, dt_name):
    case = R.case("randn", dt_name)
    assert R.visits(TABLES["frames0"]) == R.VISITS_FRAMES0
    for name, tab in TABLES.items():
        twice_the_unwindowed_error(s2v, case, impl, tab, f"impl {impl} {dt_name} N {R.N0} randn {name}")


@pytest.mark.parametrize("impl", [0, 1])
def test_the_long_loop_in_the_persistent_form(s2v, impl):
    assert LONG_TAB.N == LONG[2] and LONG_TAB.P % 64 and 422 % 64
    case = R.case("randn", "bf16", LONG)
    twice_the_unwindowed_error(s2v, case, impl, LONG_TAB, f"impl {impl} bf16 N {LONG[2]} randn frames 1", DEV)


# ------------------------------------------------------------------------------------------------ 2. bit for bit
def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("family", ["randn", "onehot", "sharp"])
def test_a_table_that_windows_nothing_returns_the_dense_launch_bit_for_bit(s2v, family):
    """N = 770 <= ATTN_PP_MAX_TOKENS: s2v_op_attention impl 0 runs attn_pp as well"""
    case = R.case(family)
    plain = run(s2v, case, 0)
    for P in (1, 20, 64, 100, R.N0):
        assert _bits(run(s2v, case, 0, R.dense_table(R.N0, P)), plain), f"every row dense, P = {P}"
    assert _bits(run(s2v, case, 1, R.dense_table(R.N0, 20)), run(s2v, case, 1)), "the generic form"


@pytest.mark.parametrize("family", ["randn", "onehot", "sharp"])
def test_a_dense_wave_inside_a_table_that_windows_the_other_waves_returns_the_dense_bits(s2v, family):
    case = R.case(family)
    B, H, N = case.B, case.H, case.N
    plain = run(s2v, case, 0).reshape(B, N, -1)
    got = run(s2v, case, 0, TABLES["dense_wave_then_frames0"]).reshape(B, N, -1)
    assert _bits(got[:, :32], plain[:, :32]), "rows 0 .. 31: a wholly dense wave"
    assert not _bits(got[:, 32:], plain[:, 32:])
    got = run(s2v, case, 0, TABLES["frames0"]).reshape(B, N, -1)
    assert not _bits(got[:, 20:32], plain[:, 20:32]), "the same rows windowed"


def test_two_runs_give_the_same_bits(s2v):
    for shape, tab in ((R.SHAPE, TABLES["frames0"]), (LONG, LONG_TAB)):
        case = R.case("randn", "bf16", shape)
        for impl in (0, 1):
            assert _bits(launch(s2v, case, impl, tab), run(s2v, case, impl, tab)), f"N {shape[2]} impl {impl}"


# ------------------------------------------------------------------------------------------------ 3. one-hot rows
@pytest.mark.parametrize("impl", [0, 1])
def test_one_hot_rows_return_their_own_value_row_and_nothing_leaks(s2v, impl):
    """every window holds the row's own key pi(i) (a row whose key lies in the prefix has an empty window): a non-trap row returns V[pi(i)] to one
    ulp; the trap rows -- queries for a code of the 64 rows that follow their sample in memory, V = 1e4 there -- follow the local restatement: a
    leak of a pad key or of the next sample takes a whole row (oracle.attn_cases.failures' rules)"""
    case = R.case("onehot")
    qm = qmode(impl)
    B, H, N = case.B, case.H, case.N
    tab = R.around_own_key(case)
    vis = R.visible(tab)
    assert bool(vis[torch.arange(N), case.pi].all()) and not bool(vis.all(dim=1)[R.P0:].any())
    got = run(s2v, case, impl, tab).double().cpu()
    assert torch.isfinite(got).all()
    g4, r4 = got.reshape(B, N, H, 64), R.local_reference(case, qm, tab).reshape(B, N, H, 64)
    scale = torch.clamp(r4.abs().amax(dim=(1, 3), keepdim=True), min=1.0)
    err = ((g4 - r4).abs() / scale)[:, case.trap].max().item()
    assert err <= AC.SOFT_BARS["bf16"], f"impl {impl}: trap rows {err:.3e} of the sample-and-head scale"
    leak = case.leak(AC.SHRINK[qm])
    assert leak <= AC.LEAK_MAX
    v = case.heads(2).transpose(1, 2)   # [B, N, H, 64]
    want = v[:, case.pi[~case.trap]]
    over = (g4[:, ~case.trap] - want).abs() - (AC.ulp_at(want, "bf16") + leak * v.abs().max())
    assert over.max().item() <= 0, f"impl {impl}: {int((over > 0).sum())} elements beyond one ulp of V[pi(i)]"


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_bad_tables_are_refused_by_name_and_launch_nothing(s2v):
    L = s2v._lib
    case = R.case("randn")
    qd = case.qkv.to(DEV)
    out = torch.zeros(2 * R.N0, 128, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(2 * 2 * 64 * 832, dtype=torch.bfloat16, device=DEV)
    for tab, match in R.bad_tables():
        P, lo, hi = tab.c()
        with pytest.raises(s2v.S2VError, match="s2v_op_attention_local: " + match):
            L.check(L.lib().s2v_op_attention_local(L.ptr(qd), L.ptr(vt), L.ptr(out), 2, 2, R.N0, L.DTYPE_BF16, 0, P, lo, hi, L.stream_ptr()))
    P, lo, hi = TABLES["frames0"].c()
    with pytest.raises(s2v.S2VError, match=r"impl 0 is bf16"):
        L.check(L.lib().s2v_op_attention_local(L.ptr(qd), L.ptr(vt), L.ptr(out), 2, 2, R.N0, L.DTYPE_F32, 0, P, lo, hi, L.stream_ptr()))
    torch.cuda.synchronize()
    assert (out == 0).all(), "a refused call launches nothing"
