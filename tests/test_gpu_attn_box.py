"""Local attention in space and time on the GPU, kernel level: s2v_op_attention_box impl 0 (attn_pp<BOX>, bf16) and impl 1 (the generic box kernel)
against the fp64 restatement of tests/attn_box_ref.py.

Shape B = 2, H = 2, P = 20, S = 150 (10 patch rows of 15), F = 5 (Ntok = 770: 13 key tiles with a ragged last one of 2 keys, 4 work items with a
ragged last one of 2 rows; every frame boundary inside a tile) with the tables of attn_box_ref.tables(); one longer launch, B = 2, H = 14, P = 473,
S = 420 (20 x 21), F = 10 (Ntok = 4673: 74 key tiles with a ragged one of 1 key, 19 x 28 = 532 work items, more than two per CU, so impl 0 runs
the persistent form there as a context does).

The error bar is the project's "2 x measured": the box launch's rel-l2 against the box restatement may be at most twice the rel-l2 of today's
un-windowed launch (s2v_op_attention) against the dense restatement on the same inputs, measured in the same run over the same rows.  The guard:
the box restatement must lie at least 4 bars from the dense restatement (over the rows that do not see everything) and from the temporal-only
restatement of the same lo / hi (over the rows the offsets narrow), or the test fails as vacuous.

Measured on an MI355X (rel-l2 over the windowed rows, un-windowed -> box):
    impl 0 bf16  N 770    2.318e-03 -> 2.059e-03 .. 2.326e-03 over the thirteen tables (ratio 0.89 .. 1.00); the fp64 box answer 0.76 .. 0.98
                          from the dense one and 0.36 .. 0.90 from the temporal-only one (the least at ends_in_ragged_tile), four bars are 1.9e-02
    impl 1 bf16  N 770    1.660e-03 -> 1.656e-03 .. 1.663e-03
    impl 1 f32   N 770    5.765e-07 -> 2.165e-07 .. 4.218e-07 (fewer keys, fewer roundings)
    impl 0 bf16  N 4673   2.333e-03 (attn_q4) -> 2.329e-03 (attn_pp<BOX>, persistent); the fp64 answers 0.92 / 0.74 apart
    impl 1 bf16  N 4673   1.656e-03 -> 1.661e-03
One-hot and sharp rows with a box around their own key, largest |out - V[pi(i)]| over the 194 560 non-trap elements (bar: one bf16 ulp of
V[pi(i)] plus the tail; the tail of sharp is the fp64 restatement's own distance from V[pi(i)], 2.7e-06):
    impl 0 onehot 0 (every element exact)      impl 0 sharp 1.562e-02 = 1.000 x its bar on the worst element, none beyond
    impl 1 onehot 0                            impl 1 sharp 0
"""
import pytest
import torch

import attn_box_ref as X
import attn_local_ref as R
from oracle import attn_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLES = X.tables()
LONG = (2, 14, 4673)
LONG_TAB = X.box_table(226, 247, 10, 20, 21, 1, 2)
_OUT = {}


def launch(s2v, case, impl, tab):
    """tab None: today's un-windowed launch (s2v_op_attention); a BoxTable: the box launch; an attn_local_ref.Table: the window launch.
    -> [B * N, H * 64] on the device"""
    L = s2v._lib
    B, H, N = case.B, case.H, case.N
    dt = L.DTYPE_OF[case.qkv.dtype]
    qd = case.qkv.to(DEV)
    out = torch.full((B * N, H * 64), float("nan"), dtype=case.qkv.dtype, device=DEV)
    vt = torch.zeros(B * H * 64 * ((N + 63) // 64 * 64), dtype=torch.bfloat16, device=DEV) if impl == 0 else None
    if tab is None:
        L.check(L.lib().s2v_op_attention(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, dt, impl, L.stream_ptr()))
    elif isinstance(tab, X.BoxTable):
        L.check(L.lib().s2v_op_attention_box(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, dt, impl, *tab.c(), L.stream_ptr()))
    else:
        L.check(L.lib().s2v_op_attention_local(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, dt, impl, *tab.c(), L.stream_ptr()))
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
        _REFS[key] = X.box_reference(case, qm, tab, device) if isinstance(tab, X.BoxTable) else R.local_reference(case, qm, tab, device)
    return _REFS[key]


def twice_the_unwindowed_error(s2v, case, impl, tab, what, device="cpu"):
    qm = qmode(impl)
    rows, narrowed = tab.windowed_rows().repeat(case.B), tab.narrowed_rows().repeat(case.B)
    ref_d, ref_t, ref_b = ref(case, qm, None, device), ref(case, qm, tab.temporal(), device), ref(case, qm, tab, device)
    got = run(s2v, case, impl, tab)
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    err_d, err_b = X.rel_l2(run(s2v, case, impl), ref_d, rows), X.rel_l2(got, ref_b, rows)
    err_all = X.rel_l2(got, ref_b)
    bar = 2 * err_d
    apart_d, apart_t = X.rel_l2(ref_d, ref_b, rows), X.rel_l2(ref_t, ref_b, narrowed)
    print(f"MEASURED {what}: un-windowed {err_d:.3e} box {err_b:.3e} (ratio {err_b / err_d:.2f}, bar {bar:.3e}; every row {err_all:.3e}); "
          f"the fp64 box answer {apart_d:.3e} from the dense, {apart_t:.3e} from the temporal one")
    assert apart_d >= 4 * bar, f"{what}: vacuous -- the fp64 box and dense answers are {apart_d:.3e} apart, under 4 x the bar {bar:.3e}"
    assert apart_t >= 4 * bar, f"{what}: vacuous -- the fp64 box and temporal answers are {apart_t:.3e} apart, under 4 x the bar {bar:.3e}"
    assert err_b <= bar, f"{what}: box rel-l2 {err_b:.3e} > 2 x the un-windowed launch's {err_d:.3e}"
    assert err_all <= 2 * X.rel_l2(run(s2v, case, impl), ref_d), f"{what}: every row, dense ones included"


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("impl,dt_name", [(0, "bf16"), (1, "bf16"), (1, "f32")])
def test_both_implementations_against_the_restatement_within_twice_the_unwindowed_error(s2v, impl, dt_name):
    case = X.case("randn", dt_name)
    for name, tab in TABLES.items():
        twice_the_unwindowed_error(s2v, case, impl, tab, f"impl {impl} {dt_name} N {X.N0} randn {name}")


@pytest.mark.parametrize("impl", [0, 1])
def test_the_long_loop_in_the_persistent_form(s2v, impl):
    assert LONG_TAB.N == LONG[2] and LONG_TAB.P == 473 and LONG_TAB.S == 420 and LONG[2] % 64 == 1
    case = X.case("randn", "bf16", LONG)
    twice_the_unwindowed_error(s2v, case, impl, LONG_TAB, f"impl {impl} bf16 N {LONG[2]} randn frames 1 rows 2", DEV)


# ------------------------------------------------------------------------------------------------ 2. bit for bit
def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("family", ["randn", "sharp"])
def test_full_offsets_return_the_window_launch_bit_for_bit(s2v, family):
    """every attn_local_ref.frames_table with full offsets: the two visit lists coincide there (tests/test_attn_box_cpu.py asserts it)"""
    case = X.case(family)
    for w in range(5):
        loc = R.frames_table(R.T_, R.R_, R.F_, R.S_, w)
        for impl in (0, 1):
            assert _bits(run(s2v, case, impl, X.from_local(loc, X.S_)), run(s2v, case, impl, loc)), f"frames = {w}, impl {impl}"
    long_case = X.case("randn", "bf16", LONG)
    loc = R.frames_table(226, 247, 10, 420, 1)
    assert _bits(run(s2v, long_case, 0, X.from_local(loc, 420)), run(s2v, long_case, 0, loc)), "the persistent form"


@pytest.mark.parametrize("family", ["randn", "onehot", "sharp"])
def test_an_all_dense_box_table_returns_the_dense_launch_bit_for_bit(s2v, family):
    """N = 770 <= ATTN_PP_MAX_TOKENS: s2v_op_attention impl 0 runs attn_pp as well"""
    case = X.case(family)
    plain = run(s2v, case, 0)
    for P in (1, 20, 64, 100, X.N0):
        for S in (64, 150, X.N0):
            assert _bits(run(s2v, case, 0, X.from_local(R.dense_table(X.N0, P), S)), plain), f"every row dense, P = {P}, S = {S}"
    assert _bits(run(s2v, case, 1, X.from_local(R.dense_table(X.N0, 20), 150)), run(s2v, case, 1)), "the generic form"


@pytest.mark.parametrize("family", ["randn", "onehot", "sharp"])
def test_a_dense_wave_inside_a_box_table_returns_the_dense_bits(s2v, family):
    case = X.case(family)
    B, H, N = case.B, case.H, case.N
    plain = run(s2v, case, 0).reshape(B, N, -1)
    got = run(s2v, case, 0, TABLES["dense_wave_then_f1r1"]).reshape(B, N, -1)
    assert _bits(got[:, :32], plain[:, :32]), "rows 0 .. 31: a wholly dense wave"
    assert not _bits(got[:, 32:], plain[:, 32:])
    got = run(s2v, case, 0, TABLES["f1r1"]).reshape(B, N, -1)
    assert not _bits(got[:, 20:32], plain[:, 20:32]), "the same rows boxed"


def test_two_runs_give_the_same_bits(s2v):
    for shape, tab in ((X.SHAPE, TABLES["f1r1"]), (LONG, LONG_TAB)):
        case = X.case("randn", "bf16", shape)
        for impl in (0, 1):
            assert _bits(launch(s2v, case, impl, tab), run(s2v, case, impl, tab)), f"N {shape[2]} impl {impl}"


# ------------------------------------------------------------------------------------------------ 3. one-hot and sharp rows
@pytest.mark.parametrize("family", ["onehot", "sharp"])
@pytest.mark.parametrize("impl", [0, 1])
def test_rows_with_a_box_around_their_own_key_return_its_value_row_and_nothing_leaks(s2v, impl, family):
    """every box holds the row's own key pi(i) (a row whose key lies in the prefix has an empty box): a non-trap row returns V[pi(i)] to one ulp;
    the trap rows -- queries for a code of the 64 rows that follow their sample in memory, V = 1e4 there -- follow the box restatement: a leak of
    a pad key or of the next sample takes a whole row (oracle.attn_cases.failures' rules)"""
    case = X.case(family)
    qm = qmode(impl)
    B, H, N = case.B, case.H, case.N
    tab = X.around_own_key(case)
    vis = X.visible(tab)
    assert bool(vis[torch.arange(N), case.pi].all()) and not bool(vis.all(dim=1)[X.P0:].any())
    got = run(s2v, case, impl, tab).double().cpu()
    assert torch.isfinite(got).all()
    g4, r4 = got.reshape(B, N, H, 64), X.box_reference(case, qm, tab).reshape(B, N, H, 64)
    scale = torch.clamp(r4.abs().amax(dim=(1, 3), keepdim=True), min=1.0)
    err = ((g4 - r4).abs() / scale)[:, case.trap].max().item()
    assert err <= AC.SOFT_BARS["bf16"], f"impl {impl}: trap rows {err:.3e} of the sample-and-head scale"
    v = case.heads(2).transpose(1, 2)   # [B, N, H, 64]
    want = v[:, case.pi[~case.trap]]
    if family == "onehot":
        leak = case.leak(AC.SHRINK[qm])
        assert leak <= AC.LEAK_MAX
        tail = leak * v.abs().max()
    else:
        # sharp: the analytic bound on the weight outside the own key (case.leak, a worst case over N keys) is 5e-3, but a box shows a row
        # some 40 keys, not N.  The tail is taken from the fp64 restatement instead: its largest distance from V[pi(i)] over these rows, which
        # must itself lie far under one ulp of a typical element (measured 2.7e-6 on the CPU) for "V[pi(i)] to one ulp" to be the right answer
        tail = (r4[:, ~case.trap] - want).abs().max()
        assert tail.item() <= 2.0 ** -16, f"the fp64 restatement is {tail.item():.3e} from V[pi(i)]: the boxed sharp rows are not one-hot here"
    dist = (g4[:, ~case.trap] - want).abs()
    over = dist - (AC.ulp_at(want, "bf16") + tail)
    print(f"MEASURED impl {impl} {family}: tail {float(tail):.3e}; largest |out - V[pi(i)]| {dist.max().item():.3e}, as a multiple of its bar "
          f"{(dist / (AC.ulp_at(want, 'bf16') + tail)).max().item():.3f}; {int((over > 0).sum())} of {over.numel()} elements beyond the bar")
    assert over.max().item() <= 0, f"impl {impl} {family}: {int((over > 0).sum())} elements beyond one ulp of V[pi(i)]"


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_bad_tables_are_refused_by_name_and_launch_nothing(s2v):
    L = s2v._lib
    case = X.case("randn")
    qd = case.qkv.to(DEV)
    out = torch.zeros(2 * X.N0, 128, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(2 * 2 * 64 * 832, dtype=torch.bfloat16, device=DEV)
    for tab, match in X.bad_tables():
        with pytest.raises(s2v.S2VError, match="s2v_op_attention_box: " + match):
            L.check(L.lib().s2v_op_attention_box(L.ptr(qd), L.ptr(vt), L.ptr(out), 2, 2, X.N0, L.DTYPE_BF16, 0, *tab.c(), L.stream_ptr()))
    with pytest.raises(s2v.S2VError, match=r"impl 0 is bf16"):
        L.check(L.lib().s2v_op_attention_box(L.ptr(qd), L.ptr(vt), L.ptr(out), 2, 2, X.N0, L.DTYPE_F32, 0, *TABLES["f1r1"].c(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert (out == 0).all(), "a refused call launches nothing"
