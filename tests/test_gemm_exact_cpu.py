"""The exact GEMM cases of oracle/gemm_cases.py without a device: their preconditions, their plans, and what they see that the randn bars do not.

1. Preconditions of every case of tests/test_gpu_gemm_exact.py: family S stays within 256 (bf16) / 2048 (fp16), every k is non-zero in every
   32-row block of A, the fp32 reference equals fp64 (all rows, or 512 sampled rows where the fp64 product would take seconds), every epilogue
   stage is exactly representable; the maps of family G hit every k; the e4m3 operands survive the row quantisation and the emulated result
   rounds to the exact value.
2. The plan of every case at 256 CUs (the MI355X) names the kernel the case is about -- the same assertion the GPU test makes at the device's
   own CU count, so a change of gemm_plan that moves a case off its kernel shows here first.
3. Mutation study.  `tiled_gemm` is a torch emulation of a tiled GEMM as the kernels are built -- operands padded to 256 rows, 256 x 256 tiles of
   64 x 64 wave tiles, K in steps of 16 accumulated in fp32, epilogue4's rounding points, the rows from m_begin on as a tail launch -- with one
   switch per way such a kernel goes wrong.  At 500 x 384 x 1024 (bf16; tail from row 256; two samples of 247 rows, text 19, reference 23):

     mutant          what goes wrong                                          exact S  exact G  randn op bars  ring anchor bar  on epilogue 2
                                                                                                (4e-3, 2e-2)   (rel-L2 1e-2)    (op / anchor)
     drop_kstep      one 16-wide K step missing in one wave tile              FAIL     FAIL     FAIL           FAIL
     drop_element    k = K - 1 missing in one row                             FAIL     FAIL     pass           pass
     w_row_shift     W row n + 1 read for one 4-column group                  FAIL     FAIL     FAIL           FAIL
     bias_shift      bias read 4 columns on for one wave tile                 FAIL     FAIL     FAIL           FAIL
     a_pad_row       row M - 1 computed from the pad row behind A             FAIL     FAIL     FAIL           FAIL
     wrong_gate      first reference row of sample 1 takes the text gate      FAIL     FAIL     pass           pass             FAIL / FAIL
     tail_overlap    the tail launch starts at m_begin - 1 (gate + residual)  FAIL     FAIL     pass           pass             FAIL / FAIL

   The randn columns are the checks as they stand: test_op_linear_mfma_bf16 (rel-L2 4e-3 and max-abs 2e-2 of max|ref|) and the ring-kernel
   anchor of test_gpu_gemm_schedules.py (rel-L2 1e-2), each on its own input distribution and with the epilogue it runs -- bias only.  There
   wrong_gate and tail_overlap change NOTHING (no gate is read; a row written twice holds the same value), so they pass; that no operator
   test ran the gate + residual epilogue or a tail launch is the gap.  The last column applies the same bars to an epilogue-2 output with randn
   gates and residual, which nothing did before: a whole wrong row of 500 is a gross error there (one K step of one wave tile is one at this
   small shape too; at the anchor's 1024 x 768 x 3072 it sits at 5e-3).  A single dropped product passes every randn bar.
   The file asserts that every mutant fails the exact families and that drop_element, wrong_gate and tail_overlap pass both randn checks as
   they stand: the reason the exact tests exist."""
import ctypes

import pytest
import torch

from oracle import gemm_cases as gc
from test_gpu_fp8 import quant_rows

NAMES = [c.name for c in gc.CASES]


# ---- 1. preconditions -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_preconditions(name):
    c = gc.BY_NAME[name]
    dt = gc.STORE[c.dt]
    A, W, b, x, gates3 = gc.s_inputs(c)
    assert (A != 0).sum(1).eq(min(c.K, c.budget)).all() and W.abs().eq(1).all()
    assert gc.s_covers(A), "a k is zero in a whole 32-row block of A"
    y = gc.s_reference(A, W, b)
    rows = torch.arange(c.M) if c.M * c.N * c.K <= 2e9 else torch.randperm(c.M, generator=torch.Generator().manual_seed(1))[:512]
    assert torch.equal(y[rows].double(), A[rows].double() @ W.double().T + b.double()), "the fp32 reference is not exact"
    if c.entry == "fp8":
        gc.fp8_claim_s(A, W, b, quant_rows)
    for epi in c.epis:
        gates = gc.gate_rows(c.M, c.tok, c.text_len, c.ref_len, *gates3) if epi == 2 else None
        gc.s_expected(A, W, b, epi, c.dt, x, gates, x)  # the bound and the exactness of every stage
        if epi == 1:
            tiny = gc.gelu64(y.to(dt)).abs() < 2.0 ** -100
            assert ((y > 0) & (y <= 8) & ~tiny).any() and ((y < 0) & (y >= -8) & ~tiny).any()
    if 2 in c.epis:
        assert c.tok % 8 != 0 and c.text_len + c.ref_len < 64 and -(-c.M // c.tok) >= 2
        t, r, v = gates3
        assert not (t == v).any() and (r is None or not ((t == r) | (r == v)).any())
        assert r is not None or c.noref
    for mirror in (False, True):
        pay, bias, amp, _, _, uniq = gc.g_inputs(c, mirror)  # asserts that the maps hit every k
        hot = c.N if mirror else c.M
        assert any(torch.equal(p, torch.arange(hot) % c.K) for _, p in uniq) and any(torch.equal(p, (c.K - hot + torch.arange(hot)) % c.K) for _, p in uniq)
        assert torch.isfinite(pay.float()).all() and (pay.float().abs() >= 2.0 ** -10).all()
        if c.entry == "fp8":
            for _, p in uniq:
                gc.fp8_claim_g(c, mirror, pay, amp, p, bias, gc.g_expected_y(c, mirror, pay, amp, p, bias), quant_rows)


def test_gelu_reference_and_ulp_distance():
    """gelu64 is the tanh form (where that form is well conditioned) and stays accurate where 1 + tanh cancels; ulp_distance counts steps"""
    y = torch.linspace(-4, 8, 1001, dtype=torch.float64)
    u = (2.0 / torch.pi) ** 0.5 * (y + 0.044715 * y ** 3)
    assert torch.allclose(gc.gelu64(y), 0.5 * y * (1 + torch.tanh(u)), rtol=1e-9, atol=1e-300)
    assert torch.allclose(gc.gelu64(y.float()).float(), torch.nn.functional.gelu(y.float(), approximate="tanh"), rtol=1e-4, atol=1e-7)
    assert gc.gelu64(torch.tensor([-9.0])).item() < 0 and abs(gc.gelu64(torch.tensor([-9.0])).item()) > 2.0 ** -100
    for dt in (torch.bfloat16, torch.float16):
        a = torch.tensor([1.0, -1.0, 0.0, 3.0], dtype=dt)
        up = (a.view(torch.int16) + 1).view(dt)
        assert gc.ulp_distance(a, up).tolist() == [1, 1, 1, 1]
        assert gc.ulp_distance(torch.tensor([0.0], dtype=dt), torch.tensor([-0.0], dtype=dt)).item() == 0


# ---- 2. plans -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def diag(s2v):
    D = s2v._lib.diag_lib()
    D.s2v_diag_gemm_plan.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]
    yield D
    D.s2v_set_gemm_impl(9)


@pytest.mark.parametrize("name", NAMES)
def test_case_plan_names_its_kernel_at_256_cus(diag, name):
    c = gc.BY_NAME[name]
    out = (ctypes.c_int32 * 5)()
    try:
        diag.s2v_set_gemm_impl(c.impl if c.impl is not None else 9)
        for epi in c.epis:
            assert diag.s2v_diag_gemm_plan(c.M, c.N, c.K, epi, c.plan_flags(), gc.NCU, c.sk, out) == 0
            assert (out[0], gc.KERNELS[out[3]], gc.KERNELS[out[4]]) == c.plan, (name, epi)
    finally:
        diag.s2v_set_gemm_impl(9)


def test_every_kernel_and_epilogue_is_reached():
    reached = {(k, e) for c in gc.CASES for k in c.plan[1:] if k != "none" for e in c.epis}
    for k in ("gemm_bf16_128", "gemm_bf16_stag", "gemm_bf16_pp64", "gemm_g4", "gemm_bf16_w8"):
        assert {(k, e) for e in (0, 1, 2, 3)} <= reached, k
    assert {("gemm_g4t", 0), ("gemm_g4t", 1), ("gemm_q4", 0), ("gemm_q4", 1), ("gemm_g4f", 0), ("gemm_g4f", 1), ("gemm_pp64_fp8", 0), ("gemm_pp64_fp8", 1)} <= reached
    assert {c.plan[0] for c in gc.CASES} >= {0, 2, 4}
    f16 = {c.plan[1] for c in gc.CASES if c.dt == "f16"} | {c.plan[2] for c in gc.CASES if c.dt == "f16"}
    assert {"gemm_bf16_128", "gemm_bf16_stag", "gemm_bf16_pp64", "gemm_g4"} <= f16


@pytest.mark.parametrize("name", [c.name for c in gc.QK_CASES])
def test_qknorm_case_plan_and_reference(diag, name):
    """the q/k-norm cases: the plan at 256 CUs names the kernel; the maps hit every k; on the first 64 rows a plain fp32 evaluation of the epilogue
    (torch LayerNorm, the rotation as the kernel writes it) stays within the bar of the fp64 reference, and the v third is the projection"""
    c = gc.QK_BY_NAME[name]
    dt = gc.STORE[c.dt]
    diag.s2v_set_gemm_g4t.argtypes = [ctypes.c_int]
    out = (ctypes.c_int32 * 5)()
    flags = (gc.PLAN_F16 if c.dt == "f16" else 0) | (gc.PLAN_ROPE if c.entry == "diag" else 0)
    try:
        diag.s2v_set_gemm_g4t(c.g4t)
        assert diag.s2v_diag_gemm_plan(c.M, c.N, c.plan_K, 4, flags, gc.NCU, 0, out) == 0
    finally:
        diag.s2v_set_gemm_g4t(1)
    assert (gc.KERNELS[out[3]], gc.KERNELS[out[4]]) == c.plan
    assert c.tok % 8 != 0 and 0 <= c.text_len < 64
    W, bias, amp, ln, cs, use = gc.qk_inputs(c)
    assert torch.cat([p for _, p in use]).unique().numel() == c.K
    rows = torch.arange(c.M - 64, c.M)  # the last rows: rotated ones where there is a table, and a sample boundary in the big cases
    y16 = gc.g_reference(W, amp[rows], use[0][1][rows], bias, dt)
    r = rows % c.tok
    sub_cs = None if cs is None else torch.cat([cs[(r - c.text_len).clamp_min(0), :]], 0)
    # qknorm_reference indexes the table by row % tok - text_len: hand it the 64 rows with tok = 64, text_len = 0 and their own table rows
    exp, bar = gc.qknorm_reference(y16, c.D, ln, sub_cs, 64, 0, 1e-6, dt)
    assert torch.equal(exp[:, 2 * c.D:], y16[:, 2 * c.D:])
    H2 = 2 * c.D // 64
    w = torch.cat([ln[0].float().expand(c.D // 64, 64), ln[2].float().expand(c.D // 64, 64)])
    b = torch.cat([ln[1].float().expand(c.D // 64, 64), ln[3].float().expand(c.D // 64, 64)])
    n = (torch.nn.functional.layer_norm(y16[:, :2 * c.D].float().view(64, H2, 64), (64,), eps=1e-6) * w + b).to(dt)
    if sub_cs is not None:
        cc, ss = sub_cs[:, None, :32], sub_cs[:, None, 32:]
        x0, x1 = n.float()[..., 0::2], n.float()[..., 1::2]
        n = torch.stack([x0 * cc - x1 * ss, x1 * cc + x0 * ss], -1).view(64, H2, 64).to(dt)
    ratio = (n.view(64, -1).double() - exp[:, :2 * c.D].double()).abs() / bar
    assert ratio.max().item() <= 1.0, ratio.max().item()


# ---- 3. mutation study ----------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("drop_kstep", "drop_element", "w_row_shift", "bias_shift", "a_pad_row", "wrong_gate", "tail_overlap")
SM, SN, SK, S_TOK, S_TEXT, S_REF, S_MBEGIN = 500, 384, 1024, 247, 19, 23, 256
DT = torch.bfloat16


def tiled_gemm(A, W, b, epi, x=None, gates3=None, mutant=None):
    """A [SM][SK], W [SN][SK], b [SN] in DT -> [SM][SN] in DT; see the module docstring"""
    Ap, Wp = gc.padded_operand(A, SK, DT).float(), gc.padded_operand(W, SK, DT).float()
    acc = torch.zeros(Ap.shape[0], Wp.shape[0])
    wm, wn = slice(64, 128), slice(128, 192)  # the wave tile the tile-local mutants sit in
    for k0 in range(0, SK, 16):
        a, w = Ap[:, k0:k0 + 16], Wp[:, k0:k0 + 16]
        if mutant == "w_row_shift":
            w = w.clone()
            w[200:204] = Wp[201:205, k0:k0 + 16]
        if mutant == "a_pad_row":
            a = a.clone()
            a[SM - 1] = Ap[SM, k0:k0 + 16]
        if mutant == "drop_element" and k0 + 16 == SK:
            a = a.clone()
            a[SM - 1, 15] = 0
        step = a @ w.T
        if mutant == "drop_kstep" and k0 == 32 * 16:
            step[wm, wn] = 0
        acc += step
    bias = b.float().expand(SM, SN).clone()
    if mutant == "bias_shift":
        bias[wm, wn] = b.float()[132:196]
    y = (acc[:SM, :SN] + bias).to(DT)
    if epi == 0:
        return y
    t, r, v = gates3
    m = torch.arange(SM)
    smp, row = m // S_TOK, m % S_TOK
    text_end = S_TEXT + (1 if mutant == "wrong_gate" else 0)
    text_rows = torch.where(smp == 1, row < text_end, row < S_TEXT)  # the mutant: `<=` for sample 1
    gates = torch.where(text_rows[:, None], t[smp], torch.where((row < S_TEXT + S_REF)[:, None], r[smp], v[smp]))
    upd = (gates.float() * y.float()).to(DT)
    out = (x.float() + upd.float()).to(DT)
    if mutant == "tail_overlap":  # row m_begin - 1 is updated by the main launch and again by the tail
        out[S_MBEGIN - 1] = (out[S_MBEGIN - 1].float() + upd[S_MBEGIN - 1].float()).to(DT)
    return out


def epi_of(mutant):
    return 2 if mutant in ("wrong_gate", "tail_overlap") else 0


def exact_checks(mutant, epi):
    """(family S passes, family G passes): bitwise against the expected output, as tests/test_gpu_gemm_exact.py compares"""
    c = gc.Case("study", "planned", SM, SN, SK, (0, 2), (0, "none", "none"), tok=S_TOK)
    A, W, b, x, gates3 = gc.s_inputs(c)
    gates = gc.gate_rows(SM, S_TOK, S_TEXT, S_REF, *gates3)
    exp, _ = gc.s_expected(A, W, b, epi, "bf16", x, gates, None)
    s_ok = torch.equal(tiled_gemm(A.to(DT), W.to(DT), b.to(DT), epi, x, gates3, mutant).view(torch.int16), exp.view(torch.int16))
    g_ok = True
    for mirror in (False, True):
        pay, bias, amp, xg, g3, uniq = gc.g_inputs(c, mirror)
        for _, p in uniq:
            y16 = gc.g_expected_y(c, mirror, pay, amp, p, bias)
            exp = gc.epilogue(y16, epi, DT, xg, gc.gate_rows(SM, S_TOK, S_TEXT, S_REF, *g3), None)
            hot = gc.one_hot(amp, p, SK, DT)
            got = tiled_gemm(pay, hot, bias, epi, xg, g3, mutant) if mirror else tiled_gemm(hot, pay, bias, epi, xg, g3, mutant)
            g_ok = g_ok and torch.equal(got.view(torch.int16), exp.view(torch.int16))
    return s_ok, g_ok


def randn_bars(mutant, epi):
    """(the bars of test_op_linear_mfma_bf16 hold, the bar of the ring-kernel anchor holds), each on its test's input distribution"""
    res = []
    for w_scale, b_scale in ((0.5, 1.0), (0.05, 0.1)):
        g = torch.Generator().manual_seed(SM + SN + SK)
        A = (torch.randn(SM, SK, generator=g) * 0.5).to(DT)
        W = (torch.randn(SN, SK, generator=g) * w_scale).to(DT)
        b = (torch.randn(SN, generator=g) * b_scale).to(DT)
        x = torch.randn(SM, SN, generator=g).to(DT)
        gates3 = tuple(torch.randn(3, SN, generator=g).to(DT) for _ in range(3))
        ref = A.float() @ W.float().T + b.float()
        if epi == 2:
            ref = x.float() + gc.gate_rows(SM, S_TOK, S_TEXT, S_REF, *gates3).float() * ref
        got = tiled_gemm(A, W, b, epi, x, gates3, mutant).float()
        rel = ((got - ref).norm() / ref.norm()).item()
        err = (got - ref).abs().max().item()
        res.append((rel < 4e-3 and err <= 2e-2 * ref.abs().max().item() + 1e-2) if w_scale == 0.5 else rel <= 1e-2)
    return tuple(res)


def test_unmutated_emulation_passes_every_check():
    for epi in (0, 2):
        assert exact_checks(None, epi) == (True, True)
        assert randn_bars(None, epi) == (True, True)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_exact_families_catch_what_the_randn_bars_let_pass(mutant):
    epi = epi_of(mutant)
    s_ok, g_ok = exact_checks(mutant, epi)
    op_ok, anchor_ok = randn_bars(mutant, 0)  # the randn tests as they stand run the bias epilogue
    word = lambda ok: "pass" if ok else "FAIL"
    line = f"MUTANT {mutant:13s} exact S {word(s_ok)}  exact G {word(g_ok)}  randn op bars {word(op_ok)}  ring anchor bar {word(anchor_ok)}"
    if epi == 2:
        line += "  on epilogue 2: " + " / ".join(word(ok) for ok in randn_bars(mutant, 2))
    print("\n" + line)
    assert not s_ok and not g_ok, f"{mutant} passes an exact family"
    if mutant in ("drop_element", "wrong_gate", "tail_overlap"):
        assert op_ok and anchor_ok, f"{mutant} is caught by a randn bar after all"
