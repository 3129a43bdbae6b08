"""Every GEMM kernel and epilogue against expected bits that do not depend on the order of summation (pytest -m gpu), through the C ABI, on the
input families of oracle/gemm_cases.py.

The bitwise-to-ring tests of test_gpu_gemm_schedules.py hold a kernel to the accumulation order of gemm_bf16_w8, and the randn bars of
test_gpu_parity.py cannot see a single wrong element, a shifted bias column, a leaking pad row or the gate of the wrong segment
(tests/test_gemm_exact_cpu.py shows it on a CPU emulation).  Here

  * family S (A in {-1, 0, 1}, W = +-1, integer bias): every product of every k counts, every partial sum is an integer, the fp32 CPU matmul is
    the exact reference and -- max|y| <= 256 (bf16) / 2048 (fp16) asserted before the launch -- every expected output is representable;
  * family G (one-hot rows times +-1, +-2, +-1/2 against arbitrary 16-bit values, and its mirror with the one-hot rows in W): the output is one
    exact product, one fp32 add and one rounding; the maps of gemm_cases.maps address every k of the shape, the first and the last K tile included;
  * epilogues 0 (bias), 2 (gate + residual: three power-of-two gates per sample and column, segment ends inside a wave's rows, one case without a
    reference gate) and 3 (residual add) are compared BITWISE with gemm_epi.h's scalar epilogue4 restated in torch; epilogue 1 (GELU) is held to
    one ulp of the fp64 function value of the exactly known pre-activation, rounded once (|fp64| < 2^-100: |got| <= 2^-100);
  * the pad rows of A and W hold 1e4, the output sits between 256 guard rows and 8 guard columns of a sentinel pattern that must survive, the
    body starts as NaN.

Every case names its kernel (gemm_cases.CASES) and asserts, through s2v_diag_gemm_plan at this device's CU count, that the plan of the launch
names it (main launch, row tail, split); a mismatch fails.  Entries: s2v_op_linear_planned (gemm_plan as a context's linear() runs it),
s2v_op_linear impl 0 / 4 (one launch as given, for the small shapes at which the plan would pick smaller tiles), s2v_op_linear_fp8; product and
diagnostics build wherever both reach the kernel.  The e4m3 cases assert on the torch emulation of test_gpu_fp8.py, before the launch, that the
operands survive the row quantisation and that the dequantised result rounds to the exact integer.

Epilogue 4 (fused q/k-norm + rotary embedding; gemm_cases.QK_CASES) runs on family G only -- the projection is then exact and the epilogue is
what is compared -- through s2v_diag_qkv_qknorm (gemm_g4t's trickled epilogue, gemm_g4's, the eight-wave kernel's and the 128 x 128 kernel's C++
epilogue; a rotary table with an angle per (position, pair); samples of 2753 / 181 rows with 19 text rows) and through s2v_op_linear_lora's
epilogue 4 with B = 0 (fp16; the plan's row tail on gemm_bf16_128).  The v third must equal the projection bitwise.  Reference: fp64 with the
kernel's two rounding points, after the affine LayerNorm and after the rotation.  Bar per element (gemm_cases.qknorm_reference states the
derivation): one ulp of the output value plus (|cos| + |sin|) times one ulp of the larger normalised value of the pair -- one rounding flip per
stage, propagated through the rotation; a row without rotation counts as the rotation by 0.  Rows that are not rotated have a single stage and
are held to ONE ulp of the output wherever w n + b does not cancel beyond 2^-10 of its larger term (99.99 % of them).

Each test prints a line `MEASURED gemm_exact ...` with the kernel, the number of compared elements and the worst GELU distance in ulps, or
`MEASURED gemm_exact_qknorm ...` with the worst ratio to the bar (profiles/r12_gemm_exact.txt).

FINDING.  Epilogues 0 - 3: none -- on the MI355X all 110 cases returned the expected bits on every kernel, dtype and build, with the guards intact,
and every GELU output was within one ulp of the correctly rounded fp64 value (worst distance 1).
Epilogue 4: no kernel fault, one limit of the arithmetic.  Held to one ulp of the output on EVERY non-rotated element, three of the eight ids
missed on a handful of elements where w n + b cancels to 2^-18 .. 2^-20 of |b|:
  qk-g4-11008x1024x2304 (diag)             2 elements, worst 2 ulps:  got -2.32831e-07, fp64 -2.34920e-07 (b = 0.0184, error 1.1 fp32 ulps of b)
  qk-lora-tail-4460x1280x256 (both builds) 10 elements, worst 10 ulps: got  6.70552e-08, fp64  7.16269e-08 (b = 0.0723, error 0.6 fp32 ulps of b)
`(x - mean) * rstd * w + b` (gemm_epi.h:257) is evaluated in fp32 without contraction; its absolute error is about one fp32 ulp of the larger
term, which exceeds a 16-bit ulp of the result once the result is below ~2^-16 of that term.  A plain fp32 torch evaluation of the same rows on
the CPU returns the kernel's value to the last bit, so the kernel is a faithful fp32 LayerNorm (the arithmetic of qk_norm_rope_k and of the
reference); the code is unchanged.  The one-ulp form is therefore asserted where its premise holds, and the two-term form of the bar elsewhere."""
import ctypes
import functools

import pytest
import torch

from oracle import gemm_cases as gc
from test_gpu_fp8 import quant_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = [(c.name, lib) for c in gc.CASES for lib in c.libs]


def libs_of(s2v):
    L = s2v._lib
    D = L.diag_lib()
    D.s2v_diag_gemm_plan.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]
    D.s2v_set_gemm_g4t.argtypes = [ctypes.c_int]
    return L, D


def assert_plan(D, c, epi):
    """the plan of this launch at the device's CU count names the kernels the case is about"""
    out = (ctypes.c_int32 * 5)()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert D.s2v_diag_gemm_plan(c.M, c.N, c.K, epi, c.plan_flags(), ncu, c.sk, out) == 0, D.s2v_last_error()
    got = (out[0], gc.KERNELS[out[3]], gc.KERNELS[out[4]])
    assert got == c.plan, f"{c.name} epilogue {epi} on {ncu} CUs: the plan is (split, main, tail) = {got}, the case is about {c.plan}"
    if c.plan[2] != "none":
        assert 0 < out[2] < c.M and out[2] % 256 == 0


class Operands:
    """one launch's inputs (CPU tensors in the case's dtype); x / gates / R as the epilogue needs them"""

    def __init__(self, A, W, b, x=None, gates3=None, R=None):
        self.A, self.W, self.b, self.x, self.gates3, self.R = A, W, b, x, gates3, R


def launch(L, lib, c, epi, op, a_dev=None, w_dev=None):
    """run one case on `lib`; returns the OutBuf.  a_dev / w_dev: a padded operand already on the device (family G builds them there)"""
    dt = gc.STORE[c.dt]
    M, N, K = c.M, c.N, c.K
    dtype = L.DTYPE_OF[dt]
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    keep = []

    def dev(t):
        t = t.to(DEV).contiguous()
        keep.append(t)
        return t

    body = op.x if epi == 2 else None
    if c.entry == "planned":
        lda, ldw, ldc, ldr = K + 8, K + 16, N + 8, N + 16
        Ad = a_dev if a_dev is not None else dev(gc.padded_operand(op.A, lda, dt))
        Wd = w_dev if w_dev is not None else dev(gc.padded_operand(op.W, ldw, dt))
        out = gc.OutBuf(M, N, ldc, dt, body, DEV)
        g = [None, None, None]
        if epi == 2:
            g = [None if t is None else dev(t) for t in op.gates3]
        Rd = None
        if epi == 3:
            Rd = torch.full((M, ldr), gc.PAD_VALUE, dtype=dt)
            Rd[:, :N] = op.R
            Rd = dev(Rd)
        rc = lib.s2v_op_linear_planned(P(Ad), lda, P(Wd), ldw, P(dev(op.b)), ctypes.c_void_p(out.buf.data_ptr() + out.body_ptr_offset()), ldc, M, N, K,
                                       epi, dtype, P(g[0]), P(g[1]), P(g[2]), N, c.tok, c.text_len, c.ref_len, P(Rd), ldr, c.tile, c.sk, L.stream_ptr())
    else:
        Ad = a_dev if a_dev is not None else dev(op.A.to(dt))
        Wd = w_dev if w_dev is not None else dev(op.W.to(dt))
        out = gc.OutBuf(M, N, N, dt, None, DEV)
        cp = ctypes.c_void_p(out.buf.data_ptr() + out.body_ptr_offset())
        if c.entry == "direct":
            rc = lib.s2v_op_linear(P(Ad), P(Wd), P(dev(op.b)), cp, M, N, K, epi, dtype, 4 if c.dt == "f16" else 0, L.stream_ptr())
        else:
            need = M * K + N * K + 4 * (M + N)
            scratch = dev(torch.zeros(need, dtype=torch.uint8))
            rc = lib.s2v_op_linear_fp8(P(Ad), P(Wd), P(dev(op.b)), cp, M, N, K, epi, P(scratch), need, L.stream_ptr())
    assert rc == 0, lib.s2v_last_error()
    torch.cuda.synchronize()
    return out


def describe(bad, p=None):
    """where the mismatches are: rows, columns, 64 x 64 wave tiles and, for a one-hot map p, the k of the offending rows"""
    idx = bad.nonzero()
    rows, cols = idx[:, 0].unique(), idx[:, 1].unique()
    tiles = torch.stack([idx[:, 0] // 64, idx[:, 1] // 64], 1).unique(dim=0)
    s = (f"{len(idx)} elements differ; rows {rows[:12].tolist()}{'...' if len(rows) > 12 else ''} columns {cols[:12].tolist()}"
         f"{'...' if len(cols) > 12 else ''} wave tiles (m / 64, n / 64) {tiles[:8].tolist()}")
    if p is not None:
        s += f"; k of those rows {p[rows[:12]].tolist()} (k % 64: {(p[rows[:12]] % 64).tolist()})"
    return s


class Tally:
    def __init__(self):
        self.compared, self.gelu_worst = 0, 0

    def check(self, c, epi, out, expected, y16, what, p=None):
        """compared on the device (plain torch on the bits the kernel left); a mismatch is described on the CPU"""
        dt = gc.STORE[c.dt]
        got = out.body()
        assert out.guards_intact(), f"{c.name} {what} epilogue {epi}: the guard rows / columns around the output changed"
        if epi == 1:
            yd = y16.to(DEV)
            worst, bad = gc.gelu_check(got, yd, dt)
            self.gelu_worst = max(self.gelu_worst, worst)
            assert bad is None, (f"{c.name} {what} GELU: more than one ulp from the fp64 value at {bad}: pre-activation {yd[tuple(bad)].item()}, "
                                 f"got {got[tuple(bad)].item()}, fp64 {gc.gelu64(yd)[tuple(bad)].item()}; worst distance {worst} ulps")
        else:
            bad = got.view(torch.int16) != expected.to(DEV).view(torch.int16)
            if bad.any().item():
                bad, got = bad.cpu(), got.cpu()
                raise AssertionError(f"{c.name} {what} epilogue {epi}: {describe(bad, p)}; first: got {got[bad][0].item()}, expected {expected[bad][0].item()}")
        self.compared += got.numel()


@functools.lru_cache(maxsize=2)
def s_inputs(name):
    """family S for a case, shared by the product and the diagnostics run"""
    return gc.s_inputs(gc.BY_NAME[name])


def s_family(L, lib, c, tally):
    dt = gc.STORE[c.dt]
    A, W, b, x, gates3 = s_inputs(c.name)
    if c.entry == "fp8":
        gc.fp8_claim_s(A, W, b, quant_rows)
    x16 = None if x is None else x.to(dt)
    op = Operands(None, None, b.to(dt), x16, gates3, x16)
    planned = c.entry == "planned"
    a_dev = (gc.padded_operand(A, c.K + 8, dt) if planned else A.to(dt)).to(DEV)
    w_dev = (gc.padded_operand(W, c.K + 16, dt) if planned else W.to(dt)).to(DEV)
    for epi in c.epis:
        gates = gc.gate_rows(c.M, c.tok, c.text_len, c.ref_len, *gates3) if epi == 2 else None
        expected, y = gc.s_expected(A, W, b, epi, c.dt, x, gates, x)  # asserts the preconditions
        out = launch(L, lib, c, epi, op, a_dev, w_dev)
        tally.check(c, epi, out, expected, y.to(dt), "family S")


def g_family(L, lib, c, tally, mirror):
    """family G (mirror: the one-hot rows in W, the payload in A).  Every map under the case's first epilogue, the first stride map and the
    identity on the last columns under the others (the K loop is the same code for every epilogue)"""
    dt = gc.STORE[c.dt]
    M, N, K = c.M, c.N, c.K
    hot = N if mirror else M
    pay, bias, amp, x, gates3, all_maps = gc.g_inputs(c, mirror)
    planned = c.entry == "planned"
    ld_pay, ld_hot = ((K + 8, K + 16) if mirror else (K + 16, K + 8)) if planned else (K, K)
    pay_dev = (gc.padded_operand(pay, ld_pay, dt) if planned else pay).to(DEV)
    op = Operands(None, None, bias, x, gates3, x)
    for epi in c.epis if not mirror else c.epis[:1]:
        for nm, p in all_maps if epi == c.epis[0] else [all_maps[0], all_maps[-1]]:
            hot_dev = torch.zeros(gc.rup(hot, 256) if planned else hot, ld_hot, dtype=dt, device=DEV)
            hot_dev[hot:] = gc.PAD_VALUE
            hot_dev[torch.arange(hot, device=DEV), p.to(DEV)] = amp.to(dt).to(DEV)
            y16 = gc.g_expected_y(c, mirror, pay, amp, p, bias)
            if c.entry == "fp8":
                gc.fp8_claim_g(c, mirror, pay, amp, p, bias, y16, quant_rows)
            gates = gc.gate_rows(M, c.tok, c.text_len, c.ref_len, *gates3) if epi == 2 else None
            expected = gc.epilogue(y16, epi, dt, x, gates, x)
            out = launch(L, lib, c, epi, op, *((pay_dev, hot_dev) if mirror else (hot_dev, pay_dev)))
            tally.check(c, epi, out, expected, y16, f"family G{' mirror' if mirror else ''} map {nm}", None if mirror else p)


@pytest.mark.parametrize("name,libname", PARAMS)
def test_gemm_kernel_returns_the_exact_bits(s2v, name, libname):
    c = gc.BY_NAME[name]
    L, D = libs_of(s2v)
    lib = L.lib() if libname == "product" else D
    tally = Tally()
    try:
        if c.impl is not None:
            assert libname == "diag"
            D.s2v_set_gemm_impl(c.impl)
        for epi in c.epis:
            assert_plan(D, c, epi)
        s_family(L, lib, c, tally)
        g_family(L, lib, c, tally, mirror=False)
        g_family(L, lib, c, tally, mirror=True)
    finally:
        D.s2v_set_gemm_impl(9)
    kernels = c.plan[1] + ("" if c.plan[2] == "none" else "+" + c.plan[2]) + (f"+gemm_g4_sk_sum(S={c.plan[0]})" if c.plan[0] else "")
    print(f"\nMEASURED gemm_exact {name} {libname} kernel={kernels} epilogues={','.join(map(str, c.epis))} compared={tally.compared} "
          f"gelu_worst_ulp={tally.gelu_worst if 1 in c.epis else '-'}")


# ---- epilogue 4: q/k-norm + rotary embedding ------------------------------------------------------------------------------------------------------
QK_PARAMS = [(c.name, lib) for c in gc.QK_CASES for lib in c.libs]
QK_EPS = 1e-6


@pytest.mark.parametrize("name,libname", QK_PARAMS)
def test_qknorm_epilogue_on_the_exact_projection(s2v, name, libname):
    """Family G makes the projection exact, so what is compared is the epilogue alone: fp64 with the kernel's two rounding points
    (gemm_cases.qknorm_reference, which also derives the bar: one ulp of the output plus (|cos| + |sin|) ulps of the larger normalised value of
    the pair); the v third must equal the projection bitwise.  Through s2v_diag_qkv_qknorm (rotary table with an angle per (position, pair),
    samples and text rows that end inside tiles) and through s2v_op_linear_lora's epilogue 4 with B = 0 (the plan's row tail)."""
    c = gc.QK_BY_NAME[name]
    dt = gc.STORE[c.dt]
    L, D = libs_of(s2v)
    lib = L.lib() if libname == "product" else D
    M, N, K = c.M, c.N, c.K
    W, bias, amp, ln, cs, use = gc.qk_inputs(c)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    diag_entry = c.entry == "diag"
    Wd, biasd, ampd = W.to(DEV), bias.to(DEV), amp.to(DEV)
    lnd = [t.to(DEV) for t in ln]
    csd = None if cs is None else cs.to(DEV)
    w_arg = gc.padded_operand(W, K, dt).to(DEV) if diag_entry else Wd
    worst, compared = 0.0, 0
    try:
        D.s2v_set_gemm_g4t(c.g4t)
        out5 = (ctypes.c_int32 * 5)()
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        flags = (gc.PLAN_F16 if c.dt == "f16" else 0) | (gc.PLAN_ROPE if diag_entry else 0)
        assert D.s2v_diag_gemm_plan(M, N, c.plan_K, 4, flags, ncu, 0, out5) == 0, D.s2v_last_error()
        assert (gc.KERNELS[out5[3]], gc.KERNELS[out5[4]]) == c.plan, f"{name} on {ncu} CUs: the plan is {(gc.KERNELS[out5[3]], gc.KERNELS[out5[4]])}"
        for nm, p in use:
            pd = p.to(DEV)
            a_dev = torch.zeros(gc.rup(M, 256) if diag_entry else M, K, dtype=dt, device=DEV)
            a_dev[M:] = gc.PAD_VALUE
            a_dev[torch.arange(M, device=DEV), pd] = ampd.to(dt)
            y16 = gc.g_reference(Wd, ampd, pd, biasd, dt)
            expected, bar = gc.qknorm_reference(y16, c.D, lnd, csd, c.tok, c.text_len, QK_EPS, dt)
            out = gc.OutBuf(M, N, N, dt, None, DEV)
            cp = ctypes.c_void_p(out.buf.data_ptr() + out.body_ptr_offset())
            if diag_entry:
                rc = lib.s2v_diag_qkv_qknorm(P(a_dev), P(w_arg), P(biasd), P(lnd[0]), P(lnd[1]), P(lnd[2]), P(lnd[3]), P(csd), cp, M, c.D, K, c.tok,
                                             c.text_len, ctypes.c_float(QK_EPS), L.stream_ptr())
            else:
                la = torch.randn(c.rank, K, device=DEV)
                lb = torch.zeros(N, c.rank, device=DEV)
                aux0, aux1 = torch.cat([lnd[0], lnd[2]]).contiguous(), torch.cat([lnd[1], lnd[3]]).contiguous()
                rc = lib.s2v_op_linear_lora(P(a_dev), P(w_arg), P(biasd), P(la), P(lb), c.rank, 1.0, cp, M, N, K, 4, P(aux0), P(aux1), L.DTYPE_OF[dt],
                                            L.stream_ptr())
            assert rc == 0, lib.s2v_last_error()
            torch.cuda.synchronize()
            got = out.body()
            assert out.guards_intact(), f"{name} map {nm}: the guard rows around the output changed"
            bad_v = got[:, 2 * c.D:].contiguous().view(torch.int16) != y16[:, 2 * c.D:].contiguous().view(torch.int16)
            assert not bad_v.any().item(), f"{name} map {nm}: the v third differs from the projection: {describe(bad_v.cpu(), p)}"
            assert torch.isfinite(got.float()).all().item()
            ratio = (got[:, :2 * c.D].double() - expected[:, :2 * c.D].double()).abs() / bar
            worst = max(worst, ratio.max().item())
            compared += got.numel()
            if worst > 1.0:
                i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
                print(f"\nMEASURED gemm_exact_qknorm {name} {libname} map {nm}: worst ratio {ratio.max().item():.3f} at {i} (row % tok {i[0] % c.tok}): got "
                      f"{got[i].item()!r}, fp64-with-rounding-points {expected[i].item()!r}, bar {bar[i].item():.3e}; {(ratio > 1).sum().item()} over the bar")
    finally:
        D.s2v_set_gemm_g4t(1)
    print(f"\nMEASURED gemm_exact_qknorm {name} {libname} kernel={'+'.join(k for k in c.plan if k != 'none')} compared={compared} worst_ratio_to_bar={worst:.3f}")
    assert worst <= 1.0, f"{name}: an element is {worst:.3f} times its bar from the fp64 reference"
