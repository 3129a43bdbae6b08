"""Addressing and masking of every attention kernel (pytest -m gpu), through the C ABI, on the sign-code inputs of oracle/attn_cases.py.

The randn comparisons of test_gpu_parity.py / test_gpu_gemm_schedules.py / test_gpu_f32m.py cannot see a kernel that reads, drops or masks the
wrong key beyond a few hundred tokens (tests/test_attention_conformance_cpu.py shows it on a CPU emulation).  Here every key is decisive for some
query:

  * one-hot (q = 4 s_pi(i), k_j = 4 s_j): the expected output is V[pi(i)] itself; bar = one ulp of the output dtype at |V[pi(i)]| plus
    leak * max|V|, the leak bound derived from the exact Gram matrix of the codes and asserted <= 2^-30 BEFORE the kernel runs.  Seven
    permutations.  The selected key mostly lies outside a row's first KV tile, so every row of attn_q4 / attn_q4h / attn_q4hh goes through the
    deferred-maximum slow path as well.
  * sharp (codes times 2): a dominant row plus a thin tail of others (own score 32, others <= ~21), against fp64 softmax on the kernel's own rounding of the scaled q, at
    the project's per-dtype bars (bf16 2e-2, fp16 2.5e-3, fp32 2e-5 of max(1, max|ref|)).
  * traps in both: the 64 slack rows after qkv (V = 1e4) and, with two batches, the first rows of batch 1 carry codes that queries of the batch
    before them ask for; the reference of those queries is the soft fp64 result over the batch's own keys.

fp8 QK^T: the codes +-4 and +-2 are powers of two and survive MX e4m3 exactly; q's prescale (scale * log2 e) moves all 32 elements of a block
alike, and the e4m3 rounding of that one magnitude changes it by at most 2^-4 relative -- every score of a row scales by the same factor, so
the one-hot margin shrinks by at most 2^-4 (checked on the emulated quantisation below, and the leak bound uses the shrunk margin).

Output buffers are pre-filled with NaN, V^T scratch is zero-filled as the ABI asks.  Lengths: attn_cases.LENGTH_CLASSES; full length (19126 and
50626 tokens, H = 2): one-hot only, since its reference needs no N x N softmax.

Every case also runs with V of each (batch, head) times its own power of two (attn_cases.V_EXPS: from 2^17, beyond the fp16 range, down to
2^-20): the kernels with an fp16 V^T (impl 3 beyond 4608 tokens, impl 4, fp8-QK with fp16 P) hold V^T per (batch, head) times a power of two
taken from its largest magnitude, and a wrong word there is a factor of 2^k in the output.

FINDING (fixed with these tests).  The kernels with an fp16 V^T missed the one-hot bar on the elements of V below 2^-18 in magnitude:
v_transpose_k converted bf16 V to fp16 as it was, which rounds values under 2^-14 into the fp16 subnormals (spacing 2^-24), an absolute error of
up to 2^-25 that exceeds one bf16 ulp of so small a value (V = -1.8179e-06 returned as -1.7881e-06 = -30 * 2^-24, 4 bf16 ulps, in eight cases
between 1250 and 5000 tokens; 6 elements, worst 244 ulps, at 19126 tokens; nothing else differed).  V^T is now stored per (batch, head) times the
power of two that puts the head's largest |V| into [2^14, 2^15), and the kernel's epilogue takes it out again (kernels.h vt_f16_shift): exact,
no saturation at 65504, and values down to 2^-29 of the largest keep every bit."""
import collections
import ctypes
import functools
import time

import pytest
import torch

from oracle import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

Entry = collections.namedtuple("Entry", "id kind arg dt qmode")
ENTRIES = [
    Entry("impl0-bf16", "op", 0, "bf16", "bf16"),        # launch_attn_bf16: attn_pp up to 4608 tokens, attn_q4 beyond
    Entry("impl3-bf16", "op", 3, "bf16", "bf16"),        # as 0 with fp16 P / V^T where the four-wave kernel runs (attn_q4h)
    Entry("impl4-bf16", "op", 4, "bf16", "bf16"),        # attn_q4h at any length
    Entry("fp8qk-bf16", "fp8", 0, "bf16", "mx"),         # attn_q4f behind v_transpose_k and qk_quant_mx_k
    Entry("fp8qk-p16-bf16", "fp8", 1, "bf16", "mx"),     # attn_q4fh: the same with fp16 P / V^T
    Entry("diag6-bf16", "diag", 6, "bf16", "bf16"),      # attn_q4 at any length
    Entry("diag7-bf16", "diag", 7, "bf16", "bf16"),      # attn_q4, persistent on a harness queue
    Entry("diag8-bf16", "diag", 8, "bf16", "bf16"),      # attn_q8
    Entry("diag10-bf16", "diag", 10, "bf16", "bf16"),    # attn_pp at any length
    Entry("diag11-bf16", "diag", 11, "bf16", "bf16"),    # attn_pp, persistent on a harness queue
    Entry("impl1-bf16", "op", 1, "bf16", "natural"),     # VALU kernel
    Entry("impl1-f32", "op", 1, "f32", "natural"),
    Entry("impl5-f32", "op", 5, "f32", "natural"),       # attn_f32m
    Entry("impl1-f16", "op", 1, "f16", "natural"),
    Entry("impl5-f16", "op", 5, "f16", "natural"),
    Entry("impl6-f16", "op", 6, "f16", "f16"),           # fp16 lock-step kernel up to 4608 tokens, attn_q4hh beyond
]
BY_ID = {e.id: e for e in ENTRIES}


@functools.lru_cache(maxsize=32)
def case_of(family, perm, v_mode, dt_name, B, H, N):
    return ac.build(family, perm, dt_name, B, H, N, device=DEV, v_mode=v_mode)


@pytest.fixture(scope="module")
def attn_queue(s2v):
    """nine zeroed counters for the persistent variants of the diagnostics library (they zero themselves again at the end of a launch)"""
    diag = s2v._lib.diag_lib()
    diag.s2v_set_attn_queue.argtypes = [ctypes.c_void_p, ctypes.c_int]
    q = torch.zeros(16, dtype=torch.int32, device=DEV)
    diag.s2v_set_attn_queue(ctypes.c_void_p(q.data_ptr()), torch.cuda.get_device_properties(0).multi_processor_count)
    yield q
    torch.cuda.synchronize()
    diag.s2v_set_attn_queue(None, 0)


def run_entry(s2v, e, case, queue):
    L = s2v._lib
    B, H, N, D = case.B, case.H, case.N, case.D
    dt = ac.STORE[e.dt]
    npad = (N + 63) // 64 * 64
    qd = case.qkv.to(DEV)
    out = torch.full((B * N, D), float("nan"), dtype=dt, device=DEV)
    vt = torch.zeros(B * H * 64 * npad, dtype=torch.float16 if e.dt == "f16" else torch.bfloat16, device=DEV)
    if e.kind == "op":
        L.check(L.lib().s2v_op_attention(L.ptr(qd), L.ptr(vt) if e.arg in (0, 3, 4, 6) else None, L.ptr(out), B, H, N, L.DTYPE_OF[dt], e.arg,
                                         L.stream_ptr()))
    elif e.kind == "fp8":
        r256 = lambda x: (x + 255) // 256 * 256
        need = r256(B * H * N * 64) + r256(B * H * N * 2) + r256(B * H * npad * 64) + r256(B * H * npad * 4) + 4 * B * H
        scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
        fn = L.lib().s2v_op_attention_fp8qk_p16 if e.arg else L.lib().s2v_op_attention_fp8qk
        L.check(fn(L.ptr(qd), L.ptr(vt), L.ptr(scratch), need, L.ptr(out), B, H, N, L.stream_ptr()))
    else:
        diag = L.diag_lib()
        try:
            diag.s2v_set_attn_variant(e.arg)
            L.check(diag.s2v_op_attention(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, L.DTYPE_BF16, 0, L.stream_ptr()))
            torch.cuda.synchronize()
        finally:
            diag.s2v_set_attn_variant(0)
        if e.arg in (7, 11):
            assert not queue.any().item(), "the persistent launch left its work counters non-zero"
    torch.cuda.synchronize()
    return out


def check_mx_claim(case):
    """what the module docstring says about MX e4m3 on these inputs, on the emulated quantisation: k exact, q one magnitude per row within 2^-4"""
    q, k = case.heads(0).float(), case.heads(1).float()
    assert torch.equal(ac.mx_e4m3_roundtrip(k), k)
    qd = ac.mx_e4m3_roundtrip(q * ac.C0).abs()
    assert (qd == qd[..., :1]).all()
    assert ((qd / (ac.FAMILY_C[case.family] * ac.C0) - 1.0).abs() <= 2.0 ** -4).all()


def run_cases(s2v, e, B, H, N, queue, cases):
    bad_all, bit_equal = [], []
    for family, perm, v_mode in cases:
        case = case_of(family, perm, v_mode, e.dt, B, H, N)
        if e.qmode == "mx":
            check_mx_claim(case)
        if family == "onehot":  # the precondition, on the margin the kernel's rounding of q leaves, before the kernel runs
            leak = case.leak(ac.SHRINK[e.qmode])
            assert leak <= ac.LEAK_MAX, f"one-hot precondition: leak {leak:.3e} (maxdot {case.maxdot})"
        got = run_entry(s2v, e, case, queue)
        bad, info = ac.failures(case, got, e.qmode, device=DEV)
        print(f"MEASURED {e.id} B{B} H{H} N{N} {family}/{perm}/{v_mode} maxdot {case.maxdot}: " + " ".join(
            f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in info.items()))
        if family == "onehot":
            bit_equal.append(info["bit_equal"])
        bad_all += [f"{family}/{perm}/{v_mode}: {name}: {detail}" for name, detail in bad]
    print(f"ONEHOT {e.id} B{B} H{H} N{N}: bit-equal to V[pi] in {sum(bit_equal)} of {len(bit_equal)} permutations")
    assert not bad_all, "\n".join(bad_all)


@pytest.mark.parametrize("entry", [e.id for e in ENTRIES])
@pytest.mark.parametrize("B,H,N", ac.LENGTH_CLASSES)
def test_attention_addressing(s2v, attn_queue, B, H, N, entry):
    run_cases(s2v, BY_ID[entry], B, H, N, attn_queue, ac.ALL_CASES)


@pytest.mark.parametrize("entry,N", [("impl0-bf16", 19126), ("impl4-bf16", 19126), ("impl0-bf16", 50626), ("fp8qk-bf16", 50626), ("fp8qk-p16-bf16", 50626)])
def test_attention_addressing_full_length(s2v, attn_queue, entry, N):
    """the lengths the product runs (49 x 480 x 720 and 49 x 720 x 1280 with 226 text tokens), two heads, one-hot: expected output V[pi] itself"""
    t0 = time.time()
    run_cases(s2v, BY_ID[entry], 1, 2, N, attn_queue, [c for c in ac.ALL_CASES if c[0] == "onehot"])
    print(f"full length {entry} N{N}: {time.time() - t0:.1f} s")
