"""KV split of the four-wave attention launch (pytest -m gpu): the two trailing q-blocks of every head run as S = 4 parts each over contiguous key ranges, and
the part that arrives last merges them (kernels.h attn_plan, attention_q4.hip attn_qx_merge).  Operator level, impl 0 (attn_q4 beyond 4608
tokens) and impl 4 (attn_q4h), at the smallest lengths at which the four-wave kernel runs and the split can go wrong:

  (B, H, N) = (1, 2, 4609)  the last split q-block has ONE real row (and 73 KV tiles: parts of 19 and 18, the last tile holds one key)
              (1, 2, 4864)  both split q-blocks are full, 76 tiles
              (2, 3, 4700)  a ragged last KV tile inside the last part, two samples, three heads
              (1, 1, 5000)

Bars: the project's own for operator-level attention against fp64 SDPA (tests/test_gpu_parity.py: ATTN_REL_L2_BARS and max-abs 2e-2 of
max(1, max|ref|)), over the whole output and separately over the rows of the split q-blocks; the constant-V bound of
test_attention_full_size_constant_value_rows.  The bit invariances are torch.equal.  The per-item == persistent comparison runs attn_q4 only: the
diagnostics variants 6 / 7 are the one way to a persistent launch of this size, and they run the bf16-P kernel."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(1, 2, 4609), (1, 2, 4864), (2, 3, 4700), (1, 1, 5000)]
IMPLS = [0, 4]
FMT = {0: 0, 4: 1}  # s2v_diag_attn_plan format of the kernel behind the impl beyond 4608 tokens: attn_q4, attn_q4h
MAX_ABS = 2e-2
ATTN_REL_L2_BARS = {"bf16": 6.3e-3}  # the rule and number of tests/test_gpu_parity.py ATTN_REL_L2_BARS (as test_gpu_gemm_schedules.py holds it)


def kv_plan(s2v, N, impl):
    """(first row of the split q-blocks, [first key of part s] + [N]) from the rule itself"""
    diag = s2v._lib.diag_lib()
    diag.s2v_diag_attn_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    out = (ctypes.c_int32 * 16)()
    assert diag.s2v_diag_attn_plan(N, FMT[impl], out) == 0
    whole, split, S = out[0], out[1], out[2]
    assert split >= 1 and S >= 2, "these lengths are split"
    return whole * 256, [min(64 * out[4 + s], N) for s in range(S + 1)]


def reference(qkv, B, H, N, keys=None):
    """fp64 softmax(q k^T / 8) v per (sample, head) on the device, as test_op_attention builds it; keys = (lo, hi): over those keys only"""
    D = H * 64
    x = qkv[: B * N].to(DEV).double().reshape(B, N, 3, H, 64)
    out = torch.empty(B, N, H, 64, dtype=torch.float64, device=DEV)
    lo, hi = keys if keys else (0, N)
    for b in range(B):
        for h in range(H):
            s = x[b, :, 0, h] @ x[b, lo:hi, 1, h].T * 0.125
            out[b, :, h] = torch.softmax(s, dim=-1) @ x[b, lo:hi, 2, h]
    return out.reshape(B * N, D)


def randn_qkv(B, H, N, seed, dt=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randn(B * N, 3 * H * 64, generator=g).to(dt), torch.zeros(64, 3 * H * 64, dtype=dt)])


def run_op(s2v, qkv, B, H, N, impl, lib=None):
    L = s2v._lib
    qd = qkv.to(DEV)
    out = torch.full((B * N, H * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(B * H * 64 * ((N + 63) // 64 * 64), dtype=torch.bfloat16, device=DEV)
    L.check((lib or L.lib()).s2v_op_attention(L.ptr(qd), L.ptr(vt), L.ptr(out), B, H, N, L.DTYPE_BF16, impl, L.stream_ptr()))
    torch.cuda.synchronize()
    return out


def split_rows(B, N, row0):
    return torch.cat([torch.arange(b * N + row0, (b + 1) * N) for b in range(B)]).to(DEV)


def assert_bars(got, ref, rows, what):
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    for name, g, r in (("whole output", got, ref), ("split rows", got[rows], ref[rows])):
        err = (g - r).abs().max().item()
        rel = ((g - r).norm() / r.norm()).item()
        print(f"MEASURED {what} {name}: rel-l2 {rel:.3e} max-abs {err:.3e} (max|ref| {r.abs().max().item():.3e})")
        assert err <= MAX_ABS * max(1.0, r.abs().max().item()), f"{what}, {name}: max-abs {err}"
        assert rel <= ATTN_REL_L2_BARS["bf16"], f"{what}, {name}: rel-l2 {rel}"


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("B,H,N", CASES)
def test_split_against_fp64_with_a_spike_in_every_part(s2v, B, H, N, impl):
    """randn inputs with the spiked key row of test_op_attention (row 5, times 6), then the spike moved from part to part: the parts' reference
    exponents differ by the spike's score, and the merge has to weigh them"""
    row0, keys = kv_plan(s2v, N, impl)
    rows = split_rows(B, N, row0)
    D = H * 64
    base = randn_qkv(B, H, N, N)
    for s in range(len(keys) - 1):
        qkv = base.clone()
        r = 5 if s == 0 else min(keys[s] + 5, keys[s + 1] - 1)
        for b in range(B):
            qkv[b * N + r, D : D + 64] *= 6.0
        assert_bars(run_op(s2v, qkv, B, H, N, impl), reference(qkv, B, H, N), rows, f"impl {impl} B{B} H{H} N{N} spike in part {s} (key {r})")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("part", [0, 2, -1])
def test_parts_whose_keys_all_lost_contribute_nothing(s2v, part, impl):
    """every key outside one part scores >= 80 natural units below that part's keys: element 0 of q is 16, of k +24 inside the part and -24
    outside (a gap of 96 in q.k / 8; the 63 random elements move a score by less than 8 either way), so the other parts' weights 2^(m_s - M)
    underflow.  The output must be the answer over that part's keys alone, finite, within the bars"""
    B, H, N = 2, 3, 4700
    row0, keys = kv_plan(s2v, N, impl)
    part %= len(keys) - 1  # -1: the last part, with the ragged tile
    D = H * 64
    qkv = randn_qkv(B, H, N, 77 + part)
    x = qkv[: B * N].reshape(B, N, 3, H, 64)
    x[:, :, 0, :, 0] = 16.0
    x[:, :, 1, :, 0] = -24.0
    x[:, keys[part] : keys[part + 1], 1, :, 0] = 24.0
    xd = x.to(DEV).float()
    rnd = max((xd[b, :, 0, h, 1:] @ xd[b, :, 1, h, 1:].T).abs().max().item() * 0.125 for b in range(B) for h in range(H))
    assert rnd < 8.0, f"precondition: the random part of a score moves it by {rnd}"
    ref = reference(qkv, B, H, N, keys=(keys[part], keys[part + 1]))
    assert_bars(run_op(s2v, qkv, B, H, N, impl), ref, split_rows(B, N, row0), f"impl {impl} only part {part} survives")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("B,H,N", CASES)
def test_constant_value_rows_through_the_merge(s2v, B, H, N, impl):
    """softmax rows sum to 1 through the merge: V constant over the keys gives that constant (the bound of
    test_attention_full_size_constant_value_rows)"""
    row0, _ = kv_plan(s2v, N, impl)
    D = H * 64
    qkv = randn_qkv(B, H, N, 3 * N)
    g = torch.Generator().manual_seed(N + 1)
    const = torch.randn(D, generator=g).bfloat16()
    qkv[:, 2 * D :] = const
    out = run_op(s2v, qkv, B, H, N, impl)
    bound = 2e-2 * const.float().abs().max().item() + 1e-3
    err_all = (out.float() - const.float().to(DEV)[None, :]).abs().max().item()
    err = (out.float()[split_rows(B, N, row0)] - const.float().to(DEV)[None, :]).abs().max().item()
    print(f"MEASURED constant V impl {impl} B{B} H{H} N{N}: split rows {err:.3e}, all rows {err_all:.3e} (bound {bound:.3e})")
    assert err <= bound and err_all <= bound, (err, err_all)


@pytest.mark.parametrize("impl", IMPLS)
def test_bits_do_not_depend_on_batch_or_head_count(s2v, impl):
    """the B = 2 call equals the two B = 1 calls on its halves, the H = 3 call equals three H = 1 calls on its head columns, and a second call
    equals the first"""
    B, H, N = 2, 3, 4700
    D = H * 64
    qkv = randn_qkv(B, H, N, 11)
    both = run_op(s2v, qkv, B, H, N, impl)
    assert torch.equal(run_op(s2v, qkv, B, H, N, impl), both), "a second call differs from the first"
    pad = torch.zeros(64, 3 * D, dtype=qkv.dtype)
    for b in range(B):
        one = run_op(s2v, torch.cat([qkv[b * N : (b + 1) * N], pad]), 1, H, N, impl)
        assert torch.equal(one, both[b * N : (b + 1) * N]), f"sample {b} alone differs from its half of the B = 2 call"
    for h in range(H):
        cols = torch.cat([torch.arange(i * D + h * 64, i * D + (h + 1) * 64) for i in range(3)])
        one = run_op(s2v, qkv[:, cols].contiguous(), B, 1, N, impl)
        assert torch.equal(one, both[:, h * 64 : (h + 1) * 64]), f"head {h} alone differs from its columns of the H = 3 call"


@pytest.fixture(scope="module")
def attn_queue(s2v):
    """nine zeroed counters for the persistent variants of the diagnostics library (the fixture of test_gpu_attention_addressing.py)"""
    diag = s2v._lib.diag_lib()
    diag.s2v_set_attn_queue.argtypes = [ctypes.c_void_p, ctypes.c_int]
    q = torch.zeros(16, dtype=torch.int32, device=DEV)
    diag.s2v_set_attn_queue(ctypes.c_void_p(q.data_ptr()), torch.cuda.get_device_properties(0).multi_processor_count)
    yield q
    torch.cuda.synchronize()
    diag.s2v_set_attn_queue(None, 0)


def run_diag(s2v, qkv, B, H, N, variant, queue, nosplit=False):
    """attn_q4 through the diagnostics library: variant 6 one workgroup per item, 7 persistent on the harness queue; afterwards the queue and the
    counters of the split (sub-item queues, arrival counters) must all be zero"""
    diag = s2v._lib.diag_lib()
    diag.s2v_diag_attn_kv_counters.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
    try:
        diag.s2v_set_attn_variant(variant)
        diag.s2v_diag_attn_kv_nosplit(1 if nosplit else 0)
        out = run_op(s2v, qkv, B, H, N, 0, lib=diag)
    finally:
        diag.s2v_set_attn_variant(0)
        diag.s2v_diag_attn_kv_nosplit(0)
    nonzero, nbytes = ctypes.c_int32(-1), ctypes.c_int64(-1)
    assert diag.s2v_diag_attn_kv_counters(ctypes.byref(nonzero), ctypes.byref(nbytes)) == 0
    assert nonzero.value == 0, f"variant {variant}: {nonzero.value} counters of the split are not zero after the launch"
    assert not queue.any().item(), f"variant {variant}: the launch left its work counters non-zero"
    return out, nbytes.value


@pytest.mark.parametrize("B,H,N", CASES)
def test_launch_forms_agree_and_whole_blocks_keep_their_bits(s2v, attn_queue, B, H, N):
    row0, keys = kv_plan(s2v, N, 0)
    qkv = randn_qkv(B, H, N, 5 * N)
    per_item, nbytes = run_diag(s2v, qkv, B, H, N, 6, attn_queue)
    assert nbytes > 0, "the split launch took no workspace: it did not split"
    persistent, _ = run_diag(s2v, qkv, B, H, N, 7, attn_queue)
    assert torch.equal(per_item, persistent), "per-item and persistent launch differ"
    again, _ = run_diag(s2v, qkv, B, H, N, 7, attn_queue)
    assert torch.equal(again, persistent), "a second persistent launch differs from the first"
    unsplit, _ = run_diag(s2v, qkv, B, H, N, 6, attn_queue, nosplit=True)
    keep = torch.ones(B * N, dtype=torch.bool, device=DEV)
    keep[split_rows(B, N, row0)] = False
    assert torch.equal(per_item[keep], unsplit[keep]), "rows of whole q-blocks changed their bits"
    rows = split_rows(B, N, row0)
    d = (per_item[rows].float() - unsplit[rows].float()).abs().max().item()
    print(f"MEASURED B{B} H{H} N{N}: split rows against the unsplit run: max-abs {d:.3e}, bit-equal {torch.equal(per_item[rows], unsplit[rows])}")
    assert_bars(per_item, reference(qkv, B, H, N), rows, f"diag variant 6 B{B} H{H} N{N}")
