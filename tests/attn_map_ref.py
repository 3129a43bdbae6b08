"""The restatement of the attention mass (csrc/attn_mass.hip; include/s2v_hip.h "Attention map"), shared by tests/test_attn_map_cpu.py,
tests/test_gpu_attn_mass.py and tests/test_gpu_attn_map.py.  Plain torch; no kernel is called here.

  mass_reference   fp64 softmax on the kernel's own rounding of the scaled q (the qmodes of oracle.attn_cases.soft_reference), range sums
  checks           every check of a case's family on a kernel's (or an emulation's) output
  emulate          the tiled online algorithm of the matrix-pipe kernel on the CPU in fp32, with the mutations the checks must catch
  recorded_forward oracle.transformer_ref.transformer_forward with q and k of every block's attention recorded
"""
import math

import torch

from oracle import attn_cases as AC
from oracle import transformer_ref as TR

KTILE = 64
RCP = 2.0 ** -22           # v_rcp_f32: one ulp at 1
EMU_BAR = 1e-5             # the fp32 emulation against fp64: exp2 of a score rounded at |s| <= 64 carries <= 2^-19 ln 2 = 1.3e-6 relative, a
                           # mass is <= 1 and a sum of such terms, and the final division adds 2^-23: 1e-5 leaves a factor of 5
MUTATIONS = ("tile_index", "no_tail_mask", "next_sample", "q0_ignored", "no_rescale")


def range_sets(N):
    a, c = N // 3 + 1, (2 * N) // 3 + 2
    return [[(0, N)], [(0, 1), (N - 1, N)], [(N // 3, min(N, N // 3 + 37))], [(5, 5)], [(0, a), (a, c), (c, N)]]


def query_sets(N):
    return [(0, N), (N // 4 + 1, N - (N // 4 + 1))]


def randn_case(dt_name, B, H, N, seed=3):
    """q, k ~ N(0, 1) in the storage type (v too; the slack rows carry large keys no real key has: an unmasked tail shows)"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N + 64, 3 * H * 64, generator=g)
    qkv[B * N:, H * 64:2 * H * 64] *= 8.0
    qkv = qkv.to(AC.STORE[dt_name])
    return AC.AttnCase("randn", "none", dt_name, B, H, N, qkv, torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.bool), 0, 0.0,
                       torch.zeros(B, H))


def scaled_q(case, qmode):
    """the kernel's rounding of the scaled q as fp64 [B, H, N, 64], and the base of its exponential"""
    q = case.heads(0)
    if qmode == "natural":
        return q * 0.125, math.e
    return (q.float() * AC.C0).to(AC.STORE[qmode]).double(), 2.0


def mass_of(qs, k, base, ranges, q0, nq):
    """fp64 [n, B, H, nq]: qs and k [B, H, N, 64], scores qs . k in units of log_base"""
    s = qs[:, :, q0:q0 + nq] @ k.transpose(-1, -2) * math.log(base)
    p = torch.softmax(s, dim=-1)
    return torch.stack([p[..., k0:k1].sum(dim=-1) for k0, k1 in ranges])


def mass_reference(case, qmode, ranges, q0, nq):
    key = (qmode, tuple(ranges), q0, nq)
    if key not in case.refs:
        qs, base = scaled_q(case, qmode)
        case.refs[key] = mass_of(qs, case.heads(1), base, ranges, q0, nq)
    return case.refs[key]


def brute_force(case, qmode, ranges, q0, nq):
    """the triple loop (python floats): only for tiny N"""
    qs, base = scaled_q(case, qmode)
    k = case.heads(1)
    out = torch.zeros(len(ranges), case.B, case.H, nq, dtype=torch.float64)
    for b in range(case.B):
        for h in range(case.H):
            for i in range(nq):
                s = [sum(float(qs[b, h, q0 + i, d]) * float(k[b, h, j, d]) for d in range(64)) * math.log(base) for j in range(case.N)]
                m = max(s)
                e = [math.exp(x - m) for x in s]
                tot = sum(e)
                for r, (k0, k1) in enumerate(ranges):
                    out[r, b, h, i] = sum(e[k0:k1]) / tot
    return out


def checks(case, got, qmode, ranges, q0, nq, bar):
    """got [n, B, H, nq] -> list of (check, detail) that failed.  One-hot family: non-trap rows against the indicator of pi(i) within
    leak + 2^-22, trap rows against the restatement within `bar`; other families: every row against the restatement within `bar`.
    Whatever the family: finite, an empty range exactly 0, the range [0, N) 1 within 2^-22, a partition sums to 1 within `bar`"""
    bad = []
    got = got.detach().cpu().double()
    n, N = len(ranges), case.N
    if tuple(got.shape) != (n, case.B, case.H, nq):
        return [("shape", f"{tuple(got.shape)}")]
    if not torch.isfinite(got).all():
        bad.append(("finite", f"{(~torch.isfinite(got)).sum().item()} non-finite"))
        got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
    ref = mass_reference(case, qmode, ranges, q0, nq)
    rows = torch.arange(q0, q0 + nq)
    trap = case.trap[rows]
    if case.family == "onehot":
        leak = case.leak(AC.SHRINK[qmode])
        assert leak <= AC.LEAK_MAX, f"one-hot precondition: leak {leak:.3e}"
        sel = ~trap
        for r, (k0, k1) in enumerate(ranges):
            want = ((case.pi[rows] >= k0) & (case.pi[rows] < k1)).double()
            err = (got[r][..., sel] - want[sel]).abs()
            if sel.any() and err.max().item() > leak + RCP:
                bad.append(("onehot", f"range {r} [{k0},{k1}): worst |mass - indicator| {err.max().item():.3e} > {leak + RCP:.3e}"))
        soft = trap
    else:
        soft = torch.ones(nq, dtype=torch.bool)
    if soft.any():
        err = (got[..., soft] - ref[..., soft]).abs().max().item()
        if err > bar:
            bad.append(("restatement", f"max-abs {err:.3e} > {bar:.3e}"))
    for r, (k0, k1) in enumerate(ranges):
        if k0 == k1 and not (got[r] == 0.0).all():
            bad.append(("empty", f"range {r} is empty and not exactly 0: max {got[r].abs().max().item():.3e}"))
        if (k0, k1) == (0, N) and (got[r] - 1.0).abs().max().item() > RCP:
            bad.append(("whole", f"range [0, N): worst |mass - 1| {(got[r] - 1.0).abs().max().item():.3e} > 2^-22"))
    if n > 1 and ranges[0][0] == 0 and ranges[-1][1] == N and all(ranges[r][1] == ranges[r + 1][0] for r in range(n - 1)):
        e = (got.sum(dim=0) - 1.0).abs().max().item()
        if e > bar:
            bad.append(("partition", f"worst |sum - 1| {e:.3e} > {bar:.3e}"))
    return bad


def max_error(case, got, qmode, ranges, q0, nq):
    """largest absolute error against the restatement (what a bar is measured from)"""
    return (got.detach().cpu().double() - mass_reference(case, qmode, ranges, q0, nq)).abs().max().item()


def emulate(case, qmode, ranges, q0, nq, mutation=None):
    """the matrix-pipe kernel's algorithm in fp32 on the CPU: q * scale * log2 e rounded to the storage type, tiles of 64 keys read from the
    buffer as it lies in memory (slack rows included), the ragged tail masked before the maximum, an online maximum, a running sum over all
    keys and one per range rescaled when the maximum moves, mass = range_sum / all_sum.  mutation: one of MUTATIONS"""
    assert mutation is None or mutation in MUTATIONS
    B, H, N, D = case.B, case.H, case.N, case.D
    buf = case.qkv.float()
    rows_total = buf.shape[0]
    out = torch.zeros(len(ranges), B, H, nq)
    qstart = 0 if mutation == "q0_ignored" else q0
    for b in range(B):
        for h in range(H):
            q = buf[b * N + qstart:b * N + qstart + nq, h * 64:(h + 1) * 64]
            qs = (q * AC.C0).to(AC.STORE[qmode]).float()
            m = torch.full((nq,), -math.inf)
            l = torch.zeros(nq)
            rs = torch.zeros(len(ranges), nq)
            for t in range((N + KTILE - 1) // KTILE):
                kv0 = t * KTILE
                idx = torch.arange(kv0, kv0 + KTILE)
                rows = (b * N + idx).clamp_max(rows_total - 1)
                k = buf[rows, D + h * 64:D + (h + 1) * 64]
                s = qs @ k.T
                if mutation == "no_tail_mask":
                    valid = torch.ones(KTILE, dtype=torch.bool)
                elif mutation == "next_sample":
                    valid = b * N + idx < B * N
                else:
                    valid = idx < N
                s = torch.where(valid[None], s, torch.full_like(s, -math.inf))
                mn = torch.maximum(m, s.max(dim=1).values)
                alpha = torch.exp2(m - mn)
                p = torch.exp2(s - mn[:, None])
                l = l * alpha + p.sum(dim=1)
                key = idx - kv0 if mutation == "tile_index" else idx
                for r, (k0, k1) in enumerate(ranges):
                    inr = ((key >= k0) & (key < k1)).float()
                    if mutation != "no_rescale":
                        rs[r] = rs[r] * alpha
                    rs[r] = rs[r] + (p * inr[None]).sum(dim=1)
                m = mn
            out[:, b, h] = rs / l[None]
    return out


def mean_reference(acc, count):
    """the head mean in the kernel's order: (acc[.,.,0] + acc[.,.,1] + ... ) * (1.0f / (H * count)), every operation in fp32"""
    n, B, H, V = acc.shape
    s = torch.zeros((n, B, V), dtype=torch.float32, device=acc.device)
    for h in range(H):
        s = s + acc[:, :, h]
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H * count), dtype=torch.float32)
    return s * inv.to(acc.device)


class _Recorder:
    """stands in for torch.nn.functional inside oracle.transformer_ref: records q and k of every scaled_dot_product_attention call and
    delegates everything, that call included"""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def scaled_dot_product_attention(self, q, k, v, *a, **kw):
        self.calls.append((q.detach().clone(), k.detach().clone()))
        return self._real.scaled_dot_product_attention(q, k, v, *a, **kw)


def recorded_forward(*args, **kw):
    """(transformer_forward(*args, **kw), [(q, k) of block 0, block 1, ...]), q and k [B, H, Ntok, 64] normed and rotated"""
    real = TR.F
    rec = _Recorder(real)
    TR.F = rec
    try:
        with torch.no_grad():
            out = TR.transformer_forward(*args, **kw)
    finally:
        TR.F = real
    return out, rec.calls


def oracle_mass(q, k, ranges, q0, nq):
    """fp64 [n, B, H, nq] of recorded q, k: softmax(q . k / 8), as F.scaled_dot_product_attention scores them"""
    return mass_of(q.double() * 0.125, k.double(), math.e, ranges, q0, nq)
