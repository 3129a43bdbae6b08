"""Attention inputs on which every key is decisive for some query, and the checks that go with them (plain torch; no kernel is called here).

The randn inputs of the older attention tests give outputs that are the mean of ~N/e value rows (rms 0.18 at N = 5000) under a bar of
2e-2 * max|ref| ~ 0.06: a kernel that drops a tile, leaks the next batch into the ragged tail or leaves pad keys unmasked stays under it
(tests/test_attention_conformance_cpu.py pins that).  Here q and k are SIGN CODES: key j of a (batch, head) is c * s_j with s_j in {+-1}^64,
seeded, distinct per row of the whole buffer (asserted through the exact Gram matrix), different per head.  A query c * s_j scores c^2 * 64 / 8
against its own key and at most c^2 * maxdot / 8 against any other, so

  * c = 4 ("onehot"): margin 2 * (64 - maxdot) >= 36 natural units -- the softmax is one-hot to below 2^-30 (precondition, asserted before a kernel
    runs) and the expected output is V[pi(i)] ITSELF, at any length, for any permutation pi.  Bar (derived): one ulp of the output dtype at
    |V[pi(i)]| plus leak * max|V|.
  * c = 2 ("sharp"): own score 32, others <= ~21: a dominant row plus a thin tail of others (a softer softmax than one-hot, not a flat one); reference = fp64 softmax on the kernel's own
    rounding of the scaled q, bars = the project's per-dtype ones against max(1, max|ref|).

Traps (both families): the 64 slack rows the ABI asks for after qkv carry codes no real key has and V = 1e4; with B = 2 the rows after batch 0
are batch 1's first keys, which batch 0 lacks as well.  A few queries per 256-row block (and the last row) ask for the code of one of the 64
rows that FOLLOW their batch in memory; their reference is the fp64 softmax over the batch's real keys -- a soft, O(1) answer -- so an unmasked
pad key or a leaked neighbour takes the whole row (error O(1) .. 1e4)."""
import functools
import math
from dataclasses import dataclass, field

import torch

C0 = 0.125 * 1.4426950408889634          # the kernels' scale * log2(e)
STORE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MANT = {"f32": 23, "bf16": 7, "f16": 10}  # stored mantissa bits: one ulp at x = 2^(floor(log2 |x|) - MANT)
EMIN = {"f32": -126, "bf16": -126, "f16": -14}
SOFT_BARS = {"bf16": 2e-2, "f16": 2.5e-3, "f32": 2e-5}   # tests/test_gpu_parity.py, test_gpu_f32m.py: max-abs against max(1, max|ref|)
PERMS = ("identity", "reversal", "random", "all_last", "all_first", "tile_first", "tile_last")
FAMILY_C = {"onehot": 4.0, "sharp": 2.0}
TRAP_V = 1.0e4
TRAP_SLOTS = (7, 100, 255)               # rows i with i % 256 in TRAP_SLOTS, and the last row, ask for a trap code
LEAK_MAX = 2.0 ** -30
SHRINK = {"natural": 1.0, "bf16": 1.0 - 2.0 ** -8, "f16": 1.0 - 2.0 ** -11, "mx": 1.0 - 2.0 ** -4}   # what a kernel's rounding of the scaled q leaves of the margin
# v_mode "spread": V of (batch b, head h) is randn times 2^V_EXPS[b * H + h] -- distinct per batch and head, beyond the fp16 range at one end
# (|V| > 65504) and deep in its subnormals at the other.  The kernels with an fp16 V^T store each (batch, head) times a power of two taken from its
# own largest magnitude: a wrong batch or head index there, or a V^T pass and an epilogue that read different words, shows as a factor of 2^k.
# fp16 storage cannot hold the ends, so its exponents are clamped to [-8, 12].
V_EXPS = (17, -20, 6, -9, 11, -3)
# (B, H, N): N mod 64 in {0, 1, 63}, N mod 256 in {0, 1, 255}, fewer than / exactly five / six KV tiles (attn_q4's last-five-tiles phase), the
# 4608-token switch between attn_pp and attn_q4, 5000, under one tile, two batches with a ragged length (below and beyond the switch), three heads
LENGTH_CLASSES = [(2, 2, 31), (1, 2, 64), (1, 2, 65), (1, 2, 127), (1, 2, 255), (1, 2, 256), (1, 2, 257), (1, 2, 320), (1, 2, 321), (1, 2, 384),
                  (2, 2, 449), (1, 3, 200), (2, 3, 1250), (1, 2, 4608), (1, 2, 4609), (1, 2, 5000), (2, 3, 4700)]


# (family, permutation, v_mode) every kernel and the CPU emulation go through at every length class
ALL_CASES = [("onehot", p, "unit") for p in PERMS] + [("sharp", "random", "unit"), ("onehot", "identity", "spread"), ("onehot", "random", "spread"),
                                                      ("sharp", "random", "spread")]


def sign_codes(rows, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2, (rows, H, 64), generator=g, dtype=torch.int8) * 2 - 1


def max_offdiag_dot(codes, device="cpu", chunk=1024):
    """largest s_i . s_j over i != j of one head's codes [rows, 64] (+-1): sums of 64 terms of +-1 are exact in fp32"""
    c = codes.to(device=device, dtype=torch.float32)
    rows = c.shape[0]
    best = -64
    for i0 in range(0, rows, chunk):
        g = c[i0:i0 + chunk] @ c.T
        idx = torch.arange(i0, min(i0 + chunk, rows), device=g.device)
        g[idx - i0, idx] = -64.0
        best = max(best, int(g.max().item()))
    return best


@functools.lru_cache(maxsize=4)
def _codes_and_maxdot(rows, H, seed, device):
    codes = sign_codes(rows, H, seed)
    return codes, max(max_offdiag_dot(codes[:, h], device) for h in range(H))


def permutation(name, N, seed):
    i = torch.arange(N)
    nt = (N + 63) // 64
    if name == "identity":
        return i
    if name == "reversal":
        return N - 1 - i
    if name == "random":
        return torch.randperm(N, generator=torch.Generator().manual_seed(seed))
    if name == "all_last":
        return torch.full((N,), N - 1)
    if name == "all_first":
        return torch.zeros(N, dtype=torch.int64)
    if name == "tile_first":
        return (i % nt) * 64
    if name == "tile_last":
        return ((i % nt) * 64 + 63).clamp_max(N - 1)
    raise ValueError(name)


def ulp_at(x, dt_name):
    e = torch.frexp(x.double().abs())[1].to(torch.float64) - 1.0
    return torch.exp2(e.clamp_min(EMIN[dt_name]) - MANT[dt_name])


def mx_e4m3_roundtrip(x):
    """MX e4m3 as qk_quant_mx_k makes it: blocks of 32 along the last dimension, power-of-two scale = the smallest with amax / scale <= 448,
    elements rounded to e4m3 (round to nearest even); returns the dequantised fp32 values"""
    xb = x.float().reshape(*x.shape[:-1], -1, 32)
    m, e = torch.frexp(xb.abs().amax(dim=-1) / 448.0)
    scale = torch.exp2((e - (m == 0.5).to(e.dtype)).float()).unsqueeze(-1)
    return ((xb / scale).to(torch.float8_e4m3fn).float() * scale).reshape(x.shape)


@dataclass
class AttnCase:
    family: str
    perm: str
    dt_name: str
    B: int
    H: int
    N: int
    qkv: torch.Tensor       # [B * N + 64, 3 * H * 64] in the storage dtype, slack rows included
    pi: torch.Tensor        # [N] key a non-trap query selects
    trap: torch.Tensor      # [N] bool: rows that ask for a code of the 64 rows after their batch
    maxdot: int
    margin: float           # natural units, before the kernel's rounding of q
    vexp: torch.Tensor = None   # [B, H] exponent of the factor on V (zeros for v_mode "unit")
    refs: dict = field(default_factory=dict, repr=False)   # soft references already formed, by qmode

    @property
    def D(self):
        return self.H * 64

    def heads(self, part):
        """q (0) / k (1) / v (2) of the real rows as fp64 [B, H, N, 64]"""
        x = self.qkv[:self.B * self.N, part * self.D:(part + 1) * self.D].double()
        return x.reshape(self.B, self.N, self.H, 64).transpose(1, 2)

    def leak(self, shrink=1.0):
        """bound on the softmax weight outside the selected key: N * exp(-margin), the margin shrunk by the kernel's rounding of the scaled q
        (bf16: 2^-8, fp16: 2^-11, MX e4m3: 2^-4 -- uniform over a code's 64 elements, so it scales every score of a row alike)"""
        return self.N * math.exp(-self.margin * shrink)


def build(family, perm, dt_name, B, H, N, seed=1, device="cpu", v_mode="unit"):
    """device: where the Gram matrix is formed (exact anywhere); everything returned lives on the CPU.  v_mode: "unit" or "spread" (V_EXPS)"""
    c = FAMILY_C[family]
    rows = B * N + 64
    D = H * 64
    for attempt in range(8):  # a draw whose closest pair of codes is too close for the one-hot precondition is drawn again (seeded: deterministic)
        codes, maxdot = _codes_and_maxdot(rows, H, seed + 7919 * attempt, str(device))
        margin = c * c * (64 - maxdot) / 8.0
        if family != "onehot" or N * math.exp(-margin * (1.0 - 2.0 ** -4)) <= LEAK_MAX:
            break
    assert maxdot < 64, "two rows carry the same code"
    g = torch.Generator().manual_seed(seed + 104729)
    v = torch.randn(rows, H, 64, generator=g)
    vexp = torch.zeros(B, H)
    if v_mode == "spread":
        assert B * H <= len(V_EXPS)
        vexp = torch.tensor(V_EXPS[:B * H], dtype=torch.float32).reshape(B, H)
        if dt_name == "f16":
            vexp = vexp.clamp(-8, 12)
        v[:B * N] *= torch.exp2(vexp).repeat_interleave(N, dim=0).unsqueeze(-1)
    else:
        assert v_mode == "unit"
    v[B * N:] = TRAP_V
    pi = permutation(perm, N, seed + 17)
    i = torch.arange(N)
    trap = torch.zeros(N, dtype=torch.bool)
    for s in TRAP_SLOTS:
        trap |= (i % 256) == s
    if N >= 2:
        trap[N - 1] = True
    tj = (i * 7) % 64
    tj[N - 1] = 0           # the last row asks for the very next row in memory: the first pad key of a ragged tail
    q = torch.zeros(rows, H, 64)
    for b in range(B):
        src = torch.where(trap, (b + 1) * N + tj, b * N + pi)
        q[b * N:(b + 1) * N] = c * codes[src].float()
    k = c * codes.float()
    qkv = torch.cat([q.reshape(rows, D), k.reshape(rows, D), v.reshape(rows, D)], dim=1).to(STORE[dt_name])
    return AttnCase(family, perm, dt_name, B, H, N, qkv, pi, trap, maxdot, margin, vexp)


def soft_reference(case, qmode, rows=None, device="cpu", chunk=2048):
    """fp64 softmax attention over each batch's real keys on the kernel's own rounding of the scaled q.  qmode: "natural" (q * 0.125 exact, exp:
    the fp32-pipe and VALU kernels), "bf16" / "f16" (q * scale * log2 e rounded to that type, exp2), "mx" (q * scale * log2 e and k as MX e4m3).
    rows: bool [N] to restrict the queries.  Returns [B, H, n, 64] on the CPU"""
    q, k, v = (case.heads(p).to(device) for p in range(3))
    if rows is not None:
        q = q[:, :, rows.to(device)]
    if qmode == "natural":
        qs, base = q * 0.125, math.e
    elif qmode in ("bf16", "f16"):
        qs, base = (q.float() * C0).to(STORE[qmode]).double(), 2.0
    elif qmode == "mx":
        qs, k, base = mx_e4m3_roundtrip(q.float() * C0).double(), mx_e4m3_roundtrip(k.float()).double(), 2.0
    else:
        raise ValueError(qmode)
    out = []
    for i0 in range(0, qs.shape[2], chunk):
        s = qs[:, :, i0:i0 + chunk] @ k.transpose(-1, -2) * math.log(base)
        out.append(torch.softmax(s, dim=-1) @ v)
    return torch.cat(out, dim=2).cpu()


def failures(case, got, qmode, device="cpu"):
    """every check of the case's family on an output [B * N, H * 64]; returns (list of (check, detail) that failed, info dict).  Magnitudes are
    taken per (batch, head) -- the leak of a row only reaches V of its own batch and head, and the soft bars' max(1, max|ref|) becomes
    max(2^vexp, max|ref| of the batch and head), the same thing at unit scale"""
    B, H, N, dt = case.B, case.H, case.N, case.dt_name
    shrink = SHRINK[qmode]
    got = got.detach().cpu().double().reshape(B, N, H, 64).transpose(1, 2)
    bad, info = [], {}
    if not torch.isfinite(got).all():
        bad.append(("finite", f"{(~torch.isfinite(got)).sum().item()} non-finite outputs"))
        got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
    v = case.heads(2)
    vmax = v.abs().amax(dim=(2, 3), keepdim=True)
    if case.family == "onehot":
        leak = case.leak(shrink)
        assert leak <= LEAK_MAX, f"one-hot precondition: leak {leak:.3e} (maxdot {case.maxdot}, N {N})"
        sel = ~case.trap
        exp = v[:, :, case.pi[sel]]
        g = got[:, :, sel]
        err = (g - exp).abs()
        over = err - (ulp_at(exp, dt) + leak * vmax)
        info["bit_equal"] = bool((g == exp).all())
        info["onehot_worst_ulps"] = (err / ulp_at(exp, dt)).max().item() if sel.any() else 0.0
        info["onehot_beyond_bar"] = int((over > 0).sum().item())
        if sel.any() and over.max().item() > 0:
            w = over.flatten().argmax().item()
            b_, h_, r_, d_ = (int(x) for x in torch.unravel_index(torch.tensor(w), over.shape))
            row = sel.nonzero().flatten()[r_].item()
            bad.append(("onehot_exact", f"{(over > 0).sum().item()} elements beyond one ulp + leak (largest |V| among them "
                                        f"{exp.abs()[over > 0].max().item():.3e}); worst at batch {b_} head {h_} query {row} "
                                        f"(key {case.pi[row].item()}) dim {d_}: got {g[b_, h_, r_, d_].item()!r} want {exp[b_, h_, r_, d_].item()!r}"))
        soft_rows = case.trap
    else:
        soft_rows = torch.ones(N, dtype=torch.bool)
    if soft_rows.any():
        if qmode not in case.refs:
            case.refs[qmode] = soft_reference(case, qmode, soft_rows, device)
        ref = case.refs[qmode]
        g = got[:, :, soft_rows]
        err = (g - ref).abs()
        scale = torch.maximum(torch.exp2(case.vexp.double())[:, :, None, None], ref.abs().amax(dim=(2, 3), keepdim=True))
        rel = err / scale
        tr = case.trap[soft_rows]
        for name, m in (("trap_rows", tr), ("sharp_rows", ~tr)):
            if not m.any():
                continue
            e = rel[:, :, m].max().item()
            info[name + "_err"] = e
            if e > SOFT_BARS[dt]:
                w = rel[:, :, m].amax(dim=(0, 1, 3)).argmax().item()
                row = soft_rows.nonzero().flatten()[m.nonzero().flatten()[w]].item()
                bad.append((name, f"max-abs {e:.3e} > {SOFT_BARS[dt]:.1e} of the batch-and-head scale; worst query {row}"))
    return bad, info
