"""The restatement of attention steering (include/s2v_hip.h "Attention steering"; csrc/attention.hip attn_pp_item<ACCT, STEER> and
attn_simple_steer_k), shared by tests/test_attn_steer_cpu.py, tests/test_gpu_attn_steer.py and tests/test_gpu_attn_steer_engine.py.  Plain
torch; no kernel is called here.

The definition, as the header states it.  For sample b, head h, query row i and key j:
    s_ij  = q_i . k_j / 8
    out_i = sum_j softmax_j(s_ij + beta_b(i, j)) v_j
    beta_b(i, j) = ln w_r  when j lies in key range r = [k0_r, k1_r), bit b of that range's sample mask is set and i lies in [q0, q1); else 0.

  Record            the ranges and the query range; .c() is the operator entry's ctypes record
  beta              fp64 [B, N, N] of a record (natural logarithm)
  steered_reference fp64 attention on the kernel's own rounding of the scaled q (the qmodes of oracle.attn_cases.soft_reference)
  emulate           the tile-classified algorithm of attn_pp<STEER> on the CPU in fp32, with the mutations the checks must catch
  steered_forward   oracle.transformer_ref.transformer_forward with the bias passed to scaled_dot_product_attention as an additive float
                    attn_mask on the listed call indices: the steered fp32 CPU oracle
"""
import math

import torch

from oracle import attn_cases as AC
from oracle import transformer_ref as TR

KTILE = 64
# the fp32 emulation against fp64: exp2 of an fp32 score at |s| <= 256 carries <= 2^-16 ln 2 = 1.1e-5 relative, the sums and the division add
# a few 2^-23: 5e-5 of max(1, max|ref|) leaves a factor of four
EMU_BAR = 5e-5
# "the bias added after the tail mask or after the maximum" is not among them as worded: after the tail mask -inf + b is -inf, and a maximum taken
# from the un-biased scores only shifts every exponent of a row by the same amount -- softmax is invariant to it and p stays below 2^(64 + 16),
# far inside fp32 and bf16 -- so neither changes a result and no check can catch it.  What an order mistake CAN break is a row sum that does
# not see the bias ("bias_after_sum": P.V biased, the sum not).
MUTATIONS = ("edge_off_by_one", "bias_outside_query", "span_on_every_sample", "natural_log", "bias_after_sum", "straddle_as_interior")


class Record:
    """ranges: [(k0, k1, w, sample_mask)], ascending and disjoint; the query rows [q0, q1)"""

    def __init__(self, ranges, q0, q1):
        self.ranges = [(int(k0), int(k1), float(w), int(m)) for k0, k1, w, m in ranges]
        self.q0, self.q1 = int(q0), int(q1)

    def c(self, lib_mod):
        r = lib_mod.SteerRecordC()
        r.n, r.q0, r.q1 = len(self.ranges), self.q0, self.q1
        for i, (k0, k1, w, m) in enumerate(self.ranges[:4]):
            r.k0[i], r.k1[i], r.w[i], r.sample_mask[i] = k0, k1, w, m & 0xFFFFFFFF
        return r

    def steered_rows(self, B, N):
        """bool [B, N]: the rows some range applies to"""
        out = torch.zeros(B, N, dtype=torch.bool)
        for b in range(B):
            if any((m >> b) & 1 and w != 1.0 for _, _, w, m in self.ranges):
                out[b, self.q0:self.q1] = True
        return out


def beta(rec, B, N, log=math.log):
    """fp64 [B, N(query), N(key)]"""
    out = torch.zeros(B, N, N, dtype=torch.float64)
    for b in range(B):
        for k0, k1, w, m in rec.ranges:
            if (m >> b) & 1:
                out[b, rec.q0:rec.q1, k0:k1] = log(w)
    return out


def scaled_q(q, qmode):
    """the kernel's rounding of the scaled q as fp64, and the base of its exponential (oracle.attn_cases.soft_reference)"""
    if qmode == "natural":
        return q * 0.125, math.e
    return (q.float() * AC.C0).to(AC.STORE[qmode]).double(), 2.0


def steered_reference(case, qmode, rec=None, device="cpu", chunk=1024):
    """fp64 [B * N, H * 64]: softmax over each sample's real keys of the scores on the kernel's own rounding of the scaled q, plus beta.
    rec None: the un-steered restatement"""
    q, k, v = (case.heads(p).to(device) for p in range(3))
    qs, base = scaled_q(q, qmode)
    B, H, N = case.B, case.H, case.N
    bt = None if rec is None else beta(rec, B, N).to(device)
    out = torch.empty(B, H, N, 64, dtype=torch.float64, device=device)
    for i0 in range(0, N, chunk):
        s = qs[:, :, i0:i0 + chunk] @ k.transpose(-1, -2) * math.log(base)
        if bt is not None:
            s = s + bt[:, None, i0:i0 + chunk]
        out[:, :, i0:i0 + chunk] = torch.softmax(s, dim=-1) @ v
    return out.transpose(1, 2).reshape(B * N, H * 64).cpu()


def rel_l2(got, ref, rows=None):
    """||got - ref|| / ||ref|| over the rows (bool [B * N]) -- the scale-free figure: every rounding of the kernels (P to bf16, the output to
    the storage type) is relative to the magnitude it rounds, so a softmax that moves its weight onto fewer keys moves max-abs with max|out|
    and leaves this figure where it is"""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    if rows is not None:
        g, r = g[rows], r[rows]
    return ((g - r).norm() / r.norm()).item()


def emulate(case, qmode, rec, mutation=None):
    """attn_pp<STEER>'s algorithm in fp32 on the CPU: q * scale * log2 e rounded to the storage type; tiles of 64 keys read from the buffer as
    it lies in memory (slack rows included); every tile classified against the ranges that apply to the sample -- outside every range: untouched;
    wholly inside one: one add per score; an edge inside: compares on the key index; the addend is log2 w on the rows of [q0, q1) and 0 on the
    others; then the tail mask's -inf, then an online softmax in base 2.  -> fp32 [B * N, H * 64].  mutation: one of MUTATIONS"""
    assert mutation is None or mutation in MUTATIONS
    B, H, N, D = case.B, case.H, case.N, case.D
    buf = case.qkv.float()
    rows_total = buf.shape[0]
    out = torch.zeros(B * N, D)
    log = math.log if mutation == "natural_log" else math.log2
    qi = torch.arange(N)
    inq = torch.ones(N, dtype=torch.bool) if mutation == "bias_outside_query" else (qi >= rec.q0) & (qi < rec.q1)
    for b in range(B):
        live = [(k0, k1, w) for k0, k1, w, m in rec.ranges if mutation == "span_on_every_sample" or (m >> b) & 1]
        for h in range(H):
            qs = (buf[b * N:(b + 1) * N, h * 64:(h + 1) * 64] * AC.C0).to(AC.STORE[qmode]).float()
            m_run = torch.full((N,), -math.inf)
            l_run = torch.zeros(N)
            o = torch.zeros(N, 64)
            for t in range((N + KTILE - 1) // KTILE):
                kv0 = t * KTILE
                idx = torch.arange(kv0, kv0 + KTILE)
                rows = (b * N + idx).clamp_max(rows_total - 1)
                s = qs @ buf[rows, D + h * 64:D + (h + 1) * 64].T
                add = torch.zeros_like(s)
                for k0, k1, w in live:
                    lo, up = max(k0, kv0), min(k1, kv0 + KTILE)
                    if lo >= up:
                        continue   # outside: untouched
                    bl = torch.where(inq, torch.tensor(log(w), dtype=torch.float32), torch.tensor(0.0))[:, None]
                    if up - lo == KTILE or mutation == "straddle_as_interior":
                        add = add + bl   # interior: the whole tile
                    else:
                        upm = up + 1 if mutation == "edge_off_by_one" else up
                        add = add + bl * ((idx >= lo) & (idx < upm)).float()[None]
                sb = s + add
                valid = (idx < N)[None]
                sb = torch.where(valid, sb, torch.full_like(sb, -math.inf))
                mn = torch.maximum(m_run, sb.max(dim=1).values)
                alpha = torch.exp2(m_run - mn)
                p = torch.exp2(sb - mn[:, None])
                if mutation == "bias_after_sum":   # the row sum sees the un-biased scores, P.V the biased ones
                    l_run = l_run * alpha + torch.exp2(torch.where(valid, s, torch.full_like(s, -math.inf)) - mn[:, None]).sum(dim=1)
                else:
                    l_run = l_run * alpha + p.sum(dim=1)
                o = o * alpha[:, None] + p @ buf[rows, 2 * D + h * 64:2 * D + (h + 1) * 64]
                m_run = mn
            out[b * N:(b + 1) * N, h * 64:(h + 1) * 64] = o / l_run[:, None]
    return out


class _SteerF:
    """stands in for torch.nn.functional inside oracle.transformer_ref: on the listed call indices (block l is call l of a forward) the bias
    goes to scaled_dot_product_attention as an additive float attn_mask; everything else, that call included, is delegated"""

    def __init__(self, real, layers, bias):
        self._real, self._layers, self._bias, self.calls = real, set(layers), bias, 0

    def __getattr__(self, name):
        return getattr(self._real, name)

    def scaled_dot_product_attention(self, q, k, v, *a, **kw):
        i, self.calls = self.calls, self.calls + 1
        if i in self._layers:
            assert not a and kw.get("attn_mask") is None, "the oracle's attention has no mask of its own"
            kw = dict(kw, attn_mask=self._bias.to(q.dtype)[:, None])   # [B, 1, N, N], broadcast over the heads
        return self._real.scaled_dot_product_attention(q, k, v, *a, **kw)


def steered_forward(layers, rec, B, N, *args, **kw):
    """transformer_forward(*args, **kw) with the blocks `layers` steered by rec (an empty list: the un-steered oracle)"""
    real = TR.F
    TR.F = _SteerF(real, layers, beta(rec, B, N).float())
    try:
        with torch.no_grad():
            return TR.transformer_forward(*args, **kw)
    finally:
        TR.F = real


# ------------------------------------------------------------------------------------------------ the cases the CPU and GPU tests share
# Key tiles are 64 keys wide, a work item is 256 query rows (32 per wave): B = 2, H = 2, N = 330 is six key tiles with a ragged last one and two
# query blocks with a ragged last one -- the smallest shape that reaches every path of the tile classification
SHAPE = (2, 2, 330)
W_HI, W_LO = 2.0 ** 16, 2.0 ** -16
BOTH, S0, S1 = 0b11, 0b01, 0b10


def range_sets(N=330):
    """name -> Record.  The weights are the ends of the allowed interval (and 2^10): on randn inputs the steered answer is far from the
    un-steered one (rel-l2 >= 0.7 over the steered rows), so a kernel that ignores the bias cannot pass.  The sign-code families keep their
    dominant key under any allowed weight (one-hot margin >= 36 natural units, sharp ~ 20, ln 2^16 = 11.1): their steered answers stay within
    0.04 .. 0.19 of the un-steered ones, and they are held to the restatement by the project's own per-dtype bars instead"""
    return {
        "inside_one_tile": Record([(70, 100, W_HI, BOTH)], 0, N),                       # both edges inside tile 1
        "straddle_interior_straddle": Record([(60, 200, W_HI, BOTH)], 0, N),            # tiles 0 | 1, 2 | 3
        "tile_aligned": Record([(64, 128, W_HI, BOTH)], 0, N),                          # exactly tile 1
        "first_tile": Record([(0, 5, W_HI, BOTH)], 0, N),                               # the tile whose maximum is adopted at t == 0
        "bias_and_tail_mask": Record([(300, N, W_HI, BOTH)], 0, N),                     # tiles 4 (edge) and 5 (edge + the -inf of the pad keys)
        "four_ranges": Record([(0, 5, W_HI, S0), (70, 100, W_LO, BOTH), (128, 192, 2.0 ** 10, S1), (300, N, W_HI, BOTH)], 0, N),
        "query_range": Record([(60, 200, W_HI, BOTH)], 37, 300),                        # starts inside wave 1, ends inside block 1
        "one_sample": Record([(64, 200, W_HI, S0)], 0, N),                              # sample 1 is outside every mask
    }


def randn_case(dt_name, B, H, N, seed=5):
    """q, k, v ~ N(0, 1) in the storage type; the slack rows carry large keys and V = 1e4 no real row has: an unmasked tail shows"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N + 64, 3 * H * 64, generator=g)
    qkv[B * N:, H * 64:2 * H * 64] *= 8.0
    qkv[B * N:, 2 * H * 64:] = AC.TRAP_V
    qkv = qkv.to(AC.STORE[dt_name])
    return AC.AttnCase("randn", "none", dt_name, B, H, N, qkv, torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.bool), 0, 0.0,
                       torch.zeros(B, H))


def sharp2_case(dt_name, B, H, N):
    """oracle.attn_cases' sharp family with q doubled (exact in every storage type): a query scores 64 natural units = 92.3 in base 2 against its
    own key and at most ~60 against any other, so with w = 2^16 on the own key's range the row sum passes the deferred-maximum threshold of
    2^64 inside a biased tile for the rows whose first-tile maximum lies low enough -- and does not without the bias"""
    case = AC.build("sharp", "random", dt_name, B, H, N)
    qkv = case.qkv.clone()
    qkv[:, :case.D] *= 2
    return AC.AttnCase("sharp2", case.perm, dt_name, B, H, N, qkv, case.pi, case.trap, case.maxdot, 4 * case.margin, case.vexp)


_CASES = {}


def case(family, dt_name="bf16", shape=SHAPE):
    key = (family, dt_name, shape)
    if key not in _CASES:
        if family == "randn":
            _CASES[key] = randn_case(dt_name, *shape)
        elif family == "sharp2":
            _CASES[key] = sharp2_case(dt_name, *shape)
        else:
            _CASES[key] = AC.build(family, "random", dt_name, *shape)
    return _CASES[key]


def crossings(c, rec, qmode="bf16"):
    """(rows whose biased base-2 score minus their first tile's biased maximum exceeds 64 at a key of a range past tile 0, the same count
    without the bias): the rows on which the deferred maximum of attn_pp takes its slow path inside a biased tile"""
    qs, _ = scaled_q(c.heads(0), qmode)
    s = qs @ c.heads(1).transpose(-1, -2)
    sb = s + beta(rec, c.B, c.N, math.log2)[:, None]
    inr = torch.zeros(c.N, dtype=torch.bool)
    for k0, k1, _, _ in rec.ranges:
        inr[max(k0, KTILE):k1] = True
    over = lambda x: int(((x[..., inr].amax(dim=-1) - x[..., :KTILE].amax(dim=-1)) > 64.0).sum().item())
    return over(sb), over(s)
