"""The restatement of local attention in time (include/s2v_hip.h "Local attention"; csrc/attention.hip attn_pp_item<ACCT, STEER, LOCAL> and
attn_simple_local_k), shared by tests/test_attn_local_cpu.py, tests/test_gpu_attn_local.py and tests/test_gpu_attn_local_engine.py.  Plain
torch; no kernel is called here, and nothing of the package's own plan code is imported: the table and the plan are stated again.

The definition, as the header states it.  For sample b, head h, query row i and key j:
    s_ij   = q_i . k_j / 8
    out_i  = sum_{j in vis(i)} softmax_{j in vis(i)}(s_ij) v_j
    vis(i) = [0, P)  union  [lo_i, hi_i)
with one P and one row table for every sample and head, 1 <= P <= Ntok, P <= lo_i <= hi_i <= Ntok.

  Table             P and the row table; .c() gives the ctypes arguments of the operator entry
  frames_table      the pipeline's family: rows below P dense, a video row of latent frame f sees frames [f - w, f + w]
  items / share     the plan: per 256-row work item the key tiles [0, np) and [w0, w1) it visits; the visited share of the dense launch's tiles
  brute_share       the same share counted tile by tile from the visibility matrix
  visible           bool [N, N]
  local_reference   fp64 attention on the kernel's own rounding of the scaled q, -inf outside vis(i)  (table None: the dense restatement)
  emulate           the visit-list + wave-classification + per-lane-mask algorithm of attn_pp<LOCAL> on the CPU in fp32, with mutations
  local_forward     oracle.transformer_ref.transformer_forward with vis passed to scaled_dot_product_attention as a boolean attn_mask on the
                    listed call indices: the windowed CPU oracle
"""
import ctypes
import math

import torch

import attn_steer_ref as SR
from oracle import attn_cases as AC
from oracle import transformer_ref as TR

KTILE, QBLOCK, WAVE = 64, 256, 32
EMU_BAR = SR.EMU_BAR
rel_l2 = SR.rel_l2
MUTATIONS = ("edge_off_by_one", "prefix_ignored", "wave_envelope_on_edge", "straddle_as_interior", "ring_by_tile", "mask_after_sum")


class Table:
    def __init__(self, P, lo, hi):
        self.P, self.lo, self.hi = int(P), [int(x) for x in lo], [int(x) for x in hi]

    @property
    def N(self):
        return len(self.lo)

    def key(self):
        return (self.P, tuple(self.lo), tuple(self.hi))

    def c(self):
        n = max(1, self.N)
        return ctypes.c_int32(self.P), (ctypes.c_int32 * n)(*self.lo), (ctypes.c_int32 * n)(*self.hi)

    def windowed_rows(self):
        """bool [N]: the rows that do not see every key"""
        return torch.tensor([not (a <= self.P and b >= self.N) for a, b in zip(self.lo, self.hi)])


def frames_table(T, R, F, S, frames):
    P = T + R
    n = P + F * S
    lo, hi = [P] * P, [n] * P
    for f in range(F):
        lo += [P + max(0, f - frames) * S] * S
        hi += [P + min(F, f + frames + 1) * S] * S
    return Table(P, lo, hi)


def dense_table(N, P=1):
    return Table(P, [P] * N, [N] * N)


def items(tab):
    """[(np, w0, w1)] per 256-row work item: prefix tiles [0, np), envelope tiles [w0, w1); one run (w0 = w1 = np) where they touch or overlap"""
    npre = -(-tab.P // KTILE)
    out = []
    for q0 in range(0, tab.N, QBLOCK):
        win = [(a, b) for a, b in zip(tab.lo[q0:q0 + QBLOCK], tab.hi[q0:q0 + QBLOCK]) if a < b]
        n_p, w0, w1 = npre, npre, npre
        if win:
            w0, w1 = min(a for a, _ in win) // KTILE, -(-max(b for _, b in win) // KTILE)
            if w0 <= n_p:
                n_p = max(n_p, w1)
                w0 = w1 = n_p
        out.append((n_p, w0, w1))
    return out


def visits(tab):
    """the tile list of every item, in loop order"""
    return [list(range(n_p)) + list(range(w0, w1)) for n_p, w0, w1 in items(tab)]


def share(tab):
    v = visits(tab)
    return sum(len(x) for x in v) / (len(v) * -(-tab.N // KTILE))


def visible(tab):
    j = torch.arange(tab.N)[None]
    lo, hi = torch.tensor(tab.lo)[:, None], torch.tensor(tab.hi)[:, None]
    return (j < tab.P) | ((j >= lo) & (j < hi))


def brute_share(tab):
    """counted tile by tile from the visibility matrix: an item visits the prefix tiles and the hull of the tiles in which some row of it sees a
    key past the prefix"""
    vis = visible(tab)
    nt = -(-tab.N // KTILE)
    total = 0
    for q0 in range(0, tab.N, QBLOCK):
        win = [t for t in range(nt) if bool(vis[q0:q0 + QBLOCK, max(t * KTILE, tab.P):(t + 1) * KTILE].any())]
        need = set(range(-(-tab.P // KTILE)))
        if win:
            need |= set(range(win[0], win[-1] + 1))
        total += len(need)
    return total / (-(-tab.N // QBLOCK) * nt)


def local_reference(case, qmode, tab=None, device="cpu", chunk=1024):
    """fp64 [B * N, H * 64]; tab None: the dense restatement (attn_steer_ref.steered_reference without a record)"""
    if tab is None:
        return SR.steered_reference(case, qmode, None, device, chunk)
    q, k, v = (case.heads(p).to(device) for p in range(3))
    qs, base = SR.scaled_q(q, qmode)
    B, H, N = case.B, case.H, case.N
    vis = visible(tab).to(device)
    out = torch.empty(B, H, N, 64, dtype=torch.float64, device=device)
    for i0 in range(0, N, chunk):
        s = qs[:, :, i0:i0 + chunk] @ k.transpose(-1, -2) * math.log(base)
        s = s.masked_fill(~vis[None, None, i0:i0 + chunk], -math.inf)
        out[:, :, i0:i0 + chunk] = torch.softmax(s, dim=-1) @ v
    return out.transpose(1, 2).reshape(B * N, H * 64).cpu()


def emulate(case, qmode, tab, mutation=None):
    """attn_pp<LOCAL>'s algorithm in fp32 on the CPU.  Per 256-row item: the visit list; iteration j reads tile visits[j] from the buffer as it lies
    in memory (slack rows included).  Per 32-row wave and tile: whole (every key below N seen by every row of the wave: inside the prefix, or
    inside [lo_max, hi_min), reaching down through the prefix when lo_max == P) -> untouched; else -inf where the LANE's own row does not see the
    key; then the tail mask's -inf; then an online softmax in base 2.  -> fp32 [B * N, H * 64].  mutation: one of MUTATIONS"""
    assert mutation is None or mutation in MUTATIONS
    B, H, N, D = case.B, case.H, case.N, case.D
    assert tab.N == N
    buf = case.qkv.float()
    rows_total = buf.shape[0]
    out = torch.zeros(B * N, D)
    P = tab.P
    lo_all, hi_all = torch.tensor(tab.lo), torch.tensor(tab.hi)
    vlist = visits(tab)
    for b in range(B):
        for h in range(H):
            for qb, tiles in enumerate(vlist):
                r0, r1 = qb * QBLOCK, min((qb + 1) * QBLOCK, N)
                n = r1 - r0
                qs = (buf[b * N + r0:b * N + r1, h * 64:(h + 1) * 64] * AC.C0).to(AC.STORE[qmode]).float()
                lo, hi = lo_all[r0:r1], hi_all[r0:r1]
                wave = torch.arange(n) // WAVE
                nw = int(wave.max()) + 1
                lo_max = torch.stack([lo[wave == w].max() for w in range(nw)])[wave]
                hi_min = torch.stack([hi[wave == w].min() for w in range(nw)])[wave]
                lo_min = torch.stack([lo[wave == w].min() for w in range(nw)])[wave]
                hi_max = torch.stack([hi[wave == w].max() for w in range(nw)])[wave]
                m_run = torch.full((n,), -math.inf)
                l_run = torch.zeros(n)
                o = torch.zeros(n, 64)
                n_p = items(tab)[qb][0]
                for j, t in enumerate(tiles):
                    kv0 = t * KTILE
                    idx = torch.arange(kv0, kv0 + KTILE)
                    src = idx if not (mutation == "ring_by_tile" and j >= n_p) else torch.arange(j * KTILE, (j + 1) * KTILE)
                    rows = (b * N + src).clamp_max(rows_total - 1)
                    s = qs @ buf[rows, D + h * 64:D + (h + 1) * 64].T
                    kend = min(kv0 + KTILE, N)
                    whole = (kend <= P) | ((kend <= hi_min) & ((kv0 >= lo_max) | (lo_max <= P)))
                    if mutation == "straddle_as_interior":
                        whole = torch.ones_like(whole)
                    mlo, mhi = (lo_min, hi_max) if mutation == "wave_envelope_on_edge" else (lo, hi)
                    if mutation == "edge_off_by_one":
                        mhi = mhi + 1
                    inwin = (idx[None] >= mlo[:, None]) & (idx[None] < mhi[:, None])
                    see = inwin if mutation == "prefix_ignored" else (idx[None] < P) | inwin
                    valid = (idx < N)[None]
                    keep = (whole[:, None] | see) & valid
                    sm = torch.where(keep, s, torch.full_like(s, -math.inf))
                    mn = torch.maximum(m_run, sm.max(dim=1).values)
                    alpha = torch.exp2(m_run - mn)
                    p = torch.exp2(sm - mn[:, None])
                    if mutation == "mask_after_sum":   # the row sum sees the un-masked scores, P.V the masked ones
                        l_run = l_run * alpha + torch.exp2(torch.where(valid, s, torch.full_like(s, -math.inf)) - mn[:, None]).sum(dim=1)
                    else:
                        l_run = l_run * alpha + p.sum(dim=1)
                    o = o * alpha[:, None] + p @ buf[rows, 2 * D + h * 64:2 * D + (h + 1) * 64]
                    m_run = mn
                out[b * N + r0:b * N + r1, h * 64:(h + 1) * 64] = o / l_run[:, None]
    return out


class _LocalF:
    """stands in for torch.nn.functional inside oracle.transformer_ref: on the listed call indices (block l is call l of a forward) vis goes to
    scaled_dot_product_attention as a boolean attn_mask (True: the key takes part); everything else, that call included, is delegated"""

    def __init__(self, real, layers, vis):
        self._real, self._layers, self._vis, self.calls = real, set(layers), vis, 0

    def __getattr__(self, name):
        return getattr(self._real, name)

    def scaled_dot_product_attention(self, q, k, v, *a, **kw):
        i, self.calls = self.calls, self.calls + 1
        if i in self._layers:
            assert not a and kw.get("attn_mask") is None, "the oracle's attention has no mask of its own"
            kw = dict(kw, attn_mask=self._vis[None, None])   # [1, 1, N, N], broadcast over samples and heads
        return self._real.scaled_dot_product_attention(q, k, v, *a, **kw)


def local_forward(layers, tab, *args, **kw):
    """transformer_forward(*args, **kw) with the blocks `layers` windowed by tab (an empty list: the plain oracle)"""
    real = TR.F
    TR.F = _LocalF(real, layers, visible(tab))
    try:
        with torch.no_grad():
            return TR.transformer_forward(*args, **kw)
    finally:
        TR.F = real


# ------------------------------------------------------------------------------------------------ the cases the CPU and GPU tests share
# B = 2, H = 2, P = 20, S = 150, F = 5: Ntok = 770 is 13 key tiles with a ragged last one of 2 keys and 4 work items with a ragged last one of 2
# rows -- the smallest shape that reaches every path: a gap after the prefix, skipped tail tiles, a prefix edge and window edges inside tiles
T_, R_, S_, F_ = 5, 15, 150, 5
P0 = T_ + R_
N0 = P0 + F_ * S_
SHAPE = (2, 2, N0)
VISITS_FRAMES0 = [list(range(13)), [0] + list(range(2, 10)), [0] + list(range(7, 13)), [0] + list(range(9, 13))]


def _hand(P, fn):
    lo, hi = zip(*[fn(i) if i >= P else (P, N0) for i in range(N0)])
    return Table(P, lo, hi)


def tables():
    """name -> Table on N0 rows"""
    f0 = frames_table(T_, R_, F_, S_, 0)
    return {
        "frames0": f0,
        "frames1": frames_table(T_, R_, F_, S_, 1),
        "empty_windows": _hand(P0, lambda i: (400, 400) if i % 3 else (P0 + (i - P0) // S_ * S_, P0 + ((i - P0) // S_ + 1) * S_)),   # prefix-only rows
        "inside_one_tile": _hand(P0, lambda i: (200, 230)),                                      # both edges inside tile 3
        "lo_is_P": _hand(P0, lambda i: (P0, min(N0, i + 1))),                                    # causal from the prefix on
        "P1": Table(1, [max(1, f0.lo[i]) if i >= P0 else 1 for i in range(N0)], [f0.hi[i] for i in range(N0)]),
        "P64": Table(64, [max(64, f0.lo[i]) if i >= 64 else 64 for i in range(N0)], [max(64, f0.hi[i]) if i >= 64 else N0 for i in range(N0)]),
        "P100": Table(100, [max(100, f0.lo[i]) if i >= 100 else 100 for i in range(N0)], [max(100, f0.hi[i]) if i >= 100 else N0 for i in range(N0)]),
        "ends_in_ragged_tile": _hand(P0, lambda i: (700, 769)),                                  # hi inside the last tile, one key short of N
        "dense_wave_then_frames0": Table(P0, [P0 if i < 32 else f0.lo[i] for i in range(N0)], [N0 if i < 32 else f0.hi[i] for i in range(N0)]),
    }


def randn_case(dt_name, B, H, N, seed=5):
    """attn_steer_ref.randn_case: q, k, v ~ N(0, 1); the slack rows carry keys x 8 and V = TRAP_V -- finite, because 0 * NaN on the matrix pipe is
    NaN in a visited tile"""
    return SR.randn_case(dt_name, B, H, N, seed)


_CASES = {}


def case(family, dt_name="bf16", shape=SHAPE):
    key = (family, dt_name, shape)
    if key not in _CASES:
        _CASES[key] = randn_case(dt_name, *shape) if family == "randn" else AC.build(family, "random", dt_name, *shape)
    return _CASES[key]


def around_own_key(c, radius=40):
    """a table on the case's rows whose every window holds the row's own key pi(i): [pi - radius, pi + radius) clipped to [P0, N); a row whose own
    key lies in the prefix gets an empty window"""
    N = c.N
    lo, hi = [], []
    for i in range(N):
        j = int(c.pi[i])
        if j < P0:
            lo.append(P0), hi.append(P0)
        else:
            lo.append(max(P0, j - radius)), hi.append(min(N, j + radius))
    return Table(P0, lo, hi)


def bad_tables(N=None, P=None):
    """(Table, the message it is refused with) on the shared shape"""
    N, P = N or N0, P or P0
    ok = frames_table(T_, R_, F_, S_, 0)

    def with_row(i, a, b, P=ok.P):
        lo, hi = list(ok.lo), list(ok.hi)
        lo[i], hi[i] = a, b
        return Table(P, lo, hi)

    return [
        (Table(0, ok.lo, ok.hi), rf"the prefix P = 0 must lie inside \[1, Ntok = {N}\] \(key 0 is visible to every row\)"),
        (Table(N + 1, ok.lo, ok.hi), rf"the prefix P = {N + 1} must lie inside \[1, Ntok = {N}\]"),
        (with_row(100, P - 1, 200), rf"row 100 has the window \[{P - 1}, 200\): P = {P} <= lo <= hi <= Ntok = {N} is required"),
        (with_row(769, 300, N + 1), rf"row 769 has the window \[300, {N + 1}\)"),
        (with_row(0, 400, 399), r"row 0 has the window \[400, 399\)"),
        (with_row(5, -3, 30), r"row 5 has the window \[-3, 30\)"),
    ]
