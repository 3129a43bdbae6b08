"""The restatement of local attention in space and time (include/s2v_hip.h "Local attention in space and time"; csrc/attention.hip
attn_pp_item<ACCT, STEER, LOCAL, BOX> and attn_simple_box_k), shared by tests/test_attn_box_cpu.py, tests/test_gpu_attn_box.py and
tests/test_gpu_attn_box_engine.py.  Plain torch; no kernel is called here, and nothing of the package's own plan code is imported: the table
and the plan are stated again.

The definition, as the header states it.  For sample b, head h, query row i and key j:
    s_ij   = q_i . k_j / 8
    out_i  = sum_{j in vis(i)} softmax_{j in vis(i)}(s_ij) v_j
    vis(i) = [0, P)  union  { j : lo_i <= j < hi_i  and  olo_i <= (j - P) mod S < ohi_i }
with one P, one period S and one row table for every sample and head; 1 <= P <= Ntok, P <= lo_i <= hi_i <= Ntok, 0 <= olo_i <= ohi_i <= S,
64 <= S.

  1. BoxTable / box_table   P, S and the row table; .c() gives the ctypes arguments of the operator entry; the pipeline's family: a video row at
                            patch row y of frame f sees the patch rows [y - rows, y + rows] of the frames [f - frames, f + frames]
  2. visible                bool [N, N]
  3. visits / share         the plan: per 256-row work item the ascending list of key tiles it visits, from the table; brute_visits / brute_share
                            the same counted tile by tile from the visibility matrix
  4. box_reference          fp64 attention on the kernel's own rounding of the scaled q, -inf outside vis(i)
  5. emulate                the visit-list + whole-bit + per-lane-mask algorithm of attn_pp<BOX> on the CPU in fp32, with mutations
"""
import ctypes
import math

import torch

import attn_local_ref as LR
import attn_steer_ref as SR
from oracle import attn_cases as AC

KTILE, QBLOCK, WAVE = LR.KTILE, LR.QBLOCK, LR.WAVE
EMU_BAR = LR.EMU_BAR
rel_l2 = LR.rel_l2
MUTATIONS = ("offset_edge_off_by_one", "no_wrap_in_tile", "whole_ignores_offsets", "frame_window_ignored", "prefix_ignored", "ring_by_tile",
             "mask_after_sum")


# ------------------------------------------------------------------------------------------------ 1. the table
class BoxTable:
    def __init__(self, P, S, lo, hi, olo, ohi):
        self.P, self.S = int(P), int(S)
        self.lo, self.hi, self.olo, self.ohi = ([int(x) for x in a] for a in (lo, hi, olo, ohi))

    @property
    def N(self):
        return len(self.lo)

    def key(self):
        return ("box", self.P, self.S, tuple(self.lo), tuple(self.hi), tuple(self.olo), tuple(self.ohi))

    def c(self):
        n = max(1, self.N)
        arr = lambda a: (ctypes.c_int32 * n)(*a)   # noqa: E731
        return ctypes.c_int32(self.P), ctypes.c_int32(self.S), arr(self.lo), arr(self.hi), arr(self.olo), arr(self.ohi)

    def temporal(self):
        """the window table of the same (lo, hi): the offsets dropped"""
        return LR.Table(self.P, self.lo, self.hi)

    def windowed_rows(self):
        """bool [N]: the rows that do not see every key"""
        return ~visible(self).all(dim=1)

    def narrowed_rows(self):
        """bool [N]: the rows that see fewer keys than the window table of the same (lo, hi) shows them"""
        return (visible(self) != LR.visible(self.temporal())).any(dim=1)


def box_table(T, R, F, Hp, Wp, frames, rows):
    P, S = T + R, Hp * Wp
    n = P + F * S
    lo, hi, olo, ohi = [P] * P, [n] * P, [0] * P, [S] * P
    for f in range(F):
        for y in range(Hp):
            lo += [P + max(0, f - frames) * S] * Wp
            hi += [P + min(F, f + frames + 1) * S] * Wp
            olo += [max(0, y - rows) * Wp] * Wp
            ohi += [min(Hp, y + rows + 1) * Wp] * Wp
    return BoxTable(P, S, lo, hi, olo, ohi)


def from_local(tab, S):
    """a window table as a box table: full offsets on every row"""
    return BoxTable(tab.P, S, tab.lo, tab.hi, [0] * tab.N, [S] * tab.N)


# ------------------------------------------------------------------------------------------------ 2. visibility
def visible(tab):
    j = torch.arange(tab.N)[None]
    lo, hi, olo, ohi = (torch.tensor(a)[:, None] for a in (tab.lo, tab.hi, tab.olo, tab.ohi))
    o = (j - tab.P) % tab.S   # python's sign: non-negative
    return (j < tab.P) | ((j >= lo) & (j < hi) & (o >= olo) & (o < ohi))


# ------------------------------------------------------------------------------------------------ 3. the plan
def visits(tab):
    """the tile list of every item, in loop order, from the TABLE: the prefix tiles, then ascending every tile that holds a key of a row's box --
    per frame base = P + f S the keys [max(base + olo, lo), min(base + ohi, hi))"""
    npre = -(-tab.P // KTILE)
    out = []
    for q0 in range(0, tab.N, QBLOCK):
        tiles = set(range(npre))
        for i in range(q0, min(q0 + QBLOCK, tab.N)):
            lo, hi, olo, ohi = tab.lo[i], tab.hi[i], tab.olo[i], tab.ohi[i]
            if lo >= hi or olo >= ohi:
                continue
            for f in range((lo - tab.P) // tab.S, (hi - 1 - tab.P) // tab.S + 1):
                a, b = max(tab.P + f * tab.S + olo, lo), min(tab.P + f * tab.S + ohi, hi)
                if a < b:
                    tiles |= set(range(a // KTILE, (b - 1) // KTILE + 1))
        out.append(sorted(tiles))
    return out


def share(tab):
    v = visits(tab)
    return sum(len(x) for x in v) / (len(v) * -(-tab.N // KTILE))


def brute_visits(tab):
    """counted tile by tile from the visibility matrix"""
    vis = visible(tab)
    nt, npre = -(-tab.N // KTILE), -(-tab.P // KTILE)
    return [[t for t in range(nt) if t < npre or bool(vis[q0:q0 + QBLOCK, t * KTILE:(t + 1) * KTILE].any())] for q0 in range(0, tab.N, QBLOCK)]


def brute_share(tab):
    v = brute_visits(tab)
    return sum(len(x) for x in v) / (len(v) * -(-tab.N // KTILE))


# ------------------------------------------------------------------------------------------------ 4. the fp64 restatement
def box_reference(case, qmode, tab, device="cpu", chunk=1024):
    """fp64 [B * N, H * 64]"""
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


# ------------------------------------------------------------------------------------------------ 5. the algorithm
def emulate(case, qmode, tab, mutation=None):
    """attn_pp<BOX>'s algorithm in fp32 on the CPU.  Per 256-row item: the visit list; iteration j reads tile visits[j] from the buffer as it lies in
    memory (slack rows included).  Per 32-row wave and tile: whole (the host's bit: every key of the tile below N is seen by every row of the wave)
    -> untouched; else -inf unless kv < P, or kv - lo < len and o - olo < olen (unsigned), o = the tile's first offset (64 t - P) mod S plus the
    key's position, less S once where it passes S; then the tail mask's -inf; then an online softmax in base 2.  -> fp32 [B * N, H * 64]"""
    assert mutation is None or mutation in MUTATIONS
    B, H, N, D = case.B, case.H, case.N, case.D
    assert tab.N == N
    buf = case.qkv.float()
    rows_total = buf.shape[0]
    out = torch.zeros(B * N, D)
    P, S = tab.P, tab.S
    lo_all, hi_all, olo_all, ohi_all = (torch.tensor(a) for a in (tab.lo, tab.hi, tab.olo, tab.ohi))
    vis_all = LR.visible(tab.temporal()) if mutation == "whole_ignores_offsets" else visible(tab)
    vlist = visits(tab)
    npre = -(-P // KTILE)
    for b in range(B):
        for h in range(H):
            for qb, tiles in enumerate(vlist):
                r0, r1 = qb * QBLOCK, min((qb + 1) * QBLOCK, N)
                n = r1 - r0
                qs = (buf[b * N + r0:b * N + r1, h * 64:(h + 1) * 64] * AC.C0).to(AC.STORE[qmode]).float()
                lo, hi, olo, ohi = lo_all[r0:r1], hi_all[r0:r1], olo_all[r0:r1], ohi_all[r0:r1]
                wave = torch.arange(n) // WAVE
                m_run = torch.full((n,), -math.inf)
                l_run = torch.zeros(n)
                o = torch.zeros(n, 64)
                for j, t in enumerate(tiles):
                    kv0 = t * KTILE
                    idx = torch.arange(kv0, kv0 + KTILE)
                    src = idx if not (mutation == "ring_by_tile" and j >= npre) else torch.arange(j * KTILE, (j + 1) * KTILE)
                    rows = (b * N + src).clamp_max(rows_total - 1)
                    s = qs @ buf[rows, D + h * 64:D + (h + 1) * 64].T
                    kend = min(kv0 + KTILE, N)
                    row_whole = vis_all[r0:r1, kv0:kend].all(dim=1)
                    whole = torch.stack([row_whole[wave == w].all() for w in range(int(wave.max()) + 1)])[wave]
                    off = (kv0 - P) % S + torch.arange(KTILE)
                    if mutation != "no_wrap_in_tile":
                        off = torch.where(off >= S, off - S, off)
                    mohi = ohi + 1 if mutation == "offset_edge_off_by_one" else ohi
                    inbox = (off[None] >= olo[:, None]) & (off[None] < mohi[:, None])
                    if mutation != "frame_window_ignored":
                        inbox = inbox & (idx[None] >= lo[:, None]) & (idx[None] < hi[:, None])
                    see = inbox if mutation == "prefix_ignored" else (idx[None] < P) | inbox
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


# ------------------------------------------------------------------------------------------------ the cases the CPU and GPU tests share
# B = 2, H = 2, P = 20, S = 150 (10 patch rows of 15 cells), F = 5: Ntok = 770 is 13 key tiles with a ragged last one of 2 keys and 4 work items
# with a ragged last one of 2 rows; every frame boundary (170, 320, 470, 620) falls inside a tile
T_, R_, HP_, WP_, F_ = 5, 15, 10, 15, 5
S_ = HP_ * WP_
P0, N0, SHAPE = LR.P0, LR.N0, LR.SHAPE
assert (P0, N0, S_) == (T_ + R_, T_ + R_ + F_ * S_, LR.S_)


def _hand(P, fn, dense_below=None):
    """fn(i) -> (lo, hi, olo, ohi) for the rows at and past dense_below (default P); the rows before it are dense"""
    d = P if dense_below is None else dense_below
    return BoxTable(P, S_, *zip(*[fn(i) if i >= d else (P, N0, 0, S_) for i in range(N0)]))


def _own_frame(P):
    def fn(i):
        f, off = (i - P) // S_, (i - P) % S_
        return P + f * S_, min(N0, P + (f + 1) * S_), max(0, off - 20), min(S_, off + 20)
    return fn


def tables():
    """name -> BoxTable on N0 rows"""
    f1r1 = box_table(T_, R_, F_, HP_, WP_, 1, 1)
    own = _own_frame(P0)
    return {
        "f1r1": f1r1,
        "f0r0": box_table(T_, R_, F_, HP_, WP_, 0, 0),
        "f1r3": box_table(T_, R_, F_, HP_, WP_, 1, 3),
        "allframes_r1": box_table(T_, R_, F_, HP_, WP_, F_, 1),                                  # one run per frame
        "offsets_inside_one_tile": _hand(P0, lambda i: (P0, P0 + S_, 70, 100)),                   # the keys [90, 120): both edges inside tile 1
        "empty_boxes": _hand(P0, lambda i: (own(i)[0], own(i)[1], 40, 40) if i % 3 == 1 else (400, 400, 0, S_) if i % 3 == 2 else own(i)),
        "hidden_end_seen_start": _hand(P0, lambda i: (P0, N0, 0, 60)),      # tile 2 = [128, 192): offsets 108 .. 149 of frame 0 hidden, 0 .. 21 of frame 1 seen
        "ohi_is_S": _hand(P0, lambda i: (P0, N0, 100, S_)),
        "P1": _hand(1, _own_frame(1), dense_below=P0),
        "P64": _hand(64, _own_frame(64)),
        "P100": _hand(100, _own_frame(100)),
        "ends_in_ragged_tile": _hand(P0, lambda i: (700, 769, 90, 149)),                          # the keys [710, 769): one key short of N
        "dense_wave_then_f1r1": BoxTable(P0, S_, *[[d if i < 32 else x for i, x in enumerate(a)]
                                                   for a, d in ((f1r1.lo, P0), (f1r1.hi, N0), (f1r1.olo, 0), (f1r1.ohi, S_))]),
    }


def case(family, dt_name="bf16", shape=SHAPE):
    return LR.case(family, dt_name, shape)


def around_own_key(c, radius=20):
    """a box on the case's rows that holds the row's own key pi(i): the frame of pi(i) and the offsets within `radius` of its own; a row whose own
    key lies in the prefix gets an empty box"""
    rows = []
    for i in range(c.N):
        j = int(c.pi[i])
        if j < P0:
            rows.append((P0, P0, 0, 0))
        else:
            f, off = (j - P0) // S_, (j - P0) % S_
            rows.append((P0 + f * S_, min(c.N, P0 + (f + 1) * S_), max(0, off - radius), min(S_, off + radius + 1)))
    return BoxTable(P0, S_, *zip(*rows))


def bad_tables():
    """(BoxTable, the message it is refused with) on the shared shape"""
    N, P, S = N0, P0, S_
    ok = box_table(T_, R_, F_, HP_, WP_, 1, 1)

    def with_row(i, a, b, oa=None, ob=None):
        lo, hi, olo, ohi = list(ok.lo), list(ok.hi), list(ok.olo), list(ok.ohi)
        lo[i], hi[i] = a, b
        if oa is not None:
            olo[i], ohi[i] = oa, ob
        return BoxTable(P, S, lo, hi, olo, ohi)

    return [
        (BoxTable(0, S, ok.lo, ok.hi, ok.olo, ok.ohi), rf"the prefix P = 0 must lie inside \[1, Ntok = {N}\] \(key 0 is visible to every row\)"),
        (BoxTable(N + 1, S, ok.lo, ok.hi, ok.olo, ok.ohi), rf"the prefix P = {N + 1} must lie inside \[1, Ntok = {N}\]"),
        (BoxTable(P, 63, ok.lo, ok.hi, [0] * N, [63] * N), r"the period S = 63 must be at least 64"),
        (with_row(100, P - 1, 200), rf"row 100 has the window \[{P - 1}, 200\): P = {P} <= lo <= hi <= Ntok = {N} is required"),
        (with_row(769, 300, N + 1), rf"row 769 has the window \[300, {N + 1}\)"),
        (with_row(0, 400, 399), r"row 0 has the window \[400, 399\)"),
        (with_row(5, 30, 40, -1, 10), rf"row 5 has the offsets \[-1, 10\): 0 <= olo <= ohi <= S = {S} is required"),
        (with_row(300, 30, 40, 10, S + 1), rf"row 300 has the offsets \[10, {S + 1}\)"),
        (with_row(768, 30, 40, 50, 49), r"row 768 has the offsets \[50, 49\)"),
    ]
