"""The restatement of steering maps (include/s2v_hip.h "Steering maps"; csrc/attention.hip attn_pp_item<.., MAP> and attn_simple_steer_map_k), shared
by tests/test_attn_steer_map_cpu.py and tests/test_gpu_attn_steer_map.py.  Plain torch; no kernel is called here.

The definition, as the header states it.  For sample b, head h, query row i and key j:
    s_ij  = q_i . k_j / 8
    out_i = sum_j softmax_j(s_ij + beta_b(i, j)) v_j
    beta_b(i, j) = ln W_p[i - q0]  when j lies in key range r = [k0_r, k1_r), p = plane[r][b] >= 0 and q0 <= i < q1; else 0.

  MapRecord             the ranges with a plane index per sample, the planes and the query range; .c() is the operator entry's ctypes record
  beta_maps             fp64 [B, N, N] of a record (natural logarithm)
  map_reference         fp64 attention on the kernel's own rounding of the scaled q (attn_steer_ref.steered_reference with beta_maps)
  wave_flags_bruteforce the liveness table [8][8 nqb] by the definition, row by row
  emulate_maps          the tile-classified algorithm of attn_pp<MAP> on the CPU in fp32 -- per-lane addends, ranges skipped where the wave's liveness
                        bit is clear -- with the mutations the checks must catch
  mapped_forward        oracle.transformer_ref.transformer_forward with the bias as an additive attn_mask on the listed blocks
"""
import ctypes
import math

import torch

import attn_steer_ref as R
from oracle import attn_cases as AC
from oracle import transformer_ref as TR

KTILE = R.KTILE
MUTATIONS = ("other_sample_plane", "row_off_by_one", "plane_from_row_0", "live_from_first_row", "natural_log", "planes_swapped")


class MapRecord:
    """ranges: [(k0, k1, [plane of sample 0, plane of sample 1, ...])] ascending and disjoint (-1: the range does not apply to the sample; missing
    samples are -1); planes: fp32 [n_planes, q1 - q0]; the query rows [q0, q1)"""

    def __init__(self, ranges, planes, q0, q1):
        self.ranges = [(int(k0), int(k1), [int(p) for p in pl]) for k0, k1, pl in ranges]
        self.planes = torch.as_tensor(planes, dtype=torch.float32).reshape(-1, int(q1) - int(q0)).contiguous()
        self.q0, self.q1 = int(q0), int(q1)

    def plane(self, r, b):
        pl = self.ranges[r][2]
        return pl[b] if b < len(pl) else -1

    def key(self):
        return (tuple((k0, k1, tuple(pl)) for k0, k1, pl in self.ranges), self.q0, self.q1, self.planes.numpy().tobytes())

    def c(self, lib_mod, n_planes=None):
        """(record, planes pointer, the array the pointer reads: keep it alive over the call)"""
        r = lib_mod.SteerMapRecordC()
        r.n, r.q0, r.q1 = len(self.ranges), self.q0, self.q1
        r.n_planes = self.planes.shape[0] if n_planes is None else n_planes
        for i in range(4):
            for b in range(8):
                r.plane[i][b] = self.plane(i, b) if i < len(self.ranges) else -1
        for i, (k0, k1, _) in enumerate(self.ranges[:4]):
            r.k0[i], r.k1[i] = k0, k1
        arr = self.planes.numpy()
        return r, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), arr

    def steered_rows(self, B, N):
        """bool [B, N]: the rows of [q0, q1) on samples some range applies to"""
        out = torch.zeros(B, N, dtype=torch.bool)
        for b in range(B):
            if any(self.plane(r, b) >= 0 for r in range(len(self.ranges))):
                out[b, self.q0:self.q1] = True
        return out


def beta_maps(rec, B, N, log=torch.log):
    """fp64 [B, N(query), N(key)]"""
    out = torch.zeros(B, N, N, dtype=torch.float64)
    for b in range(B):
        for r, (k0, k1, _) in enumerate(rec.ranges):
            p = rec.plane(r, b)
            if p >= 0:
                out[b, rec.q0:rec.q1, k0:k1] = log(rec.planes[p].double())[:, None]
    return out


def map_reference(case, qmode, rec=None, device="cpu", chunk=1024):
    """fp64 [B * N, H * 64], as attn_steer_ref.steered_reference; rec None: the un-steered restatement"""
    if rec is None:
        return R.steered_reference(case, qmode, None, device, chunk)
    q, k, v = (case.heads(p).to(device) for p in range(3))
    qs, base = R.scaled_q(q, qmode)
    B, H, N = case.B, case.H, case.N
    bt = beta_maps(rec, B, N).to(device)
    out = torch.empty(B, H, N, 64, dtype=torch.float64, device=device)
    for i0 in range(0, N, chunk):
        s = qs[:, :, i0:i0 + chunk] @ k.transpose(-1, -2) * math.log(base) + bt[:, None, i0:i0 + chunk]
        out[:, :, i0:i0 + chunk] = torch.softmax(s, dim=-1) @ v
    return out.transpose(1, 2).reshape(B * N, H * 64).cpu()


def wave_flags_bruteforce(rec, N, first_row_only=False):
    """int32 [8, 8 * ceil(N / 256)]: bit r of entry (b, w) iff plane[r][b] >= 0 and some row i of [32 w, 32 w + 32) with q0 <= i < q1 and i < N
    has W_p[i - q0] != 1.  first_row_only: the mutation -- the bit of the wave's first such row alone"""
    nqb = (N + 255) // 256
    out = torch.zeros(8, 8 * nqb, dtype=torch.int32)
    for b in range(8):
        for w in range(8 * nqb):
            for r in range(len(rec.ranges)):
                p = rec.plane(r, b)
                if p < 0:
                    continue
                rows = [i for i in range(32 * w, 32 * w + 32) if rec.q0 <= i < rec.q1 and i < N]
                if first_row_only:
                    rows = rows[:1]
                if any(float(rec.planes[p, i - rec.q0]) != 1.0 for i in rows):
                    out[b, w] |= 1 << r
    return out


def emulate_maps(case, qmode, rec, mutation=None):
    """attn_pp<MAP>'s algorithm in fp32 on the CPU: attn_steer_ref.emulate with the addend of a row read from the plane of the range and sample at
    row - q0 (0 outside [q0, q1)), and a range skipped for the rows of a wave whose liveness bit is clear.  -> fp32 [B * N, H * 64]"""
    assert mutation is None or mutation in MUTATIONS
    B, H, N, D = case.B, case.H, case.N, case.D
    buf = case.qkv.float()
    rows_total = buf.shape[0]
    out = torch.zeros(B * N, D)
    log = torch.log if mutation == "natural_log" else torch.log2
    qi = torch.arange(N)
    inq = (qi >= rec.q0) & (qi < rec.q1)
    V = rec.q1 - rec.q0
    off = {"row_off_by_one": 1 - rec.q0, "plane_from_row_0": 0}.get(mutation, -rec.q0)
    cell = (qi + off).clamp(0, V - 1)
    live = wave_flags_bruteforce(rec, N, first_row_only=mutation == "live_from_first_row")
    planes_of = [pl for _, _, pl in rec.ranges]
    if mutation == "planes_swapped" and len(planes_of) >= 2:
        planes_of = [planes_of[1], planes_of[0]] + planes_of[2:]
    for b in range(B):
        bp = (b + 1) % B if mutation == "other_sample_plane" else b
        adds = []   # per range: (k0, k1, fp32 [N] addend of each row)
        for r, (k0, k1, _) in enumerate(rec.ranges):
            p = planes_of[r][bp] if bp < len(planes_of[r]) else -1
            if p < 0:
                continue
            on = inq & (((live[b] >> r) & 1).bool().repeat_interleave(32)[:N])
            adds.append((k0, k1, torch.where(on, log(rec.planes[p][cell]), torch.zeros(N))))
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
                for k0, k1, bl in adds:
                    lo, up = max(k0, kv0), min(k1, kv0 + KTILE)
                    if lo >= up:
                        continue   # outside: untouched
                    if up - lo == KTILE:
                        s = s + bl[:, None]   # interior: the whole tile
                    else:
                        s = s + bl[:, None] * ((idx >= lo) & (idx < up)).float()[None]
                sb = torch.where((idx < N)[None], s, torch.full_like(s, -math.inf))
                mn = torch.maximum(m_run, sb.max(dim=1).values)
                alpha = torch.exp2(m_run - mn)
                p = torch.exp2(sb - mn[:, None])
                l_run = l_run * alpha + p.sum(dim=1)
                o = o * alpha[:, None] + p @ buf[rows, 2 * D + h * 64:2 * D + (h + 1) * 64]
                m_run = mn
            out[b * N:(b + 1) * N, h * 64:(h + 1) * 64] = o / l_run[:, None]
    return out


def mapped_forward(layers, rec, B, N, *args, **kw):
    """transformer_forward(*args, **kw) with the blocks `layers` steered by the map record rec (an empty list: the un-steered oracle)"""
    real = TR.F
    TR.F = R._SteerF(real, layers, beta_maps(rec, B, N).float())
    try:
        with torch.no_grad():
            return TR.transformer_forward(*args, **kw)
    finally:
        TR.F = real


# ------------------------------------------------------------------------------------------------ the records the CPU and GPU tests share
def pow2_plane(n, seed, lo=-16, hi=16):
    """n weights 2^u, u an integer drawn per row from [lo, hi]: log2 and the bf16 / fp32 roundings of it are exact"""
    g = torch.Generator().manual_seed(seed)
    return torch.exp2(torch.randint(lo, hi + 1, (n,), generator=g).float())


def geometric_mean_weight(plane):
    return float(torch.exp2(torch.log2(plane.double()).mean()))


def map_crossings(c, rec, qmode="bf16"):
    """attn_steer_ref.crossings for a map record: (rows whose biased base-2 score minus their first tile's biased maximum exceeds 64 at a key of a
    range past tile 0, the same count without the bias) -- the rows on which attn_pp's deferred maximum takes its slow path inside a biased tile"""
    qs, _ = R.scaled_q(c.heads(0), qmode)
    s = qs @ c.heads(1).transpose(-1, -2)
    sb = s + beta_maps(rec, c.B, c.N, torch.log2)[:, None]
    inr = torch.zeros(c.N, dtype=torch.bool)
    for k0, k1, _ in rec.ranges:
        inr[max(k0, KTILE):k1] = True
    over = lambda x: int(((x[..., inr].amax(dim=-1) - x[..., :KTILE].amax(dim=-1)) > 64.0).sum().item())
    return over(sb), over(s)


def map_records(N=330):
    """name -> MapRecord at B = 2: the per-row records of the operator test, and the liveness record (ones on the rows [64, 96), on the rows
    [32, 40) -- the head of a live wave, where the `live_from_first_row` mutation goes wrong -- and on all of item 1; random elsewhere)"""
    P = lambda seed, n=N: pow2_plane(n, seed)
    live = P(21)
    live[64:96] = 1.0
    live[32:40] = 1.0   # eight rows of weight 1 at the head of a live wave
    live[256:] = 1.0
    return {
        "inside_one_tile": MapRecord([(70, 100, [0, 0])], P(1), 0, N),
        "straddle_interior_straddle": MapRecord([(60, 200, [0, 0])], P(2), 0, N),
        "first_tile": MapRecord([(0, 5, [0, 0])], P(3), 0, N),
        "ragged_tile": MapRecord([(300, N, [0, 0])], P(4), 0, N),
        "four_ranges_four_planes": MapRecord([(0, 5, [0, 0]), (70, 100, [1, 1]), (128, 192, [2, 2]), (300, N, [3, 3])],
                                             torch.stack([P(5), P(6), P(7), P(8)]), 0, N),
        "two_ranges_one_plane": MapRecord([(70, 100, [0, 0]), (128, 192, [0, 0])], P(9), 0, N),
        "plane_per_sample": MapRecord([(60, 200, [0, 1])], torch.stack([P(10), P(11)]), 0, N),
        "sample_1_off": MapRecord([(64, 200, [0, -1])], P(12), 0, N),
        "query_range": MapRecord([(60, 200, [0, 0])], P(13, 263), 37, 300),
        "liveness": MapRecord([(60, 200, [0, 0])], live, 0, N),
    }


def constant_record(srec, B=2):
    """the MapRecord of an attn_steer_ref.Record: one constant plane per range, sample_mask translated to plane[r][b]"""
    V = srec.q1 - srec.q0
    ranges = [(k0, k1, [r if (m >> b) & 1 else -1 for b in range(B)]) for r, (k0, k1, _, m) in enumerate(srec.ranges)]
    planes = torch.stack([torch.full((V,), w, dtype=torch.float32) for _, _, w, _ in srec.ranges]) if srec.ranges else torch.ones(1, V)
    return MapRecord(ranges, planes, srec.q0, srec.q1)
