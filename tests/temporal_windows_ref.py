"""Temporal windows restated in torch (include/s2v_hip.h: s2v_set_windows, s2v_denoise_step_windows, s2v_op_window_blend), for the tests of the
feature.  Everything runs on the CPU in fp32, one torch operation per rounding: torch rounds every elementwise operation on its own and its
CPU division is IEEE.

  window_plan     the definition again, written independently of pipeline.window_plan
  blend_scatter   the definition of the blend: zeros, `+=` window by window in ascending order, `/`
  blend_gather    what the kernel does: batch by batch, every frame of the batch's range gathers the batch's windows that cover it, starts from
                  +0 where its first window is in the batch (a NaN in the plane shows a read that must not happen) and is divided where its
                  last one is; `mutate` breaks it in one named way, for the test that proves the checks can fail
"""
import numpy as np
import torch

MUTATIONS = ("descending", "fma", "global_weight", "drop_last_frame", "batch_wsum", "reciprocal")


def window_weights(F, weighting):
    if weighting == "flat":
        return [1.0] * F
    assert weighting == "pyramid", weighting
    up = list(range(1, (F + 1) // 2 + 1))
    return [float(x) for x in (up + up[::-1][F % 2:])]


def window_plan(L, F, s, weighting):
    assert 1 <= s <= F <= L and (L - F) % s == 0, (L, F, s)
    W = (L - F) // s + 1
    w = window_weights(F, weighting)
    wsum = [np.float32(0.0)] * L
    for k in range(W):
        for j in range(F):
            wsum[k * s + j] = np.float32(wsum[k * s + j] + np.float32(w[j]))
    return dict(L=L, F=F, s=s, W=W, starts=[k * s for k in range(W)], weights=w, wsum=[float(x) for x in wsum])


def _f32(x):
    return x.detach().to("cpu", torch.float32)


def combine(u, c, g):
    """the pair combine of sched_step_k: v = u + g * (c - u), three roundings"""
    return u + g * (c - u)


def blend_scatter(neg, pos, g, plan):
    """neg, pos [W, F, ...]: the negative and the positive prediction of every window (any dtype; taken to fp32 exactly) -> vbar [L, ...] fp32"""
    neg, pos = _f32(neg), _f32(pos)
    L, F, s, W = plan["L"], plan["F"], plan["s"], plan["W"]
    acc = torch.zeros((L,) + tuple(neg.shape[2:]), dtype=torch.float32)
    for k in range(W):
        v = combine(neg[k], pos[k], g)
        for j in range(F):
            acc[k * s + j] += plan["weights"][j] * v[j]
    # a divisor of the plane's own shape: torch may turn a division by a scalar into a multiplication by its reciprocal
    wsum = torch.tensor(plan["wsum"], dtype=torch.float32).reshape((L,) + (1,) * (neg.ndim - 2)).expand_as(acc).contiguous()
    return acc / wsum


def blend_gather(neg, pos, g, plan, per_forward, mutate=None):
    """the kernel's order of operations, launch by launch; neg, pos as for blend_scatter.  The plane starts as NaN: a cell that is read before
    this step wrote it poisons the result"""
    assert mutate is None or mutate in MUTATIONS, mutate
    neg, pos = _f32(neg), _f32(pos)
    L, F, s, W = plan["L"], plan["F"], plan["s"], plan["W"]
    w = plan["weights"]
    assert W % per_forward == 0
    acc = torch.full((L,) + tuple(neg.shape[2:]), float("nan"), dtype=torch.float32)
    for k0 in range(0, W, per_forward):
        k1 = k0 + per_forward - 1
        for f in range(k0 * s, k1 * s + F):
            k_first = 0 if f < F else (f - F) // s + 1
            k_last = min(W - 1, f // s)
            a = torch.zeros_like(acc[f]) if k_first >= k0 else acc[f].clone()
            ks = list(range(max(k_first, k0), min(k_last, k1) + 1))
            if mutate == "descending":
                ks = ks[::-1]
            wsum = np.float32(0.0)
            for k in ks:
                j = f - k * s
                wsum = np.float32(wsum + np.float32(w[j]))
                if mutate == "drop_last_frame" and j == F - 1:
                    continue
                u, c = neg[k, j], pos[k, j]
                if mutate == "fma":   # g * (c - u) + u with one rounding: exact in float64 (24 x 24 bits), then rounded once more to fp32
                    v = ((c - u).double() * float(np.float32(g)) + u.double()).float()
                else:
                    v = combine(u, c, g)
                a = a + (w[f % F] if mutate == "global_weight" else w[j]) * v
            if k_last <= k1:
                d = float(wsum) if mutate == "batch_wsum" else plan["wsum"][f]
                a = a * float(np.float32(1.0) / np.float32(d)) if mutate == "reciprocal" else a / torch.full_like(a, d)
            acc[f] = a
    return acc
