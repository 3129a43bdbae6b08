"""The guidance rescale restated (include/s2v_hip.h, "Guidance rescale"): the order of the four fp64 sums, the deviations, the factor, the
rescaled prediction, and the checks that tests/test_gpu_guidance_rescale.py holds the device to and tests/test_guidance_rescale_cpu.py holds
an emulation and its mutations to.  numpy and torch on the CPU only; nothing here needs the library.

A CANDIDATE is a dict of what an implementation produced for ONE video:
    sums    [4] fp64: sum f, sum f^2, sum v, sum v^2
    std     (std_f, std_v) fp64 -- the device does not export them: they are taken from ITS sums by the stated formula (stds_from_sums)
    k       the fp32 factor
    vprime  [n] fp32: what entered the scheduler arithmetic
and every check compares it with what this file derives from the fp32 planes themselves.
"""
import math

import numpy as np
import torch

import subject_guidance_ref as SG

CHUNK, LANES = 4096, 256   # S2V_CFG_STATS_CHUNK; the lanes of a workgroup
ULP32 = 2.0 ** -23         # the spacing of fp32 in [1, 2): one ulp of a factor, relative, is at most this
REF_BAR = 4 * 2.0 ** -24   # against the reference's formula: one ulp on the factor (2 * 2^-24), its rounding to fp32 and the product's (2^-24 each)
STD_BAR = 2.0 ** -30       # the one-pass deviation against numpy's two-pass one, relative.  The one-pass form loses about (1 + mean^2 / var) n 2^-53:
                           # under 2^-38 for the randn-scaled planes (n < 2^14, |mean| < std) of the tests; n for n - 1 moves it by 1 / (2 n) > 2^-15


def combine(planes, g, gs=None):
    """planes [2, n] (u, c) or [3, n] (u, r, f) fp32 torch -> v fp32 [n]: the step kernel's combine, every operation rounding on its own"""
    planes = planes.float()
    if planes.shape[0] == 2:
        return SG.pair_combine(planes[0], planes[1], g)
    return SG.combine(planes[0], planes[1], planes[2], gs, g)


def ordered_sum(x):
    """x [n] fp64 numpy -> its sum in the stated order: chunks of 4096; lane t adds elements t, t + 256, ... of its chunk in ascending order from
    +0; the halving tree lane[t] += lane[t + s], s = 128 .. 1; the chunk sums added in ascending order from +0.  (Padding a short chunk with +0
    changes nothing: no accumulator is ever -0, and x + 0 = x.)"""
    x = np.asarray(x, dtype=np.float64)
    nch = -(-x.size // CHUNK)
    a = np.zeros(nch * CHUNK, dtype=np.float64)
    a[:x.size] = x
    a = a.reshape(nch, CHUNK // LANES, LANES)
    acc = np.zeros((nch, LANES), dtype=np.float64)
    for r in range(CHUNK // LANES):
        acc = acc + a[:, r, :]
    s = LANES // 2
    while s >= 1:
        acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    total = np.float64(0.0)
    for c in range(nch):
        total = total + acc[c, 0]
    return total


def sums_of(f, v):
    """f, v [n] fp32 (torch or numpy) -> [4] fp64 in the stated order; the squares are exact in fp64"""
    f64, v64 = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (f, v))
    with np.errstate(all="ignore"):
        return np.array([ordered_sum(f64), ordered_sum(f64 * f64), ordered_sum(v64), ordered_sum(v64 * v64)], dtype=np.float64)


def stds_from_sums(sums, n):
    """(std_f, std_v) by the stated one-pass formula, n - 1 in the divisor; nan where it does not exist"""
    out = []
    for s, ss in ((float(sums[0]), float(sums[1])), (float(sums[2]), float(sums[3]))):
        try:
            var = (ss - s * s / n) / (n - 1.0)
            out.append(math.sqrt(var) if var >= 0 else math.nan)
        except (ZeroDivisionError, ValueError, OverflowError):
            out.append(math.nan)
    return tuple(out)


def factor_of(sums, n, phi):
    """the fp32 factor from the four sums: 1 exactly for phi = 0, n < 2, a std_v that is not finite or 0, a quotient that is not finite"""
    if phi == 0.0 or n < 2:
        return np.float32(1.0)
    std_f, std_v = stds_from_sums(sums, n)
    if not math.isfinite(std_v) or std_v == 0.0:
        return np.float32(1.0)
    q = std_f / std_v
    if not math.isfinite(q):
        return np.float32(1.0)
    return np.float32(phi * q + (1.0 - phi))


def ulps32(a, b):
    """the distance of two finite fp32 values of one sign, in representable values"""
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def reference_rescale(v, f, phi):
    """rescale_noise_cfg (diffusers/src/diffusers/pipelines/stable_diffusion/pipeline_stable_diffusion.py:67-90) on ONE sample, in torch fp64 on
    the fp32 v and f: element by element, phi * (v * (std_text / std_cfg)) + (1 - phi) * v"""
    v64, f64 = torch.as_tensor(v).double().flatten(), torch.as_tensor(f).double().flatten()
    std_text, std_cfg = f64.std(), v64.std()                     # :84-85 (torch.std: n - 1)
    rescaled = v64 * (std_text / std_cfg)                        # :87
    return phi * rescaled + (1 - phi) * v64                      # :89


# ---- the checks: each returns None or a sentence saying what failed -------------------------------------------------------------------------
def check_sums(cand, f, v):
    want = sums_of(f, v)
    got = np.asarray(cand["sums"], dtype=np.float64)
    if got.tobytes() != want.tobytes():
        return f"the four sums differ from the stated order's: {got.tolist()} against {want.tolist()}"


def check_std(cand, f, v):
    for name, got, x in (("std_f", cand["std"][0], f), ("std_v", cand["std"][1], v)):
        want = float(np.std(np.asarray(x, dtype=np.float32).astype(np.float64), ddof=1))
        if not abs(got - want) <= STD_BAR * want:
            return f"{name} = {got!r} against numpy's two-pass {want!r}: relative {abs(got - want) / want:.3e} > {STD_BAR:.3e}"


def check_factor(cand, f, v, phi):
    want = factor_of(sums_of(f, v), len(f), phi)
    if not (math.isfinite(float(cand["k"])) and ulps32(cand["k"], want) <= 1):
        return f"the factor {float(cand['k'])!r} is more than one fp32 ulp from the restatement's {float(want)!r}"


def check_vprime(cand, v):
    """with the candidate's OWN factor: v' must be the one fp32 multiply v * k, bit for bit"""
    want = (torch.as_tensor(v).float() * torch.tensor(float(cand["k"]), dtype=torch.float32)).numpy()
    if np.asarray(cand["vprime"], dtype=np.float32).tobytes() != want.tobytes():
        return "the rescaled prediction is not the one fp32 multiply v * k"


def check_reference(cand, f, v, phi):
    want = reference_rescale(v, f, phi).numpy()
    got = np.asarray(cand["vprime"], dtype=np.float32).astype(np.float64)
    rel = np.abs(got - want) / np.abs(want)
    worst = float(np.nanmax(np.where(want != 0, rel, 0.0)))
    if not worst <= REF_BAR:
        return f"against rescale_noise_cfg in fp64 the worst relative error is {worst:.3e} > {REF_BAR:.3e}"


def failures(cand, planes, g, gs, phi):
    """every check on one video's candidate; planes [2 | 3, n] fp32 torch (the values the kernel loads).  Returns the sentences of the failed ones"""
    v = combine(planes, g, gs).numpy()
    f = planes[-1].float().numpy()
    out = [check_sums(cand, f, v), check_std(cand, f, v), check_factor(cand, f, v, phi), check_vprime(cand, v), check_reference(cand, f, v, phi)]
    return [m for m in out if m]
