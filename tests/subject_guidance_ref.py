"""The torch restatement of subject guidance, shared by tests/test_subject_guidance_cpu.py and tests/test_gpu_subject_guidance.py.

Three model outputs per video -- u (negative text, null reference), r (negative text, the reference), f (positive text, the reference) -- are
combined in fp32, one separately rounded operation per line, in exactly this association:

    v = (u + g_subject * (r - u)) + g_text * (f - r)

and v enters the scheduler step unchanged (csrc/kernels.h: SchedCoef; the arithmetic tests/test_host_cpu.py pins against the reference's bits,
restated here in torch so that it runs on the tensors' own device).  Every torch elementwise op on fp32 tensors rounds once, and a Python
float that is an fp32 value enters as that fp32 value, so nothing here is contracted into an fma.
"""
import torch


def _s(x):
    """a coefficient as a 0-dim fp32 tensor: the value the kernel holds"""
    return torch.tensor(float(x), dtype=torch.float32)


def rnd(x, dt):
    """ET<T>::rnd: a round trip through the model dtype (identity for fp32)"""
    return x.to(dt).float()


def combine(u, r, f, g_subject, g_text):
    """u, r, f fp32 tensors of one shape (the values loaded from the model dtype); five operations, each rounding on its own"""
    gs, gt = _s(g_subject).to(u.device), _s(g_text).to(u.device)
    d_ru = r - u
    p_s = gs * d_ru
    s = u + p_s
    d_fr = f - r
    p_t = gt * d_fr
    v = s + p_t
    return v


def pair_combine(u, c, g_text):
    """the CFG pair's combine (custom_cogvideox_pipe.py:266-279): u + g (c - u), three roundings"""
    gt = _s(g_text).to(u.device)
    d = c - u
    p = gt * d
    return u + p


def sched_step(coef, v, x, x0_old, noise, dt):
    """the scheduler arithmetic behind the combine, on fp32 v and the model-dtype latents x (noise: model dtype, DPM only; x0_old fp32, kind 2
    only) -> (prev fp32 before the final round, x0 fp32)"""
    dev = v.device
    k = {n: _s(getattr(coef, n)).to(dev) for n in ("c_x0_x", "c_x0_v", "a_t", "b_t", "m1", "m2", "m3", "m4", "mn")}
    xf = x.float()
    x0 = rnd(xf * k["c_x0_x"], dt) - k["c_x0_v"] * v
    if coef.kind == 0:
        prev = rnd(k["a_t"] * xf, dt) + k["b_t"] * x0
    else:
        d = x0
        if coef.kind == 2:
            d = k["m3"] * x0 - k["m4"] * x0_old
        prev = (rnd(k["m1"] * xf, dt) - k["m2"] * d) + rnd(k["mn"] * noise.float(), dt)
    return prev, x0


def triple_step(coef, noise_pred, x, x0_old, noise, dt):
    """the subject-guidance step of ONE video: noise_pred [3, ...] = (u, r, f) in the model dtype or fp32 -> (prev fp32 un-rounded, x0 fp32);
    the latents the step stores are rnd(prev, dt)"""
    u, r, f = (p.float() for p in noise_pred)
    v = combine(u, r, f, coef.guidance_subject, coef.guidance)
    return sched_step(coef, v, x, x0_old, noise, dt)


def pair_step(coef, noise_pred, x, x0_old, noise, dt):
    """the pair step of one video: noise_pred [2, ...] = (uncond, cond)"""
    u, c = (p.float() for p in noise_pred)
    return sched_step(coef, pair_combine(u, c, coef.guidance), x, x0_old, noise, dt)
