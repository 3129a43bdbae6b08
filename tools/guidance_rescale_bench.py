#!/usr/bin/env python
"""What guidance rescale costs: the armed step (s2v_set_guidance_rescale, phi = 0.7: statistics kernel, finalize kernel, RESCALE step form behind
the forward) against the plain step of the same tree, 5B, 49 x 480 x 720, bf16, DDIM, hipGraph, one process, ONE engine.  The arms alternate in
blocks of `--steps` steps, `--rounds` rounds; arming and disarming drop the captured step, so every block starts with one untimed step that
captures again; every timed step is device-synchronised and timed on the host clock.  Reported: the median step of each arm and round, the
medians over the rounds with their spreads, and the difference -- three short launches and at most three more reads of 2.2 MB planes behind a
forward of some 600 ms, so the expectation is a difference inside the spread; it is reported, not gated.

The three launches alone on the [13,16,60,90] latent: the step's last kernel in its plain and its RESCALE form (HIP events around
`--kernel-reps` launches), and the statistics + finalize pair through s2v_op_cfg_stats -- that entry allocates, copies and synchronises
around its two launches, so it is timed on the host clock against the same call on ONE element per video, whose kernels are empty: the
difference is the two kernels' time on the full latent.

    python tools/guidance_rescale_bench.py [--rounds 3] [--steps 5] [--layers N] [--out profiles/r22_guidance_rescale.txt]
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the metric's own weight loader)
GT, PHI = 6.0, 0.7


def kernel_times(s2v, sch, dt, F, H, W, reps):
    """microseconds: (plain step kernel, RESCALE step kernel, statistics + finalize on the latent, the same entry on one element)"""
    lib, L = s2v.lib(), s2v._lib
    g = torch.Generator(device="cuda:0").manual_seed(7)
    npred = torch.randn((2, F, 16, H, W), generator=g, device="cuda:0").to(dt)
    x = torch.randn((1, F, 16, H, W), generator=g, device="cuda:0").to(dt)
    out = torch.empty_like(x)
    factor = torch.full((1,), 0.8125, dtype=torch.float32, device="cuda:0")
    coef = sch.coef(sch.timesteps[10], dt, GT)
    dtc, st = L.DTYPE_OF[dt], L.stream_ptr()

    def plain():
        L.check(lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(npred), L.SCHED_CFG_PAIR, L.ptr(x), L.ptr(out), None, None, x.numel(), dtc, st))

    def rescale():
        L.check(lib.s2v_sched_step_rescale(None, ctypes.byref(coef), L.ptr(npred), L.SCHED_CFG_PAIR | L.SCHED_RESCALE, L.ptr(x), L.ptr(out), None, None,
                                           x.numel(), dtc, L.ptr(factor), st))

    res = []
    for fn in (plain, rescale):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / reps)
    sums, factors = (ctypes.c_double * 4)(), (ctypes.c_float * 1)()
    gs, phi = (ctypes.c_float * 1)(GT), (ctypes.c_float * 1)(PHI)
    for n in (x.numel(), 1):
        def stats():
            L.check(lib.s2v_op_cfg_stats(L.ptr(npred), L.SCHED_CFG_PAIR, 1, n, gs, None, phi, sums, factors, dtc, st))
        for _ in range(10):
            stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            stats()
        res.append((time.perf_counter() - t0) * 1e6 / reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the model has (a quick look; the committed numbers use all)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    dev, dt, T = "cuda:0", torch.bfloat16, 226
    gf, gh, gw = 49, 480, 720
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = s2v.cogvideox_5b()
    if a.layers:
        cfg.num_layers = a.layers
    F, H, W = (gf - 1) // 4 + 1, gh // 8, gw // 8
    g = torch.Generator(device=dev).manual_seed(100)
    pos = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
    neg = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
    ref = (torch.randn(1, 1, 16, H, W, generator=g, device=dev) * 0.7).to(dt)
    lat = torch.randn(1, F, 16, H, W, generator=g, device=dev).to(dt)
    sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale)
    sch.set_timesteps(50)
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, dev)
    bench.load_synthetic(s2v, m.engine, cfg, 1234)   # bench.py's timing weights: N(0, 0.02^2) + a rank-128 LoRA merged, finalized
    eng = m.engine
    eng.set_geometry(2, T, F, H, W)
    eng.prepare_tables(gh, gw)
    eng.set_conditioning(torch.cat([neg, pos]), ref)
    say("# guidance rescale: the armed step against the plain step (tools/guidance_rescale_bench.py)")
    say(f"# cogvideox_5b x {cfg.num_layers} layers, {gf} x {gh} x {gw}, bf16, DDIM, hipGraph, {torch.cuda.get_device_name(0)}; phi = {PHI}")
    plain_bytes = eng.device_bytes()
    step_i = [0]

    def block(armed, n):
        """one untimed step that captures, then n timed steps, each device-synchronised: milliseconds per step"""
        eng.set_guidance_rescale(PHI if armed else 0.0)
        out = []
        for j in range(n + 1):
            t = sch.timesteps[step_i[0] % 50]
            step_i[0] += 1
            coef = sch.coef(t, dt, GT)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.denoise_step(lat, float(t), coef, use_graph=True)
            torch.cuda.synchronize()
            if j:
                out.append((time.perf_counter() - t0) * 1e3)
        return out

    block(True, 1)
    armed_bytes = eng.device_bytes()
    block(False, 1)
    rows = {"plain": [], "armed": []}
    factors = []
    for r in range(a.rounds):
        res = {}
        for name in ("plain", "armed"):   # alternating: one block of every arm per round
            res[name] = block(name == "armed", a.steps)
            rows[name].append(statistics.median(res[name]))
        factors.append(eng.guidance_rescale_read()["factors"][0])
        say(f"round {r}: plain {rows['plain'][-1]:.3f} ms (min {min(res['plain']):.3f}, max {max(res['plain']):.3f}), armed {rows['armed'][-1]:.3f} ms "
            f"(min {min(res['armed']):.3f}, max {max(res['armed']):.3f}) per step (median of {a.steps}): armed - plain {rows['armed'][-1] - rows['plain'][-1]:+.3f} ms")
    med = {n: statistics.median(rows[n]) for n in rows}
    spread = {n: max(rows[n]) - min(rows[n]) for n in rows}
    say(f"median step over {a.rounds} rounds: plain {med['plain']:.3f} ms (spread {spread['plain']:.3f}), armed {med['armed']:.3f} ms (spread "
        f"{spread['armed']:.3f}): armed - plain {med['armed'] - med['plain']:+.3f} ms = {(med['armed'] / med['plain'] - 1) * 100:+.4f} %")
    say(f"the last armed step's factor of every round (synthetic weights: it says nothing about a checkpoint): {', '.join(f'{f:.6f}' for f in factors)}")
    assert torch.isfinite(lat.float()).all()
    eng.set_guidance_rescale(None)
    ks = kernel_times(s2v, sch, dt, F, H, W, a.kernel_reps)
    say(f"the launches alone on [{F},16,{H},{W}] ({F * 16 * H * W} elements, {-(-F * 16 * H * W // 4096)} chunks): step kernel plain {ks[0]:.2f} us, RESCALE form "
        f"{ks[1]:.2f} us ({ks[1] - ks[0]:+.2f} us); s2v_op_cfg_stats on the host clock {ks[2]:.2f} us against {ks[3]:.2f} us on one element: statistics + "
        f"finalize {ks[2] - ks[3]:+.2f} us")
    say(f"s2v_device_bytes workspace: plain {plain_bytes[1]} bytes, armed {armed_bytes[1]} bytes (+{armed_bytes[1] - plain_bytes[1]}: partials, sums, "
        f"factors, phi and the factor log)")
    eng.close()
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
