#!/usr/bin/env python
"""What the step cache saves and how far it moves the arithmetic: the `--steps` (50) step text-to-video call with `step_cache=` at thresholds
chosen so that the plans have roughly 50, 35 and 25 full steps, against the same call without the argument.  Same process, same pipeline
object, same seed, alternating, `--rounds` rounds; DDIM, bf16, hipGraph, latents out.  The plan is printed beside each time.  Also: the reuse
step and the capture step alone against the full step (HIP events around single steps), the two streaming kernels alone at the geometry's
size against their byte count, and the relative L2 of every cached run's final latents against the uncached run.

THE WEIGHTS ARE SYNTHETIC (bench.py's timing weights).  The drift figures say how far the arithmetic moves on them; they do NOT say how a real
checkpoint's videos look, and no threshold is recommended on their strength.

    python tools/step_cache_bench.py [--geometry headline] [--rounds 2] [--steps 50] [--layers N] [--out profiles/r15_step_cache.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the metric's own weight loader)
GEOMETRIES = {"c0": ("cogvideox_2b", 9, 256, 256), "headline": ("cogvideox_5b", 49, 480, 720)}
HBM_PEAK = 8.0e12          # bytes / s, MI355X
LN_MOD_FRACTION = 0.47     # what LayerNorm-modulate reaches of it (README): the rate the streaming kernels are held against


def threshold_for(s2v, emb, full_steps):
    """the smallest threshold (bisection over the plan rule) whose plan has at most `full_steps` full steps"""
    n = emb.shape[0]
    if full_steps >= n:
        return 0.0
    lo, hi = 0.0, 1.0
    while s2v.step_cache_plan(emb, hi).count(True) > full_steps:
        hi *= 2
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if s2v.step_cache_plan(emb, mid).count(True) > full_steps:
            lo = mid
        else:
            hi = mid
    return hi


def calibration(dt, N, D):
    """bench.py's calibrated peak: torch.matmul (hipBLASLt) on the B = 2 FF1 shape, TFLOP/s in this process, on this box, now"""
    xa, xw = torch.randn(2 * N, D, device="cuda:0", dtype=dt), torch.randn(D, 4 * D, device="cuda:0", dtype=dt)
    for _ in range(3):
        torch.matmul(xa, xw)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(10):
        torch.matmul(xa, xw)
    b.record()
    torch.cuda.synchronize()
    return 2.0 * 2 * N * D * 4 * D / (a.elapsed_time(b) / 10) / 1e9


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", nargs="+", default=["headline"], choices=sorted(GEOMETRIES))
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the model has (a quick look; the committed numbers use all)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--full", type=int, nargs="+", default=[50, 35, 25], help="full steps the plans should have, roughly")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    lib, L = s2v.lib(), s2v._lib
    dev, dt, T = "cuda:0", torch.bfloat16, 226
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# step cache: the {a.steps}-step call with step_cache= against the call without it (tools/step_cache_bench.py)")
    say("# synthetic weights: the drift figures say how far the arithmetic moves, not how a real checkpoint's videos look; no threshold is recommended")
    for gname in a.geometry:
        preset, gf, gh, gw = GEOMETRIES[gname]
        cfg = getattr(s2v, preset)()
        if a.layers:
            cfg.num_layers = a.layers
        F, H, W = (gf - 1) // 4 + 1, gh // 8, gw // 8
        V, D = F * (H // 2) * (W // 2), cfg.inner_dim
        N = T + (H // 2) * (W // 2) + V
        m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, dev)
        eng = m.engine
        bench.load_synthetic(s2v, eng, cfg, 1234)   # bench.py's timing weights: N(0, 0.02^2) + a rank-128 LoRA merged, finalized
        g = torch.Generator(device=dev).manual_seed(100)
        pos = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
        neg = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
        ref = (torch.randn(1, 1, 16, H, W, generator=g, device=dev) * 0.7).to(dt)
        lat = torch.randn(1, F, 16, H, W, generator=g, device=dev).to(dt)
        sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale)
        pipe = s2v.S2VPipeline(m, sch)
        cal = calibration(dt, N, D)
        say(f"# {gname}: {preset} x {cfg.num_layers} layers, {gf} x {gh} x {gw}, bf16, DDIM, hipGraph, {a.steps} steps; calibrated peak "
            f"{cal:.1f} TFLOP/s (torch.matmul on the FF1 shape, this process)")
        emb = eng.time_embedding([float(t) for t in sch.timesteps_for(a.steps)])
        plans = []
        for want in a.full:
            th = threshold_for(s2v, emb, want)
            plan = s2v.step_cache_plan(emb, th)
            plans.append((th, plan))
            say(f"plan for ~{want} full steps: threshold {th:.6g} -> {plan.count(True)} full / {plan.count(False)} reused: "
                + "".join("F" if x else "r" for x in plan))
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, height=gh, width=gw, num_frames=gf, num_inference_steps=a.steps,
                  guidance_scale=6.0, latents=lat, use_graph=True, output_type="latent")

        def call(plan, **over):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe(step_cache=plan, **dict(kw, **over))["frames"]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        call(None, num_inference_steps=3), call([True, False, True], num_inference_steps=3)   # warm-up of the allocator and both code paths
        times = {i: [] for i in range(-1, len(plans))}
        outs = {}
        for r in range(a.rounds):
            for i in [-1] + list(range(len(plans))):
                t, out = call(None if i < 0 else plans[i][1])
                times[i].append(t)
                outs[i] = out
            say(f"round {r}: uncached {times[-1][-1]:.3f} s | " + " | ".join(f"{plans[i][1].count(True)} full {times[i][-1]:.3f} s" for i in range(len(plans))))
        base = statistics.median(times[-1])
        for i, (th, plan) in enumerate(plans):
            t = statistics.median(times[i])
            rel = float((outs[i].float() - outs[-1].float()).norm() / outs[-1].float().norm())
            say(f"{gname}: {plan.count(True)} full + {plan.count(False)} reused steps: {t:.3f} s against {base:.3f} s uncached = {base / t:.3f} x "
                f"(spread {max(times[i]) - min(times[i]):.3f} / {max(times[-1]) - min(times[-1]):.3f} s); final latents relative L2 against the "
                f"uncached run {rel:.4e} (synthetic weights), bitwise equal: {torch.equal(outs[i], outs[-1])}")
        # the three kinds of step alone
        eng.set_geometry(2, T, F, H, W)
        eng.prepare_tables(gh, gw)
        eng.set_conditioning(torch.cat([neg, pos]), ref)
        eng.step_cache_enable(True)
        sch.set_timesteps(a.steps)
        t_, x = sch.timesteps[10], lat.clone()
        coef = sch.coef(t_, dt, 6.0)
        step = lambda mode: (lambda: eng.denoise_step(x, float(t_), coef, cache=mode))
        step("capture")(), step("reuse")(), step(None)()
        full, cap, reuse = timed(step(None), 3), timed(step("capture"), 3), timed(step("reuse"), 20)
        say(f"{gname}: one step alone, eager: full {full:.3f} ms, capture {cap:.3f} ms ({cap - full:+.3f}), reuse {reuse:.3f} ms ({full / reuse:.1f} x less)")
        eng.step_cache_enable(False)
        # the streaming kernels alone on the geometry's [B = 2][Ntok][D] residual buffer against a dense [2][V][D] cache
        X = torch.randn(2, N, D, generator=g, device=dev).to(dt)
        C = torch.randn(2, V, D, generator=g, device=dev).to(dt)
        xv = X[:, N - V:]
        floor = lambda passes: passes * 2 * V * D * 2 / (LN_MOD_FRACTION * HBM_PEAK) * 1e3
        for op, name, passes in ((0, "keep (cache = IN)", 2), (1, "subtract (cache = rnd(OUT - cache))", 3), (2, "add (X = rnd(X + cache))", 3)):
            fn = lambda: L.check(lib.s2v_op_step_cache(op, xv.data_ptr(), N * D, L.ptr(C), 2, V * D, L.DTYPE_OF[dt], L.stream_ptr()))
            for _ in range(5):
                fn()
            ms = timed(fn, 50)
            mb = passes * 2 * V * D * 2 / 1e6
            say(f"{gname}: {name}: {ms * 1e3:.1f} us for {mb:.0f} MB = {mb / 1e3 / ms:.2f} TB/s ({mb / 1e3 / ms / (HBM_PEAK / 1e12):.2f} of the HBM peak); derived "
                f"floor at LayerNorm-modulate's {LN_MOD_FRACTION} of the peak: {floor(passes) * 1e3:.1f} us")
        eng.close()
        del pipe, m
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
