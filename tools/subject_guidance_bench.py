#!/usr/bin/env python
"""What subject guidance costs: the triple step (s2v_denoise_step_guided, B = 3 samples [u | r | f]) against the pair step (s2v_denoise_step,
B = 2) of the same tree, bf16, DDIM, hipGraph, one process.  Two engines hold the same synthetic timing weights (bench.py's loader), one
per geometry, so each keeps its captured step; the arms alternate in blocks of `--steps` steps, `--rounds` rounds, every step
device-synchronised and timed on the host clock.  Reported: the median step of each arm and round, the medians over the rounds, the spread of
the alternating runs, and the ratio (by row count the expectation is 1.5 x; it is reported, not gated).  The step's last kernel is timed alone in
both forms at the geometry's latent size (HIP events around `--kernel-reps` launches): the triple form reads one more model-dtype plane.
s2v_device_bytes is reported for B = 2, 3 and 6.

    python tools/subject_guidance_bench.py [--geometry headline] [--rounds 3] [--steps 5] [--layers N] [--out profiles/r18_subject_guidance.txt]
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
GEOMETRIES = {"c0": ("cogvideox_2b", 9, 256, 256), "headline": ("cogvideox_5b", 49, 480, 720)}
GS, GT = 2.5, 6.0


def kernel_times(s2v, sch, dt, F, H, W, reps):
    """(pair, triple) microseconds per launch of the step's last kernel on one [F,16,H,W] latent"""
    lib, L = s2v.lib(), s2v._lib
    g = torch.Generator(device="cuda:0").manual_seed(7)
    npred = torch.randn((3, F, 16, H, W), generator=g, device="cuda:0").to(dt)
    x = torch.randn((1, F, 16, H, W), generator=g, device="cuda:0").to(dt)
    out = torch.empty_like(x)
    sch.set_timesteps(50)
    coef = sch.coef(sch.timesteps[10], dt, GT, guidance_subject=GS)
    dtc, st = L.DTYPE_OF[dt], L.stream_ptr()
    res = []
    for flags in (L.SCHED_CFG_PAIR, L.SCHED_TRIPLE):
        def fn():
            L.check(lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(npred), flags, L.ptr(x), L.ptr(out), None, None, x.numel(), dtc, st))
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", nargs="+", default=["headline"], choices=sorted(GEOMETRIES))
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the model has (a quick look; the committed numbers use all)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    dev, dt, T = "cuda:0", torch.bfloat16, 226
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# the subject-guidance triple step against the pair step (tools/subject_guidance_bench.py)")
    for gname in a.geometry:
        preset, gf, gh, gw = GEOMETRIES[gname]
        cfg = getattr(s2v, preset)()
        if a.layers:
            cfg.num_layers = a.layers
        F, H, W = (gf - 1) // 4 + 1, gh // 8, gw // 8
        g = torch.Generator(device=dev).manual_seed(100)
        pos = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
        neg = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
        ref = (torch.randn(1, 1, 16, H, W, generator=g, device=dev) * 0.7).to(dt)
        lat0 = torch.randn(1, F, 16, H, W, generator=g, device=dev).to(dt)
        sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale)
        sch.set_timesteps(50)
        arms, models = {}, []
        for name, B in (("pair", 2), ("triple", 3)):
            m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, dev)
            bench.load_synthetic(s2v, m.engine, cfg, 1234)   # bench.py's timing weights: N(0, 0.02^2) + a rank-128 LoRA merged, finalized
            eng = m.engine
            eng.set_geometry(B, T, F, H, W)
            eng.prepare_tables(gh, gw)
            if B == 2:
                eng.set_conditioning(torch.cat([neg, pos]), ref)
            else:
                eng.set_conditioning_triples(torch.cat([neg, pos]), ref)   # the zero latent as the null reference
            arms[name] = (eng, lat0.clone())
            models.append(m)
        say(f"# {gname}: {preset} x {cfg.num_layers} layers, {gf} x {gh} x {gw}, bf16, DDIM, hipGraph; {T + (F + 1) * (H // 2) * (W // 2)} tokens per "
            f"sample: {2 * (T + (F + 1) * (H // 2) * (W // 2))} rows against {3 * (T + (F + 1) * (H // 2) * (W // 2))}")
        pos_i = {"pair": 0, "triple": 0}

        def block(name, n):
            """n steps of one arm, each device-synchronised: milliseconds per step"""
            eng, lat = arms[name]
            out = []
            for _ in range(n):
                t = sch.timesteps[pos_i[name] % 50]
                pos_i[name] += 1
                coef = sch.coef(t, dt, GT, guidance_subject=GS)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "pair":
                    eng.denoise_step(lat, float(t), coef, use_graph=True)
                else:
                    eng.denoise_step(lat, [float(t)], [coef], use_graph=True, subject=True)
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            return out

        for name in ("triple", "pair"):   # warm-up: allocator, code objects, the capture
            block(name, a.warmup)
        rows = {"pair": [], "triple": []}
        for r in range(a.rounds):
            res = {name: statistics.median(block(name, a.steps)) for name in ("pair", "triple")}   # alternating: one block of every arm per round
            for name in res:
                rows[name].append(res[name])
            say(f"round {r}: pair {res['pair']:.3f} ms, triple {res['triple']:.3f} ms per step (median of {a.steps}): ratio {res['triple'] / res['pair']:.4f}")
        med = {n: statistics.median(rows[n]) for n in rows}
        spread = {n: max(rows[n]) - min(rows[n]) for n in rows}
        ratios = [t / p for p, t in zip(rows["pair"], rows["triple"])]
        say(f"{gname}: median step pair {med['pair']:.3f} ms (spread {spread['pair']:.3f}), triple {med['triple']:.3f} ms (spread {spread['triple']:.3f}): "
            f"ratio {med['triple'] / med['pair']:.4f} (per round {min(ratios):.4f} .. {max(ratios):.4f}; by row count 1.5)")
        for name in arms:
            assert torch.isfinite(arms[name][1].float()).all()
        ks = kernel_times(s2v, s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale), dt, F, H, W, a.kernel_reps)
        say(f"the step's last kernel alone on [{F},16,{H},{W}]: pair form {ks[0]:.2f} us, triple form {ks[1]:.2f} us ({ks[1] - ks[0]:+.2f} us)")
        eng = arms["triple"][0]
        mem = {}
        for B in (2, 3, 6):
            eng.set_geometry(B, T, F, H, W)
            if B == 6:   # the reference table of two triples is part of the workspace figure
                eng.prepare_tables(gh, gw)
                eng.set_conditioning_triples(torch.cat([neg, neg, pos, pos]), torch.cat([ref, ref]))
            mem[B] = eng.device_bytes()
        say("s2v_device_bytes: weight arena " + f"{mem[3][0] / 2**20:.1f} MiB; workspace "
            + ", ".join(f"B = {B}: {mem[B][1] / 2**20:.1f} MiB" for B in (2, 3, 6)))
        for m in models:
            m.engine.close()
        del arms, models
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
