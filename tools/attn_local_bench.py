#!/usr/bin/env python
"""What local attention in time costs and saves (include/s2v_hip.h "Local attention"), one process, alternating arms, spreads reported.

1. The local launch against the un-windowed ones at one geometry (default the headline: 5B, 49 x 480 x 720, B = 2, H = 48, T / R / V =
   226 / 1350 / 17 550, bf16), operator level:
     today        s2v_op_attention impl 0 (attn_q4 beyond 4608 tokens), one workgroup per 256 query rows
     today-p      the same kernel in the persistent form a context runs (diagnostics variant 4 on a queue of this tool)
     pp           the un-windowed attn_pp at the same shape, one workgroup per item (diagnostics variant 10)
     pp-p         the un-windowed attn_pp, persistent (variant 11): what attn_pp<LOCAL> is instantiated from, in the form it runs in
     local-w      s2v_op_attention_local impl 0 with the pipeline's table at frames = w (persistent: more than two items per CU)
     local-full   the same kernel with a table whose every row sees everything: the price of the form itself
   Every local time is reported as a ratio to pp-p of the same run, beside the plan's visited-tile share; the gap is the feature's overhead.
   Every arm includes its V^T pass (the operator entries run it).  HIP events around `--reps` launches per block, `--rounds` rounds.
2. Whole calls: `--steps`-step DDIM calls of the model (hipGraph, every step device-synchronised, host clock) with every layer local at
   `--frames`, against none, alternating by call; ms per step, the ratio, and the relative L2 of the final latents against the dense call --
   arithmetic drift on synthetic weights, which says nothing about a real checkpoint.

    python tools/attn_local_bench.py [--geometry headline] [--rounds 5] [--reps 5] [--steps 10] [--calls 2] [--frames 2] [--layers N]
                                     [--skip-calls] [--out profiles/r21_attn_local.txt]
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


def launches(s2v, a, say, cfg, T, Rr, F):
    L, lib = s2v._lib, s2v.lib()
    diag = L.diag_lib()
    B, Hn, N = 2, cfg.num_attention_heads, T + Rr + F * Rr
    g = torch.Generator(device="cuda:0").manual_seed(11)
    qkv = torch.cat([torch.randn(B * N, 3 * Hn * 64, generator=g, device="cuda:0").to(torch.bfloat16),
                     torch.zeros(64, 3 * Hn * 64, dtype=torch.bfloat16, device="cuda:0")])
    out = torch.empty(B * N, Hn * 64, dtype=torch.bfloat16, device="cuda:0")
    vt = torch.zeros(B * Hn * 64 * ((N + 63) // 64 * 64), dtype=torch.bfloat16, device="cuda:0")
    queue = torch.zeros(16, dtype=torch.int32, device="cuda:0")   # the nine counters of the persistent diagnostics variants
    diag.s2v_set_attn_queue.argtypes = [ctypes.c_void_p, ctypes.c_int]
    diag.s2v_set_attn_queue(ctypes.c_void_p(queue.data_ptr()), torch.cuda.get_device_properties(0).multi_processor_count)
    tables, shares = {}, {}
    for w in (1, 2, 3):
        if w < F - 1:
            P, lo, hi = s2v.local_attention_table(T, Rr, F, Rr, w)
            tables[f"local-{w}"] = (P, L.i32_array(lo), L.i32_array(hi))
            shares[f"local-{w}"] = s2v.local_attention_share(P, lo, hi)
    tables["local-full"] = (T + Rr, L.i32_array([T + Rr] * N), L.i32_array([N] * N))
    shares["local-full"] = 1.0
    args = (L.ptr(qkv), L.ptr(vt), L.ptr(out), B, Hn, N, L.DTYPE_BF16)
    variant = {"today-p": 4, "pp": 10, "pp-p": 11}

    def run(arm):
        if arm == "today":
            L.check(lib.s2v_op_attention(*args, 0, L.stream_ptr()))
        elif arm in variant:
            diag.s2v_set_attn_variant(variant[arm])
            rc = diag.s2v_op_attention(*args, 0, L.stream_ptr())
            diag.s2v_set_attn_variant(0)
            assert rc == 0, diag.s2v_last_error()
        else:
            P, lo, hi = tables[arm]
            L.check(lib.s2v_op_attention_local(*args, 0, P, lo, hi, L.stream_ptr()))

    arms = ["today", "today-p", "pp", "pp-p"] + list(tables)
    for arm in arms:
        for _ in range(2):
            run(arm)
    torch.cuda.synchronize()
    rows = {arm: [] for arm in arms}
    for r in range(a.rounds):
        for arm in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                run(arm)
            e1.record()
            torch.cuda.synchronize()
            rows[arm].append(e0.elapsed_time(e1) / a.reps)
        say(f"round {r}: " + ", ".join(f"{arm} {rows[arm][-1]:.3f} ms" for arm in arms))
    med = {arm: statistics.median(rows[arm]) for arm in arms}
    say(f"launch + V^T pass, B {B} H {Hn} N {N} (T / R / S / F = {T} / {Rr} / {Rr} / {F}), median of {a.rounds} rounds x {a.reps} launches (spread): "
        + ", ".join(f"{arm} {med[arm]:.3f} ms ({max(rows[arm]) - min(rows[arm]):.3f})" for arm in arms))
    say(f"  pp-p / today-p {med['pp-p'] / med['today-p']:.4f}, pp / today {med['pp'] / med['today']:.4f}")
    for arm in tables:
        say(f"  {arm}: / pp-p {med[arm] / med['pp-p']:.4f} beside a visited-tile share of {shares[arm]:.3f} (overhead {med[arm] / med['pp-p'] - shares[arm]:+.4f}); "
            f"/ today-p {med[arm] / med['today-p']:.4f}")
    assert torch.isfinite(out.float()).all()
    diag.s2v_set_attn_queue(None, 0)
    return med


def calls(s2v, a, say, cfg, T, gf, gh, gw):
    dev, dt = "cuda:0", torch.bfloat16
    F, H, W = (gf - 1) // 4 + 1, gh // 8, gw // 8
    Rr = (H // 2) * (W // 2)
    g = torch.Generator(device=dev).manual_seed(100)
    pos = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
    neg = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
    ref = (torch.randn(1, 1, 16, H, W, generator=g, device=dev) * 0.7).to(dt)
    lat0 = torch.randn(1, F, 16, H, W, generator=g, device=dev).to(dt)
    sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale)
    sch.set_timesteps(a.steps)
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, dev)
    bench.load_synthetic(s2v, m.engine, cfg, 1234)   # bench.py's timing weights
    eng = m.engine
    eng.set_geometry(2, T, F, H, W)
    eng.prepare_tables(gh, gw)
    eng.set_conditioning(torch.cat([neg, pos]), ref)
    frames = min(a.frames, max(0, F - 2))
    P, lo, hi = s2v.local_attention_table(T, Rr, F, Rr, frames)
    eng.attn_local_enable(True)
    eng.attn_local_set(P, lo, hi)
    arms = {"local": list(range(cfg.num_layers)), "none": None}
    lat = lat0.clone()
    final = {}

    def call(name):
        lat.copy_(lat0)
        per = []
        for t in sch.timesteps:
            coef = sch.coef(t, dt, 6.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.denoise_step(lat, float(t), coef, use_graph=True, local_layers=arms[name])
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
        final[name] = lat.double().clone()
        return per

    for name in arms:   # warm-up: allocator, code objects, one capture per layer mask
        call(name)
    rows = {name: [] for name in arms}
    for r in range(a.calls):
        for name in arms:
            per = call(name)
            rows[name].append(statistics.median(per))
            say(f"call {r} {name}: {sum(per):.1f} ms for {a.steps} steps, median step {rows[name][-1]:.3f} ms")
    med = {n: statistics.median(rows[n]) for n in rows}
    say(f"{cfg.num_layers} layers, {gf} x {gh} x {gw}, bf16, DDIM, hipGraph, median step over {a.calls} calls (spread): "
        + ", ".join(f"{n} {med[n]:.3f} ms ({max(rows[n]) - min(rows[n]):.3f})" for n in arms))
    drift = ((final["local"] - final["none"]).norm() / final["none"].norm()).item()
    say(f"  every layer local at frames = {frames} (visited-tile share {s2v.local_attention_share(P, lo, hi):.3f}) / none {med['local'] / med['none']:.4f}")
    say(f"  relative L2 of the final latents against the dense call {drift:.3e}: arithmetic drift on synthetic weights, which says nothing about a "
        f"real checkpoint")
    assert torch.isfinite(lat.float()).all()
    eng.attn_local_enable(False)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", default="headline", choices=sorted(GEOMETRIES))
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the model has (a quick look; the committed numbers use all)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    preset, gf, gh, gw = GEOMETRIES[a.geometry]
    cfg = getattr(s2v, preset)()
    if a.layers:
        cfg.num_layers = a.layers
    T = 226
    Rr = (gh // 16) * (gw // 16)
    say("# local attention in time: the local launch against the un-windowed ones, and whole calls (tools/attn_local_bench.py)")
    say(f"# {a.geometry}: {preset}, {gf} x {gh} x {gw}, {torch.cuda.get_device_name(0)}")
    launches(s2v, a, say, cfg, T, Rr, (gf - 1) // 4 + 1)
    if not a.skip_calls:
        calls(s2v, a, say, cfg, T, gf, gh, gw)
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
