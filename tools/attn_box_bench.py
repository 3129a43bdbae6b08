#!/usr/bin/env python
"""What local attention in space and time costs and saves (include/s2v_hip.h "Local attention in space and time"), one process, alternating
arms, spreads reported.  The protocol of tools/attn_local_bench.py.

1. The box launch against the window launch and the un-windowed one at one geometry (default the headline: 5B, 49 x 480 x 720, B = 2, H = 48,
   T / R / S / F = 226 / 1350 / 1350 / 13 with 30 patch rows of 45 cells, bf16), operator level:
     pp-p           the un-windowed attn_pp, persistent (diagnostics variant 11): what the other arms are instantiated from
     local-w        s2v_op_attention_local impl 0 with the pipeline's window table at frames = w (1, 2)
     box-wxr        s2v_op_attention_box impl 0 with the pipeline's box table at frames = w (1, 2, all) and rows = r (3, 5, 7)
     box-2xfull     the box kernel on the window table of frames = 2 with full offsets: the price of the form against local-2
   Every time is reported as a ratio to pp-p of the same run beside the host-counted visited-tile share, and box-2x5 against local-2 with the
   two spreads.  Every arm includes its V^T pass.  HIP events around `--reps` launches per block, `--rounds` rounds.
2. Whole calls: `--steps`-step DDIM calls of the model (hipGraph, every step device-synchronised, host clock) with every layer boxed at
   frames x rows = 2 x 5, against every layer local at frames = 2 and against none, alternating by call; ms per step, the ratios, and the
   relative L2 of the final latents against the dense call -- arithmetic drift on synthetic weights, which says nothing about a real checkpoint.

    python tools/attn_box_bench.py [--geometry headline] [--rounds 5] [--reps 5] [--steps 10] [--calls 2] [--layers N] [--skip-calls]
                                   [--out profiles/r22_attn_box.txt]
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


def launches(s2v, a, say, cfg, T, Hp, Wp, F):
    L, lib = s2v._lib, s2v.lib()
    diag = L.diag_lib()
    Rr = Hp * Wp
    B, Hn, N = 2, cfg.num_attention_heads, T + Rr + F * Rr
    g = torch.Generator(device="cuda:0").manual_seed(11)
    qkv = torch.cat([torch.randn(B * N, 3 * Hn * 64, generator=g, device="cuda:0").to(torch.bfloat16),
                     torch.zeros(64, 3 * Hn * 64, dtype=torch.bfloat16, device="cuda:0")])
    out = torch.empty(B * N, Hn * 64, dtype=torch.bfloat16, device="cuda:0")
    vt = torch.zeros(B * Hn * 64 * ((N + 63) // 64 * 64), dtype=torch.bfloat16, device="cuda:0")
    queue = torch.zeros(16, dtype=torch.int32, device="cuda:0")   # the nine counters of the persistent diagnostics variant
    diag.s2v_set_attn_queue.argtypes = [ctypes.c_void_p, ctypes.c_int]
    diag.s2v_set_attn_queue(ctypes.c_void_p(queue.data_ptr()), torch.cuda.get_device_properties(0).multi_processor_count)
    local, box, shares = {}, {}, {}
    for w in (1, 2):
        if w < F - 1:
            P, lo, hi = s2v.local_attention_table(T, Rr, F, Rr, w)
            local[f"local-{w}"] = (P, L.i32_array(lo), L.i32_array(hi))
            shares[f"local-{w}"] = s2v.local_attention_share(P, lo, hi)
    for w, wname in ((1, "1"), (2, "2"), (F, "all")):
        for r in (3, 5, 7):
            if (w < F - 1 or wname == "all") and r < Hp - 1:
                t = s2v.local_attention_box_table(T, Rr, F, Hp, Wp, w, r)
                box[f"box-{wname}x{r}"] = (t[0], t[1]) + tuple(L.i32_array(x) for x in t[2:])
                shares[f"box-{wname}x{r}"] = s2v.local_attention_box_share(*t)
    if "local-2" in local:
        P, lo, hi = s2v.local_attention_table(T, Rr, F, Rr, 2)
        box["box-2xfull"] = (P, Rr, L.i32_array(lo), L.i32_array(hi), L.i32_array([0] * N), L.i32_array([Rr] * N))
        shares["box-2xfull"] = s2v.local_attention_box_share(P, Rr, lo, hi, [0] * N, [Rr] * N)
    args = (L.ptr(qkv), L.ptr(vt), L.ptr(out), B, Hn, N, L.DTYPE_BF16)

    def run(arm):
        if arm == "pp-p":
            diag.s2v_set_attn_variant(11)
            rc = diag.s2v_op_attention(*args, 0, L.stream_ptr())
            diag.s2v_set_attn_variant(0)
            assert rc == 0, diag.s2v_last_error()
        elif arm in local:
            L.check(lib.s2v_op_attention_local(*args, 0, *local[arm], L.stream_ptr()))
        else:
            L.check(lib.s2v_op_attention_box(*args, 0, *box[arm], L.stream_ptr()))

    arms = ["pp-p"] + list(local) + list(box)
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
    spread = {arm: max(rows[arm]) - min(rows[arm]) for arm in arms}
    say(f"launch + V^T pass (every windowed arm also builds and uploads its record on the host), B {B} H {Hn} N {N} (T / R / S / F = {T} / {Rr} / {Rr} / "
        f"{F}, {Hp} patch rows of {Wp}), median of {a.rounds} rounds x {a.reps} launches (spread): "
        + ", ".join(f"{arm} {med[arm]:.3f} ms ({spread[arm]:.3f})" for arm in arms))
    for arm in arms[1:]:
        say(f"  {arm}: / pp-p {med[arm] / med['pp-p']:.4f} beside a visited-tile share of {shares[arm]:.3f} (gap {med[arm] / med['pp-p'] - shares[arm]:+.4f})")
    for b_arm, l_arm in (("box-2x5", "local-2"), ("box-2xfull", "local-2"), ("box-1x5", "local-1")):
        if b_arm in med and l_arm in med:
            d = med[l_arm] - med[b_arm]
            say(f"  {b_arm} against {l_arm}: {med[b_arm]:.3f} ms against {med[l_arm]:.3f} ms, {d:+.3f} ms faster ({med[b_arm] / med[l_arm]:.4f} x); the two spreads "
                f"{spread[b_arm]:.3f} + {spread[l_arm]:.3f} = {spread[b_arm] + spread[l_arm]:.3f} ms")
    assert torch.isfinite(out.float()).all()
    diag.s2v_set_attn_queue(None, 0)
    return med


def calls(s2v, a, say, cfg, T, gf, gh, gw):
    dev, dt = "cuda:0", torch.bfloat16
    F, H, W = (gf - 1) // 4 + 1, gh // 8, gw // 8
    Hp, Wp = H // 2, W // 2
    Rr = Hp * Wp
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
    frames, rows = min(2, max(0, F - 2)), min(5, max(0, Hp - 2))
    win = s2v.local_attention_table(T, Rr, F, Rr, frames)
    box = s2v.local_attention_box_table(T, Rr, F, Hp, Wp, frames, rows)
    eng.attn_local_enable(True)
    every = list(range(cfg.num_layers))
    arms = {"box": every, "local": every, "none": None}
    lat = lat0.clone()
    final = {}

    def call(name):
        if name == "box":     # the other kind of table drops the captured steps: the first step of such a call captures again, and the median
            eng.attn_local_set_box(*box)   # over the steps leaves that step out
        elif name == "local":
            eng.attn_local_set(*win)
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

    for name in arms:   # warm-up: allocator, code objects
        call(name)
    times = {name: [] for name in arms}
    for r in range(a.calls):
        for name in arms:
            per = call(name)
            times[name].append(statistics.median(per))
            say(f"call {r} {name}: {sum(per):.1f} ms for {a.steps} steps, median step {times[name][-1]:.3f} ms")
    med = {n: statistics.median(times[n]) for n in times}
    say(f"{cfg.num_layers} layers, {gf} x {gh} x {gw}, bf16, DDIM, hipGraph, median step over {a.calls} calls (spread): "
        + ", ".join(f"{n} {med[n]:.3f} ms ({max(times[n]) - min(times[n]):.3f})" for n in arms))
    say(f"  every layer boxed at frames x rows = {frames} x {rows} (visited-tile share {s2v.local_attention_box_share(*box):.3f}) / none "
        f"{med['box'] / med['none']:.4f}; every layer local at frames = {frames} (share {s2v.local_attention_share(*win):.3f}) / none "
        f"{med['local'] / med['none']:.4f}; box / local {med['box'] / med['local']:.4f}")
    for n in ("box", "local"):
        drift = ((final[n] - final["none"]).norm() / final["none"].norm()).item()
        say(f"  relative L2 of the final latents of `{n}` against the dense call {drift:.3e}: arithmetic drift on synthetic weights, which says nothing "
            f"about a real checkpoint")
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
    say("# local attention in space and time: the box launch against the window launch and the un-windowed one, and whole calls (tools/attn_box_bench.py)")
    say(f"# {a.geometry}: {preset}, {gf} x {gh} x {gw}, {torch.cuda.get_device_name(0)}")
    launches(s2v, a, say, cfg, T, gh // 16, gw // 16, (gf - 1) // 4 + 1)
    if not a.skip_calls:
        calls(s2v, a, say, cfg, T, gf, gh, gw)
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
