#!/usr/bin/env python
"""What steering maps cost (include/s2v_hip.h "Steering maps"), one process, alternating arms, spreads reported.

1. The mapped launch at one geometry (default the headline: 5B, 49 x 480 x 720, B = 2, H = 48, T / R / V = 226 / 1350 / 17 550, bf16),
   operator level, one workgroup per 256 query rows in every arm:
     pp         the un-steered attn_pp (diagnostics variant 10), what the steered kernels are instantiated from
     steer-1    s2v_op_attention_steer impl 0, the reference keys [T, T + R) with one scalar weight
     map-full   s2v_op_attention_steer_map impl 0, the same range with a plane of non-1 weights on every video cell
     map-box    the same range, a box of a quarter of each frame at 8, 1 outside: the waves outside the box are not live
     map-4      four mapped ranges (three text spans on sample 1, the reference keys on both), four full planes
   Every arm includes its V^T pass (the operator entries run it); a repeated map call re-uses the uploaded table.  HIP events around `--reps`
   launches per block, `--rounds` rounds.  The live-wave share of each map arm is counted on the host from the library's liveness table.
2. Whole calls: `--steps`-step DDIM calls of the model (hipGraph, every step device-synchronised, host clock) in three arms -- every layer
   mapped (the box map), `--few` layers mapped, none -- alternating by call.

    python tools/attn_steer_map_bench.py [--geometry headline] [--rounds 5] [--reps 5] [--steps 10] [--calls 2] [--few 4] [--layers N]
                                         [--skip-calls] [--out profiles/r23_attn_steer_map.txt]
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the metric's own weight loader)
GEOMETRIES = {"c0": ("cogvideox_2b", 9, 256, 256), "headline": ("cogvideox_5b", 49, 480, 720)}


def map_record(L, ranges, planes, q0, q1):
    r = L.SteerMapRecordC()
    r.n, r.q0, r.q1, r.n_planes = len(ranges), q0, q1, planes.shape[0]
    for i in range(4):
        for b in range(8):
            r.plane[i][b] = -1
    for i, (k0, k1, idx) in enumerate(ranges):
        r.k0[i], r.k1[i] = k0, k1
        for b, p in enumerate(idx):
            r.plane[i][b] = p
    return r


def launches(s2v, a, say, cfg, T, F, Hp, Wp):
    L, lib = s2v._lib, s2v.lib()
    diag = L.diag_lib()
    Rr, V = Hp * Wp, F * Hp * Wp
    B, Hn, N = 2, cfg.num_attention_heads, T + Rr + V
    g = torch.Generator(device="cuda:0").manual_seed(11)
    qkv = torch.cat([torch.randn(B * N, 3 * Hn * 64, generator=g, device="cuda:0").to(torch.bfloat16),
                     torch.zeros(64, 3 * Hn * 64, dtype=torch.bfloat16, device="cuda:0")])
    out = torch.empty(B * N, Hn * 64, dtype=torch.bfloat16, device="cuda:0")
    vt = torch.zeros(B * Hn * 64 * ((N + 63) // 64 * 64), dtype=torch.bfloat16, device="cuda:0")
    srec = L.SteerRecordC()
    srec.n, srec.q0, srec.q1 = 1, T + Rr, N
    srec.k0[0], srec.k1[0], srec.w[0], srec.sample_mask[0] = T, T + Rr, 2.0, 3
    gen = torch.Generator().manual_seed(12)
    full = lambda: torch.exp2(torch.randint(1, 4, (V,), generator=gen).float()).numpy()   # 2, 4 or 8 on every cell: no weight is 1
    box = s2v.box_weight_map((0.25, 0.25, 0.75, 0.75), F, Hp, Wp, 8.0).reshape(1, V).numpy()
    ref = (T, T + Rr, [0, 0])
    maps = {"map-full": ([ref], full()[None]),
            "map-box": ([ref], box),
            "map-4": ([(2, 9, [-1, 0]), (40, 77, [-1, 1]), (130, 200, [-1, 2]), (T, T + Rr, [3, 3])], np.stack([full() for _ in range(4)]))}
    recs = {k: (map_record(L, r, p, T + Rr, N), np.ascontiguousarray(p, dtype=np.float32)) for k, (r, p) in maps.items()}
    for k, (r, p) in maps.items():
        say(f"{k}: {p.shape[0]} plane(s), live-wave share {s2v.attention_steer_live_share(r, p, T + Rr, N, B):.4f}"
            + (f", {float((p != 1).mean()):.4f} of the cells inside the box" if k == "map-box" else ""))
    args = (L.ptr(qkv), L.ptr(vt), L.ptr(out), B, Hn, N, L.DTYPE_BF16)

    def run(arm):
        if arm == "pp":
            diag.s2v_set_attn_variant(10)
            rc = diag.s2v_op_attention(*args, 0, L.stream_ptr())
            diag.s2v_set_attn_variant(0)
            assert rc == 0, diag.s2v_last_error()
        elif arm == "steer-1":
            L.check(lib.s2v_op_attention_steer(*args, 0, ctypes.byref(srec), L.stream_ptr()))
        else:
            r, p = recs[arm]
            L.check(lib.s2v_op_attention_steer_map(*args, 0, ctypes.byref(r), p.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), L.stream_ptr()))

    arms = ["pp", "steer-1", "map-full", "map-box", "map-4"]
    for arm in arms:
        for _ in range(2):
            run(arm)
    torch.cuda.synchronize()
    rows = {arm: [] for arm in arms}
    for r in range(a.rounds):
        for arm in arms:
            run(arm)   # a map arm uploads its table here (the arm before held another); the timed launches repeat the record
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                run(arm)
            e1.record()
            torch.cuda.synchronize()
            rows[arm].append(e0.elapsed_time(e1) / a.reps)
        say(f"round {r}: " + ", ".join(f"{arm} {rows[arm][-1]:.3f} ms" for arm in arms))
    med = {arm: statistics.median(rows[arm]) for arm in arms}
    say(f"launch + V^T pass, B {B} H {Hn} N {N} (T / R / V = {T} / {Rr} / {V}), median of {a.rounds} rounds x {a.reps} launches (spread): "
        + ", ".join(f"{arm} {med[arm]:.3f} ms ({max(rows[arm]) - min(rows[arm]):.3f})" for arm in arms))
    say(f"  steer-1 / pp {med['steer-1'] / med['pp']:.4f}, map-full / pp {med['map-full'] / med['pp']:.4f}, map-full / steer-1 {med['map-full'] / med['steer-1']:.4f}")
    say(f"  map-box / pp {med['map-box'] / med['pp']:.4f}, map-box / map-full {med['map-box'] / med['map-full']:.4f}, map-4 / pp {med['map-4'] / med['pp']:.4f}")
    assert torch.isfinite(out.float()).all()
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
    eng.attn_steer_enable(True)
    box = s2v.box_weight_map((0.25, 0.25, 0.75, 0.75), F, H // 2, W // 2, 8.0).reshape(1, -1)
    eng.attn_steer_set_maps([(T, T + Rr, [0, 0])], box)
    nl = cfg.num_layers
    few = sorted(set(int(round(i * (nl - 1) / max(1, a.few - 1))) for i in range(a.few)))
    arms = {"all": list(range(nl)), "few": few, "none": None}
    lat = lat0.clone()

    def call(name):
        lat.copy_(lat0)
        per = []
        for t in sch.timesteps:
            coef = sch.coef(t, dt, 6.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.denoise_step(lat, float(t), coef, use_graph=True, steer_layers=arms[name])
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
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
    say(f"{cfg.num_layers} layers, {gf} x {gh} x {gw}, bf16, DDIM, hipGraph, the quarter-frame box map, median step over {a.calls} calls (spread): "
        + ", ".join(f"{n} ({'-' if arms[n] is None else len(arms[n])} layers mapped) {med[n]:.3f} ms ({max(rows[n]) - min(rows[n]):.3f})" for n in arms))
    say(f"  all / none {med['all'] / med['none']:.4f}, few {few} / none {med['few'] / med['none']:.4f}")
    assert torch.isfinite(lat.float()).all()
    eng.attn_steer_enable(False)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", default="headline", choices=sorted(GEOMETRIES))
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the model has (a quick look; the committed numbers use all)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--few", type=int, default=4)
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
    F, Hp, Wp = (gf - 1) // 4 + 1, gh // 16, gw // 16
    say("# steering maps: the mapped launch against the scalar steered and the un-steered one, and whole calls (tools/attn_steer_map_bench.py)")
    say(f"# {a.geometry}: {preset}, {gf} x {gh} x {gw}, {torch.cuda.get_device_name(0)}")
    launches(s2v, a, say, cfg, T, F, Hp, Wp)
    if not a.skip_calls:
        calls(s2v, a, say, cfg, T, gf, gh, gw)
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
