"""The attention-mass kernel against the product attention launch, and a call with and without attention_map= (report, not a gate).

Part 1 (always): headline geometry, 5B: B = 2, H = 48, T / R / V = 226 / 1350 / 17550, bf16, randn q / k / v.  One process, alternating
launches, HIP events: s2v_op_attention impl 0 (V^T pass + the product kernel) against s2v_op_attn_mass impl 0 on the video queries with the
reference range and two text spans.  Derived: the mass kernel does the QK^T half on 17550 / 19126 of the queries = 0.46 x the attention
launch's matrix work, the same exponentials per (query, key) pair, no P.V.

Part 2 (--call STEPS): a STEPS-step text-to-video call of the 5B configuration at 49 x 480 x 720 (synthetic weights, DDIM, hipGraph) without
and with attention_map=AttentionMap(LAYERS, steps=...) for the stated sets, alternating, wall clock.

    python tools/attn_map_bench.py [--rounds 3] [--iters 5] [--call 50 --layers 20,30 --every 5]
"""
import argparse
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
s2v = importlib.import_module("disentangled-subject-to-vid_amd")
L = s2v._lib
DEV = "cuda:0"


def timed(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_part(rounds, iters):
    import ctypes

    B, H, T, Rr, V = 2, 48, 226, 1350, 17550
    N, D = T + Rr + V, H * 64
    g = torch.Generator(device=DEV).manual_seed(1)
    qkv = torch.randn(B * N + 64, 3 * D, device=DEV, generator=g).bfloat16()
    out = torch.empty(B * N, D, device=DEV, dtype=torch.bfloat16)
    vt = torch.zeros(B * H * 64 * ((N + 63) // 64 * 64), dtype=torch.bfloat16, device=DEV)
    ranges = (ctypes.c_int32 * 6)(T, T + Rr, 3, 9, 100, 140)
    acc = torch.zeros(3, B, H, V, dtype=torch.float32, device=DEV)
    attn = lambda: L.check(L.lib().s2v_op_attention(L.ptr(qkv), L.ptr(vt), L.ptr(out), B, H, N, L.DTYPE_BF16, 0, L.stream_ptr()))
    mass = lambda n: (lambda: L.check(L.lib().s2v_op_attn_mass(L.ptr(qkv), B, H, N, T + Rr, V, ranges, n, L.ptr(acc), 1, L.DTYPE_BF16, 0, L.stream_ptr())))
    for f in (attn, mass(1), mass(3)):
        f()
    torch.cuda.synchronize()
    res = {"attention": [], "mass n=1": [], "mass n=3": []}
    for _ in range(rounds):
        res["attention"].append(timed(attn, iters))
        res["mass n=1"].append(timed(mass(1), iters))
        res["mass n=3"].append(timed(mass(3), iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    flop_attn, flop_mass = 4.0 * 64 * N * N * B * H, 2.0 * 64 * V * N * B * H
    print(f"headline geometry B={B} H={H} T/R/V={T}/{Rr}/{V} bf16, {rounds} rounds x {iters} launches, alternating, median of the rounds")
    for k, v in res.items():
        print(f"  {k:10s} {med[k]:8.3f} ms   (rounds: {' '.join(f'{x:.3f}' for x in v)})")
    print(f"  attention launch (V^T pass + kernel): {flop_attn / med['attention'] / 1e9:.1f} TFLOP/s on {flop_attn / 1e12:.2f} TFLOP")
    for k in ("mass n=1", "mass n=3"):
        print(f"  {k}: {flop_mass / med[k] / 1e9:.1f} TFLOP/s on {flop_mass / 1e12:.2f} TFLOP (0.46 x); time ratio to the attention launch {med[k] / med['attention']:.3f}")


def call_part(steps, layers, every):
    import bench  # the metric's own weight loader

    cfg = s2v.cogvideox_5b()
    dt = torch.bfloat16
    model = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    bench.load_synthetic(s2v, model.engine, cfg, 1234)   # bench.py's timing weights: N(0, 0.02^2) + a rank-128 LoRA merged, finalized
    pipe = s2v.S2VPipeline(model, s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale))
    g = torch.Generator(device=DEV).manual_seed(2)
    T = 226
    kw = dict(prompt_embeds=torch.randn(1, T, cfg.text_embed_dim, device=DEV, generator=g).to(dt),
              negative_prompt_embeds=torch.randn(1, T, cfg.text_embed_dim, device=DEV, generator=g).to(dt),
              ref_img_states=(torch.randn(1, 1, cfg.in_channels, 60, 90, device=DEV, generator=g) * 0.7).to(dt),
              latents=torch.randn(1, 13, cfg.in_channels, 60, 90, device=DEV, generator=g).to(dt),
              height=480, width=720, num_frames=49, num_inference_steps=steps, guidance_scale=6.0, use_graph=True)
    am = s2v.AttentionMap(layers, steps=list(range(0, steps, every)))

    def run(**extra):
        torch.cuda.synchronize()
        t0 = time.time()
        out = pipe(**kw, **extra)["frames"]
        torch.cuda.synchronize()
        return time.time() - t0, out

    run()   # warm-up: captures
    rows = []
    for _ in range(2):
        t_off, a = run()
        t_on, b = run(attention_map=am)
        rows.append((t_off, t_on, torch.equal(a, b)))
    print(f"{steps}-step call, 5B 49x480x720 bf16 DDIM hipGraph; attention_map layers {layers}, steps 0::{every} ({len(am.steps)} steps, "
          f"{len(am.steps) * len(layers)} launches)")
    for t_off, t_on, same in rows:
        print(f"  without {t_off:.3f} s   with {t_on:.3f} s   (+{(t_on / t_off - 1) * 100:.2f} %)   same latents: {same}")
    print(f"  count {pipe.attention_maps['count']}, subject map min / mean / max {pipe.attention_maps['subject'].min().item():.3e} / "
          f"{pipe.attention_maps['subject'].mean().item():.3e} / {pipe.attention_maps['subject'].max().item():.3e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--call", type=int, default=0)
    ap.add_argument("--layers", default="20,30")
    ap.add_argument("--every", type=int, default=5)
    a = ap.parse_args()
    kernel_part(a.rounds, a.iters)
    if a.call:
        call_part(a.call, [int(x) for x in a.layers.split(",")], a.every)
