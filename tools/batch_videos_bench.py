#!/usr/bin/env python
"""What several videos per call buy per denoise step (include/s2v_hip.h: S2V_MAX_BATCH, s2v_denoise_step on [b] latents).

One process, one GPU, bf16, hipGraph.  Per geometry three engines with the same weights hold b = 1, 2 and 4 videos (B = 2b samples,
[negative x b | positive x b], one reference per video); they are timed alternating, `--rounds` rounds of `--steps` graph replays each,
device-synchronised around every round.  Reported per b: ms per step (median of the rounds), video-steps/s = b / step time, its ratio to b = 1, and
s2v_device_bytes (weight arena, workspace).

    python tools/batch_videos_bench.py [--geometry c0 headline] [--rounds 5] [--steps 3] [--layers N] [--out profiles/r11_batch_videos.txt]

Geometries: c0 = BASELINE configs[0] (CogVideoX-2B, 9 x 256 x 256: 1250 tokens per sample); headline = CogVideoX-5B, 49 x 480 x 720 (19 126 tokens).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", nargs="+", default=["c0", "headline"], choices=sorted(GEOMETRIES))
    ap.add_argument("--videos", nargs="+", type=int, default=[1, 2, 4])
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the model has (a quick look; the committed numbers use all)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    dev, dt, T = "cuda:0", torch.bfloat16, 226
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for gname in a.geometry:
        preset, gf, gh, gw = GEOMETRIES[gname]
        cfg = getattr(s2v, preset)()
        if a.layers:
            cfg.num_layers = a.layers
        F, H, W = (gf - 1) // 4 + 1, gh // 8, gw // 8
        ntok = T + (F + 1) * (H // 2) * (W // 2)
        sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale)
        sch.set_timesteps(50)
        coefs = [sch.coef(t, dt, 6.0) for t in sch.timesteps]
        g = torch.Generator(device=dev).manual_seed(100)
        bmax = max(a.videos)
        text = torch.randn(2 * bmax, T, cfg.text_embed_dim, generator=g, device=dev)
        ref = torch.randn(bmax, 1, 16, H, W, generator=g, device=dev) * 0.7
        lat0 = torch.randn(bmax, F, 16, H, W, generator=g, device=dev).to(dt)
        say(f"# {gname}: {preset} x {cfg.num_layers} layers, {gf} x {gh} x {gw}, {ntok} tokens per sample, bf16, hipGraph; one process, one GPU")
        engines = {}
        for b in a.videos:
            eng = s2v.S2VEngine(cfg, dt, dev)
            bench.load_synthetic(s2v, eng, cfg, 1234)   # bench.py's timing weights: N(0, 0.02^2) + a rank-128 LoRA merged, finalized
            eng.set_geometry(2 * b, T, F, H, W)
            eng.prepare_tables(gh, gw)
            eng.set_conditioning(torch.cat([text[:b], text[bmax:bmax + b]]), ref[:b])
            engines[b] = (eng, lat0[:b].contiguous().clone())
            ar, ws = eng.device_bytes()
            say(f"device_bytes b={b}: arena {ar / 2**30:.3f} GiB workspace {ws / 2**30:.3f} GiB ({2 * b * ntok} rows)")

        def run(b, n, i0):
            eng, lat = engines[b]
            for i in range(n):
                eng.denoise_step(lat, float(sch.timesteps[(i0 + i) % 50]), coefs[(i0 + i) % 50], use_graph=True)

        for b in a.videos:
            run(b, a.warmup, 0)
        torch.cuda.synchronize()
        per = {b: [] for b in a.videos}
        for r in range(a.rounds):
            for b in a.videos if r % 2 == 0 else list(reversed(a.videos)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(b, a.steps, a.warmup + r * a.steps)
                torch.cuda.synchronize()
                per[b].append((time.perf_counter() - t0) / a.steps * 1e3)
        base = 1e3 / statistics.median(per[1]) if 1 in per else None   # video-steps/s of one video per call
        for b in a.videos:
            med = statistics.median(per[b])
            vps = b / med * 1e3
            ratio = f"{vps / base:.3f} x b=1" if base else "-"
            say(f"b={b}: step ms " + " ".join(f"{x:.2f}" for x in per[b]) + f" | median {med:.2f} ms ({med / b:.2f} ms per video), "
                f"{vps:.2f} video-steps/s, {ratio}")
        for eng, lat in engines.values():
            assert torch.isfinite(lat.float()).all()
            eng.close()
        del engines
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
