#!/usr/bin/env python
"""What a sweep costs as ONE batched call against one call per video (S2VPipeline with per-video lists: every video on its own plan in the one loop of pipeline.py).

The sweep: one input video at strength 0.4 / 0.6 / 0.8 / 1.0 and `--steps` (50) inference steps, DDIM, bf16, hipGraph -- plans of 20 / 30 / 40 / 50
steps, 140 video-steps.  The one call holds 4 videos for 20 steps, then 3, 2 and 1 for 10 steps each, and re-sets geometry, tables and
conditioning at every shrink; the single calls run one video each.  Same process, same pipeline object, alternating, `--rounds` rounds.  Every
step is device-synchronised in the step-end callback, in both arms.  Reported: seconds per arm and round, video-steps/s and their ratio; for the
one call, per active count the median step time and what the first step at that count costs beyond it (the re-geometry and the graph capture).

The input video's latent comes from a stand-in VAE that returns a fixed posterior sample: the encode is not what is measured here
(tools/vae_encode_video_time.py measures it).

    python tools/batch_sweep_bench.py [--geometry c0 headline] [--rounds 2] [--steps 50] [--layers N] [--out profiles/r13_batch_sweep.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the metric's own weight loader)
GEOMETRIES = {"c0": ("cogvideox_2b", 9, 256, 256), "headline": ("cogvideox_5b", 49, 480, 720)}
STRENGTHS = [0.4, 0.6, 0.8, 1.0]


class _FixedLatentVAE:
    """encode(video).latent_dist.sample(generator) -> one fixed [1,C,Fl,h,w] draw"""

    def __init__(self, z, scaling_factor):
        self.config = SimpleNamespace(scaling_factor=scaling_factor)
        self._z = z

    def encode(self, video):
        return SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda generator=None: self._z))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", nargs="+", default=["c0", "headline"], choices=sorted(GEOMETRIES))
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the model has (a quick look; the committed numbers use all)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    dev, dt, T = "cuda:0", torch.bfloat16, 226
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# strength sweep {STRENGTHS} at {a.steps} steps: one batched call against one call per video (tools/batch_sweep_bench.py)")
    for gname in a.geometry:
        preset, gf, gh, gw = GEOMETRIES[gname]
        cfg = getattr(s2v, preset)()
        if a.layers:
            cfg.num_layers = a.layers
        F, H, W = (gf - 1) // 4 + 1, gh // 8, gw // 8
        m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, dev)
        bench.load_synthetic(s2v, m.engine, cfg, 1234)   # bench.py's timing weights: N(0, 0.02^2) + a rank-128 LoRA merged, finalized
        g = torch.Generator(device=dev).manual_seed(100)
        pos = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
        neg = torch.randn(1, T, cfg.text_embed_dim, generator=g, device=dev).to(dt)
        ref = (torch.randn(1, 1, 16, H, W, generator=g, device=dev) * 0.7).to(dt)
        z = torch.randn(1, 16, F, H, W, generator=g, device=dev).to(dt)
        pipe = s2v.S2VPipeline(m, s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale), _FixedLatentVAE(z, cfg.vae_scaling_factor))
        video = torch.zeros(1).expand(1, 3, gf, gh, gw)   # the stand-in VAE never reads it
        lens = [len(pipe.get_timesteps(a.steps, list(range(a.steps)), s)[0]) for s in STRENGTHS]
        say(f"# {gname}: {preset} x {cfg.num_layers} layers, {gf} x {gh} x {gw}, bf16, DDIM, hipGraph; plans of {lens} steps = {sum(lens)} video-steps")
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, height=gh, width=gw, num_inference_steps=a.steps,
                  guidance_scale=6.0, video=video, use_graph=True)
        marks = []

        def mark(p, i, t, tensors):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())
            return {}

        def one_call():
            marks.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe(num_videos_per_prompt=4, strength=STRENGTHS, generator=[torch.Generator().manual_seed(k) for k in range(4)],
                       callback_on_step_end=mark, **kw)["frames"]
            torch.cuda.synchronize()
            steps = [b - x for x, b in zip([t0] + marks[:-1], marks)]
            return time.perf_counter() - t0, steps, out

        def single_calls():
            total, steps, outs = 0.0, [], []
            for k, s in enumerate(STRENGTHS):
                marks.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs.append(pipe(strength=s, generator=torch.Generator().manual_seed(k), callback_on_step_end=mark, **kw)["frames"])
                torch.cuda.synchronize()
                total += time.perf_counter() - t0
                steps += [b - x for x, b in zip(marks[:-1], marks[1:])]   # without each call's first step (set-up, capture)
            return total, steps, torch.cat(outs)

        single_calls() if a.rounds > 1 else None   # warm-up of the allocator and the code paths; a one-round look goes without
        rows = []
        for r in range(a.rounds):
            t_one, steps_one, out_one = one_call()
            t_sep, steps_sep, out_sep = single_calls()
            rows.append((t_one, t_sep))
            say(f"round {r}: one call {t_one:.3f} s = {sum(lens) / t_one:.2f} video-steps/s | four single calls {t_sep:.3f} s = "
                f"{sum(lens) / t_sep:.2f} video-steps/s | one call / single calls = {t_sep / t_one:.3f} x")
        med_sep = statistics.median(steps_sep) * 1e3
        say(f"single calls: median step {med_sep:.2f} ms (b = 1)")
        active = [sum(1 for n in lens if n > i) for i in range(max(lens))]
        for b in sorted(set(active), reverse=True):
            idx = [i for i, x in enumerate(active) if x == b]
            med = statistics.median(steps_one[i] for i in idx[1:]) * 1e3
            say(f"one call, {b} active: {len(idx)} steps, median step {med:.2f} ms = {med / b:.2f} ms per video ({med_sep * b / med:.3f} x single); first "
                f"step at this count {steps_one[idx[0]] * 1e3:.1f} ms = + {steps_one[idx[0]] * 1e3 - med:.1f} ms (geometry, tables, conditioning, capture)")
        ar, ws = m.engine.device_bytes()
        say(f"device_bytes at the end (b = 1): arena {ar / 2**30:.3f} GiB workspace {ws / 2**30:.3f} GiB")
        t1, ts = statistics.median(x for x, _ in rows), statistics.median(y for _, y in rows)
        say(f"{gname}: one call {t1:.3f} s, four single calls {ts:.3f} s: {ts / t1:.3f} x")
        same = torch.equal(out_one, out_sep)
        say(f"latents of the one call equal the single calls' bit for bit: {same}" + ("" if same else " (a GEMM splits K at one of the batch sizes)"))
        m.engine.close()
        del pipe, m
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
