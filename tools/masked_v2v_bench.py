#!/usr/bin/env python
"""What the mask costs: the masked video-to-video call (S2VPipeline(video=, mask=)) against the unmasked `video=` call, `--steps` (50)
inference steps at strength 0.8 = 40 denoise steps, DDIM, bf16, hipGraph, latents out.  Same process, same pipeline object, alternating,
`--rounds` rounds; every step is device-synchronised in the step-end callback, in both arms.  Reported: seconds per call and the median step
of each arm and round, and the spread of the alternating runs that the difference has to be read against.  The step's last kernel is also
timed on its own at the geometry's latent size (s2v_sched_step against s2v_sched_step_masked, HIP events around `--kernel-reps` launches).

The mask is random 16 x 16-pixel blocks over four-frame groups, about half of them repainted.  The input video's latent comes from a stand-in
VAE that returns a fixed posterior sample: the encode is not what is measured here.

    python tools/masked_v2v_bench.py [--geometry c0 headline] [--rounds 3] [--steps 50] [--layers N] [--out profiles/r14_masked_v2v.txt]
"""
import argparse
import ctypes
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
STRENGTH = 0.8


class _FixedLatentVAE:
    """encode(video).latent_dist.sample(generator) -> one fixed [1,C,Fl,h,w] draw"""

    def __init__(self, z, scaling_factor):
        self.config = SimpleNamespace(scaling_factor=scaling_factor)
        self._z = z

    def encode(self, video):
        return SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda generator=None: self._z))


def kernel_times(s2v, sch, dt, F, H, W, mask, reps):
    """(unmasked, masked) microseconds per launch of the step's last kernel on one [F,16,H,W] latent"""
    lib, L = s2v.lib(), s2v._lib
    g = torch.Generator(device="cuda:0").manual_seed(7)
    npred, x, z0, n0 = (torch.randn(s, generator=g, device="cuda:0").to(dt) for s in ((2, F, 16, H, W),) + ((1, F, 16, H, W),) * 3)
    out = torch.empty_like(x)
    sch.set_timesteps(50)
    coef, rec = sch.coef(sch.timesteps[10], dt, 6.0), sch.blend_record(sch.timesteps[11], dt, "cuda:0")
    dtc, st = L.DTYPE_OF[dt], L.stream_ptr()

    def plain():
        L.check(lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(npred), 1, L.ptr(x), L.ptr(out), None, None, x.numel(), dtc, st))

    def masked():
        L.check(lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), L.ptr(npred), 1, L.ptr(x), L.ptr(out), None, None, L.ptr(z0),
                                          L.ptr(n0), L.ptr(mask), F, 16, H, W, dtc, st))

    res = []
    for fn in (plain, masked):
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
    ap.add_argument("--geometry", nargs="+", default=["c0", "headline"], choices=sorted(GEOMETRIES))
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the model has (a quick look; the committed numbers use all)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    dev, dt, T = "cuda:0", torch.bfloat16, 226
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# masked against unmasked video-to-video, {a.steps} steps at strength {STRENGTH} (tools/masked_v2v_bench.py)")
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
        blocks = (torch.rand(1, 1, F, gh // 16, gw // 16, generator=g, device=dev) < 0.5).float()
        mask = torch.nn.functional.interpolate(blocks, size=(4 * F, gh, gw), mode="nearest")[:, 0, 3:].to(torch.uint8).contiguous()   # [1, gf, gh, gw]
        sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale)
        pipe = s2v.S2VPipeline(m, sch, _FixedLatentVAE(z, cfg.vae_scaling_factor))
        video = torch.zeros(1).expand(1, 3, gf, gh, gw)   # the stand-in VAE never reads it
        lat_mask, _ = s2v.mask_to_latent(mask, dev)
        n_steps = len(pipe.get_timesteps(a.steps, list(range(a.steps)), STRENGTH)[0])
        say(f"# {gname}: {preset} x {cfg.num_layers} layers, {gf} x {gh} x {gw}, bf16, DDIM, hipGraph; {n_steps} denoise steps per call; "
            f"{float(lat_mask.float().mean()) * 100:.1f} % of the latent cells repainted")
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, height=gh, width=gw, num_inference_steps=a.steps,
                  guidance_scale=6.0, video=video, strength=STRENGTH, use_graph=True, output_type="latent")
        marks = []

        def mark(p, i, t, tensors):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())
            return {}

        def call(masked):
            marks.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe(mask=mask if masked else None, generator=torch.Generator().manual_seed(3), callback_on_step_end=mark, **kw)["frames"]
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            steps = [b - x for x, b in zip(marks[:-1], marks[1:])]   # without the call's first step (set-up, mask reduction, capture)
            return total, statistics.median(steps) * 1e3, out

        call(False), call(True)   # warm-up of the allocator and both code paths
        rows = []
        for r in range(a.rounds):
            t_m, s_m, out_m = call(True)
            t_u, s_u, out_u = call(False)
            rows.append((t_m, s_m, t_u, s_u))
            say(f"round {r}: masked {t_m:.3f} s, median step {s_m:.3f} ms | unmasked {t_u:.3f} s, median step {s_u:.3f} ms | "
                f"masked - unmasked = {s_m - s_u:+.3f} ms per step ({(s_m / s_u - 1) * 100:+.3f} %)")
        sm, su = [r[1] for r in rows], [r[3] for r in rows]
        say(f"{gname}: median step masked {statistics.median(sm):.3f} ms (spread {max(sm) - min(sm):.3f}), unmasked {statistics.median(su):.3f} ms "
            f"(spread {max(su) - min(su):.3f}): difference {statistics.median(sm) - statistics.median(su):+.3f} ms per step; whole call "
            f"{statistics.median(r[0] for r in rows):.3f} s against {statistics.median(r[2] for r in rows):.3f} s")
        keep = (lat_mask == 0)[:, :, None].expand_as(out_m)
        z0 = cfg.vae_scaling_factor * z.to(dt).permute(0, 2, 1, 3, 4).contiguous()
        say(f"kept cells of the masked call are the clean input latents bit for bit: {torch.equal(out_m[keep], z0[keep])}; the repainted ones "
            f"differ from the unmasked call's: {not torch.equal(out_m[~keep], out_u[~keep])}")
        k_u, k_m = kernel_times(s2v, s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale), dt, F, H, W, lat_mask, a.kernel_reps)
        say(f"the step's last kernel alone on [{F},16,{H},{W}]: sched_step_k {k_u:.2f} us, masked form {k_m:.2f} us ({k_m - k_u:+.2f} us)")
        m.engine.close()
        del pipe, m
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
