#!/usr/bin/env python
"""What the mask costs: the masked video-to-video call (S2VPipeline(video=, mask=)) against the unmasked `video=` call, `--steps` (50)
inference steps at strength 0.8 = 40 denoise steps, DDIM, bf16, hipGraph, latents out.  Same process, same pipeline object, alternating,
`--rounds` rounds; every step is device-synchronised in the step-end callback, in both arms.  Reported: seconds per call and the median step
of each arm and round, and the spread of the alternating runs that the difference has to be read against.  The step's last kernel is also
timed on its own at the geometry's latent size (s2v_sched_step against s2v_sched_step_masked, HIP events around `--kernel-reps` launches).

The mask is random 16 x 16-pixel blocks over four-frame groups, about half of them repainted.  The input video's latent comes from a stand-in
VAE that returns a fixed posterior sample: the encode is not what is measured here.

--change-map adds a third arm, S2VPipeline(video=, change_map=) with a linear ramp of levels along the width (0 over the left ninth, then
rising to 255 at the right edge), alternating with the other two in the same rounds, and times the step's last kernel in a third form: a plane of levels against keep_max = 127 (the masked form is the
same kernel on a 0 / 1 plane against keep_max = 0).

    python tools/masked_v2v_bench.py [--geometry c0 headline] [--rounds 3] [--steps 50] [--layers N] [--change-map] [--out profiles/r14_masked_v2v.txt]
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


def kernel_times(s2v, sch, dt, F, H, W, mask, reps, level=None):
    """(unmasked, masked[, levels against keep_max = 127]) microseconds per launch of the step's last kernel on one [F,16,H,W] latent"""
    lib, L = s2v.lib(), s2v._lib
    g = torch.Generator(device="cuda:0").manual_seed(7)
    npred, x, z0, n0 = (torch.randn(s, generator=g, device="cuda:0").to(dt) for s in ((2, F, 16, H, W),) + ((1, F, 16, H, W),) * 3)
    out = torch.empty_like(x)
    sch.set_timesteps(50)
    coef, rec = sch.coef(sch.timesteps[10], dt, 6.0), sch.blend_record(sch.timesteps[11], dt, "cuda:0")
    dtc, st = L.DTYPE_OF[dt], L.stream_ptr()

    def plain():
        L.check(lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(npred), 1, L.ptr(x), L.ptr(out), None, None, x.numel(), dtc, st))

    def masked(rec=rec, plane=mask):
        L.check(lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), L.ptr(npred), 1, L.ptr(x), L.ptr(out), None, None, L.ptr(z0),
                                          L.ptr(n0), L.ptr(plane), F, 16, H, W, dtc, st))

    fns = [plain, masked]
    if level is not None:
        rec_map = sch.blend_record(sch.timesteps[11], dt, "cuda:0", 127)
        fns.append(lambda: masked(rec_map, level))
    res = []
    for fn in fns:
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
    ap.add_argument("--change-map", action="store_true", help="a third arm: change_map= with a linear ramp of levels along the width")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    dev, dt, T = "cuda:0", torch.bfloat16, 226
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {'change map and ' if a.change_map else ''}masked against unmasked video-to-video, {a.steps} steps at strength {STRENGTH} "
        f"(tools/masked_v2v_bench.py)")
    arms = (["change map"] if a.change_map else []) + ["masked", "unmasked"]
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
        cmap = lat_level = None
        if a.change_map:   # level 0 over the left ninth, then a linear ramp to 255 at the right edge; the same in every row and frame
            ramp = (torch.linspace(-0.125, 1, gw, device=dev).clamp(min=0) * 255 + 0.5).to(torch.uint8)
            cmap = ramp[None, None, None, :].expand(1, gf, gh, gw).contiguous()
            lat_level, _ = s2v.map_to_latent(cmap, dev)
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

        def call(arm):
            marks.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            region = {"masked": dict(mask=mask), "change map": dict(change_map=cmap), "unmasked": {}}[arm]
            out = pipe(generator=torch.Generator().manual_seed(3), callback_on_step_end=mark, **region, **kw)["frames"]
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            steps = [b - x for x, b in zip(marks[:-1], marks[1:])]   # without the call's first step (set-up, mask reduction, capture)
            return total, statistics.median(steps) * 1e3, out

        for arm in reversed(arms):   # warm-up of the allocator and every code path
            call(arm)
        rows = {arm: [] for arm in arms}
        for r in range(a.rounds):
            res = {arm: call(arm) for arm in arms}   # alternating: one call of every arm per round
            for arm in arms:
                rows[arm].append(res[arm][:2])
            s_u = res["unmasked"][1]
            say(f"round {r}: " + " | ".join(f"{arm} {res[arm][0]:.3f} s, median step {res[arm][1]:.3f} ms" for arm in arms) + " | "
                + ", ".join(f"{arm} - unmasked = {res[arm][1] - s_u:+.3f} ms per step ({(res[arm][1] / s_u - 1) * 100:+.3f} %)" for arm in arms[:-1]))
        out_m, out_u = res["masked"][2], res["unmasked"][2]
        med = {arm: statistics.median(x[1] for x in rows[arm]) for arm in arms}
        say(f"{gname}: median step " + ", ".join(f"{arm} {med[arm]:.3f} ms (spread {max(x[1] for x in rows[arm]) - min(x[1] for x in rows[arm]):.3f})"
                                                 for arm in arms)
            + ": difference to unmasked " + ", ".join(f"{arm} {med[arm] - med['unmasked']:+.3f} ms per step" for arm in arms[:-1])
            + "; whole call " + " / ".join(f"{statistics.median(x[0] for x in rows[arm]):.3f} s" for arm in arms))
        keep = (lat_mask == 0)[:, :, None].expand_as(out_m)
        z0 = cfg.vae_scaling_factor * z.to(dt).permute(0, 2, 1, 3, 4).contiguous()
        say(f"kept cells of the masked call are the clean input latents bit for bit: {torch.equal(out_m[keep], z0[keep])}; the repainted ones "
            f"differ from the unmasked call's: {not torch.equal(out_m[~keep], out_u[~keep])}")
        if a.change_map:
            out_c = res["change map"][2]
            zero = (lat_level == 0)[:, :, None].expand_as(out_c)
            say(f"level-0 cells of the change-map call are the clean input latents bit for bit: {torch.equal(out_c[zero], z0[zero])} "
                f"({float((lat_level == 0).float().mean()) * 100:.1f} % of the cells; thresholds {s2v.change_map_plan(n_steps)[:3]} ...)")
        ks = kernel_times(s2v, s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale), dt, F, H, W, lat_mask, a.kernel_reps, lat_level)
        say(f"the step's last kernel alone on [{F},16,{H},{W}]: sched_step_k {ks[0]:.2f} us, masked form {ks[1]:.2f} us ({ks[1] - ks[0]:+.2f} us)"
            + (f", levels against keep_max 127 {ks[2]:.2f} us ({ks[2] - ks[1]:+.2f} us to the masked form)" if a.change_map else ""))
        m.engine.close()
        del pipe, m
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:   # a fresh file per run: nothing stacks in a committed profile
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
