"""Video encode (s2v_vae_encode_video) at 49 x 480 x 720 with the real VAE widths, and one video-to-video S2VPipeline call at 5B.
    python tools/vae_encode_video_time.py --flops          CPU only: algorithmic FLOPs of the encode (FlopCounterMode through the oracle on
                                                            meta tensors, the way BASELINE section 2 counted the decode)
    python tools/vae_encode_video_time.py [--steps N] [--out FILE]
                                                            GPU: encode times (bf16 / fp16, tiled / untiled, min of 3 after one warm-up),
                                                            then S2VPipeline(video=..., strength=0.8) with N steps (default 50) through
                                                            decode to uint8 frames.  Prints, and appends to FILE when given."""
import argparse
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
s2v = importlib.import_module("disentangled-subject-to-vid_amd")
F_, H_, W_ = 49, 480, 720


def enc_batches(F):
    nb, rem = max(F // 8, 1), F % 8
    return [(8 * i + (0 if i == 0 else rem), 8 * (i + 1) + rem) for i in range(nb)]


def count_flops():
    """FLOPs of the reference's _encode / tiled_encode over the oracle's encoder, meta tensors (no arithmetic runs)"""
    from torch.utils.flop_counter import FlopCounterMode

    from oracle import vae_ref

    vcfg = s2v.VAEConfig()
    cfg = dict(block_out_channels=tuple(vcfg.block_out_channels), layers_per_block=vcfg.layers_per_block,
               norm_num_groups=vcfg.norm_num_groups, latent_channels=vcfg.latent_channels, sample_height=vcfg.sample_height,
               sample_width=vcfg.sample_width, temporal_compression_ratio=vcfg.temporal_compression_ratio, scaling_factor=0.7)
    sd = {k: torch.empty(shp, device="meta") for k, shp in s2v.weights.vae_encoder_shapes(vcfg).items()}

    def untiled(x):
        cache, out = None, []
        for s, e in enc_batches(x.shape[2]):
            y, cache = vae_ref.encoder_forward(sd, cfg, x[:, :, s:e], cache)
            out.append(y)
        return torch.cat(out, dim=2)

    def tiled(x):
        tg = vae_ref.encode_tile_geometry(cfg)
        for i in range(0, x.shape[3], tg["ov_h"]):
            for j in range(0, x.shape[4], tg["ov_w"]):
                untiled(x[:, :, :, i:i + tg["ts_h"], j:j + tg["ts_w"]])

    res = {}
    for name, fn in (("untiled", untiled), ("tiled", tiled)):
        x = torch.empty(1, 3, F_, H_, W_, device="meta")
        with FlopCounterMode(display=False) as fc:
            fn(x)
        res[name] = fc.get_total_flops()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flops", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fl = count_flops()
    say(f"encode 49x480x720 algorithmic FLOPs (FlopCounterMode, oracle on meta tensors): untiled {fl['untiled'] / 1e12:.2f} T, "
        f"tiled {fl['tiled'] / 1e12:.2f} T")
    if not a.flops:
        dev = "cuda:0"
        x = (torch.rand(1, 3, F_, H_, W_, generator=torch.Generator().manual_seed(5)) * 2 - 1)
        vcfg = s2v.VAEConfig(scaling_factor=0.7)
        sd_enc = s2v.weights.synthetic_vae_encoder_state_dict(vcfg, seed=6)
        for dt in (torch.bfloat16, torch.float16):
            vae = s2v.HipAutoencoderKLCogVideoX(vcfg, dt, dev)
            vae.load_state_dict(sd_enc)
            xd = x.to(dev, dt)
            for label, tiling in (("tiled", True), ("untiled", False), ("tiled after untiled", True)):
                vae.use_tiling = tiling
                mom = vae.encode(xd).latent_dist.parameters
                torch.cuda.synchronize()
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    mom = vae.encode(xd).latent_dist.parameters
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                t = min(ts)
                f = fl["tiled" if tiling else "untiled"]
                say(f"encode {str(dt)[6:]:9s} {label:20s}: {t * 1e3:8.1f} ms  {f / t / 1e12:6.1f} TFLOP/s  moments {tuple(mom.shape)}  "
                    f"finite {bool(torch.isfinite(mom.float()).all())}")
            vae.close()
            del vae
            torch.cuda.empty_cache()
        # one video-to-video call at 5B, bf16, tiled VAE, fused step on the captured graph
        cfg = s2v.cogvideox_5b()
        m = s2v.HipCogVideoXTransformer3DModel(cfg, torch.bfloat16, dev)
        m.load_state_dict(s2v.weights.synthetic_state_dict(cfg, seed=1, device=dev))
        vcfg = s2v.VAEConfig(scaling_factor=cfg.vae_scaling_factor)
        vae = s2v.HipAutoencoderKLCogVideoX(vcfg, torch.bfloat16, dev)
        sd = dict(s2v.weights.synthetic_vae_state_dict(vcfg, seed=2, device=dev))
        sd.update(s2v.weights.synthetic_vae_encoder_state_dict(vcfg, seed=6))
        vae.load_state_dict(sd)
        vae.enable_tiling()
        pipe = s2v.S2VPipeline(m, s2v.CogVideoXDDIMScheduler(snr_shift_scale=cfg.snr_shift_scale), vae)
        g = torch.Generator(device=dev).manual_seed(3)
        pe = torch.randn(1, 226, 4096, generator=g, device=dev).bfloat16()
        ne = torch.randn(1, 226, 4096, generator=g, device=dev).bfloat16()
        ref = (torch.randn(1, 1, 16, 60, 90, generator=g, device=dev) * 0.7).bfloat16()
        xv = x.to(dev, torch.bfloat16)
        for run in range(2):  # the first call also builds the graph and the workspaces
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lat = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, ref_img_states=ref, height=H_, width=W_, num_inference_steps=a.steps,
                       guidance_scale=6.0, generator=torch.Generator(device=dev).manual_seed(4), video=xv, strength=0.8,
                       output_type="latent", use_graph=True)["frames"]
            frames = vae.frames_uint8(vae.decode_latents(lat)[0:1])
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            say(f"video2video 5B bf16 49x480x720 strength 0.8, {a.steps} steps ({int(a.steps * 0.8)} run), tiled VAE, graph, call {run}: "
                f"{t:.2f} s  frames {tuple(frames.shape)}  latents finite {bool(torch.isfinite(lat.float()).all())}")
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
