#!/usr/bin/env python
"""What the runtime adapter mode costs per denoise step (TransformerConfig.lora_runtime_rank, include/s2v_hip.h s2v_lora_attach).

One process, one GPU, the headline geometry (CogVideoX-5B, 49 x 480 x 720, bf16, CFG pair B = 2, hipGraph):
  A = the mode-off engine with a rank-r adapter MERGED (the default path), B = a runtime-mode engine with the SAME adapter ATTACHED.
  * step time A / B, alternating, `--rounds` rounds of `--steps` graph replays each, device-synchronised around every round;
  * the per-class breakdown of one eager step of each (s2v_profile_read; class 9 = the down-projections);
  * the derived floor of the overhead: the extra MFMA work of the K-extended GEMMs (K'/K - 1 of each base GEMM's time as A measures
    it in this process) + the down-projections' bytes (x once, T once) at the bandwidth LayerNorm-modulate reaches in this process;
  * the down-projection kernel's own rate against its byte floor at the HBM peak (bench.py PEAK_HBM_GBS = 8000 GB/s);
  * the wall time of attach_lora on the loaded runtime engine (reading a checkpoint directory is not timed here).
Acceptance (printed, not enforced here): overhead <= 2 x floor, down-projection >= 0.5 of its byte floor.

--weight-format fp8 | fp8-qk | fp8-auto: A = the fp8 engine with the adapter merged BEFORE the e4m3 quantisation, B = the fp8 engine created with
lora_runtime_fp8 and the same adapter attached as a 16-bit branch beside the e4m3 weights.  The floor then is: the bytes each down-projection
must read (bf16 rows for QKV / FF1, one byte per element for the out-projection and FF2 from their MX images) and write (T), the bf16 rows
LayerNorm-modulate now stores beside its e4m3 image, plus 2 R / K of each base GEMM's time -- R / K extra matrix work at the bf16 MFMA rate,
half the fp8 rate the base runs at.  No acceptance line is printed for fp8: the ratio measured / derived is reported.

    python tools/lora_runtime_bench.py [--layers 42] [--rank 128] [--rounds 5] [--steps 3] [--weight-format fp8] [--geometry 49x720x1280] [--out profiles/...txt]
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
PEAK_HBM_GBS = 8000.0
CLASSES = ["qkv", "attention", "out_proj", "ff1", "ff2", "ln_modulate", "qknorm_vt", "mod_gemv", "shard", "lora_down"]


def load_base(s2v, eng, cfg, seed):
    """N(0, 0.02^2) timing weights drawn tensor by tensor on the GPU (bench.py's load_synthetic without its merge)"""
    gen = torch.Generator(device=eng.device).manual_seed(seed)
    for k, shp in s2v.weights.state_dict_shapes(cfg).items():
        is_norm = ".norm" in k or k.startswith("norm_final") or "norm_q" in k or "norm_k" in k
        if len(shp) >= 2:
            t = torch.randn(shp, generator=gen, device=eng.device) * 0.02
        elif k.endswith("weight") and is_norm and ".linear." not in k:
            t = torch.ones(shp, device=eng.device)
        else:
            t = torch.zeros(shp, device=eng.device)
        eng.load_weight(k, t)
        eng._keep.clear()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=42)
    ap.add_argument("--rank", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--weight-format", default=None, choices=["fp8", "fp8-qk", "fp8-auto"])
    ap.add_argument("--geometry", default="49x480x720", help="frames x height x width in pixels (49x480x720, 49x720x1280)")
    a = ap.parse_args()
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    dev, dt = "cuda:0", torch.bfloat16
    gf, gh, gw = (int(v) for v in a.geometry.split("x"))
    F, H, W, T = (gf - 1) // 4 + 1, gh // 8, gw // 8, 226
    fp8 = a.weight_format is not None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def mk(rank):
        cfg = s2v.cogvideox_5b()
        cfg.num_layers = a.layers
        cfg.lora_runtime_rank = rank
        cfg.weight_format = a.weight_format
        cfg.lora_runtime_fp8 = fp8 and rank > 0
        return cfg

    lora = s2v.weights.synthetic_lora(mk(0), rank=a.rank, seed=99, device=dev, std=0.02)
    g = torch.Generator(device=dev).manual_seed(100)
    text = torch.randn(2, T, 4096, generator=g, device=dev)
    ref = torch.randn(1, 1, 16, H, W, generator=g, device=dev) * 0.7
    lat0 = torch.randn(1, F, 16, H, W, generator=g, device=dev).to(dt).contiguous()
    sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0)
    sch.set_timesteps(50)
    coefs = [sch.coef(t, dt, 6.0) for t in sch.timesteps]

    engines, load_s = {}, {}
    for name, rank in (("merged", 0), ("runtime", a.rank)):
        cfg = mk(rank)
        eng = s2v.S2VEngine(cfg, dt, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        load_base(s2v, eng, cfg, 1234)
        if rank == 0:
            for k, (A, B) in lora.items():
                eng.merge_lora(k, A, B, 0.5)
            eng.finalize_weights()
        else:
            eng.finalize_weights()
        torch.cuda.synchronize()
        load_s[name] = time.perf_counter() - t0
        if rank:
            t0 = time.perf_counter()
            eng.attach_lora(lora, 0.5)
            torch.cuda.synchronize()
            load_s["attach"] = time.perf_counter() - t0
        eng.set_geometry(2, T, F, H, W)
        eng.prepare_tables(H * 8, W * 8)
        eng.set_conditioning(text, ref)
        engines[name] = (eng, lat0.clone())
    say(f"# runtime LoRA: 5B x {a.layers} layers, {a.geometry.replace('x', ' x ')}, {a.weight_format or 'bf16'}, B = 2, rank {a.rank}, hipGraph; one process, one GPU")
    for name in engines:
        ar, ws = engines[name][0].device_bytes()
        say(f"device_bytes {name}: arena {ar / 2**30:.3f} GiB workspace {ws / 2**30:.3f} GiB")
    say(f"attach_lora on the loaded runtime engine ({len(lora)} weights, rank {a.rank}, fp32 A / B already on the device): {load_s['attach']:.2f} s")

    def run(name, n, i0=0):
        eng, lat = engines[name]
        for i in range(n):
            eng.denoise_step(lat, float(sch.timesteps[(i0 + i) % 50]), coefs[(i0 + i) % 50], use_graph=True)

    for name in engines:
        run(name, a.warmup)
    torch.cuda.synchronize()
    per = {"merged": [], "runtime": []}
    for r in range(a.rounds):
        for name in ("merged", "runtime") if r % 2 == 0 else ("runtime", "merged"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, a.steps, a.warmup + r * a.steps)
            torch.cuda.synchronize()
            per[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    for name in per:
        say(f"step ms {name}: " + " ".join(f"{x:.1f}" for x in per[name]) + f" | median {statistics.median(per[name]):.1f}")
    mA, mB = statistics.median(per["merged"]), statistics.median(per["runtime"])
    over = mB - mA
    say(f"A/B overhead of the runtime branch: {over:.1f} ms per step = {100 * over / mA:.2f} % of the merged engine's {mA:.1f} ms")
    for eng, lat in engines.values():
        assert torch.isfinite(lat.float()).all()

    # per-class breakdown of one eager step each
    prof = {}
    L = s2v._lib
    for name, (eng, lat) in engines.items():
        L.check(L.lib().s2v_profile_enable(eng._h, 1))
        eng.denoise_step(lat, float(sch.timesteps[25]), coefs[25], use_graph=False)
        ms = (ctypes.c_float * 10)()
        cnt = (ctypes.c_int32 * 10)()
        L.check(L.lib().s2v_profile_read(eng._h, ms, cnt, 10))
        L.check(L.lib().s2v_profile_enable(eng._h, 0))
        prof[name] = ([float(x) for x in ms], [int(x) for x in cnt])
        say(f"profile {name} (eager step, ms / launches): " + ", ".join(f"{c} {m:.2f}/{n}" for c, m, n in zip(CLASSES, *prof[name]) if n))

    # the floor
    D, E, M = 3072, 2, 2 * (T + (F + 1) * (H // 2) * (W // 2))
    R = (a.rank + 63) // 64 * 64 if fp8 else (a.rank + 127) // 128 * 128
    pa = prof["merged"][0]
    if fp8:  # R / K extra matrix work at the bf16 MFMA rate = 2 R / K of the fp8 GEMM's time; every QKV column meets ONE adapter
        extra = {"qkv": 2 * R / D, "out_proj": 2 * R / D, "ff1": 2 * R / D, "ff2": 2 * R / (4 * D)}
    else:
        extra = {"qkv": 3 * R / D, "out_proj": R / D, "ff1": R / D, "ff2": R / (4 * D)}
    mfma_floor = sum(pa[CLASSES.index(k)] * f for k, f in extra.items())
    ln_ms, ln_n = pa[5], prof["merged"][1][5]
    ln_gbs = (M * D * E + M * D) * ln_n / (ln_ms * 1e-3) / 1e9 if fp8 else 2 * M * D * E * ln_n / (ln_ms * 1e-3) / 1e9
    if fp8:  # x: bf16 rows twice (QKV, FF1), bytes + block scales for the out-projection (K = D) and FF2 (K = 4 D); T written four times;
        # and the bf16 rows LayerNorm-modulate stores beside its e4m3 image, twice per block
        down_bytes = a.layers * (2 * M * D * E + (M * D + M * 4 * D) * 33 // 32 + M * 6 * R * E + 2 * M * D * E)
    else:
        down_bytes = a.layers * ((3 * M * D + M * 4 * D) * E + M * 6 * R * E)
    bytes_floor = down_bytes / (ln_gbs * 1e9) * 1e3
    floor = mfma_floor + bytes_floor
    say(f"floor: extra MFMA work {mfma_floor:.2f} ms (" + ", ".join(f"{k} +{100 * f:.1f} %" for k, f in extra.items()) + f") + down-projection bytes "
        f"{down_bytes / 1e9:.2f} GB at LayerNorm-modulate's {ln_gbs:.0f} GB/s = {bytes_floor:.2f} ms -> {floor:.2f} ms per step")
    if fp8:
        say(f"measured / derived: overhead {over:.1f} ms against the floor {floor:.2f} ms = {over / floor:.2f} x")
    else:
        say(f"acceptance 1: overhead {over:.1f} ms <= 2 x floor {2 * floor:.1f} ms: {'MET' if over <= 2 * floor else 'MISSED'}")
    dn_ms = prof["runtime"][0][9]
    if fp8:
        down_bytes -= a.layers * 2 * M * D * E   # the kernels' own bytes: without LayerNorm-modulate's extra store
    dn_gbs = down_bytes / (dn_ms * 1e-3) / 1e9 if dn_ms > 0 else 0.0
    say(f"down-projection kernel: {dn_ms:.2f} ms per step over {prof['runtime'][1][9]} launches = {dn_gbs:.0f} GB/s = {dn_gbs / PEAK_HBM_GBS:.3f} of the "
        f"{PEAK_HBM_GBS:.0f} GB/s HBM peak (LayerNorm-modulate: {ln_gbs / PEAK_HBM_GBS:.3f})")
    if not fp8:
        say(f"acceptance 2: down-projection rate against its byte floor >= 0.5: {'MET' if dn_gbs / PEAK_HBM_GBS >= 0.5 else 'MISSED'}")
    pb = prof["runtime"][0]
    say("where the overhead goes (eager ms, runtime - merged): " + ", ".join(f"{c} {pb[i] - pa[i]:+.2f}" for i, c in enumerate(CLASSES) if prof["runtime"][1][i]))
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for eng, _ in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
