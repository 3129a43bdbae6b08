"""Ulysses sequence parallelism on ONE GPU: what p GPUs would do per step, measured rank by rank.

Builds the single engine and p shard contexts (s2v_set_shard) of the full model in one process, runs the in-process lockstep step
(dist.UlyssesLocal: the exchanges are device copies) and times with HIP events on the launch stream:
  * per rank: compute ms, excluding the exchanges (events around each rank's begin / resume / end segments; the packs and unpacks are inside);
  * pack / unpack ms and their effective GB/s (bytes read + written; s2v_profile_read class 8);
  * bytes per all-to-all per rank and per step, and a link-bound exchange time at an ASSUMED, UNMEASURED 153 GB/s per xGMI link (bench.py's
    constant) -- each rank sends (p - 1) / p of its chunks, one link per peer;
  * the single engine's B = 2 step in the same process, and the per-kernel-class breakdown of both.
The p-GPU step time printed is a PROJECTION: max-over-ranks compute + the link-bound exchange time; no multi-GPU node has run it.

python tools/ulysses_projection.py --workload cogvideox-5b-49x480x720 --p 2 4
"""
import argparse
import ctypes
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
s2v = importlib.import_module("disentangled-subject-to-vid_amd")
DEV = "cuda:0"
WORKLOADS = {"cogvideox-5b-49x480x720": (s2v.cogvideox_5b, 226, 13, 60, 90)}
CLASSES = ["qkv", "attn", "out", "ff1", "ff2", "lnmod", "qknorm/vt", "other", "pack/unpack"]
LINK_GBPS = 153.0


def profile(eng, fn):
    s2v._lib.check(s2v.lib().s2v_profile_enable(eng._h, 1))
    fn()
    ms = (ctypes.c_float * 9)()
    cnt = (ctypes.c_int32 * 9)()
    s2v._lib.check(s2v.lib().s2v_profile_read(eng._h, ms, cnt, 9))
    s2v._lib.check(s2v.lib().s2v_profile_enable(eng._h, 0))
    return list(ms), list(cnt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cogvideox-5b-49x480x720", choices=sorted(WORKLOADS))
    ap.add_argument("--p", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--layers", type=int, default=None, help="override the layer count (smoke runs)")
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    mk, T, F, H, W = WORKLOADS[a.workload]
    cfg = mk()
    if a.layers:
        cfg.num_layers = a.layers
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(5)
    text = torch.randn(2, T, cfg.text_embed_dim, generator=g, device=DEV)
    ref = torch.randn(1, 1, cfg.in_channels, H, W, generator=g, device=DEV) * 0.7
    lat0 = torch.randn(1, F, cfg.in_channels, H, W, generator=g, device=DEV).to(dt).contiguous()
    sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0)
    sch.set_timesteps(50)
    t = sch.timesteps[10]
    coef = sch.coef(t, dt, 6.0)
    E, D, N = 2, cfg.inner_dim, T + (H // 2) * (W // 2) * (F + 1)

    def build(shard=None, src=None):
        m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
        if src is None:
            m.load_state_dict(s2v.weights.synthetic_state_dict(cfg, seed=6, device=DEV))
        else:
            m.engine.weight_arena().copy_(src.weight_arena())
            m.engine.mark_weights_loaded()
        e = m.engine
        if shard:
            e.set_shard(*shard)
        e.set_geometry(2, T, F, H, W)
        e.prepare_tables(H * 8, W * 8)
        e.set_conditioning(text, ref)
        return e

    print(f"workload {a.workload}: {cfg.num_layers} layers, {cfg.num_attention_heads} heads, D = {D}, N = {N} tokens per sample, B = 2, bf16, DDIM step")
    e1 = build()
    lat = lat0.clone()
    e1.denoise_step(lat, float(t), coef)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms1 = []
    for _ in range(a.iters):
        lat.copy_(lat0)
        ev[0].record()
        e1.denoise_step(lat, float(t), coef)
        ev[1].record()
        torch.cuda.synchronize()
        ms1.append(ev[0].elapsed_time(ev[1]))
    single = min(ms1)
    ref_lat = lat.clone()
    prof1, _ = profile(e1, lambda: e1.denoise_step(lat.copy_(lat0), float(t), coef))
    print(f"single engine B = 2 step: {single:.1f} ms (min of {a.iters}: {', '.join(f'{x:.1f}' for x in ms1)})")
    print("  by class (ms): " + ", ".join(f"{c} {m:.1f}" for c, m in zip(CLASSES, prof1)))

    for p in a.p:
        engs = [build((p, r), e1) for r in range(p)]
        loc = s2v.dist.UlyssesLocal(engs)
        lay = engs[0].shard_layout()
        lats = [lat0.clone() for _ in range(p)]
        loc.step(lats, float(t), coef)  # warm-up; also the bitwise check against the single engine
        torch.cuda.synchronize()
        same = all(torch.equal(x, ref_lat) for x in lats)
        # timed lockstep: events around every rank's segment, exchanges (device copies) between them
        best = None
        for _ in range(a.iters):
            for x in lats:
                x.copy_(lat0)
            seg = [[] for _ in range(p)]

            def timed(r, fn):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = fn()
                e.record()
                seg[r].append((s, e))
                return out

            pend = [timed(r, lambda r=r: engs[r].shard_step_begin(lats[r], float(t), coef)) for r in range(p)]
            while True:
                loc.exchange(pend[0])
                if pend[0] == s2v._lib.SHARD_NOISE_GATHER:
                    break
                pend = [timed(r, lambda r=r: engs[r].shard_step_resume()) for r in range(p)]
            for r in range(p):
                timed(r, lambda r=r: engs[r].shard_step_end(lats[r]))
            torch.cuda.synchronize()
            comp = [sum(s.elapsed_time(e) for s, e in seg[r]) for r in range(p)]
            if best is None or max(comp) < max(best):
                best = comp
        for x in lats:
            x.copy_(lat0)
        for r in range(p):
            s2v._lib.check(s2v.lib().s2v_profile_enable(engs[r]._h, 1))
        loc.step(lats, float(t), coef)
        profs = []
        for r in range(p):
            ms = (ctypes.c_float * 9)()
            cnt = (ctypes.c_int32 * 9)()
            s2v._lib.check(s2v.lib().s2v_profile_read(engs[r]._h, ms, cnt, 9))
            s2v._lib.check(s2v.lib().s2v_profile_enable(engs[r]._h, 0))
            profs.append(list(ms))
        # bytes: per rank and per block, packs / unpacks move (read + write) these; the all-to-all sends (p - 1) / p of each chunk set
        L = cfg.num_layers
        print(f"\np = {p}: shard layout (T_r, R_r, V_r) = {lay}; lockstep latents bitwise equal to the single engine: {same}")
        worst = max(range(p), key=lambda r: best[r])
        for r in range(p):
            Tr, Rr, Vr = lay[r]
            Mr = 2 * (Tr + Rr + Vr)
            qkv_b = Mr * 3 * D * E                  # local QKV of the rank
            qkvh_b = 2 * N * 3 * (D // p) * E       # head-sharded QKV of all rows
            o_b = 2 * N * (D // p) * E              # head-sharded attention output
            xn_b = Mr * D * E
            moved = 2 * L * (qkv_b + qkvh_b + o_b + xn_b)
            pk = profs[r][8]
            sent_qkv = qkv_b * (p - 1) / p
            sent_o = o_b * (p - 1) / p
            print(f"  rank {r}: compute {best[r]:.1f} ms (excl. exchanges) = {best[r] / single:.3f} x single; pack/unpack {pk:.2f} ms for "
                  f"{moved / 1e9:.2f} GB moved = {moved / pk / 1e6 if pk > 0 else 0:.0f} GB/s")
            print(f"          all-to-all bytes sent per block: QKV {sent_qkv / 1e6:.1f} MB, O {sent_o / 1e6:.1f} MB; per step "
                  f"{L * (sent_qkv + sent_o) / 1e9:.2f} GB (+ noise gather {(p - 1) * 2 * (-(-(F * (H // 2) * (W // 2)) // p)) * cfg.out_channels * 4 * E / 1e6:.1f} MB)")
            print("          by class (ms): " + ", ".join(f"{c} {m:.1f}" for c, m in zip(CLASSES, profs[r])))
        Tr, Rr, Vr = lay[worst]
        Mr = 2 * (Tr + Rr + Vr)
        per_step = cfg.num_layers * (Mr * 3 * D * E + 2 * N * (D // p) * E) * (p - 1) / p
        link_ms = per_step / ((p - 1) * LINK_GBPS * 1e9) * 1e3
        print(f"  max-over-ranks compute {best[worst]:.1f} ms = {best[worst] / single:.3f} x the single-engine step "
              f"(target {'0.28' if p == 4 else '0.53' if p == 2 else '-'})")
        print(f"  link-bound exchange at an ASSUMED, UNMEASURED {LINK_GBPS:.0f} GB/s per xGMI link ((p - 1) links per rank): {link_ms:.1f} ms per step")
        print(f"  PROJECTION (not measured on {p} GPUs): p = {p} step ~ {best[worst] + link_ms:.1f} ms against {single:.1f} ms "
              f"({single / (best[worst] + link_ms):.2f}x) if the exchanges do not overlap compute")
        for e in engs:
            e.close()
        del engs, loc
        torch.cuda.empty_cache()
    e1.close()


if __name__ == "__main__":
    main()
