"""Ulysses sequence parallelism on ONE GPU: what p GPUs would do per step, measured rank by rank.

Builds the single engine and p shard contexts (s2v_set_shard) of the full model in one process, runs the in-process lockstep step
(dist.UlyssesLocal: the exchanges are device copies) and times with HIP events on the launch stream:
  * per rank: compute ms, excluding the exchanges (events around each rank's begin / resume / end segments; the packs and unpacks are inside);
  * pack / unpack ms and their effective GB/s (bytes read + written; s2v_profile_read class 8);
  * bytes per all-to-all per rank and per step (dist.shard_exchange_bytes, what s2v_shard_buffers reports; the fp8 weight formats carry the
    attention output as MX e4m3, set against the bf16 exchange of the same geometry), and a link-bound exchange time at an ASSUMED, UNMEASURED
    153 GB/s per xGMI link (bench.py's constant) -- each rank sends every chunk but its own, one link per peer;
  * the single engine's B = 2 step in the same process, and the per-kernel-class breakdown of both.
The p-GPU step time printed is a PROJECTION: max-over-ranks compute + the link-bound exchange time; no multi-GPU node has run it.

python tools/ulysses_projection.py --workload cogvideox-5b-49x480x720 --p 2 4
python tools/ulysses_projection.py --workload cogvideox-5b-fp8-49x720x1280 --p 2 4        (BASELINE configs[4]; -fp8auto-: the fp8-auto preset)
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
WORKLOADS = {"cogvideox-5b-49x480x720": (s2v.cogvideox_5b, 226, 13, 60, 90),
             # BASELINE configs[4] (49 x 720 x 1280, N = 50 626): fp8 linears, and the fp8-auto preset (+ fp8 QK^T at that length, fp16 P)
             "cogvideox-5b-fp8-49x720x1280": (s2v.config.cogvideox_5b_fp8, 226, 13, 90, 160),
             "cogvideox-5b-fp8auto-49x720x1280": (s2v.config.cogvideox_5b_fp8_auto, 226, 13, 90, 160)}
# max-over-ranks compute against the single-engine step: the C3 targets, and for configs[4] an ESTIMATE (the C3 figure with attention a larger share)
TARGETS = {"cogvideox-5b-49x480x720": {2: "0.53", 4: "0.28"}, "cogvideox-5b-fp8-49x720x1280": {4: "<= 0.29, an estimate"},
           "cogvideox-5b-fp8auto-49x720x1280": {4: "<= 0.29, an estimate"}}
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
    R, V = (H // 2) * (W // 2), F * (H // 2) * (W // 2)
    mx = cfg.weight_format is not None  # the fp8 formats: O exchange as MX e4m3 (D/p + D/(32p) bytes per row)

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

    fmt = f"weight_format {cfg.weight_format!r}, attn_p_format {cfg.attn_p_format!r}" if mx else "bf16"
    print(f"workload {a.workload}: {cfg.num_layers} layers, {cfg.num_attention_heads} heads, D = {D}, N = {N} tokens per sample, B = 2, {fmt}, DDIM step")
    e1 = build()
    if mx:
        print(f"  fp8 QK^T active on the single engine: {e1.fp8_qk_active}")
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
        # bytes: per rank and per block, packs / unpacks move (read + write) these; the all-to-all sends every chunk but the rank's own
        L = cfg.num_layers
        print(f"\np = {p}: shard layout (T_r, R_r, V_r) = {lay}; lockstep latents bitwise equal to the single engine: {same}")
        if mx:
            print(f"  fp8 QK^T active on the shards: {[e.fp8_qk_active for e in engs]}")
        worst = max(range(p), key=lambda r: best[r])

        def sent(x, kind, r):  # bytes rank r puts on links: every chunk but its own
            return sum(x[kind][0]) - x[kind][0][r]

        per_step = [0.0] * p
        for r in range(p):
            Tr, Rr, Vr = lay[r]
            Mr = 2 * (Tr + Rr + Vr)
            ob = 1 + 1 / 32 if mx else E            # bytes per element of the attention output as exchanged (MX: e4m3 + one scale byte per 32)
            qkv_b = Mr * 3 * D * E                  # local QKV of the rank
            qkvh_b = 2 * N * 3 * (D // p) * E       # head-sharded QKV of all rows
            o_b = 2 * N * (D // p) * ob             # head-sharded attention output
            xn_b = Mr * D * ob
            moved = 2 * L * (qkv_b + qkvh_b + o_b + xn_b)
            pk = profs[r][8]
            xb = s2v.dist.shard_exchange_bytes(2, T, R, V, p, r, D, E, cfg.out_channels, mx=mx)
            x16 = s2v.dist.shard_exchange_bytes(2, T, R, V, p, r, D, E, cfg.out_channels, mx=False)
            sent_qkv, sent_o, sent_n = sent(xb, 1, r), sent(xb, 2, r), xb[3][0][0] * (p - 1)
            per_step[r] = L * (sent_qkv + sent_o) + sent_n
            print(f"  rank {r}: compute {best[r]:.1f} ms (excl. exchanges) = {best[r] / single:.3f} x single; pack/unpack {pk:.2f} ms for "
                  f"{moved / 1e9:.2f} GB moved = {moved / pk / 1e6 if pk > 0 else 0:.0f} GB/s")
            print(f"          all-to-all bytes sent per block: QKV {sent_qkv / 1e6:.1f} MB, O {sent_o / 1e6:.1f} MB"
                  + (f" (bf16 O at this geometry: {sent(x16, 2, r) / 1e6:.1f} MB)" if mx else "")
                  + f"; per step {per_step[r] / 1e9:.2f} GB" + (f" (bf16 exchange: {(L * (sent(x16, 1, r) + sent(x16, 2, r)) + sent_n) / 1e9:.2f} GB)" if mx else "")
                  + f" incl. the noise gather {sent_n / 1e6:.1f} MB")
            print("          by class (ms): " + ", ".join(f"{c} {m:.1f}" for c, m in zip(CLASSES, profs[r])))
        link_ms = max(per_step) / ((p - 1) * LINK_GBPS * 1e9) * 1e3
        print(f"  max-over-ranks compute {best[worst]:.1f} ms = {best[worst] / single:.3f} x the single-engine step "
              f"(target {TARGETS.get(a.workload, {}).get(p, '-')})")
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
