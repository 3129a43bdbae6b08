"""Memory and per-call time of the model-wide AttnProcessor (profiles/r10_attn_processor_model.txt).

    python tools/attn_processor_model_probe.py

1. memory: HipCogVideoXAttnProcessor2_0 installed on 42 Attention modules at 5B width (48 heads, D = 3072, bf16, seeded weights), each
   module run once at C3 (49 x 480 x 720: B = 2, N = 19 126) and at configs[4] (49 x 720 x 1280: N = 50 626): the library's own bytes
   (s2v_device_bytes through memory_bytes()) and the device-wide growth (torch.cuda.mem_get_info), with the figures a one-layer engine
   per module (the seam before the pool) would hold, computed from one such engine's s2v_device_bytes;
2. time: one module at C3 through the processor against a stand-alone one-layer S2VEngine with the same weights (s2v_attn_forward),
   interleaved rounds, host clock around work that ends in a device synchronise; the outputs are compared bit for bit."""
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
s2v = importlib.import_module("disentangled-subject-to-vid_amd")
from oracle import transformer_ref as tr  # noqa: E402

DEV, HEADS, D, NMOD = "cuda:0", 48, 3072, 42
P = "transformer_blocks.0.attn1."
GEOS = {"C3": (2, 226, 13, 60, 90), "configs[4]": (2, 226, 13, 90, 160)}


class Lin:
    def __init__(self, w, b):
        self.weight, self.bias = w, b


class Attn:
    heads = HEADS
    is_cross_attention = False

    def __init__(self, sd):
        self.to_q, self.to_k, self.to_v = (Lin(sd[n + ".weight"], sd[n + ".bias"]) for n in ("to_q", "to_k", "to_v"))
        self.to_out = [Lin(sd["to_out.0.weight"], sd["to_out.0.bias"])]
        self.norm_q, self.norm_k = (Lin(sd[n + ".weight"], sd[n + ".bias"]) for n in ("norm_q", "norm_k"))


def weights(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    sd = {}
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        sd[n + ".weight"] = (torch.randn(D, D, generator=g, device=DEV) * (0.7 / D**0.5)).bfloat16()
        sd[n + ".bias"] = (0.1 * torch.randn(D, generator=g, device=DEV)).bfloat16()
    for n in ("norm_q", "norm_k"):
        sd[n + ".weight"] = (1 + 0.2 * torch.randn(64, generator=g, device=DEV)).bfloat16()
        sd[n + ".bias"] = (0.1 * torch.randn(64, generator=g, device=DEV)).bfloat16()
    return sd


def inputs(geo):
    B, T, F, H, W = geo
    R = (H // 2) * (W // 2)
    g = torch.Generator(device=DEV).manual_seed(7)
    (rc, rs), (vc, vs) = tr.pipeline_rope(H * 8, W * 8, F)
    return dict(hidden_states=torch.randn(B, F * R, D, generator=g, device=DEV).bfloat16(),
                encoder_hidden_states=torch.randn(B, T + R, D, generator=g, device=DEV).bfloat16(), image_rotary_emb=(vc.to(DEV), vs.to(DEV)),
                ref_img_seq_start=T, ref_img_seq_end=T + R, embed_ref_img=True, ref_image_rotary_emb=(rc.to(DEV), rs.to(DEV)))


def standalone(sd):
    cfg = s2v.TransformerConfig(num_layers=1, num_attention_heads=HEADS, time_embed_dim=8, text_embed_dim=64, use_rotary_positional_embeddings=True)
    eng = s2v.S2VEngine(cfg, torch.bfloat16, DEV)
    for k, v in sd.items():
        eng.load_weight(P + k, v)
    torch.cuda.synchronize()
    eng.mark_weights_loaded()
    return eng


def memory(tag, geo):
    Proc = s2v.HipCogVideoXAttnProcessor2_0
    Proc.release_pools()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    mods = [Attn(weights(300 + i)) for i in range(NMOD)]
    kw = inputs(geo)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    proc = Proc()
    t0 = time.perf_counter()
    for m in mods:
        oh, oe = proc(m, **kw)
        del oh, oe
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    grown = free0 - torch.cuda.mem_get_info()[0]
    mem = proc.memory_bytes()
    print(f"{tag}: {NMOD} modules, first call of each (weights packed + geometry carved once) {wall:.2f} s")
    print(f"{tag}: library weights {mem['weights'] / 1e9:.3f} GB ({mem['weights'] / NMOD / 1e6:.2f} MB per module), "
          f"workspace {mem['workspace'] / 1e9:.3f} GB (one), total {(mem['weights'] + mem['workspace']) / 1e9:.3f} GB")
    print(f"{tag}: device-wide growth (torch.cuda.mem_get_info) {grown / 1e9:.3f} GB")
    Proc.release_pools()
    del mods, kw
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def per_module_engine_bytes(geo):
    eng = standalone(weights(1))
    eng.set_geometry(*geo)
    a, w = eng.device_bytes()
    eng.close()
    torch.cuda.empty_cache()
    return a, w


def timing(rounds=5, iters=20):
    Proc = s2v.HipCogVideoXAttnProcessor2_0
    Proc.release_pools()
    sd = weights(42)
    attn, kw = Attn(sd), inputs(GEOS["C3"])
    proc = Proc()
    eng = standalone(sd)
    (vc, vs), (rc, rs) = kw["image_rotary_emb"], kw["ref_image_rotary_emb"]
    B, V, _ = kw["hidden_states"].shape
    R = kw["ref_img_seq_end"] - kw["ref_img_seq_start"]
    eng.set_geometry(B, kw["ref_img_seq_start"], V // R, 2, 2 * R)
    eng.set_rope(torch.cat([rc, vc]), torch.cat([rs, vs]))
    a = proc(attn, **kw)
    b = eng.attn_forward(0, kw["hidden_states"], kw["encoder_hidden_states"])
    torch.cuda.synchronize()
    same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    tp, te = [], []
    for _ in range(rounds):
        for fn, acc in ((lambda: proc(attn, **kw), tp), (lambda: eng.attn_forward(0, kw["hidden_states"], kw["encoder_hidden_states"]), te)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / iters * 1e3)
    pool = proc.pools()[0]
    t0 = time.perf_counter()
    for _ in range(1000):
        pool.weights_for(attn)
    check_us = (time.perf_counter() - t0) / 1000 * 1e6
    print(f"C3 per call, one module, {rounds} interleaved rounds x {iters} calls (ms): processor "
          + " ".join(f"{x:.3f}" for x in tp) + f" (median {sorted(tp)[rounds // 2]:.3f}); stand-alone engine "
          + " ".join(f"{x:.3f}" for x in te) + f" (median {sorted(te)[rounds // 2]:.3f})")
    print(f"C3 outputs processor vs stand-alone engine bit-identical: {same}")
    print(f"weights-slot key check (host, no device sync): {check_us:.1f} us per call")
    eng.close()
    Proc.release_pools()


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    for tag, geo in GEOS.items():
        a, w = per_module_engine_bytes(geo)
        print(f"{tag}: a one-layer engine per module (the seam before the pool): arena {a / 1e6:.1f} MB + workspace {w / 1e9:.3f} GB; "
              f"x {NMOD} = {NMOD * (a + w) / 1e9:.1f} GB")
    for tag, geo in GEOS.items():
        memory(tag, geo)
    timing()
