"""Digest what the host side of the library (csrc/api.hip) decides, for comparing two builds of it byte for byte.

    S2V_LIB=<build A>/libs2v_hip.so python tools/engine_digest.py > a.txt
    S2V_LIB=<build B>/libs2v_hip.so python tools/engine_digest.py > b.txt;  diff a.txt b.txt

One `name sha256` line per case, all on the tiny model of tests/test_gpu_lora_runtime_fp8.py (D = 256, two layers, B = 2, F = 3, 16 x 24 latent,
T = 7: M is ragged, the MX forms and all three adapter slots of the QKV are live):
  layout    every slot's (offset, rows, cols, ld) and s2v_device_bytes of four kinds of context;
  engine    forward() per dtype and weight format, per runtime-adapter configuration before attach / attached / rescaled / detached, and
            one captured denoise_step in bf16 and in fp8;
  operator  the s2v_op_*fp8* entry points and s2v_op_linear_lora at the smallest shapes their checks admit (adapter forms: scratch as well).
A refactor of the arena layout or of the launch sequences must leave the two outputs equal."""
import ctypes
import hashlib
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV, BF = "cuda:0", torch.bfloat16
GEO = dict(B=2, F=3, C=16, H=16, W=24, T=7)


def say(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t if isinstance(t, bytes) else t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    print(f"{name} {h.hexdigest()}", flush=True)


def main():
    s2v = importlib.import_module("disentangled-subject-to-vid_amd")
    L = s2v._lib
    print(f"library under test: {L.LIB_PATH}", file=sys.stderr)

    def cfg_of(fmt=None, rank=0):
        cfg = s2v.tiny(use_rope=True, heads=4, layers=2, text_dim=128, temb=64)
        cfg.max_text_seq_length = GEO["T"]
        cfg.weight_format, cfg.lora_runtime_rank, cfg.lora_runtime_fp8 = fmt, rank, bool(fmt and rank)
        return cfg

    # ---- layout
    for name, fmt, rank, kind in (("bf16", None, 0, L.CTX_MODEL), ("bf16_r8", None, 8, L.CTX_MODEL), ("fp8_r8", "fp8", 8, L.CTX_MODEL),
                                  ("attn_weights_r8", None, 8, L.CTX_ATTN_WEIGHTS)):
        e = s2v.S2VEngine(cfg_of(fmt, rank), BF, DEV, kind=kind)
        rows = []
        off, r, c, ld = (ctypes.c_int64() for _ in range(4))
        for k in s2v.weights.state_dict_shapes(cfg_of()):
            rc = L.lib().s2v_weight_slot(e._h, k.encode(), ctypes.byref(off), ctypes.byref(r), ctypes.byref(c), ctypes.byref(ld))
            rows.append(f"{k} {(off.value, r.value, c.value, ld.value) if rc == 0 else None}")
        if kind == L.CTX_MODEL:
            e.set_geometry(GEO["B"], GEO["T"], GEO["F"], GEO["H"], GEO["W"])
        say(f"layout {name}", "\n".join(rows + [str(e.device_bytes())]).encode())
        e.close()

    # ---- engine
    g = torch.Generator().manual_seed(17)
    sd = s2v.weights.synthetic_state_dict(cfg_of(), seed=5, parity=True)
    lora = s2v.weights.synthetic_lora(cfg_of(), rank=8, seed=6, std=0.05)
    lat = torch.randn(GEO["B"], GEO["F"], GEO["C"], GEO["H"], GEO["W"], generator=g).to(BF).to(DEV)
    text = torch.randn(GEO["B"], GEO["T"], 128, generator=g).to(BF)
    ref = (torch.randn(1, 1, GEO["C"], GEO["H"], GEO["W"], generator=g) * 0.7).to(BF)
    hidden = torch.randn(GEO["B"], GEO["F"] * 8 * 12, 256, generator=g).to(BF)
    encoder = torch.randn(GEO["B"], GEO["T"] + 8 * 12, 256, generator=g).to(BF)
    ts = torch.tensor([500.0] * GEO["B"])

    def ready(cfg, dtype=BF):
        e = s2v.S2VEngine(cfg, dtype, DEV)
        e.load_state_dict(sd)
        e.set_geometry(GEO["B"], GEO["T"], GEO["F"], GEO["H"], GEO["W"])
        e.prepare_tables(GEO["H"] * 8, GEO["W"] * 8)
        e.set_conditioning(text, ref)
        return e

    def through_adapter_states(name, e, run):
        lo = lora if e.kind == L.CTX_MODEL else {k: v for k, v in lora.items() if ".attn1." in k}
        for state, change in (("base", None), ("attached", lambda: e.attach_lora(lo, 0.5)), ("rescaled", lambda: e.set_lora_scale(0.25)),
                              ("detached", e.detach_lora)):
            if change:
                change()
            say(f"engine {name} {state}", *run())
            torch.cuda.synchronize()

    for name, dtype, fmt in (("bf16", BF, None), ("fp16", torch.float16, None), ("fp32", torch.float32, None), ("fp8", BF, "fp8"),
                             ("fp8-qk", BF, "fp8-qk"), ("fp8-auto", BF, "fp8-auto")):
        e = ready(cfg_of(fmt), dtype)
        say(f"engine {name} forward", e.forward(lat, ts))
        if name in ("bf16", "fp8"):
            sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0)
            sch.set_timesteps(4)
            x = lat[:1].contiguous().clone()
            e.denoise_step(x, float(sch.timesteps[0]), sch.coef(sch.timesteps[0], BF, 6.0), use_graph=True)
            say(f"engine {name} captured denoise_step", x)
        e.close()
    for name, fmt in (("bf16_r8", None), ("fp8_r8", "fp8")):
        e = ready(cfg_of(fmt, 8))
        through_adapter_states(name, e, lambda: [e.forward(lat, ts)])
        e.close()
    ws = s2v.S2VEngine(cfg_of(None, 8), BF, DEV, kind=L.CTX_ATTN_WORKSPACE)
    ws.set_geometry(GEO["B"], GEO["T"], GEO["F"], GEO["H"], GEO["W"])
    ws.prepare_tables(GEO["H"] * 8, GEO["W"] * 8)
    we = s2v.S2VEngine(cfg_of(None, 8), BF, DEV, kind=L.CTX_ATTN_WEIGHTS)
    for k, v in sd.items():
        if ".attn1." in k:
            we.load_weight(k, v)
    we.finalize_weights()
    through_adapter_states("attn_weights_r8", we, lambda: [t for l in (0, 1) for t in ws.attn_forward_with(we, l, hidden, encoder)])
    we.close()
    ws.close()

    # ---- operators
    lib, P, st = L.lib(), L.ptr, L.stream_ptr
    rnd = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(BF).to(DEV)
    M, N, K, r = 256, 256, 128, 8
    x, W, b = rnd(M, K), rnd(N, K, s=K ** -0.5), rnd(N, s=0.1)
    A, B = (torch.randn(r, K, generator=g) * 0.05).to(DEV), (torch.randn(N, r, generator=g) * 0.05).to(DEV)
    for epi in (0, 1):
        C = torch.zeros(M, N, dtype=BF, device=DEV)
        sc = torch.zeros((M * K + N * K + 4 * (M + N) + 255) // 256 * 256 + 2 * 64 * (K + N + M), dtype=torch.uint8, device=DEV)
        L.check(lib.s2v_op_linear_fp8(P(x), P(W), P(b), P(C), M, N, K, epi, P(sc), sc.numel(), st()))
        say(f"operator linear_fp8 epi {epi}", C)
        C.zero_(), sc.zero_()
        L.check(lib.s2v_op_linear_fp8_lora(P(x), P(W), P(b), P(A), P(B), r, 0.5, P(C), M, N, K, epi, P(sc), sc.numel(), st()))
        say(f"operator linear_fp8_lora epi {epi}", C)
        say(f"operator linear_fp8_lora epi {epi} scratch", sc)
    C = torch.zeros(M, N, dtype=BF, device=DEV)
    L.check(lib.s2v_op_linear_lora(P(x), P(W), P(b), P(A), P(B), r, 0.5, P(C), M, N, K, 0, None, None, L.DTYPE_BF16, st()))
    say("operator linear_lora epi 0", C)
    D = F = 256
    x, w1, b1, w2, b2 = rnd(M, D), rnd(F, D, s=D ** -0.5), rnd(F, s=0.1), rnd(D, F, s=F ** -0.5), rnd(D, s=0.1)
    ab = [(torch.randn(*s, generator=g) * 0.05).to(DEV) for s in ((r, D), (F, r), (r, F), (D, r))]
    for mx in (1, 0):
        out = torch.zeros(M, D, dtype=BF, device=DEV)
        L.check(lib.s2v_op_ff_fp8(P(x), P(w1), P(b1), P(w2), P(b2), P(out), M, D, F, mx, st()))
        say(f"operator ff_fp8 mx {mx}", out)
        out.zero_()
        sc = torch.zeros(4 * M * F + M * D + 2 * D * F + 2 * 64 * (2 * M + 2 * D + 2 * F) + 8 * M + 4 * (D + F) + 8192, dtype=torch.uint8, device=DEV)
        L.check(lib.s2v_op_ff_fp8_lora(P(x), P(w1), P(b1), P(w2), P(b2), *(P(t) for t in ab), r, 0.5, P(out), M, D, F, mx, P(sc), sc.numel(), st()))
        say(f"operator ff_fp8_lora mx {mx}", out)
        say(f"operator ff_fp8_lora mx {mx} scratch", sc)


if __name__ == "__main__":
    main()
