"""Runtime LoRA beside e4m3 weights on the GPU (pytest -m gpu; TransformerConfig.lora_runtime_fp8, include/s2v_hip.h S2V_LORA_FP8_BRANCH):
a 16-bit adapter branch beside the quantised base of the fp8 engines, attached, rescaled, swapped and removed after finalize_weights.

Contract (tests/lora_fp8_emu.py restates it in torch):
    y = epilogue((q_a . q_w^T) * a_scale[m] * w_scale[n] + T . Bs^T + bias),  T = rnd16(x^ . A^T),  Bs = rnd16(s * B)
Bars: 4e-3 rel-L2 against the emulation -- tests/test_gpu_fp8.py's bar for "bf16 output rounding + accumulation order only"; FP8_ENGINE_BAR
(1.4e-2) for an fp8 engine against the bf16 engine, here with the same adapter attached to both -- the branch adds no quantisation.  Adapter
fidelity: the branch must keep the adapter's effect on the output at least four times better than the adapter merged before the
quantisation (the emulation gives 0.047 against 0.71, tests/test_lora_runtime_fp8_cpu.py).  Everything else is BITWISE."""
import copy

import numpy as np
import pytest
import torch

import lora_fp8_emu as E
from conftest import load_golden, weights_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
FP8_ENGINE_BAR = 1.4e-2   # tests/test_gpu_fp8.py: an fp8 engine against the bf16 engine
EMU_BAR = 4e-3            # tests/test_gpu_fp8.py: bf16 output rounding + accumulation order only


def _scratch(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device=DEV)


def op_linear_fp8(s2v, x, W, b, epi):
    L = s2v._lib
    M, K = x.shape
    N = W.shape[0]
    C = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    need = M * K + N * K + 4 * (M + N)
    sc = _scratch(need)
    L.check(L.lib().s2v_op_linear_fp8(L.ptr(x), L.ptr(W), L.ptr(b), L.ptr(C), M, N, K, epi, L.ptr(sc), need, L.stream_ptr()))
    torch.cuda.synchronize()
    return C


def op_linear_fp8_lora(s2v, x, W, b, A, B, s, epi):
    L = s2v._lib
    M, K = x.shape
    N, r = B.shape
    R = (r + 63) // 64 * 64
    C = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    need = (M * K + N * K + 4 * (M + N) + 255) // 256 * 256 + 2 * R * (K + N + M)
    sc = _scratch(need)
    A, B = A.float().contiguous(), B.float().contiguous()
    L.check(L.lib().s2v_op_linear_fp8_lora(L.ptr(x), L.ptr(W), L.ptr(b), L.ptr(A), L.ptr(B), r, float(s), L.ptr(C), M, N, K, epi, L.ptr(sc), need,
                                           L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isfinite(C.float()).all()
    return C


# ------------------------------------------------------------------------------------------------ operator level
# (256, 256, 128, 8): the fallback kernel (K < 512) and rank padding; (256, 256, 512, 8): the smallest gemm_g4f launch; (512, 768, 3072, 128):
# many K-tiles, several tiles in N, the full rank
@pytest.mark.parametrize("epi", [0, 1], ids=["bias", "gelu"])
@pytest.mark.parametrize("shape", [(256, 256, 128, 8), (256, 256, 512, 8), (512, 768, 3072, 128)], ids=lambda s: "x".join(map(str, s)))
def test_op_linear_fp8_lora_contract_fidelity_and_zero_adapter(s2v, shape, epi):
    M, N, K, r = shape
    x, W, b, A, B, s = E.linear_case(M, N, K, r, device=DEV)
    y = op_linear_fp8_lora(s2v, x, W, b, A, B, s, epi).float()
    # 1. the contract
    emu = E.emu_linear(x, W, b, A, B, s, epi)
    rel = E.rel_l2(y, emu)
    print(f"MEASURED op_linear_fp8_lora {shape} epi {epi}: rel-l2 to the emulation {rel:.3e}")
    assert rel <= EMU_BAR, rel
    # 3. scale 0 and a zero B give the bytes of s2v_op_linear_fp8
    y_fp8 = op_linear_fp8(s2v, x, W, b, epi)
    y_base = op_linear_fp8_lora(s2v, x, W, b, A, B, 0.0, epi)
    assert torch.equal(y_base, y_fp8), "scale 0 differs from s2v_op_linear_fp8"
    assert torch.equal(op_linear_fp8_lora(s2v, x, W, b, A, torch.zeros_like(B), s, epi), y_fp8), "B = 0 differs from s2v_op_linear_fp8"
    # 2. adapter fidelity: the adapter's effect on the output against its fp64 value, branch vs merged-then-quantised
    truth = E.true_delta(x, W, b, A, B, s, epi)
    err_branch = E.rel_l2(y - y_base.float(), truth)
    y_merged = op_linear_fp8(s2v, x, E.merged_weight(W, A, B, s), b, epi)
    err_merged = E.rel_l2(y_merged.float() - y_fp8.float(), truth)
    print(f"MEASURED op_linear_fp8_lora {shape} epi {epi}: adapter effect rel-l2 branch {err_branch:.3f}, merged-then-quantised {err_merged:.3f}")
    assert err_branch <= err_merged / 4, (err_branch, err_merged)


# ------------------------------------------------------------------------------------------------ FF pair
@pytest.mark.parametrize("mx", [1, 0], ids=["mx", "rowq"])
@pytest.mark.parametrize("rank", [8, 128])
def test_op_ff_fp8_lora_matches_emulation_and_t_of_ff2(s2v, rank, mx):
    """M = 256, D = 256, F = 1024: FF1 (K = 256) runs the fallback kernel with the MX output epilogue, FF2 (K = 1024) gemm_g4f's MX form.
    With mx the T of FF2 is held, on its own, to rnd16(x^ . A^T) computed from the image bytes and block scales the operator left in its
    scratch: a wrong row permutation or scale byte order moves whole blocks by powers of two.  Tolerance per element: one bf16 ulp of the
    reference plus the fp32 accumulation slack sqrt(K) * 2^-23 * sum_k |x^_k A_k| (the order of the K = 1024 sum is the kernel's own)."""
    L = s2v._lib
    M, D, F = 256, 256, 1024
    c = E.ff_case(M, D, F, rank, device=DEV)
    x, w1, b1, w2, b2, A1, B1, A2, B2, s = c
    R = (rank + 63) // 64 * 64
    need = 4 * M * F + M * D + 2 * D * F + 2 * R * (2 * M + 2 * D + 2 * F) + 8 * M + 4 * (D + F) + 8192
    sc = _scratch(need)
    out = torch.full((M, D), float("nan"), dtype=BF, device=DEV)
    f32 = [t.float().contiguous() for t in (A1, B1, A2, B2)]
    L.check(L.lib().s2v_op_ff_fp8_lora(L.ptr(x), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), *(L.ptr(t) for t in f32), rank, float(s), L.ptr(out),
                                       M, D, F, mx, L.ptr(sc), need, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    emu, h, T2 = E.emu_ff(*c, mx)
    rel = E.rel_l2(out.float(), emu)
    print(f"MEASURED op_ff_fp8_lora rank {rank} mx {mx}: rel-l2 to the emulation {rel:.3e}")
    assert rel <= EMU_BAR, rel
    # the adapters matter: the pair without them is further away than the bar
    emu0, _, _ = E.emu_ff(x, w1, b1, w2, b2, A1, B1, A2, B2, 0.0, mx)
    assert E.rel_l2(emu0, emu) > 2 * EMU_BAR
    if mx:
        xhat, t_off = E.decode_mx_image(sc, M, F)
        got = sc[t_off: t_off + M * R * 2].view(BF).view(M, R).float()
        A2b = E.r16(A2)
        ref = E.r16(xhat @ A2b.T)
        slack = (F ** 0.5) * 2.0 ** -23 * (xhat.abs() @ A2b.abs().T)
        bad = (got[:, :rank] - ref).abs() > E.bf16_ulp(ref) + slack
        print(f"MEASURED T of FF2 rank {rank}: max |got - ref| / ulp {((got[:, :rank] - ref).abs() / E.bf16_ulp(ref)).max().item():.2f}, bytes equal "
              f"{(got[:, :rank] == ref).float().mean().item():.4f}")
        assert not bad.any(), f"{int(bad.sum())} elements of T differ from rnd16(x^ . A^T) by more than a bf16 ulp"
        assert (got[:, :rank] == ref).float().mean().item() > 0.9
        assert (got[:, rank:] == 0).all(), "pad columns of T must be zero"


# ------------------------------------------------------------------------------------------------ engine level
GEO = dict(B=2, F=3, C=16, H=16, W=24, T=7)   # tests/test_gpu_lora_runtime.py: ragged M


def tiny_cfg(s2v, fmt, cap=8, on=True):
    cfg = s2v.tiny(use_rope=True, heads=4, layers=2, text_dim=128, temb=64)   # D = 256
    cfg.max_text_seq_length = 7
    cfg.weight_format = fmt
    cfg.lora_runtime_rank = cap
    cfg.lora_runtime_fp8 = bool(on and fmt is not None)
    return cfg


_CASE = {}


def case(s2v):
    """weights, two adapters and inputs, made once and left unchanged"""
    if not _CASE:
        cfg = tiny_cfg(s2v, None)
        g = torch.Generator().manual_seed(17)
        _CASE.update(sd=s2v.weights.synthetic_state_dict(cfg, seed=5, parity=True),
                     LA=s2v.weights.synthetic_lora(cfg, rank=8, seed=6, std=0.05), LB=s2v.weights.synthetic_lora(cfg, rank=4, seed=8, std=0.05),
                     lat=torch.randn(GEO["B"], GEO["F"], GEO["C"], GEO["H"], GEO["W"], generator=g).to(BF).to(DEV),
                     text=torch.randn(GEO["B"], GEO["T"], 128, generator=g).to(BF),
                     ref=(torch.randn(1, 1, GEO["C"], GEO["H"], GEO["W"], generator=g) * 0.7).to(BF))
    return _CASE


def ready(s2v, cfg, lora=None, scale=0.5, B=2, text=None):
    c = case(s2v)
    m = s2v.HipCogVideoXTransformer3DModel(cfg, BF, DEV)
    m.load_state_dict(c["sd"], lora=lora, lora_scale=scale)
    e = m.engine
    e.set_geometry(B, GEO["T"], GEO["F"], GEO["H"], GEO["W"])
    e.prepare_tables(GEO["H"] * 8, GEO["W"] * 8)
    e.set_conditioning(c["text"] if text is None else text, c["ref"])
    return m, e


def fwd(e, lat, B=2, t=500.0):
    y = e.forward(lat, torch.tensor([t] * B)).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    return y


def bf16_runtime_reference(s2v):
    """the bf16 runtime engine with adapter LA attached: computed once"""
    if "y16" not in _CASE:
        _, e = ready(s2v, tiny_cfg(s2v, None), lora=case(s2v)["LA"])
        _CASE["y16"] = fwd(e, case(s2v)["lat"])
        e.close()
    return _CASE["y16"]


@pytest.mark.parametrize("fmt", ["fp8", "fp8-qk"])
def test_attach_after_finalize_fp8_engine_vs_bf16_runtime_engine(s2v, fmt):
    c = case(s2v)
    y16 = bf16_runtime_reference(s2v)
    m, e = ready(s2v, tiny_cfg(s2v, fmt))
    assert e.lora_state["attached"] == 0
    e.attach_lora(c["LA"], 0.5)      # refused on the parent commit
    st = e.lora_state
    assert st["attached"] == len(c["LA"]) and st["rank"] == 8 and st["scale"] == 0.5
    y8 = fwd(e, c["lat"])
    rel = E.rel_l2(y8, y16)
    e.detach_lora()
    y0 = fwd(e, c["lat"])
    rel0 = E.rel_l2(y0, y8)
    e.close()
    # for the record: the merged-then-quantised engine of today
    _, em = ready(s2v, tiny_cfg(s2v, fmt, cap=0), lora=c["LA"])
    relm = E.rel_l2(fwd(em, c["lat"]), y16)
    em.close()
    print(f"MEASURED {fmt} engine, adapter attached, vs bf16 runtime engine: rel-l2 {rel:.3e} (merged-then-quantised {fmt} engine: {relm:.3e}; "
          f"detached vs attached: {rel0:.3e})")
    assert 0 < rel <= FP8_ENGINE_BAR, rel
    assert rel0 > FP8_ENGINE_BAR, f"the adapter does not matter at this size: detached vs attached {rel0}"


def test_fp8_auto_attaches_and_decides_qk_as_without_the_adapter(s2v):
    c = case(s2v)
    _, e0 = ready(s2v, tiny_cfg(s2v, "fp8-auto", cap=0))
    want = e0.fp8_qk_active
    e0.close()
    _, e = ready(s2v, tiny_cfg(s2v, "fp8-auto"))
    e.attach_lora(c["LA"], 0.5)
    fwd(e, c["lat"])
    assert e.lora_state["attached"] == len(c["LA"])
    assert e.fp8_qk_active == want
    e.close()


def test_detach_rescale_swap_are_bitwise_fp8(s2v):
    c = case(s2v)
    lat = c["lat"]
    _, e_off = ready(s2v, tiny_cfg(s2v, "fp8", cap=0))          # the switch (and the mode) off: today's fp8 engine
    y_off = fwd(e_off, lat)
    e_off.close()
    _, e = ready(s2v, tiny_cfg(s2v, "fp8"))
    assert torch.equal(fwd(e, lat), y_off), "the switch on, nothing attached, differs from the fp8 engine"
    e.attach_lora(c["LA"], 0.5)
    ya = fwd(e, lat)
    assert not torch.equal(ya, y_off)
    e.set_lora_scale(0.25)
    assert e.lora_state["scale"] == 0.25
    ys = fwd(e, lat)
    assert not torch.equal(ys, ya)
    _, e2 = ready(s2v, tiny_cfg(s2v, "fp8"))
    e2.attach_lora(c["LA"], 0.25)
    assert torch.equal(ys, fwd(e2, lat)), "set_lora_scale(0.25) differs from a fresh attach at 0.25"
    e2.close()
    e.attach_lora(c["LB"], 0.5)      # rank 4: nothing of LA's columns 4..7 may survive
    yb = fwd(e, lat)
    assert not torch.equal(yb, ya)
    _, e3 = ready(s2v, tiny_cfg(s2v, "fp8"), lora=c["LB"])     # load_state_dict(lora=...) attaches in runtime mode
    assert e3.lora_state["attached"] == len(c["LB"])
    assert torch.equal(yb, fwd(e3, lat)), "swap to LB differs from a fresh engine loaded with LB"
    e3.close()
    e.attach_lora(c["LA"], 0.5)
    assert torch.equal(fwd(e, lat), ya), "A -> B -> A does not return A's bytes"
    e.detach_lora()
    assert e.lora_state["attached"] == 0
    assert torch.equal(fwd(e, lat), y_off), "detached differs from an fp8 engine created with the switch off"
    e.enable_lora()
    assert torch.equal(fwd(e, lat), ya)
    e.close()


def test_b1_fp8_runtime_engine_is_its_half_of_the_b2_engine_bitwise(s2v):
    c = case(s2v)
    lat1 = c["lat"][:1].contiguous()
    _, e2 = ready(s2v, tiny_cfg(s2v, "fp8"), lora=c["LA"])
    y2 = e2.forward(lat1, torch.tensor([321.0, 321.0]), shared_latent=True).clone()
    for slot in (0, 1):
        _, e1 = ready(s2v, tiny_cfg(s2v, "fp8"), lora=c["LA"], B=1, text=c["text"][slot:slot + 1])
        y1 = e1.forward(lat1, torch.tensor([321.0]), shared_latent=True)
        torch.cuda.synchronize()
        assert torch.isfinite(y1.float()).all()
        assert torch.equal(y1[0], y2[slot]), f"slot {slot}: the B = 1 engine differs from its half of the B = 2 engine"
        e1.close()
    assert not torch.equal(y2[0], y2[1])
    e2.close()


def test_rescale_keeps_the_captured_step_attach_and_detach_drop_it_fp8(s2v):
    c = case(s2v)
    sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0)
    sch.set_timesteps(4)
    ts = sch.timesteps

    def run(use_graph):
        _, e = ready(s2v, tiny_cfg(s2v, "fp8"), lora=c["LA"])
        x = c["lat"][:1].contiguous().clone()
        caps = []
        for i, change in enumerate((None, lambda: e.set_lora_scale(0.25), lambda: e.attach_lora(c["LB"], 0.5), e.detach_lora)):
            if change:
                change()
            e.denoise_step(x, float(ts[i]), sch.coef(ts[i], BF, 6.0), use_graph=use_graph)
            caps.append(e.lora_state["graph_captures"])
        torch.cuda.synchronize()
        e.close()
        return x.clone(), caps

    xe, ce = run(False)
    xg, cg = run(True)
    assert ce == [0, 0, 0, 0]
    assert cg == [1, 1, 2, 3], f"captures {cg}: a rescale must keep the captured step, an attach and a detach must drop it"
    assert torch.isfinite(xg.float()).all()
    assert torch.equal(xg, xe), "graph replay across rescale / attach / detach differs from the eager run"


@pytest.mark.parametrize("sched", ["ddim", "dpm"])
def test_pipeline_fp8_runtime_graph_equals_eager_bitwise(s2v, sched):
    g = load_golden("pipeline_tiny.npz")
    lora = s2v.weights.synthetic_lora(s2v.tiny(use_rope=True, text_dim=64, temb=64), rank=8, seed=21, std=0.05)

    def run(use_graph):
        cfg = s2v.tiny(use_rope=True, text_dim=64, temb=64)    # D = 128
        cfg.max_text_seq_length = 6
        cfg.weight_format, cfg.lora_runtime_rank, cfg.lora_runtime_fp8 = "fp8", 8, True
        m = s2v.HipCogVideoXTransformer3DModel(cfg, BF, DEV)
        m.load_state_dict(weights_of(g), lora=lora, lora_scale=0.5)
        assert m.engine.lora_state["attached"] == len(lora)
        S = s2v.CogVideoXDDIMScheduler if sched == "ddim" else s2v.CogVideoXDPMScheduler
        pipe = s2v.S2VPipeline(m, S(snr_shift_scale=1.0), None)
        t = lambda v: torch.from_numpy(np.asarray(v)).to(BF)
        out = pipe(prompt_embeds=t(g["prompt_embeds"]), negative_prompt_embeds=t(g["negative_prompt_embeds"]), ref_img_states=t(g["ref"]),
                   height=480, width=720, num_frames=5, num_inference_steps=3, guidance_scale=6.0, latents=t(g["latents0"]),
                   return_dict=False, output_type="latent", fused=True, use_graph=use_graph, generator=torch.Generator().manual_seed(1))[0]
        torch.cuda.synchronize()
        caps = m.engine.lora_state["graph_captures"]
        m.engine.close()
        return out.clone(), caps

    eager, c0 = run(False)
    graph, c1 = run(True)
    assert torch.isfinite(eager.float()).all() and c0 == 0 and c1 >= 1
    assert torch.equal(graph, eager), "hipGraph pipeline differs from the eager pipeline on the fp8 runtime engine"


def test_refusals_fp8_branch_leave_the_state(s2v):
    c = case(s2v)
    es = s2v.S2VEngine(tiny_cfg(s2v, "fp8"), BF, DEV)
    with pytest.raises(s2v.S2VError, match="shard"):
        es.set_shard(2, 0)
    es.close()
    _, e = ready(s2v, tiny_cfg(s2v, "fp8"), lora=c["LA"])
    y = fwd(e, c["lat"])
    st = e.lora_state
    big = s2v.weights.synthetic_lora(tiny_cfg(s2v, None), rank=16, seed=7, std=0.05)
    with pytest.raises(s2v.S2VError, match="capacity"):
        e.attach_lora(big, 0.5)
    L = s2v._lib
    A, Bm = torch.zeros(16, 256, device=DEV), torch.zeros(256, 16, device=DEV)
    assert L.lib().s2v_lora_attach(e._h, b"transformer_blocks.0.attn1.to_q.weight", L.ptr(A), L.ptr(Bm), 16, 0.5, L.stream_ptr()) != 0
    assert b"capacity" in L.lib().s2v_last_error()
    assert e.lora_state == st
    assert torch.equal(fwd(e, c["lat"]), y), "a refused attach changed the engine"
    e.close()
    # the flag bit is the only thing above the rank: anything else in reserved[1] is refused at creation
    bad = tiny_cfg(s2v, "fp8", cap=129)
    with pytest.raises(s2v.S2VError, match="lora_runtime_rank"):
        s2v.S2VEngine(bad, BF, DEV)


def test_replica_filled_from_the_arena_runs_the_attached_adapter_fp8(s2v):
    c = case(s2v)
    _, src = ready(s2v, tiny_cfg(s2v, "fp8"), lora=c["LA"])
    y = fwd(src, c["lat"])
    rep = s2v.S2VEngine(tiny_cfg(s2v, "fp8"), BF, DEV)
    rep.weight_arena().copy_(src.weight_arena())
    torch.cuda.synchronize()
    rep.mark_weights_loaded()
    st = rep.lora_state
    assert st["attached"] == len(c["LA"]) and st["rank"] == 8 and st["scale"] == 0.5
    rep.set_geometry(2, GEO["T"], GEO["F"], GEO["H"], GEO["W"])
    rep.prepare_tables(GEO["H"] * 8, GEO["W"] * 8)
    rep.set_conditioning(c["text"], c["ref"])
    assert torch.equal(fwd(rep, c["lat"]), y), "the replica differs from the engine its arena came from"
    rep.detach_lora()
    src.detach_lora()
    assert torch.equal(fwd(rep, c["lat"]), fwd(src, c["lat"]))
    rep.close()
    src.close()


def test_full_width_block_rank128_fp8_vs_bf16_runtime_engine_and_memory(s2v):
    """5B width (D = 3072, 48 heads, RoPE), 19 126 tokens x B = 2, rank 128, one block through the Block seam: the fp8 engine with the branch
    against the bf16 runtime engine with the same adapter (FP8_ENGINE_BAR), and what the switch adds to s2v_device_bytes"""
    F_, H_, W_, T_, B = 13, 60, 90, 226, 2
    from oracle import transformer_ref as tr

    def cfg_of(fmt, on):
        cfg = s2v.cogvideox_5b()
        cfg.num_layers = 1
        cfg.lora_runtime_rank = 128
        cfg.weight_format, cfg.lora_runtime_fp8 = fmt, on
        return cfg

    cfg = cfg_of(None, False)
    D, TE = cfg.inner_dim, cfg.time_embed_dim
    R = (H_ // 2) * (W_ // 2)
    V = F_ * R
    sd = s2v.weights.synthetic_state_dict(cfg, seed=21, device=DEV, parity=True)
    lora = s2v.weights.synthetic_lora(cfg, rank=128, seed=24, device=DEV, std=0.02)
    g = torch.Generator(device=DEV).manual_seed(22)
    h = torch.randn(B, V, D, generator=g, device=DEV).to(BF)
    e0 = torch.randn(B, T_, D, generator=g, device=DEV).to(BF)
    e1 = torch.randn(B, R, D, generator=g, device=DEV).to(BF)
    temb = torch.randn(B, TE, generator=g, device=DEV).to(BF)
    ref_rope, rope = tr.pipeline_rope(H_ * 8, W_ * 8, F_)
    kw = dict(image_rotary_emb=tuple(x.to(DEV) for x in rope), ref_image_rotary_emb=tuple(x.to(DEV) for x in ref_rope))
    outs, mem = {}, {}
    for name, fmt, on, lo in (("bf16", None, False, lora), ("fp8", "fp8", True, lora), ("fp8 base", "fp8", True, None)):
        m = s2v.HipCogVideoXTransformer3DModel(cfg_of(fmt, on), BF, DEV)
        m.load_state_dict(sd, lora=lo, lora_scale=0.5)
        assert m.engine.lora_state["attached"] == (len(lora) if lo else 0)
        got = m.transformer_blocks[0](hidden_states=h, encoder_hidden_states=e0, temb=temb, enc_hidden_states1=e1, embed_ref_img=True,
                                      ref_img_seq_start=T_, ref_img_seq_end=T_ + R, position_delta=0, timestep=None, layer=0, **kw)
        torch.cuda.synchronize()
        outs[name] = [t.clone() for t in got]
        mem[name] = m.engine.device_bytes()
        m.engine.close()
    e_off = s2v.S2VEngine(cfg_of("fp8", False), BF, DEV)
    e_off.set_geometry(B, T_, F_, H_, W_)
    mem["off"] = e_off.device_bytes()
    e_off.close()
    for i, name in enumerate(("video", "text", "ref")):
        y8, y16, yb = outs["fp8"][i], outs["bf16"][i], outs["fp8 base"][i]
        assert torch.isfinite(y8.float()).all()
        rel, relb = E.rel_l2(y8, y16), E.rel_l2(yb, y8)
        print(f"MEASURED 5B block rank 128, fp8 + branch vs bf16 runtime engine, {name}: rel-l2 {rel:.3e} (fp8 without the adapter vs with: {relb:.3e})")
        assert 0 < rel <= FP8_ENGINE_BAR, (name, rel)
        assert relb > 0
    (ar1, ws1), (ar0, ws0) = mem["fp8"], mem["off"]
    # the layout: A stacks 6 R D + Bs arrays (3 D + D + 4 D + D) R + base copies, T [Mpad][3 R]; R = 128, bf16; every carve rounded up to 256 bytes
    Rk, Dp = 128, (D + 255) // 256 * 256
    arena_sum = 2 * (9 * Rk * D + (3 * D + Dp + 4 * D + Dp) * Rk + (2 * 6 * D + 2 * D) * TE + Dp * cfg.in_channels * 4 + Dp * cfg.text_embed_dim) + 256 * 12
    Mpad = (B * (T_ + R + V) + 255) // 256 * 256 + 256
    print(f"MEASURED s2v_device_bytes with the switch on / off: arena {ar1} / {ar0} (+{ar1 - ar0}, derived <= {arena_sum}), "
          f"workspace {ws1} / {ws0} (+{ws1 - ws0}, derived {Mpad * 3 * Rk * 2})")
    assert 0 < ar1 - ar0 <= arena_sum
    assert ws1 - ws0 == Mpad * 3 * Rk * 2
