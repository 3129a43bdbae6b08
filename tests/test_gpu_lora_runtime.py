"""Runtime LoRA on the GPU (pytest -m gpu; include/s2v_hip.h s2v_lora_*, DESIGN sections 1 - 3): the adapter attached AFTER
finalize_weights as a branch beside the base weights, swapped, rescaled and removed without touching a base weight.

Bars: the project's own, restated from tests/test_gpu_parity.py (2 x the worst value measured over that file): bf16 rel-L2 1.3e-2 and
max-abs 2e-2 max|ref|, fp16 1.3e-3 / 2e-3, fp32 max-abs 4e-5.  The oracle runs on merge_lora(sd, lora, s): merged and unmerged are the
same function in exact arithmetic.  Everything else here is BITWISE: swap == fresh load, rescale == fresh attach, detached == an engine
without the mode, hipGraph == eager, B = 1 == its half of B = 2, re-merged small weights == a merged engine's bytes, a replica == its source.

One adapted linear per epilogue kind runs through s2v_op_linear_lora (the attach-time packing, the down-projection kernel and the K-extended
GEMM on the caller's operands): its error against fp64 must not exceed the error of PEFT's own arithmetic, with no margin."""
import numpy as np
import pytest
import torch

from conftest import load_golden, weights_of
from oracle import sched_ref, transformer_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
BARS = {"bf16": (1.3e-2, 2e-2), "f16": (1.3e-3, 2e-3)}
F32_BAR = 4e-5


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def assert_close(got, exp, dt_name, what=""):
    got, exp = got.float().cpu(), exp.float().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - exp).abs().max().item()
    if dt_name == "f32":
        print(f"MEASURED {dt_name} {what}: max-abs {err:.3e}")
        assert err <= F32_BAR, f"{what}: max-abs {err}"
    else:
        r = rel_l2(got, exp)
        br, ba = BARS[dt_name]
        print(f"MEASURED {dt_name} {what}: rel-l2 {r:.3e} max-abs/max|ref| {err / exp.abs().max().item():.3e}")
        assert r <= br and err <= ba * exp.abs().max().item(), f"{what}: rel-l2 {r}, max-abs {err} (max|ref| {exp.abs().max().item()})"


def medium_cfg(s2v, use_rope=True, rank_cap=8, scope="shipped"):
    cfg = s2v.tiny(use_rope=use_rope, heads=3, layers=2, text_dim=128, temb=64)
    cfg.max_text_seq_length = 7
    cfg.lora_runtime_rank = rank_cap
    cfg.lora_adaln_scope = scope
    return cfg


GEO = dict(B=2, F=3, C=16, H=16, W=24, T=7)


def medium_inputs(dt, seed=17):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(GEO["B"], GEO["F"], GEO["C"], GEO["H"], GEO["W"], generator=g).to(dt)
    text = torch.randn(GEO["B"], GEO["T"], 128, generator=g).to(dt)
    ref = (torch.randn(1, 1, GEO["C"], GEO["H"], GEO["W"], generator=g) * 0.7).to(dt)
    return lat, text, ref


def ready_engine(s2v, cfg, dt, sd, text, ref, lora=None, scale=0.5, B=2):
    """a loaded engine at the medium geometry with tables and conditioning set; lora goes through load_state_dict (merge with the mode off,
    attach with it on)"""
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    m.load_state_dict(sd, lora=lora, lora_scale=scale)
    eng = m.engine
    eng.set_geometry(B, GEO["T"], GEO["F"], GEO["H"], GEO["W"])
    eng.prepare_tables(GEO["H"] * 8, GEO["W"] * 8)
    eng.set_conditioning(text, ref)
    return m, eng


def fwd(eng, lat, B=2):
    y = eng.forward(lat, torch.tensor([500.0] * B)).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    return y


# ------------------------------------------------------------------------------------------------ 1. attach after finalize vs the oracle
@pytest.mark.parametrize("dt_name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("use_rope", [True, False])
def test_attach_after_finalize_medium_model_vs_oracle(s2v, dt_name, use_rope):
    """the model of test_medium_model_vs_oracle (heads 3, 2 layers, rank 8, std 0.05), the adapter attached to a FINALIZED runtime-mode engine"""
    dt = DT[dt_name]
    cfg = medium_cfg(s2v, use_rope)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=5, parity=True)
    lora = s2v.weights.synthetic_lora(cfg, rank=8, seed=6, std=0.05)
    lat, text, ref = medium_inputs(dt)
    ts = torch.tensor([500, 500])
    ocfg = dict(num_heads=3, num_layers=2, use_rope=use_rope, norm_eps=1e-5)
    rope = ref_rope = None
    kw = {}
    if use_rope:
        ref_rope, rope = tr.pipeline_rope(GEO["H"] * 8, GEO["W"] * 8, GEO["F"])
        kw = dict(image_rotary_emb=tuple(x.to(DEV) for x in rope), ref_image_rotary_emb=tuple(x.to(DEV) for x in ref_rope))
    merged = tr.merge_lora(sd, lora, 0.5)
    with torch.no_grad():
        exp = tr.transformer_forward({k: v.to(dt) for k, v in merged.items()}, ocfg, lat, text, ref, ts, rope, ref_rope)
        base = tr.transformer_forward({k: v.to(dt) for k, v in sd.items()}, ocfg, lat, text, ref, ts, rope, ref_rope)
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    m.load_state_dict(sd)                      # finalizes the base weights
    assert m.engine.lora_state["attached"] == 0
    m.engine.attach_lora(lora, 0.5)            # the entry point the parent commit does not have
    st = m.engine.lora_state
    assert st["attached"] == len(lora) and st["rank"] == 8 and st["scale"] == 0.5
    call = lambda: m(hidden_states=lat.to(DEV), encoder_hidden_states=text.to(DEV), ref_img_states=ref.to(DEV), timestep=ts.to(DEV),
                     return_dict=False, eval=True, **kw)[0]
    y = call()
    torch.cuda.synchronize()
    assert_close(y, exp, dt_name, "medium transformer, adapter attached")
    # the adapter matters at this size: the base model's output is outside the bar, so a branch that did nothing would fail above
    assert rel_l2(base.float(), exp.float()) > (BARS[dt_name][0] if dt_name != "f32" else 1e-3)
    m.disable_adapters()
    y0 = call()
    torch.cuda.synchronize()
    assert_close(y0, base, dt_name, "medium transformer, adapter detached")
    m.engine.close()


@pytest.mark.parametrize("dt_name", ["f32", "bf16", "f16"])
def test_attach_after_finalize_2b_width_denoise_step_vs_oracle(s2v, dt_name):
    """the geometry of test_cogvideox_2b_width_c1_geometry_vs_oracle (D = 1920, 1250 tokens, 2 layers): one full denoise step with a rank-8
    adapter attached after finalize against the CPU oracle on the merged weights"""
    dt = DT[dt_name]
    cfg = s2v.cogvideox_2b()
    cfg.num_layers = 2
    cfg.lora_runtime_rank = 8
    sd = s2v.weights.synthetic_state_dict(cfg, seed=11, parity=True)
    lora = s2v.weights.synthetic_lora(cfg, rank=8, seed=13, std=0.05)
    g = torch.Generator().manual_seed(12)
    F, H, W, T = 3, 32, 32, 226
    lat = torch.randn(1, F, 16, H, W, generator=g).to(dt)
    text = torch.randn(2, T, 4096, generator=g).to(dt)
    ref = (torch.randn(1, 1, 16, H, W, generator=g) * 0.7).to(dt)
    sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=3.0)
    sch.set_timesteps(10)
    t = sch.timesteps[2]
    ocfg = dict(num_heads=30, num_layers=2, use_rope=False, norm_eps=1e-5)
    merged = tr.merge_lora(sd, lora, 0.5)
    with torch.no_grad():
        npred = tr.transformer_forward({k: v.to(dt) for k, v in merged.items()}, ocfg, torch.cat([lat] * 2), text, ref,
                                       torch.tensor([int(t), int(t)]))
        v = sched_ref.cfg_combine(npred, 6.0)
        exp, _ = sched_ref.ddim_step(sched_ref.alphas_cumprod(3.0), 10, v, int(t), lat)
        exp = exp.to(dt).float()
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    m.load_state_dict(sd)
    eng = m.engine
    eng.set_geometry(2, T, F, H, W)
    eng.prepare_tables(256, 256)
    eng.set_conditioning(text, ref)
    eng.attach_lora(lora, 0.5)   # after the conditioning: the engine recomputes it (text_proj / patch_embed.proj are re-merged)
    x = lat.to(DEV).contiguous().clone()
    eng.denoise_step(x, float(t), sch.coef(t, dt, 6.0))
    torch.cuda.synchronize()
    assert_close(eng.last_noise_pred(), npred, dt_name, "2B noise_pred, adapter attached")
    assert_close(x, exp, dt_name, "2B latents after one step, adapter attached")
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. swap == fresh load, rescale == fresh attach
@pytest.mark.parametrize("dt_name", ["bf16", "f32", "f16"])
def test_swap_rescale_detach_are_bitwise_a_fresh_load(s2v, dt_name):
    dt = DT[dt_name]
    cfg = medium_cfg(s2v, rank_cap=16)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=5, parity=True)
    L1 = s2v.weights.synthetic_lora(cfg, rank=8, seed=6, std=0.05)
    L2 = s2v.weights.synthetic_lora(cfg, rank=16, seed=7, std=0.05)
    lat, text, ref = medium_inputs(dt)
    lat = lat.to(DEV)

    def fresh(lora, scale=0.5, cap=16):
        c = medium_cfg(s2v, rank_cap=cap)
        m, e = ready_engine(s2v, c, dt, sd, text, ref, lora=lora, scale=scale)
        y = fwd(e, lat)
        e.close()
        return y

    m, eng = ready_engine(s2v, cfg, dt, sd, text, ref)
    eng.attach_lora(L1, 0.5)
    y1 = fwd(eng, lat)
    assert torch.equal(y1, fresh(L1)), "attach(L1) differs from a fresh runtime-mode engine loaded with L1"
    eng.attach_lora(L2, 0.5)
    y2 = fwd(eng, lat)
    assert not torch.equal(y1, y2)
    assert torch.equal(y2, fresh(L2)), "swap to L2 (other seed, rank 16) differs from a fresh engine loaded with L2"
    eng.set_lora_scale(0.25)
    assert eng.lora_state["scale"] == 0.25
    y3 = fwd(eng, lat)
    assert not torch.equal(y3, y2)
    assert torch.equal(y3, fresh(L2, 0.25)), "set_lora_scale(0.25) differs from a fresh attach at 0.25"
    eng.attach_lora(L1, 0.5)   # back to the smaller rank: nothing of L2's columns 8..15 may survive
    assert torch.equal(fwd(eng, lat), y1)
    eng.detach_lora()
    assert eng.lora_state["attached"] == 0
    y0 = fwd(eng, lat)
    assert torch.equal(y0, fresh(None)), "detached differs from a fresh runtime-mode engine without an adapter"
    # no adapter => today's K and today's launches on operands with a larger pitch: the bytes of an engine without the mode
    assert torch.equal(y0, fresh(None, cap=0)), "detached runtime-mode engine differs from a lora_runtime_rank = 0 engine"
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. the re-merged weights equal a merged engine's
@pytest.mark.parametrize("scope", ["shipped", "intended"])
@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_remerged_weights_equal_the_merged_engine_bytes(s2v, scope, dt_name):
    dt = DT[dt_name]
    sd = s2v.weights.synthetic_state_dict(medium_cfg(s2v), seed=5, parity=True)
    lora = s2v.weights.synthetic_lora(medium_cfg(s2v), rank=8, seed=6, std=0.05)
    lat, text, ref = medium_inputs(dt)
    mm = s2v.HipCogVideoXTransformer3DModel(medium_cfg(s2v, rank_cap=0, scope=scope), dt, DEV)
    mm.load_state_dict(sd, lora=lora, lora_scale=0.5)
    mr = s2v.HipCogVideoXTransformer3DModel(medium_cfg(s2v, rank_cap=8, scope=scope), dt, DEV)
    mr.load_state_dict(sd)
    names = ["transformer_blocks.0.norm1.linear.weight", "transformer_blocks.1.norm2.linear.weight", "patch_embed.proj.weight",
             "patch_embed.text_proj.weight"]
    base = {n: mr.engine.read_weight(n).clone() for n in names}
    mr.engine.attach_lora(lora, 0.5)
    for n in names:
        a, b = mr.engine.read_weight(n), mm.engine.read_weight(n)
        assert a.shape == b.shape
        assert torch.equal(a, b), f"{n}: attached runtime engine differs from the merged engine"
    if scope == "shipped":
        assert not torch.equal(mr.engine.read_weight(names[0]), base[names[0]])
    else:  # "intended": the merge reaches the reference-image copy only; the six chunks the slot names stay the base
        assert torch.equal(mr.engine.read_weight(names[0]), base[names[0]])
    # the branch weights keep the BASE bytes under attach (the adapter lives in the tail), with the base shape and a larger ld
    q = "transformer_blocks.0.attn1.to_q.weight"
    assert torch.equal(mr.engine.read_weight(q).cpu(), sd[q].to(dt)) and mr.engine.read_weight(q).stride(0) > sd[q].shape[1]
    # and the whole forward of the two engines agrees within the bars (merge rounds W + sBA once; the branch does not)
    for m in (mm, mr):
        m.engine.set_geometry(2, GEO["T"], GEO["F"], GEO["H"], GEO["W"])
        m.engine.prepare_tables(GEO["H"] * 8, GEO["W"] * 8)
        m.engine.set_conditioning(text, ref)
    assert_close(fwd(mr.engine, lat.to(DEV)), fwd(mm.engine, lat.to(DEV)), dt_name, f"runtime vs merged engine ({scope})")
    mr.engine.detach_lora()
    for n in names:
        assert torch.equal(mr.engine.read_weight(n), base[n]), f"{n}: detach did not restore the base bytes"
    mm.engine.close()
    mr.engine.close()


# ------------------------------------------------------------------------------------------------ 5. hipGraph
@pytest.mark.parametrize("fused,use_graph", [(True, True), (False, False)], ids=["fused_graph", "seams"])
def test_pipeline_in_runtime_mode_equals_eager_bitwise(s2v, fused, use_graph):
    """S2VPipeline on a runtime-mode transformer with an adapter attached, 3 steps: hipGraph and the seams against the fused eager run"""
    g = load_golden("pipeline_tiny.npz")
    lora_cfg = s2v.tiny(use_rope=True, text_dim=64, temb=64)
    lora = s2v.weights.synthetic_lora(lora_cfg, rank=8, seed=21, std=0.05)

    def run(fused, use_graph):
        cfg = s2v.tiny(use_rope=True, text_dim=64, temb=64)
        cfg.max_text_seq_length = 6
        cfg.lora_runtime_rank = 8
        m = s2v.HipCogVideoXTransformer3DModel(cfg, torch.bfloat16, DEV)
        m.load_state_dict(weights_of(g), lora=lora, lora_scale=0.5)
        assert m.engine.lora_state["attached"] == len(lora)
        pipe = s2v.S2VPipeline(m, s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0), None)
        t = lambda x: torch.from_numpy(np.asarray(x)).to(torch.bfloat16)
        out = pipe(prompt_embeds=t(g["prompt_embeds"]), negative_prompt_embeds=t(g["negative_prompt_embeds"]), ref_img_states=t(g["ref"]),
                   height=480, width=720, num_frames=5, num_inference_steps=3, guidance_scale=6.0, latents=t(g["latents0"]),
                   return_dict=False, output_type="latent", fused=fused, use_graph=use_graph)[0]
        torch.cuda.synchronize()
        caps = m.engine.lora_state["graph_captures"]
        m.engine.close()
        return out.clone(), caps

    eager, c0 = run(True, False)
    other, c1 = run(fused, use_graph)
    assert torch.isfinite(eager.float()).all() and c0 == 0
    assert c1 == (1 if use_graph else 0)
    if fused:
        assert torch.equal(other, eager), "hipGraph pipeline differs from the eager pipeline in runtime mode"
    else:
        # seams: the transformer through its forward seam and the scheduler as an object.  Held to the bars tests/test_gpu_parity.py:355 states
        # for three coarse CFG-6 steps in bf16 (rel-L2 4.4e-2, max-abs 6.0e-2 max|ref|), the distance that file allows either mode from the reference
        r = rel_l2(other.float().cpu(), eager.float().cpu())
        ma = (other.float() - eager.float()).abs().max().item() / eager.float().abs().max().item()
        print(f"MEASURED bf16 seams vs fused, runtime mode: rel-l2 {r:.3e} max-abs/max|ref| {ma:.3e}")
        assert torch.isfinite(other.float()).all() and r <= 4.4e-2 and ma <= 6.0e-2, (r, ma)


def test_rescale_keeps_the_captured_step_and_attach_drops_it(s2v):
    dt = torch.bfloat16
    cfg = medium_cfg(s2v, rank_cap=8)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=5, parity=True)
    L1 = s2v.weights.synthetic_lora(cfg, rank=8, seed=6, std=0.05)
    L2 = s2v.weights.synthetic_lora(cfg, rank=4, seed=8, std=0.05)
    lat, text, ref = medium_inputs(dt)
    sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0)
    sch.set_timesteps(4)
    ts = sch.timesteps

    def run(use_graph):
        m, e = ready_engine(s2v, medium_cfg(s2v, rank_cap=8), dt, sd, text, ref, lora=L1)
        x = lat[:1].to(DEV).contiguous().clone()
        caps = []
        e.denoise_step(x, float(ts[0]), sch.coef(ts[0], dt, 6.0), use_graph=use_graph)
        caps.append(e.lora_state["graph_captures"])
        e.set_lora_scale(0.25)
        e.denoise_step(x, float(ts[1]), sch.coef(ts[1], dt, 6.0), use_graph=use_graph)
        caps.append(e.lora_state["graph_captures"])
        e.attach_lora(L2, 0.5)
        e.denoise_step(x, float(ts[2]), sch.coef(ts[2], dt, 6.0), use_graph=use_graph)
        caps.append(e.lora_state["graph_captures"])
        e.detach_lora()
        e.denoise_step(x, float(ts[3]), sch.coef(ts[3], dt, 6.0), use_graph=use_graph)
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


# ------------------------------------------------------------------------------------------------ 8. CFG-parallel
@pytest.mark.parametrize("dt_name", ["bf16", "f32", "f16"])
def test_b1_runtime_engine_is_its_half_of_the_b2_runtime_engine_bitwise(s2v, dt_name):
    """the argument of tests/test_gpu_cfg_parallel.py carries to the branch: the down-projection is row-wise with a fixed K order and the
    K-extended GEMMs are the kernels that test already holds"""
    dt = DT[dt_name]
    cfg = medium_cfg(s2v, rank_cap=8)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=61, parity=True)
    lora = s2v.weights.synthetic_lora(cfg, rank=8, seed=62, std=0.05)
    lat, text, ref = medium_inputs(dt, seed=63)
    lat1 = lat[:1].to(DEV).contiguous()
    m2, e2 = ready_engine(s2v, medium_cfg(s2v, rank_cap=8), dt, sd, text, ref, lora=lora)
    y2 = e2.forward(lat1, torch.tensor([321.0, 321.0]), shared_latent=True).clone()
    for slot in (0, 1):
        m1, e1 = ready_engine(s2v, medium_cfg(s2v, rank_cap=8), dt, sd, text[slot:slot + 1], ref, lora=lora, B=1)
        y1 = e1.forward(lat1, torch.tensor([321.0]), shared_latent=True)
        torch.cuda.synchronize()
        assert torch.isfinite(y1.float()).all()
        assert torch.equal(y1[0], y2[slot]), f"slot {slot}: the B = 1 runtime engine differs from its half of the B = 2 runtime engine"
        e1.close()
    assert not torch.equal(y2[0], y2[1])
    e2.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_name_the_cause_and_leave_the_state(s2v):
    dt = torch.bfloat16
    cfg = medium_cfg(s2v, rank_cap=8)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=5, parity=True)
    L1 = s2v.weights.synthetic_lora(cfg, rank=8, seed=6, std=0.05)
    big = s2v.weights.synthetic_lora(cfg, rank=16, seed=7, std=0.05)
    lat, text, ref = medium_inputs(dt)
    lat = lat.to(DEV)
    L = s2v._lib
    # rank over capacity: through the engine and through the C ABI directly
    m, eng = ready_engine(s2v, cfg, dt, sd, text, ref, lora=L1)
    y = fwd(eng, lat)
    st = eng.lora_state
    with pytest.raises(s2v.S2VError, match="capacity"):
        eng.attach_lora(big, 0.5)
    A = torch.zeros(16, 192, device=DEV)
    Bm = torch.zeros(192, 16, device=DEV)
    q = b"transformer_blocks.0.attn1.to_q.weight"
    assert L.lib().s2v_lora_attach(eng._h, q, L.ptr(A), L.ptr(Bm), 16, 0.5, L.stream_ptr()) != 0
    assert b"capacity" in L.lib().s2v_last_error()
    assert L.lib().s2v_lora_attach(eng._h, b"transformer_blocks.0.attn1.to_z.weight", L.ptr(A), L.ptr(Bm), 8, 0.5, L.stream_ptr()) != 0
    assert b"unknown tensor name" in L.lib().s2v_last_error()
    assert L.lib().s2v_lora_attach(eng._h, b"norm_out.linear.weight", L.ptr(A), L.ptr(Bm), 8, 0.5, L.stream_ptr()) != 0
    assert b"not a LoRA target" in L.lib().s2v_last_error()
    assert eng.lora_state == st
    assert torch.equal(fwd(eng, lat), y), "a refused attach changed the engine"
    eng.close()
    # the mode off
    m0, e0 = ready_engine(s2v, medium_cfg(s2v, rank_cap=0), dt, sd, text, ref, lora=L1)
    y = fwd(e0, lat)
    for call in (lambda: e0.attach_lora(L1, 0.5), lambda: e0.set_lora_scale(0.25), lambda: e0.detach_lora()):
        with pytest.raises(s2v.S2VError, match="mode is off"):
            call()
    A8, B8 = torch.zeros(8, 192, device=DEV), torch.zeros(192, 8, device=DEV)
    assert L.lib().s2v_lora_attach(e0._h, q, L.ptr(A8), L.ptr(B8), 8, 0.5, L.stream_ptr()) != 0
    assert b"mode is off" in L.lib().s2v_last_error()
    assert e0.lora_state["attached"] == 0 and torch.equal(fwd(e0, lat), y)
    e0.close()
    # a shard context refuses the mode in s2v_set_shard
    es = s2v.S2VEngine(medium_cfg(s2v, rank_cap=8), dt, DEV)
    with pytest.raises(s2v.S2VError, match="shard"):
        es.set_shard(3, 0)
    es.close()
    # fp8 weight format (bf16, inner_dim % 128 == 0): the context exists, attach is refused by name, a forward still runs
    cf = s2v.tiny(use_rope=True, heads=2, layers=1, text_dim=64, temb=64)
    cf.weight_format, cf.lora_runtime_rank = "fp8", 8
    sdf = s2v.weights.synthetic_state_dict(cf, seed=5, parity=True)
    mf = s2v.HipCogVideoXTransformer3DModel(cf, dt, DEV)
    lf = s2v.weights.synthetic_lora(cf, rank=8, seed=6, std=0.05)
    with pytest.raises(s2v.S2VError, match="fp8"):
        mf.load_state_dict(sdf, lora=lf)
    ef = mf.engine
    A8, B8 = torch.zeros(8, 128, device=DEV), torch.zeros(128, 8, device=DEV)
    assert L.lib().s2v_lora_attach(ef._h, q, L.ptr(A8), L.ptr(B8), 8, 0.5, L.stream_ptr()) != 0
    assert b"fp8" in L.lib().s2v_last_error()
    assert ef.lora_state["attached"] == 0
    g = torch.Generator().manual_seed(1)
    ef.set_geometry(2, 5, 2, 8, 12)
    ef.prepare_tables(64, 96)
    ef.set_conditioning(torch.randn(2, 5, 64, generator=g).to(dt), (torch.randn(1, 1, 16, 8, 12, generator=g) * 0.7).to(dt))
    yf = ef.forward(torch.randn(2, 2, 16, 8, 12, generator=g).to(dt), torch.tensor([500.0, 500.0]))
    torch.cuda.synchronize()
    assert torch.isfinite(yf.float()).all()
    ef.close()


# ------------------------------------------------------------------------------------------------ 6. AttnProcessor, lora="runtime"
P = "transformer_blocks.0.attn1."


class Lin:
    def __init__(self, w, b):
        self.weight, self.bias = w, b


class Tuner:
    """a peft.tuners.lora.LoraLayer, duck-typed as in tests/test_gpu_attn_processor_model.py: adapters keyed by name"""

    def __init__(self, base, adapters):
        self.base_layer = base
        self.lora_A = {k: Lin(A, None) for k, (A, B, s) in adapters.items()}
        self.lora_B = {k: Lin(B, None) for k, (A, B, s) in adapters.items()}
        self.scaling = {k: s for k, (A, B, s) in adapters.items()}
        self.use_dora = {k: False for k in adapters}
        self.active_adapters = [next(iter(adapters))]
        self.merged = False
        self.disable_adapters = False

    @property
    def weight(self):
        return self.base_layer.weight

    @property
    def bias(self):
        return self.base_layer.bias


class Attn:
    is_cross_attention = False

    def __init__(self, heads, sd):
        self.heads = heads
        self.to_q, self.to_k, self.to_v = (Lin(sd[n + ".weight"], sd[n + ".bias"]) for n in ("to_q", "to_k", "to_v"))
        self.to_out = [Lin(sd["to_out.0.weight"], sd["to_out.0.bias"])]
        self.norm_q, self.norm_k = (Lin(sd[n + ".weight"], sd[n + ".bias"]) for n in ("norm_q", "norm_k"))


LIN = ("to_q", "to_k", "to_v", "to_out.0")


def attn_case(heads, dt, seed):
    D = heads * 64
    g = torch.Generator(device=DEV).manual_seed(seed)
    sd = {}
    for n in LIN:
        sd[n + ".weight"] = (torch.randn(D, D, generator=g, device=DEV) * (0.7 / D**0.5)).to(dt)
        sd[n + ".bias"] = (0.1 * torch.randn(D, generator=g, device=DEV)).to(dt)
    for n in ("norm_q", "norm_k"):
        sd[n + ".weight"] = (1 + 0.2 * torch.randn(64, generator=g, device=DEV)).to(dt)
        sd[n + ".bias"] = (0.1 * torch.randn(64, generator=g, device=DEV)).to(dt)
    ads = {}
    for n in LIN:  # adapter tensors in the model dtype, as PEFT holds them
        ads[n] = {name: ((torch.randn(r, D, generator=g, device=DEV) / D**0.5).to(dt), (0.1 * torch.randn(D, r, generator=g, device=DEV)).to(dt), s)
                  for name, r, s in (("default", 16, 0.5), ("other", 8, 1.5))}
    B, T, F, H, W = 2, 5, 2, 8, 8
    R = (H // 2) * (W // 2)
    h = torch.randn(B, F * R, D, generator=g, device=DEV).to(dt)
    e = torch.randn(B, T + R, D, generator=g, device=DEV).to(dt)
    (rc, rs), (vc, vs) = tr.pipeline_rope(H * 8, W * 8, F)
    kw = dict(hidden_states=h, encoder_hidden_states=e, attention_mask=None, image_rotary_emb=(vc.to(DEV), vs.to(DEV)),
              ref_img_seq_start=T, ref_img_seq_end=T + R, position_delta=0, embed_ref_img=True, ref_image_rotary_emb=(rc.to(DEV), rs.to(DEV)))
    return sd, ads, kw


def peft_attn_fp32(sd, heads, kw, active):
    """the PEFT model's attention evaluated in fp32 on the given (model-dtype) operands.  peft/tuners/lora/layer.py Linear.forward is
    base(x) + lora_B(lora_A(x)) * scaling per active adapter; in fp32 that equals x (W + sum s B A)^T up to the summation order (~1e-6
    relative, three orders under the bars), which is the form the attention oracle takes: W + sum s B A is formed in fp64 here"""
    cpu = {P + k: v.float().cpu() for k, v in sd.items()}
    for n, adapters in active.items():
        w = cpu[P + n + ".weight"].double()
        for A, B, s in adapters:
            w = w + s * (B.double().cpu() @ A.double().cpu())
        cpu[P + n + ".weight"] = w.float()
    (vc, vs), (rc, rs) = kw["image_rotary_emb"], kw["ref_image_rotary_emb"]
    with torch.no_grad():
        return tr.attn_forward(cpu, P, heads, kw["hidden_states"].float().cpu(), kw["encoder_hidden_states"].float().cpu(),
                               (vc.cpu(), vs.cpu()), (rc.cpu(), rs.cpu()), kw["ref_img_seq_start"], kw["ref_img_seq_end"])


@pytest.mark.parametrize("dt_name", ["bf16", "f32", "f16"])
def test_attn_processor_runtime_mode_follows_peft_switches_without_repacking(s2v, dt_name):
    dt, heads = DT[dt_name], 8
    s2v.HipCogVideoXAttnProcessor2_0.release_pools()
    sd, ads, kw = attn_case(heads, dt, 400)
    attn = Attn(heads, sd)
    tun = {n: Tuner(Lin(sd[n + ".weight"], sd[n + ".bias"]), ads[n]) for n in LIN}
    attn.to_q, attn.to_k, attn.to_v, attn.to_out = tun["to_q"], tun["to_k"], tun["to_v"], [tun["to_out.0"]]
    proc = s2v.HipCogVideoXAttnProcessor2_0(lora="runtime", lora_runtime_rank=24)

    def check(active_names, what):
        got = proc(attn, **kw)
        torch.cuda.synchronize()
        active = {n: [ads[n][a][:2] + (tun[n].scaling[a],) for a in active_names] for n in LIN}   # the tuner's CURRENT scaling
        eh, ee = peft_attn_fp32(sd, heads, kw, active)
        assert_close(got[0], eh, dt_name, f"runtime processor, {what}: hidden")
        assert_close(got[1], ee, dt_name, f"runtime processor, {what}: encoder")
        return got

    y_def = check(["default"], "adapter 'default'")
    pool = proc.pools()[0]
    ctx = pool.slots[id(attn)][0]
    assert ctx.lora_state["attached"] == 4
    for t in tun.values():                       # another scaling
        t.scaling["default"] = 0.25
    y_s = check(["default"], "scaling 0.25")
    assert not torch.equal(y_s[0], y_def[0])
    for t in tun.values():
        t.scaling["default"] = 0.5
    for t in tun.values():                       # disable_adapters: the base layer alone
        t.disable_adapters = True
    y_off = check([], "adapters disabled")
    assert pool.slots[id(attn)][0].lora_state["attached"] == 0
    base = proc(Attn(heads, sd), **kw)           # a module without tuner layers: the same bytes
    torch.cuda.synchronize()
    assert torch.equal(y_off[0], base[0]) and torch.equal(y_off[1], base[1])
    for t in tun.values():
        t.disable_adapters = False
    for t in tun.values():                       # switch the active adapter
        t.active_adapters = ["other"]
    check(["other"], "adapter 'other'")
    for t in tun.values():                       # both active: 16 + 8 <= 24, concatenated along r
        t.active_adapters = ["default", "other"]
    check(["default", "other"], "both adapters")
    for t in tun.values():
        t.active_adapters = ["default"]
    again = proc(attn, **kw)
    torch.cuda.synchronize()
    assert torch.equal(again[0], y_def[0]) and torch.equal(again[1], y_def[1])
    assert pool.slots[id(attn)][0] is ctx, "a change of the adapter settings re-packed the module's weights context"
    # over the capacity: 16 + 8 > 16
    small = s2v.HipCogVideoXAttnProcessor2_0(lora="runtime", lora_runtime_rank=16)
    for t in tun.values():
        t.active_adapters = ["default", "other"]
    with pytest.raises(s2v.S2VError, match="capacity"):
        small(attn, **kw)
    # DoRA stays refused; lora="merge" is untouched (its own tests hold it): it still merges and gives the merged engine's answer
    for t in tun.values():
        t.active_adapters = ["default"]
    merged = s2v.HipCogVideoXAttnProcessor2_0()(attn, **kw)
    torch.cuda.synchronize()
    eh, ee = peft_attn_fp32(sd, heads, kw, {n: [ads[n]["default"]] for n in LIN})
    assert_close(merged[0], eh, dt_name, "merge processor: hidden")
    tun["to_v"].use_dora["default"] = True
    with pytest.raises(NotImplementedError):
        proc(attn, **kw)
    s2v.HipCogVideoXAttnProcessor2_0.release_pools()


def test_attn_forward_with_refuses_another_lora_runtime_rank(s2v):
    mk = lambda r: s2v.TransformerConfig(num_layers=1, num_attention_heads=2, time_embed_dim=8, text_embed_dim=64,
                                         use_rotary_positional_embeddings=True, lora_runtime_rank=r)
    ws = s2v.S2VEngine(mk(8), torch.bfloat16, DEV, kind=s2v._lib.CTX_ATTN_WORKSPACE)
    w0 = s2v.S2VEngine(mk(0), torch.bfloat16, DEV, kind=s2v._lib.CTX_ATTN_WEIGHTS)
    g = torch.Generator().manual_seed(2)
    for n in LIN:
        w0.load_weight(P + n + ".weight", torch.randn(128, 128, generator=g))
        w0.load_weight(P + n + ".bias", torch.randn(128, generator=g))
    for n in ("norm_q", "norm_k"):
        w0.load_weight(P + n + ".weight", torch.ones(64))
        w0.load_weight(P + n + ".bias", torch.zeros(64))
    w0.finalize_weights()
    ws.set_geometry(1, 3, 1, 4, 4)
    ws.clear_rope()
    h = torch.zeros(1, 4, 128, dtype=torch.bfloat16, device=DEV)
    e = torch.zeros(1, 7, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(s2v.S2VError, match="lora_runtime_rank"):
        ws.attn_forward_with(w0, 0, h, e)
    ws.close()
    w0.close()


# ------------------------------------------------------------------------------------------------ 7. full width once
def test_full_width_block_rank128_vs_oracle_and_memory(s2v):
    """5B width (D = 3072, 48 heads, RoPE), 19 126 tokens x B = 2 (M = 38 252 rows), rank 128, one block through the Block seam in bf16 against
    the CPU oracle on the merged weights (the tests/test_gpu_fullsize_oracle.py pattern; the parity bars of this file), and the growth of
    s2v_device_bytes over a mode-off engine against the sum the layout gives."""
    dt = torch.bfloat16
    F_, H_, W_, T_, B = 13, 60, 90, 226, 2
    cfg = s2v.cogvideox_5b()
    cfg.num_layers = 1
    cfg.lora_runtime_rank = 128
    D, heads, TE, TX = cfg.inner_dim, cfg.num_attention_heads, cfg.time_embed_dim, cfg.text_embed_dim
    R = (H_ // 2) * (W_ // 2)
    V = F_ * R
    sd = {k: v.to(dt).float() for k, v in s2v.weights.synthetic_state_dict(cfg, seed=21, parity=True).items()}
    lora = s2v.weights.synthetic_lora(cfg, rank=128, seed=24, std=0.02)
    g = torch.Generator().manual_seed(22)
    h = torch.randn(B, V, D, generator=g).to(dt).float()
    e0 = torch.randn(B, T_, D, generator=g).to(dt).float()
    e1 = torch.randn(B, R, D, generator=g).to(dt).float()
    temb = torch.randn(B, TE, generator=g).to(dt).float()
    ref_rope, rope = tr.pipeline_rope(H_ * 8, W_ * 8, F_)
    merged = tr.merge_lora(sd, lora, 0.5)
    with torch.no_grad():
        exp = tr.block_forward(merged, "transformer_blocks.0.", heads, h, e0, e1, temb, rope, ref_rope)
        base = tr.block_forward(sd, "transformer_blocks.0.", heads, h, e0, e1, temb, rope, ref_rope)
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    m.load_state_dict(sd, lora=lora, lora_scale=0.5)
    assert m.engine.lora_state["attached"] == len(lora)
    kw = dict(image_rotary_emb=tuple(x.to(DEV) for x in rope), ref_image_rotary_emb=tuple(x.to(DEV) for x in ref_rope))
    got = m.transformer_blocks[0](hidden_states=h.to(DEV, dt), encoder_hidden_states=e0.to(DEV, dt), temb=temb.to(DEV, dt),
                                  enc_hidden_states1=e1.to(DEV, dt), embed_ref_img=True, ref_img_seq_start=T_, ref_img_seq_end=T_ + R,
                                  position_delta=0, timestep=None, layer=0, **kw)
    torch.cuda.synchronize()
    for name, y, e, b in zip(("video", "text", "ref"), got, exp, base):
        assert_close(y, e, "bf16", f"5B block, rank 128 attached: {name}")
        print(f"MEASURED 5B block {name}: base vs merged oracle rel-l2 {rel_l2(b, e):.3e}")
    # memory: what the layout adds (elements of the model dtype, E = 2 bytes; every carve is rounded up to 256 bytes)
    ar1, ws1 = m.engine.device_bytes()
    c0 = s2v.cogvideox_5b()
    c0.num_layers = 1
    e0_ = s2v.S2VEngine(c0, dt, DEV)
    e0_.set_geometry(B, T_, F_, H_, W_)
    ar0, ws0 = e0_.device_bytes()
    e0_.close()
    E, lr, L = 2, 128, 1
    up = lambda x, m_: (x + m_ - 1) // m_ * m_
    Dp, Kp = up(D, 256), cfg.in_channels * 4
    tails = L * (up(3 * D, 256) * 3 * lr + Dp * lr + up(4 * D, 256) * lr + Dp * lr)
    stacks = L * (3 * lr * D + lr * D + lr * D + lr * 4 * D)
    mod_rows = 2 * L * 6 * D + 2 * D
    base_copies = mod_rows * TE + Dp * Kp + Dp * TX
    # rescaling re-reads fp32 A and B: the library keeps no copy, the Python engine keeps them as torch tensors OUTSIDE s2v_device_bytes and
    # reports them as lora_kept_bytes -- held here to the sum over the adapter's shapes
    kept_b = 0
    kept = sum((A.numel() + B.numel()) * 4 for A, B in lora.values())
    print(f"MEASURED fp32 adapter copies kept by the engine: {m.engine.lora_kept_bytes} bytes (derived {kept})")
    assert m.engine.lora_kept_bytes == kept
    carves = L * 8 + 3
    arena_sum = (tails + stacks + base_copies + kept_b) * E + 256 * carves
    Mpad = up(B * (T_ + R + V), 256) + 256
    pitch_sum = Mpad * (3 * lr + lr) * E + 256 * 2
    print(f"MEASURED device_bytes growth: arena {ar1 - ar0} (derived <= {arena_sum}), workspace {ws1 - ws0} (derived <= {pitch_sum})")
    assert 0 < ar1 - ar0 <= arena_sum, (ar1 - ar0, arena_sum)
    assert 0 < ws1 - ws0 <= pitch_sum, (ws1 - ws0, pitch_sum)
    m.engine.close()


# ------------------------------------------------------------------------------------------------ replicas carry an attached adapter
def test_replica_filled_from_the_arena_runs_the_attached_adapter(s2v):
    """tails, A stacks, base copies AND the attached state live inside the weight arena: a context whose arena is a copy of another's
    (what s2v_bcast_weights / dist.broadcast_arena deliver) and that is marked loaded gives the sender's bytes"""
    dt = torch.bfloat16
    cfg = medium_cfg(s2v, rank_cap=8)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=5, parity=True)
    lora = s2v.weights.synthetic_lora(cfg, rank=8, seed=6, std=0.05)
    lat, text, ref = medium_inputs(dt)
    lat = lat.to(DEV)
    m, src = ready_engine(s2v, cfg, dt, sd, text, ref, lora=lora)
    y = fwd(src, lat)
    rep = s2v.S2VEngine(medium_cfg(s2v, rank_cap=8), dt, DEV)
    rep.weight_arena().copy_(src.weight_arena())
    torch.cuda.synchronize()
    rep.mark_weights_loaded()
    st = rep.lora_state
    assert st["attached"] == len(lora) and st["rank"] == 8 and st["scale"] == 0.5
    rep.set_geometry(2, GEO["T"], GEO["F"], GEO["H"], GEO["W"])
    rep.prepare_tables(GEO["H"] * 8, GEO["W"] * 8)
    rep.set_conditioning(text, ref)
    assert torch.equal(fwd(rep, lat), y), "the replica differs from the engine its arena came from"
    rep.detach_lora()
    src.detach_lora()
    assert rep.lora_state["attached"] == 0
    assert torch.equal(fwd(rep, lat), fwd(src, lat))
    rep.close()
    src.close()


# ------------------------------------------------------------------------------------------------ 2. not worse than the reference's own arithmetic
def _peft_lin(x, W, b, A, B, s, dt):
    """peft/tuners/lora/layer.py Linear.forward in the model dtype (restated, peft is not installed): every op rounds to dt, matmuls accumulate in fp32"""
    r = lambda v: v.to(dt).float()
    return r(r(x @ W.T + b) + r(r(r(x @ A.T) @ B.T) * r(torch.tensor(s))))


def _ln64(y, w, b, n_cols):
    """per-head LayerNorm(64, eps 1e-6, affine) on columns < n_cols, in y's precision"""
    out = y.clone()
    h = y[:, :n_cols].reshape(y.shape[0], -1, 64)
    nh = h.shape[1] // 2
    ww = torch.cat([w[0].expand(nh, 64), w[1].expand(nh, 64)]).to(y.dtype)
    bb = torch.cat([b[0].expand(nh, 64), b[1].expand(nh, 64)]).to(y.dtype)
    mu = h.mean(-1, keepdim=True)
    var = ((h - mu) ** 2).mean(-1, keepdim=True)
    out[:, :n_cols] = ((h - mu) / torch.sqrt(var + 1e-6) * ww + bb).reshape(y.shape[0], n_cols)
    return out


EPI_NAMES = {0: "bias", 1: "gelu", 2: "gate_res", 4: "qknorm"}


@pytest.mark.parametrize("dt_name", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [(512, 3072, 512, 128), (300, 192, 192, 8)], ids=["512x3072x512r128", "300x192x192r8"])
@pytest.mark.parametrize("epi", [0, 1, 2, 4], ids=["bias", "gelu", "gate_res", "qknorm"])
def test_adapted_linear_is_not_worse_than_peft_arithmetic(s2v, epi, shape, dt_name):
    """W, A ~ 0.02 N(0,1), B ~ 2e-2 N(0,1), s = 0.5, x ~ N(0,1); truth in fp64 from the same rounded operands.  The bar is the reference's own
    error: rel-L2(device) <= rel-L2(PEFT restatement), no margin.  The fused q/k-norm epilogue takes N = 3 * qk_D only, so its large case
    runs N = 576 instead of 512 (192 is 3 * 64 already)."""
    dt = DT[dt_name]
    M, K, N, rank = shape
    if epi == 4 and N % 192:
        N = 576
    s = 0.5
    g = torch.Generator().manual_seed(1000 + epi)
    r = lambda v: v.to(dt).float()
    x, W, b = r(torch.randn(M, K, generator=g)), r(torch.randn(N, K, generator=g) * 0.02), r(torch.randn(N, generator=g) * 0.02)
    A32, B32 = torch.randn(rank, K, generator=g) * 0.02, torch.randn(N, rank, generator=g) * 2e-2
    A, B = r(A32), r(B32)      # PEFT holds lora_A / lora_B in the model dtype; the engine is handed the same values as fp32
    X0 = r(torch.randn(M, N, generator=g))
    gate = r(torch.randn(N, generator=g))
    lw, lb = r(1 + 0.2 * torch.randn(2, 64, generator=g)), r(0.1 * torch.randn(2, 64, generator=g))
    d = lambda v: v.double()
    lin64 = d(x) @ d(W).T + d(b) + s * ((d(x) @ d(A).T) @ d(B).T)
    peft = _peft_lin(x, W, b, A, B, s, dt)
    if epi == 0:
        truth, ref = lin64, peft
    elif epi == 1:
        truth, ref = torch.nn.functional.gelu(lin64, approximate="tanh"), r(torch.nn.functional.gelu(peft, approximate="tanh"))
    elif epi == 2:   # hidden + gate * out, each op rounded (cogvideox_transformer_3d.py:165-167)
        truth, ref = d(X0) + d(gate) * lin64, r(X0 + r(gate * peft))
    else:            # norm_q / norm_k on the q and k thirds (attention_processor.py:2060-2066); v passes through
        nqk = 2 * N // 3
        truth, ref = _ln64(lin64, d(lw), d(lb), nqk), r(_ln64(peft, lw, lb, nqk))
    L = s2v._lib
    dev = lambda v, t=dt: v.to(DEV, t).contiguous()
    xd, Wd, bd, Ad, Bd = dev(x), dev(W), dev(b), dev(A, torch.float32), dev(B, torch.float32)
    C = dev(X0) if epi == 2 else torch.empty(M, N, dtype=dt, device=DEV)
    aux0 = dev(gate) if epi == 2 else (dev(lw) if epi == 4 else None)
    aux1 = dev(lb) if epi == 4 else None
    L.check(L.lib().s2v_op_linear_lora(L.ptr(xd), L.ptr(Wd), L.ptr(bd), L.ptr(Ad), L.ptr(Bd), rank, s, L.ptr(C), M, N, K, epi,
                                       L.ptr(aux0), L.ptr(aux1), L.DTYPE_OF[dt], L.stream_ptr()))
    torch.cuda.synchronize()
    got = C.float().cpu()
    assert torch.isfinite(got).all()
    e_dev, e_peft = rel_l2(got, truth), rel_l2(ref, truth)
    print(f"MEASURED {dt_name} {EPI_NAMES[epi]} M {M} K {K} N {N} r {rank}: device rel-l2 {e_dev:.4e}  PEFT restatement rel-l2 {e_peft:.4e}  ratio {e_dev / e_peft:.3f}")
    assert e_dev <= e_peft, (e_dev, e_peft)


# ------------------------------------------------------------------------------------------------ swap -> disable -> enable
def test_model_switches_follow_the_adapter_attached_last(s2v, tmp_path):
    """checkpoint.swap_lora attaches through the engine; the model's disable_adapters / enable_adapters / set_adapters_scale must switch THAT
    adapter at its current scale, whether or not the model was loaded with one -- bitwise against fresh engines"""
    from safetensors.torch import save_file
    dt = torch.bfloat16
    cfg = medium_cfg(s2v, rank_cap=8)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=5, parity=True)
    LA = s2v.weights.synthetic_lora(cfg, rank=8, seed=6, std=0.05)
    LB = s2v.weights.synthetic_lora(cfg, rank=4, seed=9, std=0.05)
    flat = {}
    for k, (A, B) in LB.items():
        stem = k[:-len(".weight")]
        flat[f"transformer.{stem}.lora_A.weight"] = A.contiguous()
        flat[f"transformer.{stem}.lora_B.weight"] = B.contiguous()
    ldir = tmp_path / "lora_b"
    ldir.mkdir()
    save_file(flat, str(ldir / "pytorch_lora_weights.safetensors"))
    lat, text, ref = medium_inputs(dt)
    lat = lat.to(DEV)

    def fresh(lora, scale):
        m_, e_ = ready_engine(s2v, medium_cfg(s2v, rank_cap=8), dt, sd, text, ref, lora=lora, scale=scale)
        y_ = fwd(e_, lat)
        e_.close()
        return y_

    yB, yB25, y0 = fresh(LB, 64 / 128), fresh(LB, 0.25), fresh(None, 0.5)
    for loaded in (LA, None):   # a model loaded with adapter A, and one loaded without any
        m, eng = ready_engine(s2v, medium_cfg(s2v, rank_cap=8), dt, sd, text, ref, lora=loaded)
        keys = s2v.checkpoint.swap_lora(m, str(ldir), lora_alpha=64, rank=128)
        assert len(keys) == len(LB)
        assert torch.equal(fwd(eng, lat), yB)
        m.disable_adapters()
        assert torch.equal(fwd(eng, lat), y0)
        m.enable_adapters()
        assert eng.lora_state["rank"] == 4
        assert torch.equal(fwd(eng, lat), yB), "enable_adapters did not restore the adapter that swap_lora attached"
        m.set_adapters_scale(0.25)
        m.disable_adapters()
        m.enable_adapters()
        assert torch.equal(fwd(eng, lat), yB25), "enable_adapters did not keep the scale set last"
        eng.close()
    # nothing ever attached: enable_adapters says so
    m, eng = ready_engine(s2v, medium_cfg(s2v, rank_cap=8), dt, sd, text, ref)
    with pytest.raises(s2v.S2VError, match="no adapter has been attached"):
        m.enable_adapters()
    # a name that is no LoRA target fails before anything changes; the engine stays as it was
    eng.attach_lora(LA, 0.5)
    yA = fwd(eng, lat)
    bad = dict(LA)
    bad["norm_out.linear.weight"] = (torch.zeros(8, 64), torch.zeros(2 * 192, 8))
    with pytest.raises(s2v.S2VError):
        eng.attach_lora(bad, 0.5)
    st = eng.lora_state
    assert st["attached"] in (0, len(LA))   # never half attached
    if st["attached"]:
        assert torch.equal(fwd(eng, lat), yA)
    else:
        assert torch.equal(fwd(eng, lat), y0)
    eng.close()
