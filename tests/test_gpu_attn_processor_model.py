"""Model-wide AttnProcessor seam (pytest -m gpu): HipCogVideoXAttnProcessor2_0 installed on all 42 Attention modules of a model, as the
reference's `transformer.set_attn_processor(proc)` does (cogvideox_transformer_3d.py:376-408).  Every module of one (device, dtype, heads,
inner dim, force_simple) runs on ONE process-wide workspace with its own attention-only weights context (s2v_attn_forward_with), follows
changes of its weights, and honours PEFT LoRA tuner layers (duck-typed here as the existing seam test duck-types Attention / Linear).

Bars: the ones tests/test_gpu_parity.py holds this seam to against the oracle (F32_BAR, BARS, restated below); against today's
one-layer S2VEngine per module (a fresh engine with the same weights) the outputs are bit-identical, because the launches are."""
import pytest
import torch

from oracle import transformer_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# tests/test_gpu_parity.py: bf16 relative L2 / max-abs over max|ref|; fp32 max-abs
BARS = {"bf16": (1.3e-2, 2e-2), "f16": (1.3e-3, 2e-3)}
F32_BAR = 4e-5
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
P = "transformer_blocks.0.attn1."
NMOD = 42  # CogVideoX-5B's transformer_blocks
C3 = (2, 226, 13, 60, 90)          # B, T, latent frames, latent H, W: 49 x 480 x 720
CONFIGS0 = (2, 226, 3, 32, 32)     # 9 x 256 x 256
CONFIGS4 = (2, 226, 13, 90, 160)   # 49 x 720 x 1280
MB = 1e6


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
        assert r <= br and err <= ba * exp.abs().max().item(), f"{what}: rel-l2 {r}, max-abs {err}"


class Lin:
    def __init__(self, w, b):
        self.weight, self.bias = w, b


class Tuner:
    """a peft.tuners.lora.LoraLayer, duck-typed: `weight` / `bias` return the BASE layer's, as peft's do"""

    def __init__(self, base, A, B, scaling=0.5):
        self.base_layer = base
        self.lora_A, self.lora_B = {"default": Lin(A, None)}, {"default": Lin(B, None)}
        self.scaling = {"default": scaling}
        self.use_dora = {"default": False}
        self.active_adapters = ["default"]
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


def attn_weights(heads, seed, dtype):
    """attn1 weights scaled as weights.synthetic_state_dict(parity=True) scales them, drawn on the device"""
    D = heads * 64
    g = torch.Generator(device=DEV).manual_seed(seed)
    sd = {}
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        sd[n + ".weight"] = (torch.randn(D, D, generator=g, device=DEV) * (0.7 / D**0.5)).to(dtype)
        sd[n + ".bias"] = (0.1 * torch.randn(D, generator=g, device=DEV)).to(dtype)
    for n in ("norm_q", "norm_k"):
        sd[n + ".weight"] = (1 + 0.2 * torch.randn(64, generator=g, device=DEV)).to(dtype)
        sd[n + ".bias"] = (0.1 * torch.randn(64, generator=g, device=DEV)).to(dtype)
    return sd


def module_bytes(sd):
    return sum(t.numel() * t.element_size() for t in sd.values())


def inputs(geo, D, dtype, seed=7):
    """the processor's keyword arguments at a geometry, as the fork calls it (cogvideox_transformer_3d.py:510-512)"""
    B, T, F, H, W = geo
    R = (H // 2) * (W // 2)
    g = torch.Generator(device=DEV).manual_seed(seed)
    h = torch.randn(B, F * R, D, generator=g, device=DEV).to(dtype)
    e = torch.randn(B, T + R, D, generator=g, device=DEV).to(dtype)
    (rc, rs), (vc, vs) = tr.pipeline_rope(H * 8, W * 8, F)
    return dict(hidden_states=h, encoder_hidden_states=e, attention_mask=None, image_rotary_emb=(vc.to(DEV), vs.to(DEV)),
                ref_img_seq_start=T, ref_img_seq_end=T + R, position_delta=0, embed_ref_img=True,
                ref_image_rotary_emb=(rc.to(DEV), rs.to(DEV)))


def standalone(s2v, sd, heads, dtype, loras=()):
    """today's path: a complete one-layer S2VEngine holding one module's attention weights (loras: (name, A, B, scale) merged in)"""
    cfg = s2v.TransformerConfig(num_layers=1, num_attention_heads=heads, time_embed_dim=8, text_embed_dim=64,
                                use_rotary_positional_embeddings=True)
    eng = s2v.S2VEngine(cfg, dtype, DEV)
    for k, v in sd.items():
        eng.load_weight(P + k, v)
    for name, A, B, sc in loras:
        eng.merge_lora(P + name + ".weight", A, B, sc)
    torch.cuda.synchronize()
    eng.mark_weights_loaded()
    return eng


def standalone_call(eng, kw):
    h, e = kw["hidden_states"], kw["encoder_hidden_states"]
    B, V, _ = h.shape
    T, R = kw["ref_img_seq_start"], kw["ref_img_seq_end"] - kw["ref_img_seq_start"]
    geo = (B, T, V // R, 2, 2 * R)
    if eng.geometry != geo:
        eng.set_geometry(*geo)
    (vc, vs), (rc, rs) = kw["image_rotary_emb"], kw["ref_image_rotary_emb"]
    eng.set_rope(torch.cat([rc, vc]), torch.cat([rs, vs]))
    return eng.attn_forward(0, h, e)


def oracle(sd, heads, kw, dtype):
    cpu = {P + k: v.cpu() for k, v in sd.items()}
    (vc, vs), (rc, rs) = kw["image_rotary_emb"], kw["ref_image_rotary_emb"]
    with torch.no_grad():
        return tr.attn_forward(cpu, P, heads, kw["hidden_states"].cpu().to(dtype), kw["encoder_hidden_states"].cpu().to(dtype),
                               (vc.cpu(), vs.cpu()), (rc.cpu(), rs.cpu()), kw["ref_img_seq_start"], kw["ref_img_seq_end"])


def workspaces(pool):
    """contexts of a pool that hold an activation workspace, by the library's own count (s2v_device_bytes)"""
    return sum(1 for e in [pool.engine] + [s[0] for s in pool.slots.values()] if e.device_bytes()[1] > 0)


@pytest.fixture
def fresh_pools(s2v):
    s2v.HipCogVideoXAttnProcessor2_0.release_pools()
    torch.cuda.synchronize()
    yield
    s2v.HipCogVideoXAttnProcessor2_0.release_pools()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 1. one pool at small width
@pytest.mark.parametrize("dt_name", ["f32", "bf16"])
def test_pool_of_42_modules_at_small_width(s2v, fresh_pools, dt_name):
    dt, heads = DT[dt_name], 8
    sds = [attn_weights(heads, 100 + i, dt) for i in range(NMOD)]
    mods = [Attn(heads, sd) for sd in sds]
    kw = inputs((2, 5, 2, 8, 8), heads * 64, dt)
    proc = s2v.HipCogVideoXAttnProcessor2_0()
    outs = [proc(m, **kw) for m in mods]
    torch.cuda.synchronize()
    (pool,) = proc.pools()
    assert len(pool.slots) == NMOD and workspaces(pool) == 1
    mem, own = proc.memory_bytes(), sum(module_bytes(sd) for sd in sds)
    print(f"MEASURED {dt_name}: library weights {mem['weights'] / MB:.2f} MB for {own / MB:.2f} MB of module attention weights, "
          f"workspace {mem['workspace'] / MB:.2f} MB")
    assert mem["weights"] <= 1.05 * own and mem["workspace"] > 0
    for i in (0, NMOD // 2, NMOD - 1):
        eh, ee = oracle(sds[i], heads, kw, dt)
        assert_close(outs[i][0], eh, dt_name, f"module {i} hidden")
        assert_close(outs[i][1], ee, dt_name, f"module {i} encoder")
    # a dict of separate instances (set_attn_processor({name: proc_i})) draws from the same pool: no second workspace, no re-pack
    procs = [s2v.HipCogVideoXAttnProcessor2_0() for _ in mods]
    again = [p(m, **kw) for p, m in zip(procs, mods)]
    torch.cuda.synchronize()
    assert all(p.pools() == [pool] for p in procs) and workspaces(pool) == 1 and proc.memory_bytes() == mem
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(again, outs))


# ------------------------------------------------------------------------------------------------ 2. bit identity at full size
def test_bit_identical_to_standalone_engine_at_5b_c3(s2v, fresh_pools):
    dt, heads = torch.bfloat16, 48
    sds = [attn_weights(heads, 200 + i, dt) for i in range(NMOD)]
    mods = [Attn(heads, sd) for sd in sds]
    kw = inputs(C3, heads * 64, dt)
    proc = s2v.HipCogVideoXAttnProcessor2_0()
    outs = [proc(m, **kw) for m in mods]
    torch.cuda.synchronize()
    for i in (0, NMOD - 1):
        eng = standalone(s2v, sds[i], heads, dt)
        eh, ee = standalone_call(eng, kw)
        torch.cuda.synchronize()
        assert torch.equal(outs[i][0], eh) and torch.equal(outs[i][1], ee), f"module {i}"
        eng.close()


# ------------------------------------------------------------------------------------------------ 3. memory at full size
def _install_and_measure(s2v, geo, tag):
    dt, heads = torch.bfloat16, 48
    sds = [attn_weights(heads, 300 + i, dt) for i in range(NMOD)]
    mods = [Attn(heads, sd) for sd in sds]
    kw = inputs(geo, heads * 64, dt)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    proc = s2v.HipCogVideoXAttnProcessor2_0()
    for m in mods:
        oh, oe = proc(m, **kw)
        del oh, oe
    torch.cuda.synchronize()
    device_growth = free0 - torch.cuda.mem_get_info()[0]
    mem = proc.memory_bytes()
    (pool,) = proc.pools()
    print(f"MEASURED {tag}: {NMOD} modules at 5B width, library weights {mem['weights'] / 1e9:.3f} GB + workspace "
          f"{mem['workspace'] / 1e9:.3f} GB; device-wide growth (torch.cuda.mem_get_info) {device_growth / 1e9:.3f} GB")
    assert workspaces(pool) == 1
    return mem, device_growth


def test_memory_of_42_modules_at_5b_c3(s2v, fresh_pools):
    mem, grown = _install_and_measure(s2v, C3, "C3")
    assert mem["weights"] + mem["workspace"] <= NMOD * 75.5e6 * 1.05 + mem["workspace"] + 0.5e9
    assert mem["weights"] <= NMOD * 75.5e6 * 1.05
    assert grown < 8e9


def test_memory_of_42_modules_at_5b_configs4(s2v, fresh_pools):
    mem, grown = _install_and_measure(s2v, CONFIGS4, "configs[4]")
    assert mem["weights"] <= NMOD * 75.5e6 * 1.05
    assert grown < 12e9


# ------------------------------------------------------------------------------------------------ 4. PEFT LoRA tuner layers
def _lora(D, rank, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = torch.randn(rank, D, generator=g, device=DEV) / D**0.5
    B = 0.1 * torch.randn(D, rank, generator=g, device=DEV)
    return A, B


def test_peft_tuner_layers_are_merged(s2v, fresh_pools):
    dt, heads, D = torch.float32, 8, 512
    sd = attn_weights(heads, 400, dt)
    kw = inputs((2, 5, 2, 8, 8), D, dt)
    names = ("to_q", "to_k", "to_v", "to_out.0")
    ab = {n: _lora(D, 16, 410 + i) for i, n in enumerate(names)}
    peft = Attn(heads, sd)
    peft.to_q, peft.to_k, peft.to_v = (Tuner(getattr(peft, n), *ab[n]) for n in ("to_q", "to_k", "to_v"))
    peft.to_out = [Tuner(peft.to_out[0], *ab["to_out.0"])]
    merged_sd = dict(sd)
    for n in names:
        A, B = ab[n]
        merged_sd[n + ".weight"] = sd[n + ".weight"] + 0.5 * (B @ A)
    proc = s2v.HipCogVideoXAttnProcessor2_0()
    got = proc(peft, **kw)
    plain = proc(Attn(heads, merged_sd), **kw)
    base = proc(Attn(heads, sd), **kw)
    torch.cuda.synchronize()
    # the merge rounds W + 0.5 B A in its own summation order: equal to torch's W + 0.5 * (B @ A) up to the last fp32 bits
    for g_, p_ in zip(got, plain):
        assert (g_ - p_).abs().max().item() <= 1e-5
    eh, ee = oracle(merged_sd, heads, kw, dt)
    assert_close(got[0], eh, "f32", "peft hidden")
    assert_close(got[1], ee, "f32", "peft encoder")
    assert (got[0] - base[0]).abs().max().item() > 100 * F32_BAR  # the adapters matter at this scale
    # merged: the delta already sits in base_layer.weight (not added twice); disable_adapters: the base layer alone
    for flag in ("merged", "disable_adapters"):
        for t in (peft.to_q, peft.to_k, peft.to_v, peft.to_out[0]):
            setattr(t, flag, True)
        out = proc(peft, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1]), flag
        for t in (peft.to_q, peft.to_k, peft.to_v, peft.to_out[0]):
            setattr(t, flag, False)
    again = proc(peft, **kw)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    peft.to_v.use_dora["default"] = True
    with pytest.raises(NotImplementedError):
        proc(peft, **kw)


# ------------------------------------------------------------------------------------------------ 5. weight refresh
def test_in_place_weight_changes_are_followed(s2v, fresh_pools):
    dt, heads, D = torch.bfloat16, 8, 512
    sd = attn_weights(heads, 500, dt)
    kw = inputs((2, 5, 2, 8, 8), D, dt)
    A, B = _lora(D, 16, 510)
    attn = Attn(heads, sd)
    attn.to_q = Tuner(attn.to_q, A, B)
    proc = s2v.HipCogVideoXAttnProcessor2_0()
    first = proc(attn, **kw)
    with torch.no_grad():
        attn.to_v.weight.copy_(attn_weights(heads, 501, dt)["to_v.weight"])
        attn.to_q.lora_B["default"].weight.mul_(-2.0)
    got = proc(attn, **kw)
    eng = standalone(s2v, sd, heads, dt, loras=[("to_q", A, attn.to_q.lora_B["default"].weight, 0.5)])
    exp = standalone_call(eng, kw)
    torch.cuda.synchronize()
    assert not torch.equal(got[0], first[0])
    assert torch.equal(got[0], exp[0]) and torch.equal(got[1], exp[1])
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. geometry changes
def test_geometry_changes_recarve_once(s2v, fresh_pools):
    dt, heads = torch.bfloat16, 48
    sds = [attn_weights(heads, 600 + i, dt) for i in range(NMOD)]
    mods = [Attn(heads, sd) for sd in sds]
    proc = s2v.HipCogVideoXAttnProcessor2_0()
    refs = {i: standalone(s2v, sds[i], heads, dt) for i in (0, NMOD - 1)}
    changes = []
    for geo in (C3, CONFIGS0, C3):
        kw = inputs(geo, heads * 64, dt)
        outs = [proc(m, **kw) for m in mods]
        (pool,) = proc.pools()
        changes.append(pool.geometry_changes)
        for i, eng in refs.items():
            eh, ee = standalone_call(eng, kw)
            torch.cuda.synchronize()
            assert torch.equal(outs[i][0], eh) and torch.equal(outs[i][1], ee), (geo, i)
        del outs
    assert changes == [1, 2, 3]
    for eng in refs.values():
        eng.close()


# ------------------------------------------------------------------------------------------------ 7. the C entry point refuses mismatches
def test_attn_forward_with_refuses_mismatches(s2v):
    L = s2v._lib

    def cfg(heads):
        return s2v.TransformerConfig(num_layers=1, num_attention_heads=heads, time_embed_dim=8, text_embed_dim=64,
                                     use_rotary_positional_embeddings=True)

    def weights(heads, dt, finalize=True):
        e = s2v.S2VEngine(cfg(heads), dt, DEV, kind=L.CTX_ATTN_WEIGHTS)
        for k, v in attn_weights(heads, 700, dt).items():
            e.load_weight(P + k, v)
        if finalize:
            e.finalize_weights()
        return e

    ws = s2v.S2VEngine(cfg(2), torch.bfloat16, DEV, kind=L.CTX_ATTN_WORKSPACE)
    ws.set_geometry(1, 3, 1, 4, 4)
    R, V, D = 4, 4, 128
    h, e = torch.randn(1, V, D, device=DEV, dtype=torch.bfloat16), torch.randn(1, 3 + R, D, device=DEV, dtype=torch.bfloat16)
    ok = weights(2, torch.bfloat16)
    ws.attn_forward_with(ok, 0, h, e)
    torch.cuda.synchronize()
    for bad in (weights(2, torch.float32), weights(4, torch.bfloat16), weights(2, torch.bfloat16, finalize=False)):
        with pytest.raises(s2v.S2VError):
            ws.attn_forward_with(bad, 0, h, e)
    with pytest.raises(s2v.S2VError):
        ws.attn_forward_with(ok, 1, h, e)  # no such layer
    fp8 = s2v.S2VEngine(s2v.TransformerConfig(num_layers=1, num_attention_heads=2, time_embed_dim=8, text_embed_dim=64,
                                              use_rotary_positional_embeddings=True, weight_format="fp8"), torch.bfloat16, DEV)
    fp8.set_geometry(1, 3, 1, 4, 4)
    with pytest.raises(s2v.S2VError):
        fp8.attn_forward_with(ok, 0, h, e)  # weight_format
    shard = s2v.S2VEngine(cfg(2), torch.bfloat16, DEV)
    shard.set_shard(1, 0)
    shard.set_geometry(1, 3, 1, 4, 4)
    with pytest.raises(s2v.S2VError):
        shard.attn_forward_with(ok, 0, h, e)
    # each half does only its own job
    with pytest.raises(s2v.S2VError):
        ok.set_geometry(1, 3, 1, 4, 4)
    with pytest.raises(s2v.S2VError):
        ws.finalize_weights()
    with pytest.raises(s2v.S2VError):
        ws.attn_forward(0, h, e)
    with pytest.raises(s2v.S2VError):
        ws.set_shard(1, 0)
    assert ws.device_bytes()[0] == 0 and ws.device_bytes()[1] > 0
    assert ok.device_bytes()[1] == 0 and ok.device_bytes()[0] > 0
