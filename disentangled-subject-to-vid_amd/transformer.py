"""Drop-in objects for the reference's three Python plug-in seams of the transformer:

  HipCogVideoXTransformer3DModel  -- the Transformer object   (cogvideox_transformer_3d.py:450-462,557-560)
  HipCogVideoXBlock               -- a transformer_blocks[i]  (cogvideox_transformer_3d.py:122-136,186)
  HipCogVideoXAttnProcessor2_0    -- an AttnProcessor         (attention_processor.py:2024-2036,2094-2097)

Same call signatures, argument meaning and error behaviour as the reference objects; all arithmetic runs in
libs2v_hip.so.  Arguments the fork accepts but never honours are accepted and ignored the same way; arguments whose
honouring would need code that does not exist here raise NotImplementedError instead of silently deviating.
"""
from types import SimpleNamespace

import torch

from . import _lib
from .config import TransformerConfig
from .engine import S2VEngine
from .weights import concat_lora


def _rope_pair(image_rotary_emb, ref_image_rotary_emb, R):
    """[ref | video] cos/sin tables for the packed sequence; a missing ref table means identity rotation."""
    cos, sin = image_rotary_emb
    if ref_image_rotary_emb is not None:
        rc, rs = ref_image_rotary_emb
    else:
        rc = torch.ones((R, cos.shape[1]), dtype=cos.dtype, device=cos.device)
        rs = torch.zeros((R, cos.shape[1]), dtype=cos.dtype, device=cos.device)
    return torch.cat([rc.to(cos.device), cos], dim=0), torch.cat([rs.to(sin.device), sin], dim=0)


class _Cache:
    """recompute the conditioning only when the caller's tensors changed (the rotary tables have the same kind of key on the engine
    itself: S2VEngine.ensure_rope).

    The key holds STRONG references to the tensors (so their storage cannot be freed and handed to a different tensor at the
    same address) and compares object identity + in-place version; it also records the engine's epoch for its kind of state
    ("rope" / "cond"), which every S2VEngine.set_rope / set_pos_embed / set_conditioning / set_geometry bumps -- a write that
    did not go through this cache (the fused pipeline, another seam object sharing the engine) invalidates it."""

    def __init__(self, kind):
        self.kind = kind
        self.key = None

    def changed(self, engine, *tensors):
        epoch = engine.epoch[self.kind]
        k = self.key
        same = (k is not None and k[0] == epoch and len(k[1]) == len(tensors)
                and all((a is None and t is None) or (a is not None and t is not None and a[0] is t and a[1] == t._version)
                        for a, t in zip(k[1], tensors)))
        return not same

    def store(self, engine, *tensors):
        """call AFTER the engine was updated: records the post-update epoch"""
        self.key = (engine.epoch[self.kind], tuple(None if t is None else (t, t._version) for t in tensors))


class HipCogVideoXTransformer3DModel:
    def __init__(self, cfg: TransformerConfig, dtype=torch.bfloat16, device="cuda:0", force_simple=False):
        self.engine = S2VEngine(cfg, dtype, device, force_simple)
        self.config = SimpleNamespace(
            in_channels=cfg.in_channels, out_channels=cfg.out_channels, patch_size=cfg.patch_size,
            attention_head_dim=cfg.attention_head_dim, num_attention_heads=cfg.num_attention_heads,
            num_layers=cfg.num_layers, time_embed_dim=cfg.time_embed_dim, text_embed_dim=cfg.text_embed_dim,
            use_rotary_positional_embeddings=cfg.use_rotary_positional_embeddings)
        self.dtype = dtype
        self.device = self.engine.device
        self.qk_replace = False  # set by CustomCogVideoXPipeline.__init__ (custom_cogvideox_pipe.py:41); never read
        self._cond_cache = _Cache("cond")
        self.transformer_blocks = [HipCogVideoXBlock(self.engine, i) for i in range(cfg.num_layers)]

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def load_state_dict(self, sd, lora=None, lora_scale=0.5, strict=True):
        self.engine.load_state_dict(sd, lora, lora_scale)

    # PEFT's switches on a runtime-mode model (TransformerConfig.lora_runtime_rank > 0); the engine refuses them with the mode off.  The
    # engine alone knows which adapter was attached last and at which scale (load_state_dict, engine.attach_lora, checkpoint.swap_lora)
    def set_adapters_scale(self, scale):
        self.engine.set_lora_scale(scale)

    def disable_adapters(self):
        self.engine.detach_lora()

    def enable_adapters(self):
        self.engine.enable_lora()

    def __call__(self, hidden_states, ref_img_states=None, encoder_hidden_states=None, timestep=None,
                 timestep_cond=None, image_rotary_emb=None, ref_image_rotary_emb=None, attention_kwargs=None,
                 return_dict=True, eval=False):
        if timestep_cond is not None:
            raise NotImplementedError("timestep_cond: TimestepEmbedding.cond_proj does not exist in CogVideoX")
        if ref_img_states is None:
            raise TypeError("ref_img_states is required (cogvideox_transformer_3d.py:496 dereferences it)")
        B, F, C, H, W = hidden_states.shape
        if not eval and ref_img_states.shape[0] != B:
            raise RuntimeError("eval=False needs ref_img_states with the batch of hidden_states "
                               "(the reference only duplicates it under eval=True, :503-504)")
        if eval and B != 2 * ref_img_states.shape[0]:
            raise RuntimeError(f"Sizes of tensors must match: eval=True duplicates ref_img_states exactly x2 "
                               f"(:503-504) but hidden_states has batch {B}")
        if B > S2VEngine.MAX_BATCH:
            raise NotImplementedError(f"a batch of {B} samples: at most {S2VEngine.MAX_BATCH} per call (the CFG pairs of "
                                      f"{S2VEngine.MAX_BATCH // 2} videos)")
        # eval=True: ref_img_states [b] is duplicated over [negative x b | positive x b], sample j sees reference j mod b (:503-504);
        # eval=False: one row per sample.  The engine maps sample j to reference j mod n_ref in both cases
        use_rope = self.config.use_rotary_positional_embeddings
        if use_rope and image_rotary_emb is None:
            raise TypeError("'NoneType' object is not subscriptable: a RoPE model needs image_rotary_emb")
        eng = self.engine
        T = encoder_hidden_states.shape[1]
        if eng.geometry != (B, T, F, H, W):
            eng.set_geometry(B, T, F, H, W)
            if not use_rope:
                eng.prepare_tables(H * 8, W * 8)  # the reference rebuilds this table on every forward (:433-446)
        if image_rotary_emb is not None:
            ref = ref_image_rotary_emb
            key = (image_rotary_emb[0], image_rotary_emb[1], None if ref is None else ref[0], None if ref is None else ref[1])
            eng.ensure_rope(key, lambda: _rope_pair(image_rotary_emb, ref, (H // 2) * (W // 2)))
        if self._cond_cache.changed(eng, encoder_hidden_states, ref_img_states):
            eng.set_conditioning(encoder_hidden_states, ref_img_states)
            self._cond_cache.store(eng, encoder_hidden_states, ref_img_states)
        t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep] * B)
        out = eng.forward(hidden_states, t.reshape(-1).float())
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)

    forward = __call__


class HipCogVideoXBlock(torch.nn.Module):
    """transformer.transformer_blocks[i] replacement (Block-module seam).  An nn.Module (without parameters: the weights live in the
    engine's arena) so that `transformer.transformer_blocks[i] = HipCogVideoXBlock(engine, i)` is accepted by the reference's
    nn.ModuleList (cogvideox_transformer_3d.py:315-330)."""

    def __init__(self, engine: S2VEngine, layer: int):
        super().__init__()
        self.engine, self.layer = engine, layer

    def forward(self, hidden_states, encoder_hidden_states, temb, enc_hidden_states1=None, image_rotary_emb=None,
                 embed_ref_img=False, ref_img_seq_start=None, ref_img_seq_end=None, position_delta=None,
                 timestep=None, layer=None, ref_image_rotary_emb=None):
        if enc_hidden_states1 is None:
            raise TypeError("enc_hidden_states1 is required (normalization.py:482 / cogvideox_transformer_3d.py:167)")
        if position_delta is not None and (torch.is_tensor(position_delta) or position_delta != 0):
            raise NotImplementedError("position_delta != 0 (the fork always passes 0, cogvideox_transformer_3d.py:513)")
        eng = self.engine
        B, V, D = hidden_states.shape
        T, R = encoder_hidden_states.shape[1], enc_hidden_states1.shape[1]
        if V % R != 0:
            raise RuntimeError("video tokens must be a whole number of frames of the reference image's token count")
        geo = (B, T, V // R, 2, 2 * R)
        if eng.geometry != geo:
            eng.set_geometry(*geo)
        if image_rotary_emb is not None:
            ref = ref_image_rotary_emb if embed_ref_img else None
            key = (image_rotary_emb[0], image_rotary_emb[1], None if ref is None else ref[0], None if ref is None else ref[1])
            eng.ensure_rope(key, lambda: _rope_pair(image_rotary_emb, ref, R))
        else:
            eng.ensure_no_rope()
        return eng.block_forward(self.layer, hidden_states, encoder_hidden_states, enc_hidden_states1, temb)


_ATTN_PARTS = (("to_q", lambda a: a.to_q), ("to_k", lambda a: a.to_k), ("to_v", lambda a: a.to_v), ("to_out.0", lambda a: a.to_out[0]),
               ("norm_q", lambda a: a.norm_q), ("norm_k", lambda a: a.norm_k))
_TUNER_ATTRS = ("base_layer", "lora_A", "lora_B", "scaling", "active_adapters", "merged", "disable_adapters")


def _is_tuner_layer(mod):
    """a PEFT LoRA tuner layer, duck-typed: what peft.tuners.lora.LoraLayer exposes"""
    return all(hasattr(mod, a) for a in _TUNER_ATTRS)


def _attn_state(attn, split=False):
    """[(key name, base weight, base bias, [(A [r, in], B [out, r], scale) of the adapters to merge])] of the six attn1 parts, and the flat list
    of what the weights depend on (tensors and adapter settings) that _AttnPool keys a module's slot on.  split (lora="runtime"): the list
    comes as (base weights and whether they hold a merged delta, adapter tensors and settings): a change of the second re-attaches, it does not re-pack"""
    parts, deps, base_deps = [], [], []
    for name, get in _ATTN_PARTS:
        mod = get(attn)
        deltas = []
        if _is_tuner_layer(mod):
            base = mod.base_layer
            merged, disabled = bool(mod.merged), bool(mod.disable_adapters)
            active = mod.active_adapters
            active = [active] if isinstance(active, str) else list(active)
            deps += [merged, disabled, tuple(active)]
            base_deps.append(merged)
            if not merged and not disabled:  # merged: the delta is in base_layer.weight already; disabled: the base layer alone
                for a in active:
                    if a not in mod.lora_A:
                        continue  # peft skips an active adapter this layer does not carry
                    if getattr(mod, "use_dora", {}).get(a, False):
                        raise NotImplementedError(f"DoRA adapter {a!r} on {name}: only plain LoRA (W + scaling * B A) is merged")
                    A, B, sc = mod.lora_A[a].weight, mod.lora_B[a].weight, float(mod.scaling[a])
                    deltas.append((A, B, sc))
                    deps += [A, B, sc]
        else:
            base = mod
        parts.append((name, base.weight, base.bias, deltas))
        deps += [base.weight, base.bias]
        base_deps += [base.weight, base.bias]
    if split:
        nb = set(map(id, base_deps))
        return parts, (base_deps, [d for d in deps if not (torch.is_tensor(d) and id(d) in nb)])
    return parts, deps


def _dep_key(deps):
    """identity + in-place version + storage address of every tensor (held by STRONG reference, as _Cache does), the value of every setting"""
    return tuple((d, d._version, d.data_ptr()) if torch.is_tensor(d) else (None, d, None) for d in deps)


def _same_key(key, deps):
    return (key is not None and len(key) == len(deps)
            and all((k[0] is d and k[1] == d._version and k[2] == d.data_ptr()) if torch.is_tensor(d) else (k[0] is None and k[1] == d)
                    for k, d in zip(key, deps)))


class _AttnPool:
    """Every Attention module of one (device, dtype, heads, inner dim, force_simple) runs on ONE workspace engine (geometry, activation
    workspace, rotary tables: S2V_CTX_ATTN_WORKSPACE) with its own attention-weights engine (the module's attn1 weights alone, re-packed
    as a model packs them: S2V_CTX_ATTN_WEIGHTS), through s2v_attn_forward_with."""

    def __init__(self, heads, dtype, device, force_simple, lora_runtime_rank=0):
        # the workspace engine owns the activation pitch, every weights engine the tails and the A stacks: one lora_runtime_rank for all
        self.cfg = TransformerConfig(num_layers=1, num_attention_heads=heads, time_embed_dim=8, text_embed_dim=64,
                                     use_rotary_positional_embeddings=True, lora_runtime_rank=lora_runtime_rank)
        self.dtype, self.device, self.force_simple = dtype, device, force_simple
        self.engine = S2VEngine(self.cfg, dtype, device, force_simple, kind=_lib.CTX_ATTN_WORKSPACE)
        self.slots = {}       # id(attn) -> (weights engine, key, attn); the module is kept alive: id(attn) stays unique
        self.geometry_changes = 0

    def weights_for_runtime(self, attn):
        """lora="runtime": the slot keys the base weights and the adapter separately -- (weights engine, (base key, adapter key), attn).  A changed
        scaling, disable_adapters or another active adapter re-attaches (the tails and A stacks: megabytes) on the SAME weights engine"""
        parts, (base_deps, ad_deps) = _attn_state(attn, split=True)
        slot = self.slots.get(id(attn))
        p = "transformer_blocks.0.attn1."
        if slot is not None and _same_key(slot[1][0], base_deps):
            eng = slot[0]
            if _same_key(slot[1][1], ad_deps):
                return eng
        else:
            eng = None
        # the capacity is checked before anything is allocated or changed
        lora, cap = {}, self.cfg.lora_runtime_rank
        for name, _, _, deltas in parts:
            if not deltas:
                continue
            total = sum(int(A.shape[0]) for A, _, _ in deltas)
            if total > cap:
                raise _lib.S2VError(f"{name}: the active adapters' ranks sum to {total}, over the capacity lora_runtime_rank = {cap} "
                                    f"(several active adapters are concatenated along r)")
            # several active adapters on one layer: [A_1; A_2], [s_1 B_1 | s_2 B_2] at scale 1 is the sum of the branches
            lora[p + name + ".weight"] = concat_lora([(A.detach(), B.detach(), sc) for A, B, sc in deltas])
        fresh = eng is None
        if fresh:
            eng = S2VEngine(self.cfg, self.dtype, self.device, self.force_simple, kind=_lib.CTX_ATTN_WEIGHTS)
        try:
            if fresh:
                for name, w, b, _ in parts:
                    eng.load_weight(p + name + ".weight", w.detach())
                    eng.load_weight(p + name + ".bias", b.detach())
                eng.finalize_weights()
            if lora:
                eng.attach_lora(lora, 1.0)
            elif eng.lora_state["attached"]:
                eng.detach_lora()
        except Exception:
            if fresh:
                eng.close()               # the old slot, if any, stays as it was
            else:
                self.slots.pop(id(attn))  # attach_lora left it detached: the next call re-packs
                eng.close()
            raise
        eng.forget_lora()                 # the module owns its adapter tensors: no second copy kept for a detached context
        if fresh and slot is not None:
            slot[0].close()
        self.slots[id(attn)] = (eng, (_dep_key(base_deps), _dep_key(ad_deps)), attn)
        return eng

    def weights_for(self, attn):
        if self.cfg.lora_runtime_rank > 0:
            return self.weights_for_runtime(attn)
        parts, deps = _attn_state(attn)
        slot = self.slots.get(id(attn))
        if slot is not None and _same_key(slot[1], deps):
            return slot[0]
        eng = S2VEngine(self.cfg, self.dtype, self.device, self.force_simple, kind=_lib.CTX_ATTN_WEIGHTS)
        p = "transformer_blocks.0.attn1."
        for name, w, b, _ in parts:
            eng.load_weight(p + name + ".weight", w.detach())
            eng.load_weight(p + name + ".bias", b.detach())
        for name, _, _, deltas in parts:
            for A, B, sc in deltas:
                eng.merge_lora(p + name + ".weight", A.detach(), B.detach(), sc)
        eng.finalize_weights()
        if slot is not None:
            slot[0].close()
        self.slots[id(attn)] = (eng, _dep_key(deps), attn)
        return eng

    def set_geometry(self, geo):
        self.engine.set_geometry(*geo)
        self.geometry_changes += 1

    def memory_bytes(self):
        weights = sum(s[0].device_bytes()[0] for s in self.slots.values()) + self.engine.device_bytes()[0]
        return {"weights": weights, "workspace": self.engine.device_bytes()[1]}

    def close(self):
        for s in self.slots.values():
            s[0].close()
        self.slots.clear()
        self.engine.close()


_POOLS = {}  # (device, dtype, heads, inner dim, force_simple) -> _AttnPool, shared by every HipCogVideoXAttnProcessor2_0 of the process


class HipCogVideoXAttnProcessor2_0:
    """AttnProcessor seam: `attn.set_processor(HipCogVideoXAttnProcessor2_0())`, or model-wide through the reference's
    `transformer.set_attn_processor(proc)` (cogvideox_transformer_3d.py:376-408) -- one instance or a dict of instances alike.

    Weights are read from the Attention module that owns them (to_q/to_k/to_v/to_out[0]/norm_q/norm_k, attention_processor.py:2049-2090)
    and re-packed into an attention-only weights context per module; every module of a (device, dtype, heads, inner dim, force_simple)
    runs on ONE process-wide workspace (_AttnPool): one activation workspace and one rotary-table upload per model, not per module.
    A module is re-packed before the call whenever what its weights depend on changed (identity, in-place version and storage of its
    twelve tensors and of its adapter tensors, and the adapter settings): load_state_dict, an in-place copy_, a fuse / unfuse or
    enable / disable of adapters.  Writes through `.data` that keep the storage escape the version counter.

    PEFT LoRA tuner layers (duck-typed: base_layer, lora_A / lora_B keyed by adapter name, scaling, active_adapters, merged,
    disable_adapters) are honoured by merging W + sum over the active adapters of scaling[a] * B_a A_a into the module's weights context
    (s2v_merge_lora, fp32 A and B, rounded once per adapter to the model dtype) with the bias of base_layer; nothing is added when
    `merged` (the delta is in base_layer.weight already), the base layer alone when `disable_adapters`.  This is the merge the engine
    applies to checkpoints and the default, lora="merge": it costs nothing per call.

    lora="runtime" runs the adapter as the reference does, as a branch beside the base weights (include/s2v_hip.h, s2v_lora_attach:
    T = rnd(x A^T), rnd(s B) in the weight's tail, one fp32 accumulator under the unchanged epilogue): a tuner layer that is unmerged and
    enabled is ATTACHED to the module's weights context, whose slot keys the base weights and the adapter separately, so a changed scaling,
    disable_adapters or another active adapter re-attaches and does not re-pack the module.  Several active adapters on one layer are
    concatenated along r while their ranks sum to at most lora_runtime_rank (S2VError otherwise).  The PEFT runtime path is pinned by
    tests/test_gpu_lora_runtime.py against PEFT's Linear.forward restated in fp32.  DoRA adapters raise NotImplementedError in both modes."""

    def __init__(self, force_simple=False, lora="merge", lora_runtime_rank=128):
        if lora not in ("merge", "runtime"):
            raise ValueError(f"lora must be 'merge' or 'runtime', got {lora!r}")
        self._force_simple = force_simple
        self._rank = int(lora_runtime_rank) if lora == "runtime" else 0
        self._keys = set()

    def _pool_for(self, attn, dtype, device, D):
        key = (device, dtype, attn.heads, D, self._force_simple) + ((self._rank,) if self._rank else ())
        if key not in _POOLS:
            _POOLS[key] = _AttnPool(attn.heads, dtype, device, self._force_simple, self._rank)
        self._keys.add(key)
        return _POOLS[key]

    def pools(self):
        """the pools this processor has run on (and that release_pools has not dropped)"""
        return [_POOLS[k] for k in self._keys if k in _POOLS]

    def memory_bytes(self):
        """{"weights", "workspace"}: device bytes the library holds for the pools this processor runs on (s2v_device_bytes): every module's
        attention-weights context, and each pool's one workspace"""
        out = {"weights": 0, "workspace": 0}
        for pool in self.pools():
            for k, v in pool.memory_bytes().items():
                out[k] += v
        return out

    @staticmethod
    def release_pools():
        """free every pool of the process (weights contexts and workspaces); a processor called afterwards re-packs its modules"""
        for pool in _POOLS.values():
            pool.close()
        _POOLS.clear()

    def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask=None, image_rotary_emb=None,
                 ref_img_seq_start=0, ref_img_seq_end=0, position_delta=None, embed_ref_img=False,
                 ref_image_rotary_emb=None):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask: the CogVideoX path always passes None (:2083-2085)")
        if position_delta is not None and (torch.is_tensor(position_delta) or position_delta != 0):
            raise NotImplementedError("position_delta != 0 (the fork always passes 0)")
        if getattr(attn, "is_cross_attention", False):
            raise NotImplementedError("cross-attention variant is not part of this path")
        B, V, D = hidden_states.shape
        TR = encoder_hidden_states.shape[1]
        if not embed_ref_img or ref_img_seq_end != TR or not (0 <= ref_img_seq_start < ref_img_seq_end):
            raise NotImplementedError("the fork always calls with embed_ref_img=True and the reference-image tokens at "
                                      "the tail of encoder_hidden_states (cogvideox_transformer_3d.py:510-512)")
        T, R = ref_img_seq_start, ref_img_seq_end - ref_img_seq_start
        pool = self._pool_for(attn, hidden_states.dtype, hidden_states.device, D)
        weights = pool.weights_for(attn)
        eng = pool.engine
        geo = (B, T, V // R, 2, 2 * R)
        if V % R != 0:
            raise RuntimeError("video tokens must be a whole number of frames of the reference image's token count")
        if eng.geometry != geo:
            pool.set_geometry(geo)
        if image_rotary_emb is not None:
            ref = ref_image_rotary_emb
            key = (image_rotary_emb[0], image_rotary_emb[1], None if ref is None else ref[0], None if ref is None else ref[1])
            eng.ensure_rope(key, lambda: _rope_pair(image_rotary_emb, ref, R))
        else:
            eng.ensure_no_rope()
        return eng.attn_forward_with(weights, 0, hidden_states, encoder_hidden_states)
