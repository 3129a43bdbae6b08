"""Thin object wrapper over the C ABI context (include/s2v_hip.h).  torch is used for device memory and streams
only; every arithmetic step of the path runs in libs2v_hip.so."""
import ctypes

import numpy as np
import torch

from . import _lib, tables
from .config import TransformerConfig


class _ArenaView:
    """exposes a raw device range through __cuda_array_interface__ so torch.distributed can broadcast it"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def _is_seq(x):
    return isinstance(x, (list, tuple)) or (isinstance(x, (torch.Tensor, np.ndarray)) and x.ndim > 0)


def _per_video(name, x, b):
    """x as a list of b entries: a sequence of b, or one value repeated"""
    xs = list(x) if _is_seq(x) else [x]
    if len(xs) == 1 and not _is_seq(x):
        xs = xs * b
    if len(xs) != b:
        raise _lib.S2VError(f"denoise_step: `{name}` has {len(xs)} entries for b = {b} videos (one per video, or a scalar for all)")
    return xs


def mask_to_latent(mask, device=None):
    """pixel masks [r,F,H,W] (uint8 / bool: non-zero repaints; float32 / bfloat16 / float16: binarised at 0.5 as image_processor.py:535-536
    does; anything else goes through float32) -> (latent mask uint8 [r,(F-1)/4+1,H/8,W/8], binarised pixel mask uint8 [r,F,H,W]), one
    s2v_mask_to_latent launch per row: a latent cell repaints if ANY pixel it covers does (include/s2v_hip.h)"""
    if mask.ndim != 4:
        raise _lib.S2VError(f"mask_to_latent: the masks must be [rows, F, H, W], got {tuple(mask.shape)}")
    r, F, H, W = mask.shape
    if (F - 1) % 4 or H % 8 or W % 8 or min(r, H, W) < 1:
        raise _lib.S2VError(f"mask_to_latent: F = 4k + 1 frames of H x W pixels, both multiples of 8, got {tuple(mask.shape)}")
    m = mask.to(device or mask.device)
    if m.dtype == torch.bool:
        m = m.view(torch.uint8) if m.is_contiguous() else m.to(torch.uint8)
    elif m.dtype != torch.uint8 and m.dtype not in _lib.DTYPE_OF:
        m = m.float()
    m = m.contiguous()
    md = _lib.MASK_DTYPE_U8 if m.dtype == torch.uint8 else _lib.DTYPE_OF[m.dtype]
    lat = torch.empty((r, (F - 1) // 4 + 1, H // 8, W // 8), dtype=torch.uint8, device=m.device)
    pix = torch.empty((r, F, H, W), dtype=torch.uint8, device=m.device)
    for k in range(r):
        _lib.check(_lib.lib().s2v_mask_to_latent(_lib.ptr(m[k]), md, F, H, W, _lib.ptr(lat[k]), _lib.ptr(pix[k]), _lib.stream_ptr()))
    return lat, pix


def map_to_latent(change_map, device=None):
    """change maps [r,F,H,W] (uint8: levels 0..255; float32 / bfloat16 / float16: values in [0, 1], level = floor(clamp(v, 0, 1) * 255 + 0.5),
    NaN -> 0; anything else goes through float32) -> (latent levels uint8 [r,(F-1)/4+1,H/8,W/8], pixel mask `level > 0` uint8 [r,F,H,W]), one
    s2v_map_to_latent launch per row: a latent cell takes the MAXIMUM level of the pixels it covers (include/s2v_hip.h)"""
    if change_map.ndim != 4:
        raise _lib.S2VError(f"map_to_latent: the maps must be [rows, F, H, W], got {tuple(change_map.shape)}")
    r, F, H, W = change_map.shape
    if (F - 1) % 4 or H % 8 or W % 8 or min(r, H, W) < 1:
        raise _lib.S2VError(f"map_to_latent: F = 4k + 1 frames of H x W pixels, both multiples of 8, got {tuple(change_map.shape)}")
    m = change_map.to(device or change_map.device)
    if m.dtype != torch.uint8 and m.dtype not in _lib.DTYPE_OF:
        m = m.float()
    m = m.contiguous()
    md = _lib.MASK_DTYPE_U8 if m.dtype == torch.uint8 else _lib.DTYPE_OF[m.dtype]
    lat = torch.empty((r, (F - 1) // 4 + 1, H // 8, W // 8), dtype=torch.uint8, device=m.device)
    pix = torch.empty((r, F, H, W), dtype=torch.uint8, device=m.device)
    for k in range(r):
        _lib.check(_lib.lib().s2v_map_to_latent(_lib.ptr(m[k]), md, F, H, W, _lib.ptr(lat[k]), _lib.ptr(pix[k]), _lib.stream_ptr()))
    return lat, pix


class S2VEngine:
    def __init__(self, cfg: TransformerConfig, dtype=torch.bfloat16, device="cuda:0", force_simple=False, kind=_lib.CTX_MODEL):
        """kind: _lib.CTX_MODEL (a whole model), or one of the two halves of the model-wide AttnProcessor (include/s2v_hip.h, S2V_CTX_*):
        CTX_ATTN_WEIGHTS (the attn1 weights of cfg.num_layers blocks, no workspace) / CTX_ATTN_WORKSPACE (geometry, workspace and rotary
        tables, no weights; runs another engine's weights through attn_forward_with)"""
        if dtype not in _lib.DTYPE_OF:
            raise _lib.S2VError(f"unsupported model dtype {dtype} (float32, bfloat16 and float16 are implemented)")
        if cfg.attention_head_dim != 64:
            raise _lib.S2VError("attention_head_dim must be 64")
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.D = cfg.inner_dim
        torch.cuda.set_device(self.device)
        c = _lib.ModelConfigC()
        c.num_layers, c.num_heads = cfg.num_layers, cfg.num_attention_heads
        c.in_channels, c.out_channels, c.patch_size = cfg.in_channels, cfg.out_channels, cfg.patch_size
        c.time_embed_dim, c.text_embed_dim = cfg.time_embed_dim, cfg.text_embed_dim
        c.use_rope = int(cfg.use_rotary_positional_embeddings)
        c.dtype = _lib.DTYPE_OF[dtype]
        c.norm_eps = cfg.norm_eps
        c.force_simple = int(force_simple)
        if cfg.weight_format not in (None, "fp8", "fp8-qk", "fp8-auto"):
            raise _lib.S2VError(f"unknown weight_format {cfg.weight_format!r} (None, 'fp8', 'fp8-qk' or 'fp8-auto')")
        c.weight_format = {None: 0, "fp8": 1, "fp8-qk": 2, "fp8-auto": 3}[cfg.weight_format]
        if cfg.lora_adaln_scope not in ("shipped", "intended"):
            raise _lib.S2VError(f"unknown lora_adaln_scope {cfg.lora_adaln_scope!r} ('shipped' or 'intended')")
        c.lora_adaln_scope = 1 if cfg.lora_adaln_scope == "intended" else 0
        if cfg.attn_p_format not in ("bf16", "f16", "auto"):
            raise _lib.S2VError(f"unknown attn_p_format {cfg.attn_p_format!r} ('bf16', 'f16' or 'auto')")
        c.attn_p_format = 0 if cfg.attn_p_format == "bf16" else 1
        c.reserved[0] = kind
        # reserved[1]: the rank in the low 16 bits, S2V_LORA_FP8_BRANCH above it (include/s2v_hip.h): cfg.lora_runtime_fp8 asks an fp8
        # weight_format for the 16-bit adapter branch beside its e4m3 weights
        c.reserved[1] = int(getattr(cfg, "lora_runtime_rank", 0) or 0)
        if c.reserved[1] > 0 and c.weight_format != 0 and getattr(cfg, "lora_runtime_fp8", False):
            c.reserved[1] |= _lib.LORA_FP8_BRANCH
        self.kind = kind
        # runtime adapter mode: the attached adapter's fp32 device copies {name: (A2, B2)} (set_lora_scale re-reads them), and the last
        # adapter attached with its current scale, kept across detach_lora so that enable_lora can put it back (lora_kept_bytes counts it)
        self._lora = None
        self._lora_last = None
        # "auto" (opt-in): start with fp16 P (faster on smooth score distributions) and look at the slow-path census after the first denoise
        # step of a geometry (re-armed by set_geometry); more than AUTO_SLOW_FRACTION of the (wave, KV tile) pairs on the slow path -> bf16 P
        # (threshold 2^64).  The census read synchronises the device (s2v_attn_slow_stats): the deciding step runs eagerly, never inside a
        # caller's stream capture; forward() / the seam objects take no census and keep the format they find.
        self.attn_p_format = "f16" if c.attn_p_format else "bf16"
        self._attn_auto_pending = cfg.attn_p_format == "auto"
        self.attn_slow_fraction = None
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib().s2v_create(ctypes.byref(c), ctypes.byref(self._h)))
        self.geometry = None
        self._keep = []
        # bumped by every write of the engine-side RoPE / positional table ("rope") and conditioning ("cond"): the seam
        # adapters' caches (transformer._Cache) are valid only for the epoch they were stored at
        self.epoch = {"rope": 0, "cond": 0}
        self._rope_key, self.have_rope = None, None  # ensure_rope / ensure_no_rope

    def close(self):
        if self._h:
            torch.cuda.synchronize(self.device)
            _lib.lib().s2v_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights -----------------------------------------------------------------------------------------
    def load_weight(self, name, tensor):
        t = tensor.to(self.device)
        if t.dtype not in _lib.DTYPE_OF:
            t = t.float()
        t = t.contiguous()
        shape = (ctypes.c_int64 * t.ndim)(*t.shape)
        _lib.check(_lib.lib().s2v_load_weight(self._h, name.encode(), _lib.ptr(t), shape, t.ndim,
                                              _lib.DTYPE_OF[t.dtype], _lib.stream_ptr()))
        self._keep.append(t)  # alive until the stream has consumed it

    def load_state_dict(self, sd, lora=None, lora_scale=0.5):
        """sd: {reference state-dict key: tensor}; lora: {weight key: (A [r,in..], B [out,r])} merged as
        W + lora_scale * B A (src/inference.py:218-229: alpha/r = 64/128).  In the runtime adapter mode (cfg.lora_runtime_rank > 0) the
        base weights are finalized as they are and the adapter is attached (attach_lora) instead of merged."""
        for k, v in sd.items():
            if "pos_embedding" in k:
                continue  # non-persistent buffer, rebuilt by tables.sincos_table
            self.load_weight(k, v)
        if self.cfg.lora_runtime_rank > 0:
            self.finalize_weights()
            self.unexpected_lora_keys = []
            if lora:
                self.attach_lora(lora, lora_scale)
            return
        placed = self._place_lora(lora)
        for k, (A, B) in placed.items():
            self.merge_lora(k, A, B, lora_scale)
        self.finalize_weights()

    def _place_lora(self, lora):
        """the adapter keys this model has; the others are reported as the reference does (src/inference.py:96-105) and skipped"""
        known, placed = None, {}
        self.unexpected_lora_keys = []
        for k, ab in (lora or {}).items():
            if known is None:
                from .weights import state_dict_shapes
                known = set(state_dict_shapes(self.cfg))
            if k not in known:
                self.unexpected_lora_keys.append(k)
                continue
            placed[k] = ab
        if self.unexpected_lora_keys:
            print(f"Loading adapter weights led to unexpected keys not found in the model: {self.unexpected_lora_keys}")
        return placed

    # ---- runtime adapters (cfg.lora_runtime_rank > 0; include/s2v_hip.h, s2v_lora_*) --------------------------------------------------
    def _lora_refusals(self, what, rank=0):
        """the library's own refusals, taken before anything is changed (attach_lora detaches first): the state stays as it was"""
        if self.cfg.lora_runtime_rank <= 0:
            raise _lib.S2VError(f"{what}: the runtime adapter mode is off (lora_runtime_rank = 0: this engine merges LoRA at load time)")
        if self.cfg.weight_format is not None and not getattr(self.cfg, "lora_runtime_fp8", False):
            raise _lib.S2VError(f"{what}: fp8 weight formats have no runtime adapter branch (weight_format {self.cfg.weight_format!r}) unless the "
                                f"engine is created with TransformerConfig.lora_runtime_fp8 = True")
        if self.shard is not None:
            raise _lib.S2VError(f"{what}: a shard engine (set_shard) does not support runtime adapters")
        if rank > self.cfg.lora_runtime_rank:
            raise _lib.S2VError(f"{what}: rank {rank} is over the capacity lora_runtime_rank = {self.cfg.lora_runtime_rank}")

    def attach_lora(self, lora, scale=0.5):
        """replace the attached adapter by lora = {weight key: (A [r, in..], B [out, r])} at `scale`, after finalize_weights: the six token
        linears of every block run base + branch, the other targets are re-merged from their base copy; no base weight is touched"""
        ranks = [int(A.shape[0]) for A, _ in lora.values()]
        self._lora_refusals("attach_lora", max(ranks, default=0))
        placed = self._place_lora(lora) if self.kind == _lib.CTX_MODEL else dict(lora)
        dev = {k: (A.to(self.device).float().reshape(A.shape[0], -1).contiguous(), B.to(self.device).float().contiguous())
               for k, (A, B) in placed.items()}
        for k, (A2, B2) in dev.items():
            if B2.ndim != 2 or B2.shape[1] != A2.shape[0]:
                raise _lib.S2VError(f"attach_lora: {k}: A {tuple(A2.shape)} and B {tuple(B2.shape)} do not share a rank")
        # every name is checked before anything changes: s2v_weight_slot knows the names of THIS context (an attention-weights context
        # holds the attn1 keys only) and the base shapes
        off, rows, cols, ld = (ctypes.c_int64() for _ in range(4))
        for k, (A2, B2) in dev.items():
            _lib.check(_lib.lib().s2v_weight_slot(self._h, k.encode(), ctypes.byref(off), ctypes.byref(rows), ctypes.byref(cols), ctypes.byref(ld)))
            if (B2.shape[0], A2.shape[1]) != (rows.value, cols.value):
                raise _lib.S2VError(f"attach_lora: {k}: B A is {B2.shape[0]} x {A2.shape[1]}, the weight is {rows.value} x {cols.value}")
        _lib.check(_lib.lib().s2v_lora_detach(self._h, _lib.stream_ptr()))
        self._lora = None
        try:
            for k, (A2, B2) in dev.items():
                _lib.check(_lib.lib().s2v_lora_attach(self._h, k.encode(), _lib.ptr(A2), _lib.ptr(B2), A2.shape[0], float(scale), _lib.stream_ptr()))
        except Exception:
            # a refusal part way (a name that is no LoRA target of this context): never half attached -- the base model, loudly
            _lib.lib().s2v_lora_detach(self._h, _lib.stream_ptr())
            self._lora_changed()
            raise
        self._lora = dev
        self._lora_last = (dev, float(scale))
        self._lora_changed()

    def set_lora_scale(self, scale):
        """the attached adapter at another scale: bit for bit what attach_lora(lora, scale) gives; a captured denoise step is kept"""
        self._lora_refusals("set_lora_scale")
        if not self._lora:
            raise _lib.S2VError("set_lora_scale: no adapter is attached")
        for k, (A2, B2) in self._lora.items():
            _lib.check(_lib.lib().s2v_lora_set_scale(self._h, k.encode(), _lib.ptr(A2), _lib.ptr(B2), A2.shape[0], float(scale), _lib.stream_ptr()))
        self._lora_last = (self._lora, float(scale))
        self._lora_changed()

    def detach_lora(self):
        """the base model"""
        self._lora_refusals("detach_lora")
        _lib.check(_lib.lib().s2v_lora_detach(self._h, _lib.stream_ptr()))
        self._lora = None
        self._lora_changed()

    def enable_lora(self):
        """put back the adapter that was attached last (attach_lora, load_state_dict, checkpoint.swap_lora) at the scale it had last"""
        self._lora_refusals("enable_lora")
        if self._lora is not None:
            return
        if self._lora_last is None:
            raise _lib.S2VError("enable_lora: no adapter has been attached to this engine")
        self.attach_lora(*self._lora_last)

    def forget_lora(self):
        """drop the kept fp32 copies of a detached adapter (enable_lora then has nothing to put back)"""
        if self._lora is None:
            self._lora_last = None

    @property
    def lora_kept_bytes(self):
        """device bytes of the fp32 A / B copies this engine keeps for set_lora_scale / enable_lora (torch tensors: outside s2v_device_bytes)"""
        kept = self._lora_last[0] if self._lora_last else (self._lora or {})
        return sum(A.numel() * 4 + B.numel() * 4 for A, B in kept.values())

    @property
    def lora_state(self):
        """{"attached": names attached, "rank", "scale": of the last attach / rescale, "graph_captures": hipGraph captures so far}"""
        n, r, s, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_float(), ctypes.c_int64()
        _lib.check(_lib.lib().s2v_lora_state(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(s), ctypes.byref(g)))
        return {"attached": n.value, "rank": r.value, "scale": s.value, "graph_captures": g.value}

    def merge_lora(self, name, A, B, scale):
        """W[name] += scale * B A (s2v_merge_lora: A [r, in..] and B [out, r] as fp32, after load_weight(name), before finalize_weights)"""
        A2 = A.to(self.device).float().reshape(A.shape[0], -1).contiguous()
        B2 = B.to(self.device).float().contiguous()
        _lib.check(_lib.lib().s2v_merge_lora(self._h, name.encode(), _lib.ptr(A2), _lib.ptr(B2), A2.shape[0],
                                             float(scale), _lib.stream_ptr()))
        self._keep += [A2, B2]  # the merge is stream-ordered

    def finalize_weights(self):
        _lib.check(_lib.lib().s2v_finalize_weights(self._h, _lib.stream_ptr()))
        torch.cuda.synchronize(self.device)
        self._keep.clear()

    def weight_arena(self):
        """uint8 CUDA tensor aliasing the packed, context-owned weights (one RCCL broadcast replicates a model)."""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(_lib.lib().s2v_weight_arena(self._h, ctypes.byref(p), ctypes.byref(n)))
        return torch.as_tensor(_ArenaView(p.value, n.value), device=self.device)

    def weight_arenas(self):
        return [self.weight_arena()]

    def read_weight(self, name):
        """one state-dict tensor as it sits in the arena (after load / LoRA merge), [rows, cols] in the model dtype: a strided view
        of weight_arena() located by s2v_weight_slot (biases / norm vectors come back as [1, n]; conv weights flattened to
        [out, in * kh * kw])"""
        off, rows, cols, ld = (ctypes.c_int64() for _ in range(4))
        _lib.check(_lib.lib().s2v_weight_slot(self._h, name.encode(), ctypes.byref(off), ctypes.byref(rows), ctypes.byref(cols), ctypes.byref(ld)))
        esz = torch.empty((), dtype=self.dtype).element_size()
        flat = self.weight_arena()[off.value : off.value + ((rows.value - 1) * ld.value + cols.value) * esz].view(self.dtype)
        return flat.as_strided((rows.value, cols.value), (ld.value, 1))

    def mark_weights_loaded(self):
        _lib.check(_lib.lib().s2v_mark_weights_loaded(self._h))

    def device_bytes(self):
        """(weight arena, workspace): device bytes the library holds for this context (s2v_device_bytes)"""
        a, w = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.lib().s2v_device_bytes(self._h, ctypes.byref(a), ctypes.byref(w)))
        return a.value, w.value

    # ---- geometry / tables / conditioning ----------------------------------------------------------------------
    def _bump(self, *kinds):
        for k in kinds:
            self.epoch[k] += 1

    @property
    def fp8_qk_active(self):
        """whether QK^T of the attention runs in fp8 at the current geometry ("fp8-qk": always; "fp8-auto": from the library's token threshold on).
        The library took the decision at s2v_set_geometry and is asked for it (s2v_fp8_qk_active): nothing is re-derived here."""
        if self.cfg.weight_format not in ("fp8-qk", "fp8-auto"):
            return False
        on = ctypes.c_int32()
        _lib.check(_lib.lib().s2v_fp8_qk_active(self._h, ctypes.byref(on)))
        return bool(on.value)

    MAX_BATCH = 8   # S2V_MAX_BATCH (include/s2v_hip.h): the CFG pairs of at most four videos per call

    def set_geometry(self, B, T, F, H, W):
        new = self.geometry != (B, T, F, H, W)
        _lib.check(_lib.lib().s2v_set_geometry(self._h, B, T, F, H, W))
        self.geometry = (B, T, F, H, W)
        if new and self.cfg.attn_p_format == "auto":  # a new geometry is new data to the kernel: decide again, starting from fp16
            if self.attn_p_format != "f16":
                self.set_attn_p_format("f16")
            self._attn_auto_pending = True
        self._rope_key, self.have_rope = None, None
        self._cond_args = None
        self.triples = False
        self.windows = None   # the library clears temporal windows with every set_geometry
        self._bump("rope", "cond")

    def clear_rope(self):
        _lib.check(_lib.lib().s2v_set_rope(self._h, None, None, _lib.stream_ptr()))
        self._rope_key, self.have_rope = None, False
        self._bump("rope")

    # One rotary-table cache PER ENGINE: the transformer object, its 42 block objects and an AttnProcessor all write the same device
    # table, so the "did the caller's tensors change" key lives here (a per-object key made every block re-upload the tables --
    # a stream sync, two D2H copies and a host scan each -- because its neighbour's upload had invalidated it).
    def ensure_rope(self, key_tensors, build):
        """key_tensors: the caller's table tensors (or None entries), compared by identity + in-place version, held by STRONG reference
        so their storage cannot be recycled under the key; build() -> (cos, sin) for set_rope when they changed"""
        k = self._rope_key
        same = (k is not None and len(k) == len(key_tensors)
                and all((a is None and t is None) or (a is not None and t is not None and a[0] is t and a[1] == t._version)
                        for a, t in zip(k, key_tensors)))
        if not same:
            self.set_rope(*build())
            self._rope_key = tuple(None if t is None else (t, t._version) for t in key_tensors)

    def ensure_no_rope(self):
        if self.have_rope is not False:
            self.clear_rope()

    def set_rope(self, cos, sin):
        cos = cos.to(self.device, torch.float32).contiguous()
        sin = sin.to(self.device, torch.float32).contiguous()
        B, T, F, H, W = self.geometry
        n = (H // 2) * (W // 2) * (F + 1)
        if tuple(cos.shape) != (n, 64) or tuple(sin.shape) != (n, 64):
            raise _lib.S2VError(f"RoPE tables must be [{n}, 64] ([ref | video] rows)")
        _lib.check(_lib.lib().s2v_set_rope(self._h, _lib.ptr(cos), _lib.ptr(sin), _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()
        self._rope_key, self.have_rope = None, True
        self._bump("rope")

    def set_pos_embed(self, table):
        t = table.to(self.device, self.dtype).contiguous()
        _lib.check(_lib.lib().s2v_set_pos_embed(self._h, _lib.ptr(t), _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()
        self._rope_key = None
        self._bump("rope")

    def prepare_tables(self, height, width):
        """build + upload the step-invariant positional tables for a video of height x width pixels"""
        B, T, F, H, W = self.geometry
        if self.cfg.use_rotary_positional_embeddings:
            cos, sin = tables.rope_tables(height, width, F)
            self.set_rope(torch.from_numpy(cos), torch.from_numpy(sin))
        else:
            pe = tables.sincos_table(self.D, H // 2, W // 2, F, self.cfg.spatial_interpolation_scale,
                                     self.cfg.temporal_interpolation_scale)
            self.set_pos_embed(torch.from_numpy(pe))

    def set_conditioning(self, text, ref_latent):
        """text [B,T,text_embed_dim]; ref_latent [n_ref,1,C,H,W] with n_ref in {1, B/2, B}: sample j of the batch takes reference j mod n_ref
        (1: one subject for every sample; B/2: the reference's eval=True duplication over [negative x b | positive x b]; B: one per sample)"""
        text = text.to(self.device, self.dtype).contiguous()
        ref = ref_latent.to(self.device, self.dtype).contiguous()
        B, T, F, H, W = self.geometry
        if tuple(text.shape) != (B, T, self.cfg.text_embed_dim):
            raise _lib.S2VError(f"text embeddings must be [{B},{T},{self.cfg.text_embed_dim}], got {tuple(text.shape)}")
        per_ref = self.cfg.in_channels * H * W
        if ref.numel() % per_ref != 0 or (ref.numel() != per_ref and (ref.ndim != 5 or ref.shape[0] * per_ref != ref.numel())):
            raise _lib.S2VError("ref_img_states must be [n_ref,1,C,H,W] with the geometry's H, W")
        n_ref = ref.numel() // per_ref
        if n_ref not in {1, B} | ({B // 2} if B % 2 == 0 else set()):
            raise _lib.S2VError(f"ref_img_states has {n_ref} rows: n_ref must be 1, B/2 or B for a batch of {B} samples "
                                f"(sample j takes reference j mod n_ref)")
        if n_ref == 1:
            _lib.check(_lib.lib().s2v_set_conditioning(self._h, _lib.ptr(text), _lib.ptr(ref), _lib.stream_ptr()))
        else:
            _lib.check(_lib.lib().s2v_set_conditioning_refs(self._h, _lib.ptr(text), _lib.ptr(ref), n_ref, _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()
        self._cond_args = (text, ref) if self.cfg.lora_runtime_rank > 0 else None
        self.triples = False
        self._bump("cond")

    _cond_args = None
    triples = False   # the conditioning holds subject-guidance triples [u x b | r x b | f x b] (set_conditioning_triples), not CFG pairs

    def set_conditioning_triples(self, text, ref_latent, null_ref_latent=None):
        """subject guidance on a geometry of B = 3b samples [u x b | r x b | f x b], b = 1 or 2 (s2v_set_conditioning_triples): text
        [2b,T,text_embed_dim] = [negative x b | positive x b] (the negative rows serve the u and the r sample of their video), ref_latent
        [b,1,C,H,W] one reference per video, null_ref_latent [1 or b,1,C,H,W] the reference of the u samples (None: zeros, the zero latent)"""
        B, T, F, H, W = self.geometry
        if B % 3 or B // 3 > 2:
            raise _lib.S2VError(f"set_conditioning_triples: a geometry of B = 3b samples with b = 1 or 2 videos is required, got B = {B}")
        b = B // 3
        text = text.to(self.device, self.dtype).contiguous()
        ref = ref_latent.to(self.device, self.dtype).contiguous()
        if tuple(text.shape) != (2 * b, T, self.cfg.text_embed_dim):
            raise _lib.S2VError(f"set_conditioning_triples: text embeddings must be [{2 * b},{T},{self.cfg.text_embed_dim}] "
                                f"([negative x {b} | positive x {b}]), got {tuple(text.shape)}")
        want = (1, self.cfg.in_channels, H, W)
        if ref.ndim != 5 or tuple(ref.shape[1:]) != want or ref.shape[0] != b:
            raise _lib.S2VError(f"set_conditioning_triples: ref_img_states must be [{b},1,{self.cfg.in_channels},{H},{W}] (one reference per video), "
                                f"got {tuple(ref.shape)}")
        null = torch.zeros_like(ref[:1]) if null_ref_latent is None else null_ref_latent.to(self.device, self.dtype).contiguous()
        if null.ndim != 5 or tuple(null.shape[1:]) != want or null.shape[0] not in (1, b):
            raise _lib.S2VError(f"set_conditioning_triples: negative_ref_img_states must be [1 or {b},1,{self.cfg.in_channels},{H},{W}], "
                                f"got {tuple(null.shape)}")
        _lib.check(_lib.lib().s2v_set_conditioning_triples(self._h, _lib.ptr(text), _lib.ptr(ref), _lib.ptr(null), null.shape[0], _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()
        self._cond_args = (text, ref, null) if self.cfg.lora_runtime_rank > 0 else None
        self.triples = True
        self._bump("cond")

    def _lora_changed(self):
        """patch_embed.proj / text_proj may have been re-merged: the hoisted conditioning is computed again from the inputs it was set with"""
        torch.cuda.current_stream().synchronize()
        if self.kind == _lib.CTX_MODEL and self._cond_args is not None and self.geometry is not None:
            (self.set_conditioning_triples if self.triples else self.set_conditioning)(*self._cond_args)

    # ---- step cache (include/s2v_hip.h: s2v_step_cache_*) ------------------------------------------------------------------------------
    _CACHE_MODES = {None: _lib.STEP_FULL, "full": _lib.STEP_FULL, "capture": _lib.STEP_CAPTURE, "reuse": _lib.STEP_REUSE}

    def step_cache_enable(self, on=True):
        """after set_geometry: True / 1 allocates the residual cache [B,V,D] of the current geometry, 2 additionally the buffer that keeps the
        embedded video rows of every forward for step_cache_read(0) (diagnostics), False / 0 frees both"""
        _lib.check(_lib.lib().s2v_step_cache_enable(self._h, int(on)))

    def step_cache_state(self):
        """{"enabled": 0 / 1 / 2, "valid": a residual is held, "bytes": device bytes of the cache buffers}"""
        e, v, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        _lib.check(_lib.lib().s2v_step_cache_state(self._h, ctypes.byref(e), ctypes.byref(v), ctypes.byref(n)))
        return {"enabled": e.value, "valid": bool(v.value), "bytes": n.value}

    def step_cache_read(self, which):
        """[B,V,D] in the model dtype: 0 the video rows as the last forward embedded them (enable 2 only), 1 the video rows as its tail read
        them, 2 the residual"""
        B, T, F, H, W = self.geometry
        out = torch.empty((B, F * (H // 2) * (W // 2), self.D), dtype=self.dtype, device=self.device)
        _lib.check(_lib.lib().s2v_step_cache_read(self._h, int(which), _lib.ptr(out), _lib.stream_ptr()))
        return out

    def time_embedding(self, timesteps):
        """[n, time_embed_dim] in the model dtype: row i is the timestep embedding a step at timesteps[i] computes (s2v_time_embedding): the
        indicator of step_cache_plan.  Needs finalized weights only"""
        ts = [float(t) for t in (timesteps.reshape(-1).tolist() if isinstance(timesteps, (torch.Tensor, np.ndarray)) else timesteps)]
        out = torch.empty((len(ts), self.cfg.time_embed_dim), dtype=self.dtype, device=self.device)
        _lib.check(_lib.lib().s2v_time_embedding(self._h, (ctypes.c_float * len(ts))(*ts), len(ts), _lib.ptr(out), _lib.stream_ptr()))
        return out

    def _arm(self, cache):
        """the step-cache mode of the next forward: None / "full", "capture" (a full step that also stores the block stack's contribution to
        the video rows) or "reuse" (embed, add the stored contribution, tail)"""
        if cache not in self._CACHE_MODES:
            raise _lib.S2VError(f"unknown cache mode {cache!r} (None, 'capture' or 'reuse')")
        if self._CACHE_MODES[cache] != _lib.STEP_FULL:
            _lib.check(_lib.lib().s2v_step_cache_arm(self._h, self._CACHE_MODES[cache]))

    # ---- attention map (include/s2v_hip.h: s2v_attn_map_*) -----------------------------------------------------------------------------
    _attn_map_n = 0

    def attn_map_enable(self, on=True, text_spans=()):
        """after set_geometry: allocates (and zeroes) the sums [1 + spans, B, H, V] fp32 of the current geometry; range 0 is the reference
        stream, text_spans up to three (k0, k1) token ranges inside [0, T).  False frees them"""
        spans = [int(x) for s in text_spans for x in s]
        if len(spans) != 2 * len(text_spans):
            raise _lib.S2VError("attn_map_enable: every text span is a pair (k0, k1)")
        arr = (ctypes.c_int32 * max(1, len(spans)))(*spans)
        _lib.check(_lib.lib().s2v_attn_map_enable(self._h, int(bool(on)), arr, len(text_spans)))
        self._attn_map_n = 1 + len(text_spans) if on else 0

    def attn_map_reset(self):
        """zero the sums and the count"""
        _lib.check(_lib.lib().s2v_attn_map_reset(self._h))

    def attn_map_read(self, per_head=False):
        """(sums, count): per_head the raw sums [n, B, H, V] fp32 over the armed layer launches since the last reset; otherwise their head mean
        [n, B, V] divided by the count (count >= 1).  n = 1 + text spans, row 0 the reference stream"""
        B, T, F, H, W = self.geometry
        V, nh = F * (H // 2) * (W // 2), self.cfg.num_attention_heads
        shape = (self._attn_map_n, B, nh, V) if per_head else (self._attn_map_n, B, V)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        count = ctypes.c_int64()
        _lib.check(_lib.lib().s2v_attn_map_read(self._h, int(bool(per_head)), _lib.ptr(out), ctypes.byref(count), _lib.stream_ptr()))
        return out, count.value

    def _arm_attn(self, attn_layers):
        """the layers whose attention the mass kernel follows in the next forward (one-shot; after attn_map_enable)"""
        if attn_layers is None:
            return
        mask = 0
        for l in attn_layers:
            if int(l) != l or l < 0 or l >= 64:
                raise _lib.S2VError(f"attn_layers: {l!r} is no block index")
            mask |= 1 << int(l)
        _lib.check(_lib.lib().s2v_attn_map_arm(self._h, mask))

    # ---- attention steering (include/s2v_hip.h: s2v_attn_steer_*) -------------------------------------------------------------------------
    def attn_steer_enable(self, on=True):
        """after set_geometry: allocates the steer record's device table (holding a record that steers nothing); False frees it.  Drops a
        captured step"""
        _lib.check(_lib.lib().s2v_attn_steer_enable(self._h, int(bool(on))))

    def attn_steer_set(self, ranges):
        """up to four (k0, k1, w, sample_mask): the keys [k0, k1) of the samples whose bit is set weigh w times their softmax weight on the video
        query rows, out_i = sum_j softmax_j(s_ij + ln w) v_j.  Disjoint, ascending, inside [0, Ntok), 2^-16 <= w <= 2^16.  A captured step is kept
        and replays with the new weights"""
        ranges = list(ranges)
        if len(ranges) > _lib.STEER_MAX_RANGES or any(len(r) != 4 for r in ranges):
            raise _lib.S2VError(f"attn_steer_set: at most {_lib.STEER_MAX_RANGES} ranges, each (k0, k1, w, sample_mask)")
        arr = (_lib.SteerRangeC * max(1, len(ranges)))(*[_lib.SteerRangeC(int(k0), int(k1), float(w), int(m) & 0xFFFFFFFF) for k0, k1, w, m in ranges])
        _lib.check(_lib.lib().s2v_attn_steer_set(self._h, len(ranges), arr))

    def attn_steer_set_maps(self, ranges, planes):
        """steering maps: up to four (k0, k1, plane) with plane a sequence of up to 8 plane indices, one per sample, -1 where the range does not apply
        (missing entries are -1); planes [n_planes, V] fp32 weights per video cell (f * Hp + y) * Wp + x, n_planes <= 16, 2^-16 <= w <= 2^16:
        out_i = sum_j softmax_j(s_ij + ln W_p[i - (T + R)]) v_j on the keys of the ranges.  Replaces a scalar record (attn_steer_set) and the reverse:
        a context holds one.  A captured step is kept, and replays with the new maps, while the plane count fits the allocation"""
        ranges = list(ranges)
        if len(ranges) > _lib.STEER_MAX_RANGES or any(len(r) != 3 for r in ranges):
            raise _lib.S2VError(f"attn_steer_set_maps: at most {_lib.STEER_MAX_RANGES} ranges, each (k0, k1, plane per sample)")
        pl = np.ascontiguousarray(planes.detach().cpu().numpy() if hasattr(planes, "detach") else planes, dtype=np.float32)
        V = self.geometry[2] * (self.geometry[3] // 2) * (self.geometry[4] // 2)
        if pl.ndim != 2 or pl.shape[1] != V:
            raise _lib.S2VError(f"attn_steer_set_maps: planes must be [n_planes, V = {V}] (one weight per video cell), got {tuple(pl.shape)}")
        arr = (_lib.SteerMapRangeC * max(1, len(ranges)))()
        for i, (k0, k1, idx) in enumerate(ranges):
            idx = [int(x) for x in idx]
            if len(idx) > _lib.STEER_MAP_BATCH or any(x < -128 or x > 127 for x in idx):
                raise _lib.S2VError(f"attn_steer_set_maps: range {i} names {len(idx)} planes; at most {_lib.STEER_MAP_BATCH} int8 plane indices, one per sample")
            arr[i].k0, arr[i].k1 = int(k0), int(k1)
            for b in range(_lib.STEER_MAP_BATCH):
                arr[i].plane[b] = idx[b] if b < len(idx) else -1
        _lib.check(_lib.lib().s2v_attn_steer_set_maps(self._h, len(ranges), arr, pl.shape[0], pl.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))

    def _arm_steer(self, steer_layers):
        """the layers whose attention launch is the steered kernel in the next forward (one-shot; after attn_steer_enable)"""
        if steer_layers is None:
            return
        mask = 0
        for l in steer_layers:
            if int(l) != l or l < 0 or l >= 64:
                raise _lib.S2VError(f"steer_layers: {l!r} is no block index")
            mask |= 1 << int(l)
        _lib.check(_lib.lib().s2v_attn_steer_arm(self._h, mask))

    # ---- local attention in time (include/s2v_hip.h: s2v_attn_local_*) -----------------------------------------------------------------------
    def attn_local_enable(self, on=True):
        """after set_geometry: allocates the local-attention record's device table (holding a table that windows nothing); False frees it.  Drops
        a captured step"""
        _lib.check(_lib.lib().s2v_attn_local_enable(self._h, int(bool(on))))

    def attn_local_set(self, P, rows_lo, rows_hi):
        """row i of every sample and head sees the keys [0, P) and [rows_lo[i], rows_hi[i]): out_i = sum over those keys of their softmax times v.
        Ntok rows each, 1 <= P <= Ntok, P <= lo <= hi <= Ntok (lo == hi: the prefix only).  A captured step is kept and replays with the new table"""
        B, T, F, H, W = self.geometry
        if len(rows_lo) != len(rows_hi):
            raise _lib.S2VError(f"attn_local_set: {len(rows_lo)} lower and {len(rows_hi)} upper bounds")
        p = self.cfg.patch_size
        ntok = T + (F + 1) * (H // p) * (W // p)   # [text | one reference frame | F latent frames]
        if len(rows_lo) != ntok:
            raise _lib.S2VError(f"attn_local_set: the row table has {len(rows_lo)} rows, the geometry {ntok} tokens")
        _lib.check(_lib.lib().s2v_attn_local_set(self._h, int(P), _lib.i32_array(rows_lo), _lib.i32_array(rows_hi)))

    def attn_local_set_box(self, P, S, rows_lo, rows_hi, offs_lo, offs_hi):
        """the box table of local attention in space and time: row i sees the keys [0, P) and the keys j of [rows_lo[i], rows_hi[i]) whose offset in
        their frame, (j - P) mod S, lies in [offs_lo[i], offs_hi[i]).  Ntok rows each, 1 <= P <= Ntok, P <= lo <= hi <= Ntok, 0 <= olo <= ohi <= S,
        S >= 64.  Replaces a window table (attn_local_set) and the reverse -- the captured steps are then dropped; a new table of the same kind
        keeps them"""
        B, T, F, H, W = self.geometry
        p = self.cfg.patch_size
        ntok = T + (F + 1) * (H // p) * (W // p)   # [text | one reference frame | F latent frames]
        for name, arr in (("rows_lo", rows_lo), ("rows_hi", rows_hi), ("offs_lo", offs_lo), ("offs_hi", offs_hi)):
            if len(arr) != ntok:
                raise _lib.S2VError(f"attn_local_set_box: {name} has {len(arr)} rows, the geometry {ntok} tokens")
        _lib.check(_lib.lib().s2v_attn_local_set_box(self._h, int(P), int(S), _lib.i32_array(rows_lo), _lib.i32_array(rows_hi), _lib.i32_array(offs_lo),
                                                     _lib.i32_array(offs_hi)))

    def _arm_local(self, local_layers):
        """the layers whose attention launch is the local kernel in the next forward (one-shot; after attn_local_enable)"""
        if local_layers is None:
            return
        mask = 0
        for l in local_layers:
            if int(l) != l or l < 0 or l >= 64:
                raise _lib.S2VError(f"local_layers: {l!r} is no block index")
            mask |= 1 << int(l)
        _lib.check(_lib.lib().s2v_attn_local_arm(self._h, mask))

    # ---- compute -------------------------------------------------------------------------------------------
    def forward(self, latents, timesteps, shared_latent=False, cache=None, attn_layers=None, steer_layers=None, local_layers=None):
        """CogVideoXTransformer3DModel.forward seam: latents [B,F,C,H,W]; with shared_latent [n,F,C,H,W], n dividing B: sample j embeds latent
        j mod n (n = 1: every sample the same latent; n = B/2: the CFG batch cat([latents] * 2) of B/2 videos without the copy).
        cache: the step-cache mode of this forward (_arm; after step_cache_enable)
        attn_layers: the block indices whose attention mass is added to the attention map by this forward (after attn_map_enable)
        steer_layers: the block indices whose attention runs steered in this forward (after attn_steer_enable / attn_steer_set)
        local_layers: the block indices whose attention runs windowed in this forward (after attn_local_enable / attn_local_set)"""
        B, T, F, H, W = self.geometry
        lat = latents.to(self.device, self.dtype).contiguous()
        n_lat = lat.numel() // (F * self.cfg.in_channels * H * W)
        if lat.numel() != n_lat * F * self.cfg.in_channels * H * W or n_lat < 1 or (B % n_lat if shared_latent else n_lat != B):
            raise _lib.S2VError(f"latents {tuple(lat.shape)} do not fit the geometry: [{B},{F},{self.cfg.in_channels},{H},{W}]"
                                + (f", or with shared_latent [n,...] with n dividing {B}" if shared_latent else ""))
        t = timesteps.to(self.device, torch.float32).contiguous()
        if t.numel() != B:
            t = t.reshape(-1)[:1].expand(B).contiguous()
        out = torch.empty((B, F, self.cfg.out_channels, H, W), dtype=self.dtype, device=self.device)
        self._arm(cache)
        self._arm_attn(attn_layers)
        self._arm_steer(steer_layers)
        self._arm_local(local_layers)
        if shared_latent and n_lat > 1:
            _lib.check(_lib.lib().s2v_transformer_forward_videos(self._h, _lib.ptr(lat), n_lat, _lib.ptr(t), _lib.ptr(out), _lib.stream_ptr()))
            return out
        stride = 0 if shared_latent else F * self.cfg.in_channels * H * W
        _lib.check(_lib.lib().s2v_transformer_forward(self._h, _lib.ptr(lat), stride, _lib.ptr(t), _lib.ptr(out),
                                                      _lib.stream_ptr()))
        return out

    def block_forward(self, layer, hidden, enc0, enc1, temb):
        hidden, enc0, enc1, temb = (x.to(self.device, self.dtype).contiguous() for x in (hidden, enc0, enc1, temb))
        oh, o0, o1 = torch.empty_like(hidden), torch.empty_like(enc0), torch.empty_like(enc1)
        _lib.check(_lib.lib().s2v_block_forward(self._h, layer, _lib.ptr(hidden), _lib.ptr(enc0), _lib.ptr(enc1),
                                                _lib.ptr(temb), _lib.ptr(oh), _lib.ptr(o0), _lib.ptr(o1),
                                                _lib.stream_ptr()))
        return oh, o0, o1

    def attn_forward(self, layer, hidden, encoder):
        hidden, encoder = (x.to(self.device, self.dtype).contiguous() for x in (hidden, encoder))
        oh, oe = torch.empty_like(hidden), torch.empty_like(encoder)
        _lib.check(_lib.lib().s2v_attn_forward(self._h, layer, _lib.ptr(hidden), _lib.ptr(encoder), _lib.ptr(oh),
                                               _lib.ptr(oe), _lib.stream_ptr()))
        return oh, oe

    def attn_forward_with(self, weights, layer, hidden, encoder):
        """attn_forward on this engine's geometry, workspace and rotary tables with layer `layer` of the engine `weights`
        (s2v_attn_forward_with: same dtype, heads and weight_format; bit-identical to an engine holding those weights itself)"""
        hidden, encoder = (x.to(self.device, self.dtype).contiguous() for x in (hidden, encoder))
        oh, oe = torch.empty_like(hidden), torch.empty_like(encoder)
        _lib.check(_lib.lib().s2v_attn_forward_with(self._h, weights._h, layer, _lib.ptr(hidden), _lib.ptr(encoder), _lib.ptr(oh),
                                                    _lib.ptr(oe), _lib.stream_ptr()))
        return oh, oe

    AUTO_SLOW_FRACTION = 5e-3   # a slow path costs ~2.5 KV tiles of time, fp16 P saves ~4 %: break-even near 1.7 % of the pairs

    def attn_slow_stats(self, reset=False):
        """(slow paths taken, (wave, KV tile) pairs run) by the four-wave attention kernels since the last reset; synchronises the device"""
        slow, total = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(_lib.lib().s2v_attn_slow_stats(self._h, ctypes.byref(slow), ctypes.byref(total), int(reset)))
        return slow.value, total.value

    def set_attn_p_format(self, fmt):
        if fmt not in ("bf16", "f16"):
            raise _lib.S2VError(f"unknown attn_p_format {fmt!r} ('bf16' or 'f16')")
        _lib.check(_lib.lib().s2v_set_attn_p_format(self._h, 1 if fmt == "f16" else 0))
        self.attn_p_format = fmt

    # ---- masked video-to-video (include/s2v_hip.h: s2v_set_blend, s2v_denoise_step_masked) ---------------------------------------------
    _blend = None

    def set_blend(self, z0, noise0, latent_mask):
        """the blend operands of a masked call for the b = B/2 videos of the geometry (B/3 under set_conditioning_triples): z0 and noise0 [b,F,C,H,W] in the model dtype, latent_mask
        uint8 [b,F,H,W] (mask_to_latent's 0 / 1, or map_to_latent's levels: a cell is kept where it is <= the record's keep_max); the tensors are held until clear_blend or the next set_blend.  Drops a captured step"""
        B, T, F, H, W = self.geometry
        b = B // 3 if self.triples else B // 2
        want = (b, F, self.cfg.in_channels, H, W)
        for name, x in (("z0", z0), ("noise0", noise0)):
            if x.dtype != self.dtype or tuple(x.shape) != want or not x.is_contiguous():
                raise _lib.S2VError(f"set_blend: {name} must be contiguous {list(want)} in the model dtype for the b videos of the geometry, "
                                    f"got {list(x.shape)} {x.dtype}")
        if latent_mask.dtype != torch.uint8 or tuple(latent_mask.shape) != (b, F, H, W) or not latent_mask.is_contiguous():
            raise _lib.S2VError(f"set_blend: latent_mask must be contiguous uint8 {[b, F, H, W]}, got {list(latent_mask.shape)} {latent_mask.dtype}")
        _lib.check(_lib.lib().s2v_set_blend(self._h, _lib.ptr(z0), _lib.ptr(noise0), _lib.ptr(latent_mask), b))
        self._blend = (z0, noise0, latent_mask)

    def clear_blend(self):
        if self._blend is not None:
            torch.cuda.current_stream().synchronize()   # the last masked step still reads the tensors about to be released
            _lib.check(_lib.lib().s2v_set_blend(self._h, None, None, None, 0))
            self._blend = None

    # ---- guidance rescale (include/s2v_hip.h: s2v_set_guidance_rescale, s2v_guidance_rescale_read) ------------------------------------------
    def set_guidance_rescale(self, phi):
        """phi in [0, 1] for the videos of the geometry (B/2, or B/3 under set_conditioning_triples): a float for all of them or a sequence with
        one entry per video; None clears (the factor log goes too).  Armed (any phi > 0), every denoise_step scales each video's guided
        prediction by k = phi * std(f) / std(v) + 1 - phi before the scheduler arithmetic; all zero arms nothing.  The values live in device
        memory: new values for the same videos keep a captured step.  set_geometry disarms (the log stays)"""
        if phi is None:
            _lib.check(_lib.lib().s2v_set_guidance_rescale(self._h, None, 0))
            return
        if self.geometry is None:
            raise _lib.S2VError("set_guidance_rescale: call set_geometry first (the values belong to the geometry's videos)")
        B = self.geometry[0]
        b = B // 3 if self.triples else max(B // 2, 1)
        vals = [float(p) for p in _per_video("guidance_rescale", phi, b)]
        _lib.check(_lib.lib().s2v_set_guidance_rescale(self._h, (ctypes.c_float * b)(*vals), b))

    def guidance_rescale_read(self, log_only=False):
        """{"sums": [b][4] fp64 (sum f, sum f^2, sum v, sum v^2) and "factors": [b] of the last armed step (left out with log_only, or when
        nothing is armed), "log": the factor rows [steps][4] of every armed step since the log was allocated (columns past the step's videos
        are 0), "count": the steps logged}.  Synchronises the device"""
        n = ctypes.c_int32()
        log = (ctypes.c_float * (_lib.CFG_LOG_STEPS * _lib.CFG_LOG_COLS))()
        _lib.check(_lib.lib().s2v_guidance_rescale_read(self._h, None, None, log, ctypes.byref(n)))
        rows = min(n.value, _lib.CFG_LOG_STEPS)
        out = {"log": [[log[r * _lib.CFG_LOG_COLS + k] for k in range(_lib.CFG_LOG_COLS)] for r in range(rows)], "count": n.value}
        if not log_only and self.geometry is not None:
            B = self.geometry[0]
            b = B // 3 if self.triples else max(B // 2, 1)
            sums, factors = (ctypes.c_double * (4 * b))(), (ctypes.c_float * b)()
            if _lib.lib().s2v_guidance_rescale_read(self._h, sums, factors, None, None) == 0:   # refused: nothing is armed
                out["sums"] = [[sums[4 * k + q] for q in range(4)] for k in range(b)]
                out["factors"] = [factors[k] for k in range(b)]
        return out

    def denoise_step(self, latents, timestep, coef, x0_hist=None, noise=None, use_graph=False, blend=None, cache=None, attn_layers=None, subject=False,
                     steer_layers=None, local_layers=None):
        """one iteration of the denoise loop, latents [b,F,C,H,W] (model dtype) updated in place: b = B/2 videos of a geometry of B = 2b samples
        [negative x b | positive x b] (b = 1 for B = 1 or 2); x0_hist (fp32) and noise have the shape of latents.  timestep and coef are scalars
        (one timestep and one SchedCoefC for every video: s2v_denoise_step) or sequences of b of each, video k at timestep[k] stepped with
        coef[k] -- its own kind, guidance and scalars (s2v_denoise_step_videos); a scalar beside a sequence is repeated.
        blend: the masked step (s2v_denoise_step_masked, after set_blend): one _lib.BlendC, or a sequence of b, video k blended with blend[k]
        cache: the step-cache mode of this step's forward (_arm; after step_cache_enable): "capture", "reuse" or None
        attn_layers: the block indices whose attention mass this step adds to the attention map (after attn_map_enable; not with "reuse")
        steer_layers: the block indices whose attention runs steered in this step (after attn_steer_enable / attn_steer_set; not with "reuse",
        attn_layers or subject: the library refuses those by name)
        local_layers: the block indices whose attention runs windowed in this step (after attn_local_enable / attn_local_set; not with "reuse",
        attn_layers, steer_layers or subject: the library refuses those by name)
        subject: the subject-guidance step (s2v_denoise_step_guided, after set_conditioning_triples): b = B/3 videos of a geometry of B = 3b
        samples [u x b | r x b | f x b], video k combined with coef[k].guidance_subject and coef[k].guidance; with blend its masked form"""
        if latents.dtype != self.dtype or not latents.is_contiguous():
            raise _lib.S2VError("latents must be a contiguous model-dtype tensor (it is updated in place)")
        B, T, F, H, W = self.geometry
        if subject:
            return self._denoise_step_guided(latents, timestep, coef, x0_hist, noise, use_graph, blend, cache, attn_layers, steer_layers, local_layers)
        if B > 2:
            if B % 2:
                raise _lib.S2VError(f"denoise_step: a geometry of {B} samples is no whole number of CFG pairs")
            want = (B // 2, F, self.cfg.in_channels, H, W)
            for name, x in (("latents", latents), ("x0_hist", x0_hist), ("noise", noise)):
                if x is not None and (tuple(x.shape) != want or not x.is_contiguous()):
                    raise _lib.S2VError(f"denoise_step: {name} must be contiguous {list(want)} for {B // 2} videos per call, got {list(x.shape)}")
        per_video = blend is not None or not isinstance(coef, _lib.SchedCoefC) or _is_seq(timestep)
        if per_video:
            b = B // 2 if B >= 2 else 1
            ts = _per_video("timestep", timestep, b)
            cs = _per_video("coef", coef, b)
            t_arr = (ctypes.c_float * b)(*[float(t) for t in ts])
            c_arr = (_lib.SchedCoefC * b)(*cs)
            if blend is not None:
                b_arr = (_lib.BlendC * b)(*_per_video("blend", blend, b))
        auto = self._attn_auto_pending
        if auto:
            self.attn_slow_stats(reset=True)
        self._arm(cache)
        self._arm_attn(attn_layers)
        self._arm_steer(steer_layers)
        self._arm_local(local_layers)
        if blend is not None:
            _lib.check(_lib.lib().s2v_denoise_step_masked(self._h, _lib.ptr(latents), t_arr, c_arr, b_arr, _lib.ptr(x0_hist), _lib.ptr(noise),
                                                          int(use_graph and not auto), _lib.stream_ptr()))
        elif per_video:
            _lib.check(_lib.lib().s2v_denoise_step_videos(self._h, _lib.ptr(latents), t_arr, c_arr, _lib.ptr(x0_hist), _lib.ptr(noise),
                                                          int(use_graph and not auto), _lib.stream_ptr()))
        else:
            _lib.check(_lib.lib().s2v_denoise_step(self._h, _lib.ptr(latents), float(timestep), ctypes.byref(coef),
                                                   _lib.ptr(x0_hist), _lib.ptr(noise), int(use_graph and not auto), _lib.stream_ptr()))
        if auto:
            self._settle_attn_auto()

    def _settle_attn_auto(self):
        """the first step of an "auto" engine runs eagerly; its census decides the format of every later step"""
        slow, total = self.attn_slow_stats()
        self.attn_slow_fraction = slow / total if total else 0.0
        if self.attn_slow_fraction > self.AUTO_SLOW_FRACTION:
            self.set_attn_p_format("bf16")
        self._attn_auto_pending = False

    def _denoise_step_guided(self, latents, timestep, coef, x0_hist, noise, use_graph, blend, cache, attn_layers, steer_layers=None, local_layers=None):
        B, T, F, H, W = self.geometry
        if B % 3:
            raise _lib.S2VError(f"denoise_step(subject=True): a geometry of {B} samples is no whole number of triples [u | r | f]")
        b = B // 3
        want = (b, F, self.cfg.in_channels, H, W)
        for name, x in (("latents", latents), ("x0_hist", x0_hist), ("noise", noise)):
            if x is not None and (tuple(x.shape) != want or not x.is_contiguous()):
                raise _lib.S2VError(f"denoise_step(subject=True): {name} must be contiguous {list(want)} for {b} videos per call, got {list(x.shape)}")
        t_arr = (ctypes.c_float * b)(*[float(t) for t in _per_video("timestep", timestep, b)])
        c_arr = (_lib.SchedCoefC * b)(*_per_video("coef", coef, b))
        b_arr = None if blend is None else (_lib.BlendC * b)(*_per_video("blend", blend, b))
        auto = self._attn_auto_pending
        if auto:
            self.attn_slow_stats(reset=True)
        self._arm(cache)            # the library refuses an armed step by name: the step cache and the attention map assume pairs
        self._arm_attn(attn_layers)
        self._arm_steer(steer_layers)
        self._arm_local(local_layers)
        _lib.check(_lib.lib().s2v_denoise_step_guided(self._h, _lib.ptr(latents), t_arr, c_arr, b_arr, _lib.ptr(x0_hist), _lib.ptr(noise),
                                                      int(use_graph and not auto), _lib.stream_ptr()))
        if auto:
            self._settle_attn_auto()

    # ---- temporal windows (include/s2v_hip.h: s2v_set_windows, s2v_denoise_step_windows) -------------------------------------------------------
    windows = None   # (L, stride, per_forward) while set

    def set_windows(self, L, stride, weights, per_forward=1):
        """a long latent of L frames is stepped as W = (L - F) / stride + 1 windows of the geometry's F frames, stride frames apart, per_forward
        windows per forward: after set_geometry(2 * per_forward, T, F, H, W) and set_conditioning with the text pair repeated per_forward times
        and one shared reference row.  weights: F fp32 values, the weight of each frame of a window (pipeline.window_plan).  Allocates the fp32
        plane [L,C,H,W] (device_bytes counts it); set_geometry and clear_windows free it"""
        w = [float(x) for x in weights]
        _lib.check(_lib.lib().s2v_set_windows(self._h, int(L), int(stride), int(per_forward), (ctypes.c_float * len(w))(*w)))
        self.windows = (int(L), int(stride), int(per_forward))

    def clear_windows(self):
        if self.windows is not None:
            _lib.check(_lib.lib().s2v_set_windows(self._h, 0, 0, 0, None))
            self.windows = None

    def denoise_step_windows(self, latents, timestep, coef, x0_hist=None, noise=None, use_graph=False):
        """one iteration of the denoise loop on a long latent [1,L,C,H,W] (model dtype), updated in place, after set_windows: the forward on
        every window, the windows' CFG pairs combined and averaged where they overlap, one scheduler step on the L frames
        (s2v_denoise_step_windows); x0_hist (fp32) and noise have the shape of latents"""
        if latents.dtype != self.dtype or not latents.is_contiguous():
            raise _lib.S2VError("latents must be a contiguous model-dtype tensor (it is updated in place)")
        if self.windows is not None:   # without windows the library refuses by name
            B, T, F, H, W = self.geometry
            want = (1, self.windows[0], self.cfg.in_channels, H, W)
            for name, x in (("latents", latents), ("x0_hist", x0_hist), ("noise", noise)):
                if x is not None and (tuple(x.shape) != want or not x.is_contiguous()):
                    raise _lib.S2VError(f"denoise_step_windows: {name} must be contiguous {list(want)} (the long latent), got {list(x.shape)}")
        auto = self._attn_auto_pending
        if auto:
            self.attn_slow_stats(reset=True)
        _lib.check(_lib.lib().s2v_denoise_step_windows(self._h, _lib.ptr(latents), float(timestep), ctypes.byref(coef), _lib.ptr(x0_hist),
                                                       _lib.ptr(noise), int(use_graph and not auto), _lib.stream_ptr()))
        if auto:
            self._settle_attn_auto()

    # ---- CFG-parallel: this engine holds ONE sample of the CFG pair (geometry B = 1); include/s2v_hip.h, dist.CfgPair ---------------------------
    def cfg_pair(self):
        """the context-owned pair buffer [2, F, C, H, W] (model dtype): half `slot` is written by denoise_split_begin, the other by the exchange"""
        B, T, F, H, W = self.geometry
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(_lib.lib().s2v_cfg_pair(self._h, ctypes.byref(p), ctypes.byref(n)))
        raw = torch.as_tensor(_ArenaView(p.value, 2 * n.value), device=self.device)
        return raw.view(self.dtype).view(2, F, self.cfg.out_channels, H, W)

    def _no_auto_in_a_pair(self):
        if self.cfg.attn_p_format == "auto":  # "auto" settles per engine from its own census: the two ranks of a pair could settle differently
            raise _lib.S2VError("attn_p_format 'auto' is per-engine; the two ranks of a CFG-parallel pair must run the same arithmetic: use 'bf16' or 'f16'")

    def denoise_split_begin(self, latents, timestep, coef, slot, use_graph=False):
        self._no_auto_in_a_pair()
        if latents.dtype != self.dtype or not latents.is_contiguous():
            raise _lib.S2VError("latents must be a contiguous model-dtype tensor")
        _lib.check(_lib.lib().s2v_denoise_split_begin(self._h, _lib.ptr(latents), float(timestep), ctypes.byref(coef), int(slot), int(use_graph),
                                                      _lib.stream_ptr()))

    def denoise_split_end(self, latents, x0_hist=None, noise=None):
        _lib.check(_lib.lib().s2v_denoise_split_end(self._h, _lib.ptr(latents), _lib.ptr(x0_hist), _lib.ptr(noise), _lib.stream_ptr()))

    def denoise_step_cfg_parallel(self, comm, slot, latents, timestep, coef, x0_hist=None, noise=None, use_graph=False):
        """begin + s2v_rccl_allgather + end in ONE library call over an RcclComm of the two ranks of the pair"""
        self._no_auto_in_a_pair()
        if latents.dtype != self.dtype or not latents.is_contiguous():
            raise _lib.S2VError("latents must be a contiguous model-dtype tensor (it is updated in place)")
        _lib.check(_lib.lib().s2v_denoise_step_cfg_parallel(self._h, comm._h, int(slot), _lib.ptr(latents), float(timestep), ctypes.byref(coef),
                                                            _lib.ptr(x0_hist), _lib.ptr(noise), int(use_graph), _lib.stream_ptr()))

    # ---- Ulysses sequence parallelism: p engines share one video's step, attention sharded by heads (include/s2v_hip.h, dist.UlyssesGroup) ----------
    def set_shard(self, world, rank):
        """before set_geometry: this engine holds rank `rank`'s rows [T_r | R_r | V_r] of every sample and heads [rank*H/world, (rank+1)*H/world)"""
        if self.cfg.attn_p_format == "auto":  # "auto" settles per engine from its own census: the ranks could settle on different arithmetic
            raise _lib.S2VError("attn_p_format 'auto' is per-engine; the ranks of a Ulysses shard must run the same arithmetic: use 'bf16' or 'f16'")
        _lib.check(_lib.lib().s2v_set_shard(self._h, int(world), int(rank)))
        if self.shard != (int(world), int(rank)):
            self.geometry = None
            self.windows = None
        self.shard = (int(world), int(rank))

    shard = None

    def shard_layout(self):
        """[(T_r, R_r, V_r) for every rank r] of the current geometry"""
        p = self.shard[0]
        out = (ctypes.c_int32 * (3 * p))()
        _lib.check(_lib.lib().s2v_shard_layout(self._h, out))
        return [tuple(out[3 * r:3 * r + 3]) for r in range(p)]

    def shard_buffers(self, kind):
        """(send, recv, send_counts, send_displs, recv_counts, recv_displs) of an exchange kind (_lib.SHARD_*): uint8 CUDA views of the
        context-owned buffers and per-rank byte counts / displacements (lists)"""
        p = self.shard[0]
        s, r = ctypes.c_void_p(), ctypes.c_void_p()
        arr = [(ctypes.c_int64 * p)() for _ in range(4)]
        _lib.check(_lib.lib().s2v_shard_buffers(self._h, int(kind), ctypes.byref(s), ctypes.byref(r), *arr))
        sc, sd, rc, rd = ([int(x) for x in a] for a in arr)
        send = torch.as_tensor(_ArenaView(s.value, max(d + n for d, n in zip(sd, sc))), device=self.device)
        recv = torch.as_tensor(_ArenaView(r.value, max(d + n for d, n in zip(rd, rc))), device=self.device)
        return send, recv, sc, sd, rc, rd

    def _shard_checks(self, latents, use_graph=False):
        if self.shard is None:
            raise _lib.S2VError("not a shard engine: call set_shard(world, rank) before set_geometry")
        if use_graph:
            raise _lib.S2VError("use_graph is not supported for a Ulysses shard: the step is staged around its exchanges and runs eagerly")
        if latents is not None and (latents.dtype != self.dtype or not latents.is_contiguous()):
            raise _lib.S2VError("latents must be a contiguous model-dtype tensor (it is updated in place)")

    def shard_step_begin(self, latents, timestep, coef):
        """local rows up to the first exchange; returns the pending exchange kind (_lib.SHARD_QKV_EXCHANGE)"""
        self._shard_checks(latents)
        pending = ctypes.c_int32()
        _lib.check(_lib.lib().s2v_shard_step_begin(self._h, _lib.ptr(latents), float(timestep), ctypes.byref(coef), ctypes.byref(pending),
                                                   _lib.stream_ptr()))
        return pending.value

    def shard_step_resume(self):
        """after the pending exchange has filled the recv buffer: runs up to the next exchange point and returns its kind"""
        pending = ctypes.c_int32()
        _lib.check(_lib.lib().s2v_shard_step_resume(self._h, ctypes.byref(pending), _lib.stream_ptr()))
        return pending.value

    def shard_step_end(self, latents, x0_hist=None, noise=None):
        """after the noise gather: CFG + scheduler step on the whole latent, run by every rank (latents updated in place)"""
        _lib.check(_lib.lib().s2v_shard_step_end(self._h, _lib.ptr(latents), _lib.ptr(x0_hist), _lib.ptr(noise), _lib.stream_ptr()))

    def denoise_step_ulysses(self, comm, latents, timestep, coef, x0_hist=None, noise=None, use_graph=False):
        """the whole staged step with s2v_rccl_alltoallv exchanges over an RcclComm of the shard's ranks, stream-ordered"""
        self._shard_checks(latents, use_graph)
        _lib.check(_lib.lib().s2v_denoise_step_ulysses(self._h, comm._h, _lib.ptr(latents), float(timestep), ctypes.byref(coef),
                                                       _lib.ptr(x0_hist), _lib.ptr(noise), _lib.stream_ptr()))

    def last_noise_pred(self):
        B, T, F, H, W = self.geometry
        p = ctypes.c_void_p()
        _lib.check(_lib.lib().s2v_last_noise_pred(self._h, ctypes.byref(p)))
        n = B * F * self.cfg.out_channels * H * W * (4 if self.dtype == torch.float32 else 2)
        raw = torch.as_tensor(_ArenaView(p.value, n), device=self.device)
        return raw.view(self.dtype).view(B, F, self.cfg.out_channels, H, W).clone()
