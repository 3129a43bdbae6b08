"""Torch restatement of the step cache (include/s2v_hip.h: S2V_STEP_*; pipeline.step_cache_plan), used by tests/test_step_cache_cpu.py and
tests/test_gpu_step_cache.py.

plan_ref restates the plan rule on its own.  cached_forward_ref is the transformer forward of oracle/transformer_ref.py cut at the two places
the cache cuts it: embed -> (blocks | + delta) -> tail.  The pieces are the oracle's own functions, imported; only the tail -- which the oracle
has inline in transformer_forward -- is written out here, and tests/test_step_cache_cpu.py holds the uncached composition to
transformer_forward bit for bit.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.transformer_ref import block_forward, patch_tokens, sincos_3d, timestep_sinusoid


def plan_ref(emb, threshold, coefficients=(1.0, 0.0), keep_first=1, keep_last=1):
    """True = full step.  emb [n, temb] -> float64."""
    e = torch.as_tensor(np.asarray(emb, dtype=np.float64)) if not isinstance(emb, torch.Tensor) else emb.double()
    n, acc, out = e.shape[0], 0.0, []
    for i in range(n):
        if i == 0 or i < keep_first or i >= n - keep_last:
            acc = 0.0
            out.append(True)
            continue
        d = float((e[i] - e[i - 1]).abs().mean() / e[i - 1].abs().mean())
        p = 0.0
        for c in coefficients:   # Horner, highest power first
            p = p * d + c
        acc += p
        if acc < threshold:
            out.append(False)
        else:
            acc = 0.0
            out.append(True)
    return out


def time_embedding_ref(sd, D, timestep, dt):
    te = timestep_sinusoid(timestep, D).to(dt)
    emb = F.linear(te, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    return F.linear(F.silu(emb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])


def cached_forward_ref(sd, cfg, hidden_states, encoder_hidden_states, ref_img_states, timestep, rope=None, ref_rope=None, mode="full", delta=None):
    """mode "full": transformer_forward.  "capture": the same, and also returns delta = OUT - IN of the video stream.  "reuse": IN + delta
    instead of the blocks.  Returns (noise prediction [B,F,C,H,W], delta or None)."""
    heads = cfg["num_heads"]
    D = heads * 64
    B, Fr, C, H, W = hidden_states.shape
    dt = hidden_states.dtype
    eps = cfg.get("norm_eps", 1e-5)
    emb = time_embedding_ref(sd, D, timestep, dt)
    h = patch_tokens(sd, hidden_states)
    if not cfg["use_rope"]:
        h = h + sincos_3d(D, W // 2, H // 2, Fr, cfg.get("spatial_scale", 1.875), cfg.get("temporal_scale", 1.0))[None].to(dt)
    h_in = h
    if mode == "reuse":
        h = (h_in.float() + delta.float()).to(dt)
    else:
        e0 = F.linear(encoder_hidden_states, sd["patch_embed.text_proj.weight"], sd["patch_embed.text_proj.bias"])
        e1 = patch_tokens(sd, ref_img_states)
        e1 = torch.cat([e1] * B, dim=0) if e1.shape[0] != B else e1
        for i in range(cfg["num_layers"]):
            h, e0, e1 = block_forward(sd, f"transformer_blocks.{i}.", heads, h, e0, e1, emb, rope, ref_rope, eps)
        if mode == "capture":
            delta = (h.float() - h_in.float()).to(dt)
    # the tail of transformer_forward
    h = F.layer_norm(h, (D,), sd["norm_final.weight"], sd["norm_final.bias"], eps)
    m = F.linear(F.silu(emb), sd["norm_out.linear.weight"], sd["norm_out.linear.bias"])
    shift, scale = m.chunk(2, dim=1)
    h = F.layer_norm(h, (D,), sd["norm_out.norm.weight"], sd["norm_out.norm.bias"], eps)
    h = h * (1 + scale[:, None, :]) + shift[:, None, :]
    y = F.linear(h, sd["proj_out.weight"], sd["proj_out.bias"])
    y = y.reshape(B, Fr, H // 2, W // 2, -1, 2, 2).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4)
    return y, (delta if mode != "full" else None)
