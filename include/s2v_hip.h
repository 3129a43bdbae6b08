/*
 * s2v_hip.h -- C ABI of libs2v_hip.so: the MI355X (gfx950) implementation of the CogVideoX denoise hot path that
 * carpedkm/disentangled-subject-to-vid drives from src/custom_cogvideox_pipe.py.
 *
 * The reference has no FFI: its plug-in seams are Python protocols.  Each entry point below
 * names the reference interface it stands behind (paths relative to the reference checkout).  The ctypes binding a
 * maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every tensor argument is a DEVICE pointer to a dense row-major array of the model dtype (S2V_F32 / S2V_BF16)
 *     unless stated otherwise; the caller owns it and keeps it alive until the stream has passed the call;
 *   - weights are copied (and re-packed: fused QKV, stacked AdaLN linears, padded tiles) into context-owned buffers by
 *     s2v_load_weight, the caller may free its copy afterwards;
 *   - every compute entry point is asynchronous on the given hipStream_t;
 *   - return value 0 = ok, < 0 = error; s2v_last_error() returns a thread-local message; no C++ exception crosses;
 *   - one context must not be used from two host threads at once; distinct contexts (one per GPU) are independent.
 */
#ifndef S2V_HIP_H
#define S2V_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the shared library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#if defined(__GNUC__)
#define S2V_API __attribute__((visibility("default")))
#else
#define S2V_API
#endif

typedef struct s2v_ctx s2v_ctx;
typedef void* s2v_stream; /* hipStream_t */

/* F16 (round 5): the dtype the reference selects for every non-5B checkpoint (src/inference.py:191,209: transformer, VAE and text
 * encoder alike).  Transformer contexts (s2v_create), the VAE decoder / encoder (s2v_vae_create, s2v_vae_enc_create), the T5 encoder
 * (s2v_t5_create), the scheduler step and the operator-level entry points all take it. */
enum { S2V_DTYPE_F32 = 0, S2V_DTYPE_BF16 = 1, S2V_DTYPE_F16 = 2 };

/* CogVideoXTransformer3DModel.__init__ hyper-parameters
 * (diffusers/src/diffusers/models/transformers/cogvideox_transformer_3d.py:253-280) */
typedef struct s2v_model_config {
    int32_t num_layers;       /* 30 (2B) / 42 (5B) */
    int32_t num_heads;        /* 30 / 48; head_dim is fixed at 64 */
    int32_t in_channels;      /* 16 */
    int32_t out_channels;     /* 16 */
    int32_t patch_size;       /* 2 */
    int32_t time_embed_dim;   /* 512 */
    int32_t text_embed_dim;   /* 4096 */
    int32_t use_rope;         /* use_rotary_positional_embeddings: 0 (2B) / 1 (5B) */
    int32_t dtype;            /* S2V_DTYPE_* : storage + rounding points of the model */
    float norm_eps;           /* 1e-5 */
    int32_t force_simple;     /* 1 = run the model on the generic VALU kernels (bf16: instead of the bf16 MFMA path; fp32: instead of the fp32-MFMA kernels, which return the same GEMM bits); cross-check only */
    int32_t weight_format;    /* 0 = the model dtype; 1 = W8A8 fp8 (BASELINE configs[4]): the four big linears of every block
                               * (fused QKV, attention out, FF1, FF2) keep OCP e4m3 weights with per-output-channel scales
                               * (quantised by s2v_finalize_weights after any LoRA merge) and take per-token e4m3 activations,
                               * on v_mfma_scale_f32_32x32x64_f8f6f4; bf16 model dtype only, inner_dim % 128 == 0;
                               * 2 = 1 plus fp8 QK^T (an option BEYOND configs[4]'s "fp8 weights", off unless asked for): after the per-head LayerNorm and
                               * rotary embedding q (times scale * log2 e) and k are re-quantised as MX e4m3 (one power-of-two scale per
                               * 32 head-dim elements) and S = K.Q^T of the attention runs on the same scaled fp8 MFMA; softmax, P and P.V
                               * stay fp32 / bf16;
                               * 3 = 1 below 40 000 tokens per sample, 2 from there on (decided at s2v_set_geometry): at the configs[4] geometry
                               * (N = 50 626) the attention is > 80 % of the step, fp8 QK^T takes 11-14 % off it and adds nothing measurable to the
                               * fp8 engine's whole-run drift on synthetic weights (profiles/r05_whole_run_c5_10steps.txt).  Opt-in like 2: the package's
                               * configs[4] preset is 1; its "cogvideox-5b-fp8-auto" preset asks for 3.  s2v_fp8_qk_active reports the decision.
                               * The reference has no fp8 path: parity unpinned, tolerance stated in tests/test_gpu_fp8.py */
    int32_t lora_adaln_scope; /* where the subject-LoRA acts inside CogVideoXLayerNormZero (normalization.py:467-484):
                               * 0 = as shipped: `enable_lora([self.linear], False)` sets an attribute nothing reads, so the LoRA
                               *     is active on both evaluations of norm{1,2}.linear and is merged into it (SURVEY preamble 6);
                               * 1 = as the authors' comments intend (:470-476): base weights for the video / text modulation, the
                               *     LoRA only for the reference-image chunks (cond_shift, cond_scale, cond_gate): the context keeps
                               *     a second copy of rows [0, 3D) of each norm{1,2}.linear, s2v_merge_lora on those names merges
                               *     into that copy only, and the reference-image rows are modulated / gated with it */
    int32_t attn_p_format;    /* softmax probabilities P and V^T of the four-wave attention kernel (sequences > 4608 tokens, and the fp8 engines):
                               * 0 = bf16 (P.V on v_mfma_f32_32x32x16_bf16, row sums in fp32, deferred maximum 2^64);
                               * 1 = fp16 (P.V on v_mfma_f32_32x32x16_f16; P keeps 11 significant bits instead of 8; row sums by packed fp16
                               *     adds on the P registers, flushed to fp32 per KV tile; the deferred maximum falls to 2^14, i.e. the slow
                               *     path re-adopts the row maximum when a later score exceeds it by ~9.7 natural units -- faster on smooth
                               *     score distributions, slower on spiky ones; tests/test_gpu_parity.py holds both against fp64 SDPA) */
    int32_t reserved[2];      /* reserved[0]: the kind of context s2v_create makes (S2V_CTX_*, 0 = a whole model);
                               * reserved[1] = lora_runtime_rank: 0 = LoRA exists only as the load-time merge (s2v_merge_lora; the default: it costs
                               *     nothing per step); r in 1 .. 128 = the runtime adapter mode with room for adapters of rank <= r per layer
                               *     (s2v_lora_attach below): the arena and the workspace are carved larger, the arithmetic without an adapter is
                               *     unchanged.  The rank sits in the low 16 bits (S2V_LORA_RANK_MASK); bit 16, S2V_LORA_FP8_BRANCH, asks an fp8
                               *     weight_format (1 / 2 / 3) for the 16-bit adapter branch beside its e4m3 weights (below); without the flag an fp8
                               *     context carves nothing and s2v_lora_attach refuses it; weight_format 0 ignores the flag */
} s2v_model_config;
/* flag bits of reserved[1] above the rank */
enum { S2V_LORA_RANK_MASK = 0xffff, S2V_LORA_FP8_BRANCH = 1 << 16 };

/* reserved[0] of s2v_model_config.  The AttnProcessor seam installed on every Attention module of a model
 * keeps each module's attention weights in an S2V_CTX_ATTN_WEIGHTS context and runs all of them with ONE S2V_CTX_ATTN_WORKSPACE
 * context's geometry, workspace and rotary tables (s2v_attn_forward_with): one activation workspace per model instead of one per module. */
enum {
    S2V_CTX_MODEL = 0,          /* a whole model: weight arena of num_layers blocks + embeddings; workspace at s2v_set_geometry; every entry point */
    S2V_CTX_ATTN_WEIGHTS = 1,   /* attention weights only: num_layers x transformer_blocks.<l>.attn1.{to_q,to_k,to_v,to_out.0,norm_q,norm_k}.{weight,bias}
                                 * in the fused QKV / out-projection layout of a model's arena (s2v_load_weight, s2v_merge_lora, s2v_finalize_weights on
                                 * those keys).  It never carves a workspace (s2v_set_geometry refuses it) and runs nothing itself; weight_format 0 */
    S2V_CTX_ATTN_WORKSPACE = 2  /* geometry, workspace and rotary tables without weights (no arena): s2v_set_geometry, s2v_set_rope, then
                                 * s2v_attn_forward_with; s2v_finalize_weights / s2v_mark_weights_loaded refuse it, so every entry point that needs
                                 * its own weights does too; weight_format 0 */
};

S2V_API const char* s2v_last_error(void);
S2V_API const char* s2v_version(void);

S2V_API int s2v_create(const s2v_model_config* cfg, s2v_ctx** out);
S2V_API void s2v_destroy(s2v_ctx* ctx);

/* Load one state-dict tensor.  `name` is the reference's own key, e.g.
 * "transformer_blocks.3.attn1.to_q.weight", "patch_embed.proj.weight" [D,16,2,2], "norm_out.linear.bias"
 * (key list: SURVEY.md section 8b).  src_dtype may differ from the model dtype (converted on the fly).
 * Replaces ModelMixin.from_pretrained/.to(device,dtype) for this model (src/inference.py:191-215). */
S2V_API int s2v_load_weight(s2v_ctx* ctx, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim,
                    int32_t src_dtype, s2v_stream stream);
/* W[name] += scale * B.A   (A:[r,in] B:[out,r], fp32 device tensors; Conv2d patch_embed.proj takes A as [r,in*k*k]).
 * The merge the reference's PEFT LoRA is equivalent to (src/inference.py:218-229, alpha/r = 0.5).
 * Must be called after s2v_load_weight(name) and before s2v_finalize_weights. */
S2V_API int s2v_merge_lora(s2v_ctx* ctx, const char* name, const float* A, const float* B, int32_t rank, float scale,
                   s2v_stream stream);
/* Checks that every tensor was loaded; after this call the base weights are immutable (a runtime-mode context then takes adapters:
 * s2v_lora_attach). */
S2V_API int s2v_finalize_weights(s2v_ctx* ctx, s2v_stream stream);
/* Total bytes of context-owned weights (for the broadcast) and access to the packed arena so that ONE
 * collective can replicate a finalized model rank0 -> all. */
S2V_API int s2v_weight_arena(s2v_ctx* ctx, void** dev_ptr, int64_t* bytes);
/* Where one state-dict tensor lives inside the arena: byte offset of element [0][0], its rows x cols and the leading dimension
 * in elements of the model dtype (rows of the fused QKV / stacked modulation buffers are `ld` apart).  What a checkpoint tool
 * needs to read a merged weight back (W + (alpha/r) B A of src/inference.py:218-229) without knowing the packing. */
S2V_API int s2v_weight_slot(s2v_ctx* ctx, const char* name, int64_t* offset_bytes, int64_t* rows, int64_t* cols, int64_t* ld);

/* ---- runtime adapters (lora_runtime_rank = reserved[1] > 0): what the reference's PEFT model does, the adapter NOT merged -----------------
 * src/inference.py:218-229 attaches the subject-LoRA with PEFT and never merges it: every adapted Linear computes
 * base(x) + scaling * lora_B(lora_A(x)) at run time.  In this mode the six token linears of every block -- attn1.to_q / to_k / to_v (the fused
 * QKV), attn1.to_out.0, ff.net.0.proj, ff.net.2 -- run the branch beside the base weight, for W [N, K], A [r, K], B [N, r], scale s:
 *     T  = rnd(x . A^T)                     a down-projection kernel of its own; the point where PEFT rounds lora_A's output
 *     Bs = rnd(s * B)                       once, at attach / rescale time, the product taken in fp32
 *     y  = epilogue(x . W^T + T . Bs^T + b) ONE fp32 accumulator under the unchanged epilogue (q/k-norm + RoPE, GELU, gate + residual)
 * as a K extension of the base GEMM: y = [x | T] . [W | Bs]^T with K' = K + R (R = the rank padded to 64 / 128 with zero columns; the fused
 * QKV carries a block-diagonal tail of 3 R).  Without an adapter the launches use K and produce the bytes of a lora_runtime_rank = 0 context.
 * The other LoRA targets (patch_embed.proj, patch_embed.text_proj, norm{1,2}.linear: two rows, hoisted conditioning, or K = 64 < r) are
 * RE-MERGED: the context keeps a base copy of them and attach / rescale / detach rebuild the live weight from it with s2v_merge_lora's
 * arithmetic, so their bytes equal a merged context's (lora_adaln_scope 1 included).  Tails, A stacks and base copies live inside the weight
 * arena: s2v_weight_arena, s2v_bcast_weights and the replica path carry an attached adapter; s2v_weight_slot keeps returning the base
 * [rows, cols] with the larger ld; s2v_device_bytes counts all of it.
 * fp8 weight formats (weight_format 1 / 2 / 3) created with S2V_LORA_FP8_BRANCH run the same adapters beside e4m3 weights.  Merged before the
 * quantisation, W + s B A is rounded to three mantissa bits as one number and most of a subject-sized delta is lost; here the base stays the
 * quantised W and the branch stays 16-bit:
 *     y  = epilogue((q_a . q_w^T) * a_scale[m] * w_scale[n] + T . Bs^T + b)      one fp32 accumulator, one rounding at the epilogue
 *     T  = rnd16(x^ . A^T), x^ = the operand the base GEMM sees at the best precision in which it exists: the bf16 LayerNorm-modulate rows for
 *          the QKV and FF1 projections, the attention's / the FF1 epilogue's MX e4m3 image dequantised exactly (e4m3(byte) * 2^(scale - 127))
 *          for the out-projection and FF2
 * The fp8 GEMM kernels dequantise their accumulator tile in place after the K loop and accumulate T . Bs^T onto it on the bf16 matrix
 * instruction, before bias, GELU, gate + residual, q/k-norm + RoPE and FF1's MX output quantisation.  e4m3 rows cannot take 16-bit tail columns:
 * the arena holds a Bs array [N_pad][R] per adapted linear and the A stacks (R = the rank padded to 64), the workspace a T buffer [M_pad][3 R].
 * Attach / rescale / detach, the re-merged targets, hipGraph handling, replicas and the refusals are the ones described here; shards stay refused.
 * s2v_lora_attach: the arguments of s2v_merge_lora (fp32 device pointers, the reference's weight name, conv A as [r, C * 2 * 2]), legal AFTER
 *   s2v_finalize_weights; replaces what is attached under `name`.  Refused, with a message that says which: the mode off, an fp8
 *   weight_format created without S2V_LORA_FP8_BRANCH, a shard context, a rank over lora_runtime_rank, a name that is unknown or no LoRA target of the context (an
 *   S2V_CTX_ATTN_WEIGHTS context takes the four attn1 names).  hipGraph: an attach or a detach changes K' and drops the captured step (as
 *   s2v_set_rope does; it is re-captured at its next use).
 * s2v_lora_set_scale: the same A and B under another scale; the result equals, bit for bit, attaching them at that scale.  It rewrites
 *   values only (the tail of a branch weight, a re-merged weight) and KEEPS a captured step.  The caller keeps A and B (the library keeps no
 *   fp32 copy).
 * s2v_lora_detach: the base model; zeroes every tail (fp8 branch: every Bs array) and A stack, restores the re-merged weights.
 * Conditioning: patch_embed.proj and patch_embed.text_proj made the hoisted conditioning, so after an attach, rescale or detach that
 *   reaches them the forward entry points ask for s2v_set_conditioning again (a captured step reads the buffers it rewrites and stays valid).
 * Replicas: the attached state (names attached, rank, scale) is kept inside the arena too; s2v_mark_weights_loaded on a context whose arena was
 *   filled from another's (s2v_bcast_weights) reads it and runs the adapter it received.
 *   Such a replica holds the values but not the names: s2v_lora_set_scale on it is refused until it has attached an adapter itself, and
 *   s2v_lora_state reports the count, rank and scale its source wrote last.
 * s2v_lora_state: names attached, rank and scale of the last attach / rescale, hipGraph captures this context has made so far. */
S2V_API int s2v_lora_attach(s2v_ctx* ctx, const char* name, const float* A, const float* B, int32_t rank, float scale, s2v_stream stream);
S2V_API int s2v_lora_set_scale(s2v_ctx* ctx, const char* name, const float* A, const float* B, int32_t rank, float scale, s2v_stream stream);
S2V_API int s2v_lora_detach(s2v_ctx* ctx, s2v_stream stream);
S2V_API int s2v_lora_state(s2v_ctx* ctx, int32_t* attached, int32_t* rank, float* scale, int64_t* graph_captures);

/* Token geometry of the next calls: batch B (2 = the CFG pair of one video, 2b = the pairs of b videos in the reference's order
 * [negative x b | positive x b], custom_cogvideox_pipe.py:196,246-248; 1 <= B <= S2V_MAX_BATCH), text tokens T, latent frames F and latent H x W
 * (R = (H/2)(W/2) reference-image tokens, V = F*R video tokens, sequence order [text | ref | video]).
 * Allocates the activation workspace (no allocation happens inside the compute calls). */
#define S2V_MAX_BATCH 8   /* samples per call: the CFG pairs of at most four videos */
S2V_API int s2v_set_geometry(s2v_ctx* ctx, int32_t B, int32_t T, int32_t F, int32_t H, int32_t W);

/* whether QK^T of the attention runs in MX e4m3 at the current geometry: weight_format 2 always, 3 from its token threshold on (the decision
 * s2v_set_geometry took), 0 otherwise -- callers report this instead of re-deriving the threshold */
S2V_API int s2v_fp8_qk_active(s2v_ctx* ctx, int32_t* active);

/* RoPE tables, fp32 [R + V, 64] (reference rows first): cos/sin as produced by
 * get_3d_rotary_pos_embed (embeddings.py:505-570) and sliced in custom_cogvideox_pipe.py:223-235.
 * A setup call: it synchronises `stream` and inspects the tables on the host once per geometry -- tables that repeat every value
 * twice (repeat_interleave(2), what the reference builds) are also kept in a packed form that lets the QKV projection apply the
 * rotary embedding in its epilogue; any other table is honoured through the separate q/k pass. */
S2V_API int s2v_set_rope(s2v_ctx* ctx, const float* cos_dev, const float* sin_dev, s2v_stream stream);
/* 2B only: additive 3-D sincos table for the video tokens, model dtype [V, D] (embeddings.py:380-401,440-446). */
S2V_API int s2v_set_pos_embed(s2v_ctx* ctx, const void* table_dev, s2v_stream stream);

/* Step-invariant conditioning: text [B,T,text_embed_dim] -> patch_embed.text_proj; ref image latent [1,1,C,H,W] ->
 * patch_embed.proj, duplicated over the batch (cogvideox_transformer_3d.py:494-504).  The n_ref = 1 case of s2v_set_conditioning_refs. */
S2V_API int s2v_set_conditioning(s2v_ctx* ctx, const void* text_dev, const void* ref_latent_dev, s2v_stream stream);
/* One reference image per video: ref_latents [n_ref,1,C,H,W] contiguous, n_ref in {1, B/2, B}; sample j of the batch takes reference j mod n_ref.
 * 1 = one subject for every sample; B/2 = the reference's eval=True duplication `cat([ref, ref])` over [negative x b | positive x b]
 * (cogvideox_transformer_3d.py:503-504); B = eval=False, one row per sample.  The hoisted projections run per video -- the text projection on the
 * [negative | positive] pair of each video, the patch embedding on each reference -- with launches of a one-video call's shape, so a sample's
 * conditioning holds the bits it gets alone wherever the two geometries agree on split K: the split-K workspace is carved per geometry from
 * B * Ntok, and at a size where one video has it and the batch has not (configs[0]: 2500 against 5000 rows) the text projection (K =
 * text_embed_dim) sums in another order -- within bf16 rounding, not bitwise.  References beyond the first live in a buffer allocated here (a set-up call) and counted by
 * s2v_device_bytes as workspace; a change of n_ref drops a captured step. */
S2V_API int s2v_set_conditioning_refs(s2v_ctx* ctx, const void* text_dev, const void* ref_latents_dev, int32_t n_ref, s2v_stream stream);

/* CogVideoXTransformer3DModel.forward (cogvideox_transformer_3d.py:450-560) with eval=True.
 * latents [B,F,C,H,W] (lat_bstride = elements between samples, 0 = all samples share one latent), timesteps fp32
 * DEVICE [B]; out [B,F,C,H,W]. */
S2V_API int s2v_transformer_forward(s2v_ctx* ctx, const void* latents, int64_t lat_bstride, const float* timesteps_dev,
                            void* out, s2v_stream stream);
/* the same on latents [n_lat,F,C,H,W] contiguous that the B samples share: sample j embeds latent j mod n_lat (n_lat divides B; n_lat = B/2 is the
 * CFG batch `cat([latents] * 2)` of b videos, custom_cogvideox_pipe.py:246-248, without the copy) */
S2V_API int s2v_transformer_forward_videos(s2v_ctx* ctx, const void* latents, int32_t n_lat, const float* timesteps_dev, void* out,
                                   s2v_stream stream);

/* CogVideoXBlock.forward (cogvideox_transformer_3d.py:122-186) for layer `layer`: three residual streams in/out,
 * hidden [B,V,D], enc0 (text) [B,T,D], enc1 (ref) [B,R,D], temb [B,time_embed_dim]. */
S2V_API int s2v_block_forward(s2v_ctx* ctx, int32_t layer, const void* hidden, const void* enc0, const void* enc1,
                      const void* temb, void* out_hidden, void* out_enc0, void* out_enc1, s2v_stream stream);

/* CogVideoXAttnProcessor2_0.__call__ (attention_processor.py:2024-2097) with layer `layer`'s attn1 weights:
 * hidden [B,V,D] and encoder [B,T+R,D] are the already-modulated inputs; outputs have the same shapes. */
S2V_API int s2v_attn_forward(s2v_ctx* ctx, int32_t layer, const void* hidden, const void* encoder, void* out_hidden,
                     void* out_encoder, s2v_stream stream);
/* s2v_attn_forward with another context's weights: ctx's geometry, workspace and rotary tables (ctx: S2V_CTX_ATTN_WORKSPACE, or a model),
 * `weights`' layer `layer` (weights: a finalized S2V_CTX_ATTN_WEIGHTS context, or a model).  The same launches as s2v_attn_forward -- the
 * fused QKV GEMM with the q/k-norm + RoPE epilogue, the attention, the out-projection -- so the outputs are bit-identical to a model
 * context holding the same weights at the same geometry.  Refuses a ctx without a geometry, differing dtype, num_heads, inner dim or
 * weight_format or lora_runtime_rank (the workspace context owns the activation pitch, the weights context the tails and the A stacks), a shard
 * context on either side (s2v_set_shard), and weights that are not loaded.  Weights with an attached adapter run the branch. */
S2V_API int s2v_attn_forward_with(s2v_ctx* ctx, const s2v_ctx* weights, int32_t layer, const void* hidden, const void* encoder,
                          void* out_hidden, void* out_encoder, s2v_stream stream);
/* Device bytes the context holds: its weight arena (0 for S2V_CTX_ATTN_WORKSPACE) and its activation workspace (0 before s2v_set_geometry
 * and for S2V_CTX_ATTN_WEIGHTS).  The fixed buffers of a few KiB and the transient LoRA-merge scratch are not counted. */
S2V_API int s2v_device_bytes(s2v_ctx* ctx, int64_t* arena, int64_t* workspace);

/* Per-step scheduler scalars, computed on the host exactly as scheduling_ddim_cogvideox.py:364-394 /
 * scheduling_dpm_cogvideox.py:306-434 do (fp64), then cast; see s2v schedulers.py. */
typedef struct s2v_sched_coef {
    int32_t kind;      /* 0 DDIM, 1 DPM first/last step, 2 DPM multistep */
    float guidance;    /* classifier-free guidance scale of this step */
    float c_x0_x, c_x0_v, a_t, b_t, m1, m2, m3, m4, mn;
    float guidance_subject;   /* subject guidance scale of the triple combine (flags bit3, s2v_denoise_step_guided); the pair paths never read it */
} s2v_sched_coef;

/* scheduler.step (+ optional CFG combine, custom_cogvideox_pipe.py:266-296); ctx may be NULL.
 * flags bit0: noise_pred is the CFG pair [2,n] (uncond, cond) and is combined with coef->guidance;
 *       bit1: noise_pred is fp32 (what the reference hands to scheduler.step after .float());
 *       bit2: latents_out is fp32 and un-rounded (scheduler.step's own return value) instead of `dtype`;
 *       bit3: noise_pred is the subject-guidance triple [3,n] = (u, r, f) -- u: negative text, null reference; r: negative text, the reference;
 *             f: positive text, the reference -- combined in fp32 as
 *                 v = (u + coef->guidance_subject * (r - u)) + coef->guidance * (f - r)
 *             five operations that each round on their own, in this association.  guidance_subject = 1 is the pair's r + g (f - r)
 *             mathematically, and a u plane that holds the r plane's bits gives the pair's result bit for bit for ANY guidance_subject
 *             (r - u = +0).  Bit0 and bit3 together are refused.
 *       bit4: the RESCALE form (guidance rescale, below): refused here by name -- the device factor rides in s2v_sched_step_rescale.
 * latents in/out [n] (may alias); x0_hist fp32 [n] (DPM: read as old x0, then overwritten; may be NULL for DDIM);
 * noise [n] in `dtype` (DPM only). */
S2V_API int s2v_sched_step(s2v_ctx* ctx, const s2v_sched_coef* coef_host, const void* noise_pred, int32_t flags,
                   const void* latents_in, void* latents_out, float* x0_hist, const void* noise, int64_t n,
                   int32_t dtype, s2v_stream stream);

/* scheduler.add_noise of the video-to-video start (scheduling_ddim_cogvideox.py:405-431, scheduling_dpm_cogvideox.py:442;
 * pipeline_cogvideox_video2video.py:389): out = sqrt_alpha * sample + sqrt_one_minus_alpha * noise over n elements of `dtype`.  sqrt_alpha / sqrt_one_minus_alpha = alphas_cumprod[t] ** 0.5 and (1 - alphas_cumprod[t]) ** 0.5 taken in
 * `dtype` by the host (schedulers.py); each product and the sum round to `dtype` like torch's elementwise ops.  out may alias sample. */
S2V_API int s2v_add_noise(const void* sample, const void* noise, int64_t n, float sqrt_alpha, float sqrt_one_minus_alpha, void* out,
                          int32_t dtype, s2v_stream stream);

/* One iteration of the denoise loop (custom_cogvideox_pipe.py:241-296): transformer on the CFG pair sharing
 * `latents` [1,F,C,H,W], fp32 CFG, scheduler step, round to the model dtype; latents updated IN PLACE.
 * Several videos per call: with a geometry of B = 2b samples (b <= S2V_MAX_BATCH / 2) `latents`, `x0_hist` and `noise` are [b][F,C,H,W] contiguous,
 * sample j embeds video j mod b (no staged copy), the model output is [2b] = [negative x b | positive x b] and the CFG + scheduler step runs on
 * n = b F C H W elements with one timestep, guidance and coefficient set (per video: s2v_denoise_step_videos).  B = 1 is one sample without CFG.  A batched call runs on one GPU: the
 * CFG-parallel and Ulysses entry points below keep requiring B = 1 or 2.
 * use_graph != 0 captures the launch sequence into a hipGraph on first use and replays it afterwards
 * (timestep and coefficients live in device memory, so one graph serves all steps). */
S2V_API int s2v_denoise_step(s2v_ctx* ctx, void* latents, float timestep, const s2v_sched_coef* coef_host, float* x0_hist,
                     const void* noise, int32_t use_graph, s2v_stream stream);
/* The same iteration with the step's scalars PER VIDEO: on a geometry of B = 2b samples [negative x b | positive x b] (B = 1 or 2: b = 1)
 * `timesteps` and `coefs` are HOST arrays of b entries; sample j runs at timesteps[j mod b] (time embedding and every AdaLN modulation are per
 * sample) and video k is stepped with coefs[k] -- its own kind, guidance scale and scalars, so a video on its first DPM step (kind 1) may sit
 * beside videos on multistep steps (kind 2), and DDIM beside DPM.  x0_hist and noise are required as soon as one kind is not 0.  The timesteps
 * and the coefficient sets each go up in one asynchronous copy; the captured graph does not depend on their values, so one graph serves every
 * step.  s2v_denoise_step is this call with its scalar repeated b times, bit for bit.  Shard contexts are refused as s2v_denoise_step refuses
 * them; the CFG-parallel and Ulysses entry points stay single-scalar. */
S2V_API int s2v_denoise_step_videos(s2v_ctx* ctx, void* latents, const float* timesteps, const s2v_sched_coef* coefs, float* x0_hist,
                            const void* noise, int32_t use_graph, s2v_stream stream);
/* ---- masked video-to-video: repaint inside a mask, keep the rest (pipeline_stable_diffusion_inpaint.py:1271-1285, the 4-channel branch) ------
 * After every scheduler step the latents OUTSIDE the mask are overwritten with the input video's latents noised to the video's next timestep
 * -- with the noise that started the loop -- and after its last step with the clean input latents.  The mask is exactly 0 or 1, so the
 * reference's (1 - m) * proper + m * latents is a select on the step's result as it is stored today (rounded to the model dtype T):
 *   m = 1:             the step's result
 *   m = 0, not last:   rnd_T(rnd_T(sqrt_alpha * z0) + rnd_T(sqrt_one_minus_alpha * noise0))      (s2v_add_noise's arithmetic, no fma)
 *   m = 0, last:       z0, bit for bit (a flag, not the coefficients (1, 0), which would turn -0 into +0)
 * x0_hist keeps the unblended x0: the scheduler's state is left alone, as in the reference.
 * Change map (differential diffusion, e.g. pipeline_stable_diffusion_xl_differential_img2img.py:1316-1347): the plane holds LEVELS 0..255
 * (unsigned bytes; 255 = repaint from the first step, 0 = keep the input -- the reference's `map` is 1 - level / 255) and the test is
 *   kept  <=>  level <= keep_max
 * with keep_max the video's threshold of this step.  A 0 / 1 mask is the case keep_max = 0.  For a video whose plan runs n steps the pipeline
 * passes, after step j (0-based), keep_max_j = max(0, (255 (n - j - 1) - 1) / n) (integer division): for j < n - 1 exactly
 * level * n < 255 (n - j - 1), the reference's map > (j + 1) / n in integers; 0 on the last step, where only level-0 cells are kept, as the
 * clean z0.  The map never multiplies a latent: every step is still the select above.  Two deliberate differences from the reference's loop:
 * it keeps nothing after its last step (here level 0 stays the input, as a mask's 0 does), and with strength < 1 it divides by the full
 * schedule without offsetting the step index (here n and j count the steps actually run). */
typedef struct s2v_blend {
    float sqrt_alpha, sqrt_one_minus_alpha;   /* of the video's NEXT timestep, taken in T by the host as for s2v_add_noise */
    int32_t last;                             /* != 0: this is the video's last step */
    int32_t keep_max;                         /* 0..255: cells whose level is <= keep_max are kept; 0 for a 0 / 1 mask */
} s2v_blend;
#define S2V_MASK_DTYPE_U8 3   /* s2v_mask_to_latent: a uint8 mask, non-zero = repaint (beside S2V_DTYPE_*: binarised at 0.5); s2v_map_to_latent: levels */
/* The pixel mask of one video [F,H,W] (F = 4k + 1; H, W multiples of 8; mask_dtype S2V_DTYPE_* -- value < 0.5 -> 0, >= 0.5 -> 1 as
 * image_processor.py:535-536 binarises -- or S2V_MASK_DTYPE_U8) -> latent_mask uint8 [(F-1)/4+1, H/8, W/8], one plane for all latent channels:
 * a cell is 1 (repaint) if ANY pixel it covers is 1 -- its 8 x 8 block of pixel frame 0 for latent frame 0, of pixel frames 4j-3 .. 4j for latent
 * frame j >= 1, the causal grouping of the VAE encode.  (Beyond the reference, whose prepare_mask_latents :747-760 takes the nearest pixel and
 * has no time axis: a latent any of whose pixels the caller asked to change is never kept.)  pixel_mask, when not NULL, receives the
 * binarised pixel mask uint8 [F,H,W] (what the masked post-processes take).  One launch. */
S2V_API int s2v_mask_to_latent(const void* mask, int32_t mask_dtype, int32_t F, int32_t H, int32_t W, uint8_t* latent_mask, uint8_t* pixel_mask,
                               s2v_stream stream);
/* The change map of one video [F,H,W] (same sizes as s2v_mask_to_latent) -> latent_level uint8 [(F-1)/4+1, H/8, W/8].  Every value becomes a
 * level 0..255: map_dtype S2V_MASK_DTYPE_U8 means LEVELS here, the byte itself (not "non-zero"); S2V_DTYPE_F32 / _BF16 / _F16 are values in
 * [0, 1] quantised as level = floor(clamp(v, 0, 1) * 255 + 0.5) in fp32, one multiply and one add, no fma; NaN gives 0.  A cell takes the
 * MAXIMUM level over the pixels it covers, the block s2v_mask_to_latent reduces with "any": a cell any of whose pixels asked for more change is
 * never changed less.  pixel_mask, when not NULL, receives level > 0 as uint8 0 / 1 [F,H,W] (what the masked post-processes take: a pixel whose
 * own level is 0 is the input video's).  One launch. */
S2V_API int s2v_map_to_latent(const void* map, int32_t map_dtype, int32_t F, int32_t H, int32_t W, uint8_t* latent_level, uint8_t* pixel_mask,
                              s2v_stream stream);
/* The blend operands of the call on the context: z0 (the clean input latents, scaled) and noise0 (the noise that started the loop), both
 * [b,F,C,H,W] in the model dtype, and latent_mask uint8 [b,F,H,W] (a 0 / 1 mask, or the levels of s2v_map_to_latent), for the b = B/2 videos of the geometry.  The pointers are HELD, nothing is
 * copied: they must stay valid until they are replaced or cleared (all NULL, b = 0).  Setting or clearing drops a captured step (the operands
 * are part of its key).  s2v_denoise_step / s2v_denoise_step_videos never read them. */
S2V_API int s2v_set_blend(s2v_ctx* ctx, const void* z0, const void* noise0, const uint8_t* latent_mask, int32_t b);
/* s2v_denoise_step_videos with the blend in the step's last kernel: `blends` is a HOST array of b records, video k blended with blends[k]
 * (its own next timestep and last-step flag, so a video on its last step may sit beside videos that go on).  The records go up beside the
 * coefficient sets, so one captured graph serves every step of a masked call.  Refused: a geometry with B = 1 (one sample of a CFG-parallel
 * pair: the split entries have no masked form), a shard context, operands not set for b = B/2, a keep_max outside 0..255. */
S2V_API int s2v_denoise_step_masked(s2v_ctx* ctx, void* latents, const float* timesteps, const s2v_sched_coef* coefs, const s2v_blend* blends,
                            float* x0_hist, const void* noise, int32_t use_graph, s2v_stream stream);
/* s2v_sched_step followed by the blend, for ONE video whose latent is [F,C,H,W]: latents_out in `dtype` (flags bit2 is refused: the blend runs
 * on the rounded result), z0 / noise0 [F,C,H,W] in `dtype`, latent_mask uint8 [F,H,W] (mask or levels); a keep_max outside 0..255 is refused;
 * ctx may be NULL. */
S2V_API int s2v_sched_step_masked(s2v_ctx* ctx, const s2v_sched_coef* coef_host, const s2v_blend* blend_host, const void* noise_pred, int32_t flags,
                          const void* latents_in, void* latents_out, float* x0_hist, const void* noise, const void* z0, const void* noise0,
                          const uint8_t* latent_mask, int32_t F, int32_t C, int32_t H, int32_t W, int32_t dtype, s2v_stream stream);
/* ---- subject guidance: a scale of its own for the reference image ------------------------------------------------------------------------------
 * The CFG pair gives both samples the reference, so `guidance` amplifies text against no text.  Three samples per video separate the two:
 * u (negative text, a null reference), r (negative text, the reference), f (positive text, the reference), combined as flags bit3 of
 * s2v_sched_step states.  Geometry: B = 3b samples [u x b | r x b | f x b], b = 1 or 2 videos (S2V_MAX_BATCH stays 8).
 * s2v_set_conditioning_triples: text [2b,T,text_embed_dim] = [negative x b | positive x b], ref_latents [b,1,C,H,W], null_ref_latents
 * [n_null,1,C,H,W] with n_null = 1 (one for every video) or b.  Video v's [negative | positive] pair is projected by one launch of a one-video
 * call's shape (M = 2T) and its negative rows go to samples u_v and r_v; every reference and null reference runs the per-reference patch
 * embedding.  Samples r and f therefore hold the bits a pair call's conditioning holds, wherever the two geometries agree on split K (as
 * s2v_set_conditioning_refs words it).  The reference table is one entry per sample, [null x b | ref x b | ref x b] (n_ref = B), allocated here
 * and counted as workspace.  A change of layout (pairs <-> triples) drops a captured step; the context records which layout it holds, since
 * B = 6 is three pairs or two triples by shape alone.
 * s2v_denoise_step_guided: the whole step on that geometry -- the forward on the triples sharing each video's latent (`latents`, `x0_hist`,
 * `noise` [b][F,C,H,W]; timesteps / coefs HOST arrays of b entries as s2v_denoise_step_videos), then the triple combine with
 * coefs[k].guidance_subject and coefs[k].guidance and the scheduler step, in place.  blends != NULL: the masked form, b records, after
 * s2v_set_blend for b videos.  One captured graph serves every step; it is another graph than a pair step's.
 * Refused by name: B not a multiple of 3 or b > 2; conditioning not set by s2v_set_conditioning_triples; a shard context; a pending
 * CFG-parallel split; an armed step-cache mode or attention map (both assume pairs).  s2v_denoise_step, _videos and _masked refuse a context
 * conditioned as triples. */
S2V_API int s2v_set_conditioning_triples(s2v_ctx* ctx, const void* text_dev, const void* ref_latents_dev, const void* null_ref_latents_dev,
                                         int32_t n_null, s2v_stream stream);
S2V_API int s2v_denoise_step_guided(s2v_ctx* ctx, void* latents, const float* timesteps, const s2v_sched_coef* coefs, const s2v_blend* blends,
                                    float* x0_hist, const void* noise, int32_t use_graph, s2v_stream stream);
/* pointer to the [B,F,C,H,W] model output of the last s2v_denoise_step (context-owned, model dtype); [3b,...] after s2v_denoise_step_guided */
S2V_API int s2v_last_noise_pred(s2v_ctx* ctx, void** dev_ptr);

/* ---- Temporal windows: a long latent denoised as overlapping windows, averaged per step ----------------------------------------------------
 * The model sees at most 13 latent frames (49 video frames).  A long latent [L][C][H W] is stepped as W = (L - F) / stride + 1 windows of the
 * geometry's F frames, window k over latent frames [k stride, k stride + F): equally spaced, so a forward's windows are a pointer into the
 * long latent and a stride.  With g the step's coef->guidance, weights w[F] and wsum[f] the sum of the weights of the windows covering frame f
 * (added up in window order), one step is, in fp32, every operation rounding on its own:
 *     acc = +0;   for k = 0 .. W - 1, frame j of window k:   v = u_k + g * (f_k - u_k);   acc[k stride + j] = acc[k stride + j] + w[j] * v
 *     vbar = acc / wsum[frame]                                (IEEE division)
 * and then the scheduler arithmetic of s2v_sched_step (flags bit1, no bit0) on the L frames from vbar.  Every window shares the step's
 * timestep, the text pair and the reference.
 * s2v_set_windows: after s2v_set_geometry with B = 2 per_forward ([negative x per_forward | positive x per_forward]: the text rows repeated
 * per_forward times, one shared reference row) and F = the window's frames.  weights: HOST array [F].  Requires 1 <= stride <= F, L >= F,
 * (L - F) % stride == 0 and per_forward dividing W.  Allocates the fp32 plane [L][C][H][W] with the weights and their sums behind it, counted
 * by s2v_device_bytes as workspace; with windows never set s2v_device_bytes reports what it reports without this feature.  L = 0 clears and
 * frees; s2v_set_geometry (the same geometry included) and s2v_set_shard clear too.  Setting or clearing drops a captured step.
 * Refused by name: a shard context, B = 1 (a CFG-parallel half), a context conditioned as triples, an armed step-cache mode, an armed
 * attention map, B != 2 per_forward.
 * s2v_denoise_step_windows: the whole step -- latents / x0_hist / noise are [L][C][H][W] (model dtype / fp32 / model dtype), updated in place:
 * W / per_forward rounds of the forward on the next per_forward windows followed by the blend kernel, then one scheduler step on the L frames.
 * use_graph: one captured graph of its own key holds every forward of the step.  Refuses a context without windows; s2v_denoise_step,
 * _videos, _masked and _guided refuse a context with windows. */
S2V_API int s2v_set_windows(s2v_ctx* ctx, int32_t L, int32_t stride, int32_t per_forward, const float* weights);
S2V_API int s2v_denoise_step_windows(s2v_ctx* ctx, void* latents, float timestep, const s2v_sched_coef* coef_host, float* x0_hist,
                                     const void* noise, int32_t use_graph, s2v_stream stream);

/* ---- Guidance rescale: the guided prediction scaled back to the spread of the text-conditioned one, per video ---------------------------------
 * (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4; diffusers' rescale_noise_cfg,
 * pipelines/stable_diffusion/pipeline_stable_diffusion.py:67-90.)  THE DEFINITION -- kernels and tests restate it.  For video k of a step:
 *   n      = F C H W elements
 *   f      its text-conditioned prediction as fp32: the positive half of a pair, the f plane of a triple
 *   v      its guided prediction exactly as the step combines it (s2v_sched_step flags bit0 / bit3: the same separately rounded fp32 operations)
 *   phi_k  in [0, 1]
 * Four sums in fp64 over the fp32 values widened to fp64 (so every square is exact), each add rounding on its own:
 *   Sf = sum f    Sff = sum f^2    Sv = sum v    Svv = sum v^2
 * in THIS order, whatever the grid, the CU count or the timing (no floating-point atomics).  The video is cut into chunks of
 * S2V_CFG_STATS_CHUNK = 4096 consecutive elements (the last one may be short).  Within chunk c, lane t of 256 adds its elements
 * c 4096 + t + 256 r for r = 0, 1, ... in ascending r, starting from +0; the 256 lane sums meet in the halving tree
 * lane[t] = lane[t] + lane[t + s] for t < s, s = 128, 64, ..., 1; lane[0] is the chunk's sum.  The video's sum adds the chunk sums in ascending
 * c, starting from +0.
 * Deviations with n - 1 in the divisor, as torch.std:    std_x = sqrt((Sxx - Sx Sx / n) / (n - 1))     (fp64, every operation rounding on its own)
 * The factor, in fp64, rounded once to fp32:              k = float(phi (std_f / std_v) + (1 - phi))
 * k = 1.0f exactly when phi == 0, when n < 2, when std_v is not finite (an inf or NaN anywhere in v), when std_v == 0, or when the quotient is
 * not finite.  (A constant v has std_v == 0 exactly only where its sums are exact in fp64 -- small dyadic constants; the cancellation in
 * Sxx - Sx Sx / n is the textbook one; fp64 sums over fp32 data keep it harmless unless the mean dwarfs the deviation.)
 * The rescaled prediction is one more separately rounded fp32 multiply ahead of the scheduler arithmetic:    v' = v k
 * A DELIBERATE DIFFERENCE from diffusers, which computes phi (v std_f / std_v) + (1 - phi) v element by element: one factor per video is the same
 * value mathematically with fewer roundings.  The statistics cover the whole video, on a masked or change-map step too, as the reference's do.
 *
 * s2v_set_guidance_rescale: context state, like the blend operands.  phi: HOST array of b values for the b videos of the geometry (B = 2b pairs, or
 * B = 3b triples).  The values live in device memory: new values for the same b re-capture nothing.  A first arming allocates, beside the
 * workspace, the chunk partials [b][ceil(n / 4096)][4] fp64 with the sums, factors and phi behind them, and the factor log; s2v_device_bytes
 * COUNTS both as workspace while the context is armed, and neither otherwise.  All values zero: nothing is armed -- the partials are freed, every step entry runs
 * the launches it ran and returns the bytes it returned; the log is kept (a shrinking batch may arm again).  phi = NULL with b = 0 clears: the
 * log is freed too and s2v_device_bytes reports what it reports without this feature.  s2v_set_geometry (the same geometry included) and
 * s2v_set_shard disarm as all-zero values do.  Arming, disarming and a change of b drop a captured step.
 * Armed, s2v_denoise_step, _videos, _masked and _guided (plain and masked) run, behind the forward: the statistics kernel, the finalize kernel,
 * and the RESCALE form of the step kernel -- on every step-cache mode, reuse steps included.  The captured graph of an armed step has a key of its
 * own.  Every finalize appends its b factors (0 in the columns past b) to row `count` of the log [S2V_CFG_LOG_STEPS][S2V_MAX_BATCH / 2] fp32 while
 * count < S2V_CFG_LOG_STEPS and advances the device-side count, so graph replays log too.
 * Refused by name: a value outside [0, 1] or NaN; b that is not the geometry's videos; no geometry; B = 1 (no CFG: the CFG-parallel split entries
 * refuse an armed context too); a shard context; temporal windows (s2v_denoise_step_windows combines the windows before its one scheduler step, and
 * a statistic per window is another feature); an attention-only context.
 * s2v_guidance_rescale_read: synchronises the device.  sums [b][4] fp64 (Sf, Sff, Sv, Svv) and factors [b] of the LAST armed step (either may be
 * NULL; non-NULL needs an armed context); log: HOST buffer of S2V_CFG_LOG_STEPS x S2V_MAX_BATCH / 2 floats receiving the first
 * min(count, S2V_CFG_LOG_STEPS) rows (may be NULL); log_count: the steps logged since the log was allocated (may be NULL; 0 without a log). */
#define S2V_CFG_STATS_CHUNK 4096
#define S2V_CFG_LOG_STEPS 1024
S2V_API int s2v_set_guidance_rescale(s2v_ctx* ctx, const float* phi, int32_t b);
S2V_API int s2v_guidance_rescale_read(s2v_ctx* ctx, double* sums, float* factors, float* log, int32_t* log_count);
/* The RESCALE form of s2v_sched_step / s2v_sched_step_masked: the same arguments with `flags` bit4 (S2V_SCHED_RESCALE) set and `factors`, a DEVICE
 * pointer to the one fp32 factor of the one video, behind them: v' = v factors[0] ahead of the scheduler arithmetic.  (The two entries above keep
 * their signatures and refuse bit4 by name, pointing here.) */
#define S2V_SCHED_RESCALE 16
S2V_API int s2v_sched_step_rescale(s2v_ctx* ctx, const s2v_sched_coef* coef_host, const void* noise_pred, int32_t flags, const void* latents_in,
                                   void* latents_out, float* x0_hist, const void* noise, int64_t n, int32_t dtype, const float* factors,
                                   s2v_stream stream);
S2V_API int s2v_sched_step_masked_rescale(s2v_ctx* ctx, const s2v_sched_coef* coef_host, const s2v_blend* blend_host, const void* noise_pred,
                                          int32_t flags, const void* latents_in, void* latents_out, float* x0_hist, const void* noise,
                                          const void* z0, const void* noise0, const uint8_t* latent_mask, int32_t F, int32_t C, int32_t H,
                                          int32_t W, int32_t dtype, const float* factors, s2v_stream stream);

/* ---- Step cache: a step whose timestep embedding barely moved skips the block stack ---------------------------------------------------------
 * Opt-in state on a model context.  X is the packed residual buffer [B][Ntok][D]; its video rows are rows [T + R, T + R + V) of each sample.
 * The cache is dense [B][V][D] in the model dtype T.  Every forward (s2v_transformer_forward*, s2v_denoise_step, _videos, _masked) runs in the
 * mode that was armed for it:
 *   S2V_STEP_FULL     the launches the entry runs without a cache, not one more.
 *   S2V_STEP_CAPTURE  those launches plus two: after the streams are embedded the video rows IN are copied to the cache, and after the last
 *                     block the cache becomes  delta = rnd_T(float(OUT) - float(IN))  (round to nearest even; a plain subtraction in fp32),
 *                     OUT being the video rows the tail is about to read.  The residual is valid from then on.
 *   S2V_STEP_REUSE    time embedding; the modulation GEMV of the norm_out rows only (the last 2 D rows of the stack, the ones the tail
 *                     reads); patchify; the patch-embed linear of every sample (plus the sincos table where the model has no RoPE) -- text
 *                     and reference rows are not copied, nothing reads them; X_video = rnd_T(float(IN') + float(delta)); the tail
 *                     (norm_final, norm_out, proj_out); unpatchify.  The residual and its validity stay as they are.
 * s2v_step_cache_enable: after s2v_set_geometry; on = 1 allocates the cache for the current geometry (B V D elements), on = 2 additionally a
 * second buffer of the same size that keeps IN of EVERY forward for s2v_step_cache_read (diagnostics: one more copy launch per forward, FULL
 * included), on = 0 frees both.  While off, s2v_device_bytes reports what it reports without this feature; while on, the buffers count as
 * workspace.  A new geometry re-sizes the buffers.  Refused on a shard context.  A change of `on` drops a captured step.
 * s2v_step_cache_arm: the mode of the NEXT forward only; after it (or after anything that clears the validity) the mode is S2V_STEP_FULL
 * again, so a forgotten arm costs time, never correctness.  Refused by name: CAPTURE / REUSE on a shard context, without enable, and REUSE
 * without a valid residual; a s2v_denoise_split_begin that finds CAPTURE / REUSE armed refuses (CFG-parallel has its own forward per rank: the
 * step cache runs on one GPU).
 * The validity is cleared by everything that makes the stored residual belong to another computation: s2v_set_geometry, s2v_set_conditioning
 * / _refs, s2v_load_weight, s2v_merge_lora, s2v_finalize_weights, s2v_mark_weights_loaded, s2v_lora_attach / _set_scale / _detach,
 * s2v_set_rope, s2v_set_pos_embed, s2v_set_attn_p_format, s2v_set_shard, s2v_step_cache_enable.
 * A captured step is kept per mode: a plan that alternates captures each kind once. */
#define S2V_STEP_FULL 0
#define S2V_STEP_CAPTURE 1
#define S2V_STEP_REUSE 2
S2V_API int s2v_step_cache_enable(s2v_ctx* ctx, int32_t on);
S2V_API int s2v_step_cache_arm(s2v_ctx* ctx, int32_t mode);
/* enabled: 0 / 1 / 2 as given to s2v_step_cache_enable; valid: a residual is held; bytes: device bytes of the cache buffers */
S2V_API int s2v_step_cache_state(s2v_ctx* ctx, int32_t* enabled, int32_t* valid, int64_t* bytes);
/* diagnostics read-out into out_dev [B][V][D] (model dtype): which = 0 IN, the video rows as the last forward embedded them (enable 2 only);
 * 1 OUT, the video rows of X as the last forward's tail read them; 2 the residual (valid only) */
S2V_API int s2v_step_cache_read(s2v_ctx* ctx, int32_t which, void* out_dev, s2v_stream stream);
/* the timestep embedding of n HOST timesteps -> out_dev [n][time_embed_dim] (model dtype), in chunks of at most S2V_MAX_BATCH: row i is exactly
 * what a step at timesteps_host[i] holds as its embedding (the indicator of the step-cache plan).  Finalized weights only, no geometry;
 * synchronises the stream */
S2V_API int s2v_time_embedding(s2v_ctx* ctx, const float* timesteps_host, int32_t n, void* out_dev, s2v_stream stream);

/* ---- Attention map: the softmax mass a video query puts on the reference-image keys (and on text-token spans) ---------------------------------
 * Every block runs joint attention over [text T | reference R | video V].  With q_i, k_j the normed and rotated rows of one (sample, head),
 * s_ij = q_i . k_j / 8 over the sample's own Ntok keys and  mass_r(b, h, i) = sum over j in range r of softmax_j(s_i.)  in fp32.  Opt-in state
 * on a model context; while off every entry runs the launches it runs without this feature and s2v_device_bytes reports what it reports
 * without it.
 * s2v_attn_map_enable: after s2v_set_geometry; on != 0 allocates the raw sums acc [1 + n_spans][B][H][V] fp32 (zeroed, counted as workspace
 * while on), on = 0 frees them.  Range 0 is always the reference stream [T, T + R); text_spans_host holds n_spans <= 3 pairs (k0, k1), token
 * ranges inside [0, T); the queries are the video rows [T + R, Ntok).  A new geometry re-sizes and zeroes the buffer (a span that no longer fits
 * refuses the geometry call and leaves the map off).  Refused on a shard context and on attention-only contexts.  Drops a captured step.
 * s2v_attn_map_arm: the layers (bit l = block l) of the NEXT forward only (s2v_transformer_forward*, s2v_denoise_step, _videos, _masked); after
 * it the mask is 0 again.  After the attention launch of every armed layer the forward launches the mass kernel (csrc/attn_mass.hip) on the
 * same stream, which adds mass to acc in one fp32 add per element (no atomics: two armed forwards hold the fp32 sum of each alone, bit for bit),
 * and the host count goes up by one per armed layer launch.  The kernel only reads the forward's q / k buffer: an armed step returns the bits of
 * the un-armed step.  Refused by name: on a shard context, without enable, while fp8 QK^T is active at the geometry (weight_format 2, or 3 beyond
 * its token threshold: q and k exist normed only as MX e4m3 images; the plain fp8 weight format with its 16-bit attention is allowed), together
 * with S2V_STEP_REUSE (either order of the two arms: the block stack does not run), a bit at or beyond num_layers; a s2v_denoise_split_begin
 * that finds a mask armed refuses (a CFG-parallel split holds one sample of the pair per rank).
 * An armed step is another launch sequence: a captured step (use_graph) is kept per (step-cache mode, layer mask), and an un-armed step never
 * replays an armed executable nor the reverse.
 * s2v_attn_map_read: per_head != 0 copies the raw sums [n][B][H][V] to out_dev; per_head = 0 writes the head mean [n][B][V],
 * (acc[.][.][0][i] + ... + acc[.][.][H-1][i], in that order, fp32) * (1.0f / (H * count)), which needs count >= 1.  *count: the armed layer
 * launches since the last reset.  s2v_attn_map_reset zeroes the sums and the count (synchronises the device).
 * Engines whose attention runs on the matrix pipe (bf16, fp16) run the MFMA form (impl 0 of s2v_op_attn_mass), an fp32 engine the generic one. */
S2V_API int s2v_attn_map_enable(s2v_ctx* ctx, int32_t on, const int32_t* text_spans_host, int32_t n_spans);
S2V_API int s2v_attn_map_arm(s2v_ctx* ctx, uint64_t layer_mask);
S2V_API int s2v_attn_map_read(s2v_ctx* ctx, int32_t per_head, void* out_dev, int64_t* count, s2v_stream stream);
S2V_API int s2v_attn_map_reset(s2v_ctx* ctx);

/* ---- Attention steering: a logit bias on key ranges (prompt-to-prompt style reweighting, softmax(s + ln w)) -------------------------------------
 * ONE definition, which the kernels (csrc/attention.hip), tests/attn_steer_ref.py and this comment state alike.  For sample b, head h, query row
 * i and key j of the joint attention over [text T | reference R | video V]:
 *     s_ij  = q_i . k_j / 8
 *     out_i = sum_j softmax_j(s_ij + beta_b(i, j)) v_j
 *     beta_b(i, j) = ln w_r  when all three hold: j lies in key range r = [k0_r, k1_r), bit b of that range's sample_mask is set, and i lies in the
 *                    query range [q0, q1);  otherwise beta_b(i, j) = 0.
 * At most four key ranges, disjoint and ascending, each non-empty and inside [0, Ntok); w finite with 2^-16 <= w <= 2^16 (no w = 0: a first key
 * tile that is entirely -inf would break the kernel's adoption of the first tile's maximum); B <= 32 samples.  In the MFMA kernel the bias is
 * log2 w, added to the exp2-domain score before the tail mask's -inf and before everything its softmax segment does (the row-sum vote of the
 * deferred maximum, the slow path's maximum, exp2); the generic kernel adds ln w before its maximum and expf.
 * Rows outside [q0, q1) and samples outside every mask are un-steered rows: a sample outside the masks, and a 32-row wave of the MFMA kernel with
 * no row inside [q0, q1), run the un-steered code on every key tile and return the un-steered launch's bits (both attn_pp, i.e. bf16 up to 4608
 * tokens; beyond, the un-steered product kernel is attn_q4, within rounding).  The rows outside [q0, q1) of a wave that also holds rows inside
 * get 0.0f added and return the same bits unless a steered row of their wave changes the wave-wide vote of the deferred maximum past the first
 * key tile (a row sum beyond 2^64): the slow path re-sums a tile in another order, within rounding.
 * Engines: a steered layer of a bf16 engine runs attn_pp<STEER> at EVERY length (persistent under the rule of the un-steered launch); an fp32
 * engine runs the steered generic kernel -- fp32 is the parity mode and its speed is no goal.  Un-steered layers, and every call with steering
 * off, run the launches they run without this feature.
 * s2v_attn_steer_enable: after s2v_set_geometry; on != 0 allocates the record's device table (counted by s2v_device_bytes as workspace while on) holding
 * a record that steers nothing, on = 0 frees it.  Drops a captured step.  While off every entry runs what it runs without this feature.
 * s2v_attn_steer_set: n <= 4 ranges; the query range is the geometry's video rows [T + R, Ntok).  Checks the ranges against the current geometry
 * (inside [0, Ntok), order, overlap, weight bounds) with an error that names what is wrong, BEFORE anything is replaced; synchronises the device and
 * uploads.  The table is data, not a launch argument: a captured step is kept and replays with the new weights.  A later s2v_set_geometry re-checks
 * the held ranges; one that no longer fits refuses the geometry call and leaves steering off.
 * s2v_attn_steer_arm: the layers (bit l = block l) of the NEXT forward only (s2v_transformer_forward*, s2v_denoise_step, _videos, _masked).  An
 * armed step is another launch sequence: captured steps are kept per (step-cache mode, map layer mask, steer layer mask), and an un-armed step
 * never replays an armed executable nor the reverse.
 * Refused by name: fp16 engines; every fp8 weight format (their attention writes the MX output); attn_p_format 1 (fp16 V^T); shard contexts;
 * attention-only contexts; triple-conditioned contexts and s2v_denoise_step_guided; contexts with temporal windows and s2v_denoise_step_windows;
 * s2v_denoise_split_begin (CFG-parallel); an armed attention map or S2V_STEP_REUSE together with an armed steer, in either order of the two arms; a
 * layer bit at or beyond num_layers; s2v_block_forward and the s2v_attn_forward* / AttnProcessor seams while a steer is armed. */
typedef struct s2v_attn_steer_range {
    int32_t k0, k1;          /* keys [k0, k1) of every sample's Ntok */
    float w;                 /* the softmax weight of those keys is multiplied by w before normalisation */
    uint32_t sample_mask;    /* bit b: the range applies to sample b */
} s2v_attn_steer_range;
/* the operator-level record: the ranges as arrays plus the query range */
typedef struct s2v_attn_steer_record {
    int32_t n, q0, q1, reserved;
    int32_t k0[4], k1[4];
    float w[4];
    uint32_t sample_mask[4];
} s2v_attn_steer_record;
S2V_API int s2v_attn_steer_enable(s2v_ctx* ctx, int32_t on);
S2V_API int s2v_attn_steer_set(s2v_ctx* ctx, int32_t n, const s2v_attn_steer_range* ranges_host);
S2V_API int s2v_attn_steer_arm(s2v_ctx* ctx, uint64_t layer_mask);
/* the steered kernel on its own: qkv / vt_scratch / out as s2v_op_attention takes them.  impl 0: attn_pp<STEER> (bf16, any Ntok, one workgroup
 * per 256 query rows); impl 1: the steered generic kernel (any dtype).  The record is copied to ONE table per process on the device current at the
 * first call, ordered on `stream`: such calls stay on that device and on the stream of the first call (another stream is refused by name), and
 * the entry is not thread-safe -- a test and benchmark entry; contexts hold their own table.  Refused by name: a bad record (as
 * s2v_attn_steer_set), impl 0 with another dtype than bf16 */
S2V_API int s2v_op_attention_steer(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok, int32_t dtype, int32_t impl,
                                   const s2v_attn_steer_record* record_host, s2v_stream stream);

/* ---- Steering maps: the same bias with a weight per query row -- per video cell through the context entries ("put the subject here") ------------
 * ONE definition, which the kernels (csrc/attention.hip, MAP), tests/attn_steer_map_ref.py and this comment state alike:
 *     s_ij  = q_i . k_j / 8
 *     out_i = sum_j softmax_j(s_ij + beta_b(i, j)) v_j
 *     beta_b(i, j) = ln W_p[i - q0]  when j lies in key range r = [k0_r, k1_r), p = plane[r][b] >= 0, and q0 <= i < q1;  otherwise 0.
 * Up to four key ranges, ascending and disjoint, as above; up to 16 planes W_p of q1 - q0 >= 1 fp32 weights each, finite with 2^-16 <= w <= 2^16;
 * plane[r][b] is an int8 per range and sample (S2V_MAX_BATCH of them), -1: range r does not apply to sample b (it replaces sample_mask).  Through
 * the context entries the query range is the video rows [T + R, Ntok) and a plane is indexed by video cell (f * Hp + y) * Wp + x, Hp = H / 2,
 * Wp = W / 2 of the latent (H / 16, W / 16 of the pixels): tokens are frame-major, then row-major inside a frame.  The MFMA kernel adds log2 w, the
 * generic kernel ln w, each rounded to fp32 once on the host by the expressions of the scalar record: a constant plane gives the scalar call's bits.
 * Liveness: per sample and 32-row wave of the MFMA kernel the host keeps the ranges that have a weight != 1 on a row of the wave; a wave looks at
 * those ranges only, and a wave with none runs the un-steered code on every tile and returns the un-steered launch's bits (attn_pp).
 * s2v_attn_steer_set_maps: after s2v_attn_steer_enable.  planes_host is [n_planes][V].  Everything is checked before anything is replaced, by name:
 * the ranges as s2v_attn_steer_set checks them, n_planes in 1..16, a plane index outside [-1, n_planes), a plane index on a sample >= B, a weight
 * that is NaN or out of bounds (the message names plane and cell).  Synchronises the device, builds the log planes and the liveness table, uploads.
 * The table is data: a later call with no more planes than the allocation holds keeps a captured step, which replays with the new maps.  A context
 * holds ONE record, scalar (s2v_attn_steer_set) or maps: setting the other kind drops the captured steps.  The table counts in s2v_device_bytes as
 * workspace while held; s2v_attn_steer_enable(0) frees it.  A later s2v_set_geometry with another V refuses by name and leaves steering off.
 * s2v_attn_steer_enable / _arm are the entries above: an armed layer runs the map kernels while the held record is maps.  Everything the scalar
 * record is refused on is refused here by the same entries. */
typedef struct s2v_attn_steer_map_range {
    int32_t k0, k1;                  /* keys [k0, k1) of every sample's Ntok */
    int8_t plane[S2V_MAX_BATCH];     /* the plane of sample b, or -1 */
} s2v_attn_steer_map_range;
/* the operator-level record: the ranges as arrays plus the query range; the planes come beside it as [n_planes][q1 - q0] */
typedef struct s2v_attn_steer_map_record {
    int32_t n, q0, q1;
    int32_t k0[4], k1[4];
    int8_t plane[4][S2V_MAX_BATCH];
    int32_t n_planes;
} s2v_attn_steer_map_record;
S2V_API int s2v_attn_steer_set_maps(s2v_ctx* ctx, int32_t n, const s2v_attn_steer_map_range* ranges_host, int32_t n_planes, const float* planes_host);
/* the mapped kernel on its own, as s2v_op_attention_steer: impl 0 attn_pp<MAP> (bf16, one workgroup per 256 query rows), impl 1 the mapped generic
 * kernel (any dtype), impl 2 attn_pp<MAP> in the persistent launch form the engine uses beyond two rounds of items, here at any size on a queue of
 * the process (bf16; the same work items, so the bits of impl 0); one table per
 * process on the first call's device and stream (another stream is refused by name); the call synchronises the stream.  B <= S2V_MAX_BATCH */
S2V_API int s2v_op_attention_steer_map(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok, int32_t dtype, int32_t impl,
                                       const s2v_attn_steer_map_record* record_host, const float* planes_host, s2v_stream stream);
/* host only: the wave liveness table of a VALID record, out[S2V_MAX_BATCH][8 * ceil(Ntok / 256)] int32, bit r of entry (b, w): range r is live on
 * the rows [32 w, 32 w + 32) of sample b.  plane is [4][S2V_MAX_BATCH], planes [.][q1 - q0] */
S2V_API int s2v_attn_steer_map_wave_flags(int32_t n, int32_t q0, int32_t q1, int32_t Ntok, const int8_t* plane, const float* planes, int32_t* out);

/* ---- Local attention in time: video rows attend a window of frames (the training-free temporal sliding window) ------------------------------------
 * ONE definition, which the kernels (csrc/attention.hip), tests/attn_local_ref.py and this comment state alike.  For sample b, head h, query row
 * i and key j of the joint attention over [text T | reference R | video V]:
 *     s_ij   = q_i . k_j / 8
 *     out_i  = sum_{j in vis(i)} softmax_{j in vis(i)}(s_ij) v_j
 *     vis(i) = [0, P)  union  [lo_i, hi_i)
 * Every sample and head uses the same P and the same row table (lo_i, hi_i), i in [0, Ntok).  Any table with 1 <= P <= Ntok and
 * P <= lo_i <= hi_i <= Ntok is taken; lo_i == hi_i is an empty window: that row sees the prefix only.  P >= 1 is required: key 0 is then visible
 * to every row, so the first key tile a work item visits holds a visible key for each of its rows, which the kernel's adoption of the first
 * tile's maximum needs.  Anything outside these bounds is refused by name.
 * The MFMA kernel (attn_pp<LOCAL>) visits, per 256-row work item, the 64-key tiles of the prefix and of the envelope of the item's windows, and
 * skips every other tile; in a visited tile it sets the scores of the keys a row does not see to -inf, before everything its softmax segment does
 * (the row-sum vote of the deferred maximum, the slow path's maximum, exp2).  A 32-row wave all of whose rows see all of a tile runs the
 * un-windowed code on it: a table whose every row sees everything returns the bits of the un-windowed attn_pp, and so do the 32 rows of a wave
 * whose rows are all dense (lo = P, hi = Ntok) inside a table that windows other waves.  The generic kernel masks before its maximum and expf.
 * Engines: a local layer of a bf16 engine runs attn_pp<LOCAL> at EVERY length (persistent under the rule of the un-windowed launch); an fp32
 * engine runs the local generic kernel -- fp32 is the parity mode and its speed is no goal.  Layers that are not local, and every call with the
 * feature off, run the launches they run without it.
 * s2v_attn_local_enable: after s2v_set_geometry; on != 0 allocates the record's device table for the geometry's Ntok (counted by s2v_device_bytes
 * as workspace while on) holding a table that windows nothing, on = 0 frees it.  Drops a captured step.
 * s2v_attn_local_set: P and two host arrays of Ntok rows, checked against the current geometry with an error that names what is wrong BEFORE
 * anything is replaced; synchronises the device and uploads.  The table is data, not a launch argument: a captured step is kept and replays with
 * the new table.  A later s2v_set_geometry with another Ntok switches the feature off (the table is one row per token).
 * s2v_attn_local_arm: the layers (bit l = block l) of the NEXT forward only (s2v_transformer_forward*, s2v_denoise_step, _videos, _masked).  An
 * armed step is another launch sequence: captured steps are kept per (step-cache mode, map mask, steer mask, local mask), and an un-armed step
 * never replays an armed executable nor the reverse.
 * Refused by name: fp16 engines; every fp8 weight format; attn_p_format 1 (fp16 V^T); shard contexts; attention-only contexts; triple-conditioned
 * contexts and s2v_denoise_step_guided; contexts with temporal windows and s2v_denoise_step_windows; s2v_denoise_split_begin (CFG-parallel); an
 * armed attention map, an armed steer or S2V_STEP_REUSE together with an armed local mask, in either order of the two arms; a layer bit at or
 * beyond num_layers; s2v_block_forward and the s2v_attn_forward* / AttnProcessor seams while a local mask is armed. */
S2V_API int s2v_attn_local_enable(s2v_ctx* ctx, int32_t on);
S2V_API int s2v_attn_local_set(s2v_ctx* ctx, int32_t P, const int32_t* rows_lo, const int32_t* rows_hi);
S2V_API int s2v_attn_local_arm(s2v_ctx* ctx, uint64_t layer_mask);
/* the local kernel on its own: qkv / vt_scratch / out as s2v_op_attention takes them.  impl 0: attn_pp<LOCAL> (bf16, any Ntok, one work item
 * per 256 query rows, persistent when the launch has more than two items per CU); impl 1: the local generic kernel (any dtype).  The record is
 * made from (P, rows_lo, rows_hi) and copied to ONE table per process on the device current at the first call; the entry synchronises `stream`
 * first and is not thread-safe -- a test and benchmark entry; contexts hold their own table.  Refused by name: a bad table (as
 * s2v_attn_local_set), impl 0 with another dtype than bf16 */
S2V_API int s2v_op_attention_local(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok, int32_t dtype, int32_t impl,
                                   int32_t P, const int32_t* rows_lo, const int32_t* rows_hi, s2v_stream stream);

/* ---- Local attention in space and time: a window of frames and of patch rows (the 3-D sliding window) ------------------------------------------
 * ONE definition, which the kernels (csrc/attention.hip), tests/attn_box_ref.py and this comment state alike.  For sample b, head h, query row i
 * and key j:
 *     s_ij   = q_i . k_j / 8
 *     out_i  = sum_{j in vis(i)} softmax_{j in vis(i)}(s_ij) v_j
 *     vis(i) = [0, P)  union  { j : lo_i <= j < hi_i  and  olo_i <= (j - P) mod S < ohi_i }
 * One P, one period S (the rows of a latent frame: inside a frame the token order is row-major, so a window of patch rows is one contiguous
 * range of offsets per frame) and one row table (lo_i, hi_i, olo_i, ohi_i), i in [0, Ntok), serve every sample and head.  Taken: 1 <= P <= Ntok,
 * P <= lo_i <= hi_i <= Ntok, 0 <= olo_i <= ohi_i <= S, 64 <= S (a 64-key tile then holds at most one frame boundary); anything else is refused
 * by name, with the row where a row is at fault.  olo = 0, ohi = S on every row is exactly the window table of "Local attention" above; an empty
 * box (lo == hi or olo == ohi) leaves the row the prefix only; key 0 stays visible to every row, as the adoption of the first tile's maximum
 * requires.
 * The MFMA kernel (attn_pp<BOX>) visits, per 256-row work item, the prefix tiles [0, ceil(P / 64)) and after them, ascending, every later 64-key
 * tile that holds a key some row of the item sees -- a list the host makes once per table (csrc/kernels.h, "local attention in space and time")
 * and the kernel maps its loop iteration through, fetching each entry an iteration ahead of its use.  A 32-row wave all of whose rows see every
 * key of a tile (a bit the host puts beside the entry) runs the un-windowed code on it; any other visited tile sets the scores of the keys a
 * lane's row does not see to -inf where "Local attention" does, before everything the softmax segment does.  A table every row of which sees
 * everything returns the bits of the un-windowed attn_pp, and so do the rows of a dense wave inside a table that boxes others; a table with full
 * offsets returns the bits of s2v_op_attention_local on the same (lo, hi).  The generic kernel masks before its maximum and skips the tiles its
 * row sees nothing of; it is what an fp32 engine runs on a box layer.
 * s2v_attn_local_set_box: beside s2v_attn_local_set, after s2v_attn_local_enable; arming is s2v_attn_local_arm.  A context holds ONE table, of
 * either kind: setting the other kind replaces it and drops the captured steps (the kernel choice is baked into them); a new table of the same
 * kind keeps them and re-captures nothing.  Checked against the current geometry with an error that names what is wrong BEFORE anything is
 * replaced; synchronises the device.  s2v_device_bytes counts the box table as workspace from the first call until the feature goes off.
 * Refused by name: everything s2v_attn_local_enable / _set / _arm refuse, on the same engines, contexts and compositions. */
S2V_API int s2v_attn_local_set_box(s2v_ctx* ctx, int32_t P, int32_t S, const int32_t* rows_lo, const int32_t* rows_hi, const int32_t* offs_lo,
                                   const int32_t* offs_hi);
/* the box kernel on its own, as s2v_op_attention_local: impl 0 attn_pp<BOX> (bf16, persistent when the launch has more than two items per CU),
 * impl 1 the generic box kernel (any dtype).  One table per process; a test and benchmark entry, not thread-safe */
S2V_API int s2v_op_attention_box(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok, int32_t dtype, int32_t impl,
                                 int32_t P, int32_t S, const int32_t* rows_lo, const int32_t* rows_hi, const int32_t* offs_lo, const int32_t* offs_hi,
                                 s2v_stream stream);

/* Live per-kernel timing for the roofline report (bench.py): HIP events are recorded on the launch stream around
 * every launch of a class; classes 0 qkv GEMM, 1 attention, 2 out-proj GEMM, 3 FF1 GEMM, 4 FF2 GEMM,
 * 5 LN-modulate, 6 qk-norm/rope/V^T, 7 the modulation GEMV, 8 the Ulysses packs, 9 the runtime-LoRA down-projections.  Not recorded inside a captured graph.  s2v_profile_read synchronises the
 * device, returns total ms and launch counts per class since the previous read, and resets the counters. */
S2V_API int s2v_profile_enable(s2v_ctx* ctx, int32_t on);
S2V_API int s2v_profile_read(s2v_ctx* ctx, float* ms_by_class, int32_t* launches_by_class, int32_t nclass);
/* Average SHADER CLOCK (MHz) under the profiled launches of every class since s2v_profile_enable(1): one designated workgroup of the
 * profiled kernel (the four-wave GEMM / attention kernels; workgroup 0 of a persistent launch, the middle one otherwise) reads s_memtime
 * (shader-clock cycles) and s_memrealtime (constant 100 MHz) at its entry and exit; clock = sum of cycle spans / sum of tick spans x 100;
 * 0 for a class whose kernels carry no stamps.  The part is power-managed (1.1-1.9 GHz under the MFMA loops against the 2.4 GHz
 * the datasheet peak assumes): this is the figure that relates a measured TFLOP/s to the matrix pipe's cycles.  Synchronises. */
S2V_API int s2v_profile_read_clocks(s2v_ctx* ctx, float* mhz_by_class, int32_t nclass);
/* Marks every tensor as loaded on a replica whose arena was filled by a broadcast of s2v_weight_arena. */
S2V_API int s2v_mark_weights_loaded(s2v_ctx* ctx);

/* ---- replicas over RCCL: one process per GPU, ONE collective -- the weight broadcast root -> all ----------
 * No reference code (the reference is single-process); replaces what a maintainer would otherwise write around
 * torch.distributed.broadcast.  RCCL is bound at first use (dlopen librccl.so.1; a process that already loaded PyTorch-ROCm's copy
 * shares it); every call fails with a message when it is absent.  Protocol: the root calls s2v_rccl_unique_id, ships the 128 bytes
 * to the other ranks by any means (a file, a socket, torch.distributed's store), every rank -- with ITS GPU current -- calls
 * s2v_rccl_comm_create, then s2v_bcast_weights / s2v_rccl_bcast on a stream of that GPU. */
typedef struct s2v_rccl_comm s2v_rccl_comm;
/* 0 when librccl and every symbol this file needs can be bound (dlopen + dlsym only: no bootstrap thread, no socket, no communicator);
 * < 0 with the reason in s2v_last_error() otherwise.  What every rank calls before the ranks agree on the native path. */
S2V_API int s2v_rccl_available(void);
S2V_API int s2v_rccl_unique_id(void* id128 /* out: 128 bytes */);
S2V_API int s2v_rccl_comm_create(const void* id128, int32_t rank, int32_t world, s2v_rccl_comm** out);
S2V_API void s2v_rccl_comm_destroy(s2v_rccl_comm* comm);
/* any device range (s2v_vae_weight_arena, s2v_t5_weight_arena ...), in place, asynchronous on `stream`, 256-MiB collectives */
S2V_API int s2v_rccl_bcast(s2v_rccl_comm* comm, void* dev_ptr, int64_t bytes, int32_t root, s2v_stream stream);
/* ncclAllGather of bytes: every rank contributes bytes_per_rank from `send`; `recv` (world x bytes_per_rank, rank order) is the same on every
 * rank afterwards; send == recv + rank * bytes_per_rank is the in-place form.  The per-step exchange of CFG-parallel below. */
S2V_API int s2v_rccl_allgather(s2v_rccl_comm* comm, const void* send, void* recv, int64_t bytes_per_rank, s2v_stream stream);
/* the transformer's finalized arena (merged LoRA, fused QKV, fp8 copies + scales) root -> all; receivers are marked loaded */
S2V_API int s2v_bcast_weights(s2v_ctx* ctx, s2v_rccl_comm* comm, int32_t root, s2v_stream stream);

/* ---- CFG-parallel: ONE video on TWO GPUs (SURVEY.md section 8e "noted for later"; round 6) -----------------------------------------
 * The CFG pair the reference batches (custom_cogvideox_pipe.py:255-265: latents duplicated, [negative | positive] embeddings, reference tokens
 * duplicated x2 at cogvideox_transformer_3d.py:503-504) is two independent forwards that meet only in the guidance formula (:266-279).  Each rank
 * of a pair sets a B = 1 geometry, s2v_set_conditioning with ITS half of the embeddings ([1,T,text_embed_dim]) and the one reference latent, and
 * runs per step:
 *   s2v_denoise_split_begin  the rank's forward into half `slot` (0 = unconditional / negative prompt, 1 = conditional) of the context's pair
 *                            buffer; use_graph != 0 replays a captured forward-only hipGraph;
 *   the exchange             s2v_rccl_allgather on s2v_cfg_pair's buffer in place (or any other transport), OUTSIDE the graph;
 *   s2v_denoise_split_end    fp32 CFG + scheduler step + round to the model dtype (:266-296) on the pair, by BOTH ranks redundantly: their latents
 *                            stay bit-identical without a second collective (DPM: the caller hands both ranks the same `noise`).
 * s2v_denoise_step_cfg_parallel is the three in one call over the library's own communicator (a 2-rank s2v_rccl_comm).  Per sample the arithmetic
 * is the B = 2 engine's: tests/test_gpu_cfg_parallel.py holds the pair to s2v_denoise_step bit for bit. */
S2V_API int s2v_denoise_split_begin(s2v_ctx* ctx, const void* latents, float timestep, const s2v_sched_coef* coef_host, int32_t slot,
                                    int32_t use_graph, s2v_stream stream);
/* the pair buffer [2][F,C,H,W] (model dtype, context-owned) and the bytes of one half */
S2V_API int s2v_cfg_pair(s2v_ctx* ctx, void** dev_ptr, int64_t* bytes_per_half);
/* one end per begin (the step's coefficients are the ones begin uploaded); x0_hist / noise as s2v_denoise_step (required for the DPM kinds) */
S2V_API int s2v_denoise_split_end(s2v_ctx* ctx, void* latents, float* x0_hist, const void* noise, s2v_stream stream);
/* comm: a communicator of exactly the pair's two ranks whose rank equals `slot` (the in-place all-gather puts rank r's bytes into half r) */
S2V_API int s2v_denoise_step_cfg_parallel(s2v_ctx* ctx, s2v_rccl_comm* comm, int32_t slot, void* latents, float timestep,
                                          const s2v_sched_coef* coef_host, float* x0_hist, const void* noise, int32_t use_graph,
                                          s2v_stream stream);

/* ---- Ulysses sequence parallelism: ONE video's step on p GPUs, attention sharded by heads -------
 * p ranks share one video's denoise step with both samples of the CFG pair (B = 2, or B = 1).  Each rank calls s2v_set_shard(p, r) BEFORE
 * s2v_set_geometry and then the usual set-up with FULL-size arguments: s2v_set_geometry(B, T, F, H, W), s2v_set_rope / s2v_set_pos_embed with the
 * whole tables, s2v_set_conditioning with the whole [B, T, text_embed_dim] embeddings; the context keeps its rank's rows.
 *   Shard geometry: every stream is split separately, rank r keeping rows [r*n/p, (r+1)*n/p) (integer division) of the text (n = T), the
 *   reference (n = R = H/2 * W/2) and the video (n = V = F * R) tokens of each sample: its mini-sequence [T_r | R_r | V_r].  Every row-wise
 *   kernel (LayerNorm-modulate, the linears and their epilogues, q/k-norm + RoPE, the tail) runs on those rows; the attention runs on heads
 *   [r*H/p, (r+1)*H/p) of all N = T + R + V tokens in global token order.  Shards are ragged (19 126 tokens at p = 4: text shards 56/57/56/57).
 *   Requirements: p divides num_heads; the fp8 weight formats (1, 2, 3) need an even number of heads per rank, (inner_dim / p) % 128 == 0 (their
 *   attention output is MX e4m3 whose block-scale dwords span one 128-column K-tile = two heads); every rank holds >= 1 video row.  p = 1 computes
 *   what s2v_denoise_step does.  fp8: the linears quantise per row as the single engine does; weight_format 3 decides fp8 QK^T on the whole
 *   sequence N, not on the rank's rows, so every rank takes the single engine's decision.
 *   A shard context runs ONLY the staged step below (s2v_denoise_step, s2v_transformer_forward, the seams and CFG-parallel are refused), eagerly:
 *   hipGraph capture is not supported for shard contexts.  Bit-identity with the single engine: split-K is never chosen on a shard (a rank's
 *   row count must not pick another reduction order); geometries on which the single engine splits K (few row tiles and K >= 2048) differ.
 * Staged step (any transport):
 *   s2v_shard_step_begin   time embedding, modulation GEMV, patchify + patch embed, layer 0 LN1, QKV (+ q/k-norm, RoPE), pack
 *                          -> *pending = S2V_SHARD_QKV_EXCHANGE;
 *   the caller exchanges   s2v_shard_buffers(kind = *pending): all-to-all-v of bytes, send + send_displs[g] (send_counts[g] bytes) to rank g,
 *                          recv + recv_displs[g] (recv_counts[g] bytes) from rank g;
 *   s2v_shard_step_resume  after QKV: unpack, V^T, attention, pack -> S2V_SHARD_O_EXCHANGE;  after O: unpack, out-projection (gate + residual),
 *                          LN2, FF, then the next layer's LN1 + QKV + pack -> S2V_SHARD_QKV_EXCHANGE, or after the last layer the tail norm
 *                          and projection of the rank's V_r rows -> S2V_SHARD_NOISE_GATHER (an all-gather: every rank sends the same
 *                          [B][ceil(V/p)][Cout] rows to every rank, counts and displacements say so);
 *   s2v_shard_step_end     unpatchify of the gathered prediction, fp32 CFG + scheduler step on every rank redundantly: all ranks end with
 *                          bit-identical latents (DPM: every rank is handed the same noise).
 * s2v_denoise_step_ulysses is the whole sequence over the library's own communicator (world = p, rank = r), the exchanges being
 * s2v_rccl_alltoallv stream-ordered on `stream`, without a host synchronisation. */
#define S2V_SHARD_QKV_EXCHANGE 1   /* QKV rows -> heads: to rank g the rank's rows of head group g ([M_r][q_g | k_g | v_g]) */
#define S2V_SHARD_O_EXCHANGE 2     /* attention output heads -> rows: to rank g its rows of this rank's head group: bf16 [M_g][D/p]; fp8 weight formats:
                                      the MX e4m3 image the out-projection reads -- bytes [M_g][D/p], then the E8M0 scales [M_g][D/(128p)] dwords
                                      (four 32-column blocks each), padded to 16 bytes: D/p + D/(32p) bytes per row */
#define S2V_SHARD_NOISE_GATHER 3   /* projected video rows [B][ceil(V/p)][Cout] to every rank */
S2V_API int s2v_set_shard(s2v_ctx* ctx, int32_t world, int32_t rank);
/* (T_r, R_r, V_r) of every rank: out[3 * p]; after s2v_set_geometry */
S2V_API int s2v_shard_layout(s2v_ctx* ctx, int32_t* out);
/* the send / recv buffers (context-owned device memory) and per-peer byte counts / displacements (arrays of p) of an exchange kind */
S2V_API int s2v_shard_buffers(s2v_ctx* ctx, int32_t kind, void** send, void** recv, int64_t* send_counts, int64_t* send_displs,
                              int64_t* recv_counts, int64_t* recv_displs);
S2V_API int s2v_shard_step_begin(s2v_ctx* ctx, const void* latents, float timestep, const s2v_sched_coef* coef_host, int32_t* pending,
                                 s2v_stream stream);
S2V_API int s2v_shard_step_resume(s2v_ctx* ctx, int32_t* pending, s2v_stream stream);
/* x0_hist / noise as s2v_denoise_step (required for the DPM kinds); s2v_last_noise_pred then holds the whole [B, F, C, H, W] prediction */
S2V_API int s2v_shard_step_end(s2v_ctx* ctx, void* latents, float* x0_hist, const void* noise, s2v_stream stream);
/* all-to-all-v of bytes over `comm` (grouped ncclSend / ncclRecv; the self part is a device copy), on `stream` */
S2V_API int s2v_rccl_alltoallv(s2v_rccl_comm* comm, const void* send, const int64_t* send_counts, const int64_t* send_displs, void* recv,
                               const int64_t* recv_counts, const int64_t* recv_displs, s2v_stream stream);
/* comm: world and rank equal to the shard's */
S2V_API int s2v_denoise_step_ulysses(s2v_ctx* ctx, s2v_rccl_comm* comm, void* latents, float timestep, const s2v_sched_coef* coef_host,
                                     float* x0_hist, const void* noise, s2v_stream stream);

/* ---- CogVideoX 3-D causal VAE decode ------------------------------------------------------------------------- */
typedef struct s2v_vae s2v_vae;
/* AutoencoderKLCogVideoX.__init__ (models/autoencoders/autoencoder_kl_cogvideox.py:1020-1052), decoder part */
typedef struct s2v_vae_config {
    int32_t latent_channels;          /* 16 */
    int32_t out_channels;             /* 3 */
    int32_t num_blocks;               /* len(block_out_channels) = 4 */
    int32_t block_out_channels[8];    /* (128, 256, 256, 512): encoder order, the decoder walks it reversed */
    int32_t layers_per_block;         /* 3 */
    int32_t norm_num_groups;          /* 32 */
    int32_t temporal_compression_ratio; /* 4 */
    int32_t sample_height, sample_width; /* 480, 720: only used for the tile geometry */
    int32_t dtype;                    /* S2V_DTYPE_* */
    int32_t force_simple;             /* 1 = generic kernels only (cross-check) */
    float scaling_factor;             /* 1.15258426 (2B) / 0.7 (5B) */
    float norm_eps;                   /* 1e-6 */
    int32_t reserved[4];
} s2v_vae_config;

S2V_API int s2v_vae_create(const s2v_vae_config* cfg, s2v_vae** out);
S2V_API void s2v_vae_destroy(s2v_vae* vae);
/* name = the reference's state-dict key ("decoder.conv_in.conv.weight", "decoder.up_blocks.1.resnets.0.conv_shortcut.
 * weight", "decoder.mid_block.resnets.0.norm1.conv_y.conv.bias", ...); conv weights are re-packed to
 * [cout][(dt,dy,dx)][cin] for the channels-last implicit GEMM. */
S2V_API int s2v_vae_load_weight(s2v_vae* vae, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim,
                        int32_t src_dtype, s2v_stream stream);
S2V_API int s2v_vae_finalize(s2v_vae* vae);
/* Replicas ("11.14 GB transformer + 0.25 GB VAE decoder" are broadcast rank0 -> all): every weight of
 * a handle (decoder, or encoder for an s2v_vae_enc_create handle) lives in ONE device range; the receiving rank copies into
 * it and calls s2v_vae_mark_weights_loaded instead of s2v_vae_load_weight + s2v_vae_finalize.  Stands where the reference
 * would call .to(device) on every rank after from_pretrained (src/inference.py:191-215). */
S2V_API int s2v_vae_weight_arena(s2v_vae* vae, void** dev_ptr, int64_t* bytes);
S2V_API int s2v_vae_mark_weights_loaded(s2v_vae* vae);
/* workspace sets (= tiles in flight) and bytes per set that the last tiled decode ran with: the count follows the free HBM
 * and a byte cap of a quarter of the device's memory (S2V_VAE_WORKSPACE_MAX_GB overrides, <= 0 lifts it); at most six
 * (S2V_VAE_TILES_IN_FLIGHT overrides); for reporting */
S2V_API int s2v_vae_workspace_info(s2v_vae* vae, int32_t* sets, int64_t* bytes_per_set);
/* output extent of s2v_vae_decode for latents [1,F,C,h,w] */
S2V_API int s2v_vae_out_shape(s2v_vae* vae, int32_t F, int32_t h, int32_t w, int32_t tiling, int32_t* Fo, int32_t* Ho, int32_t* Wo);
/* CogVideoXPipeline.decode_latents (pipeline_cogvideox.py:346-351) = 1/scaling_factor * latents, then
 * AutoencoderKLCogVideoX.decode (:1259-1282): frame batches (3,2,2,...) with conv_cache, GroupNorm statistics per
 * frame batch (and per tile when tiling != 0: tiled_decode :1374-1455 incl. its raster-order in-place blends).
 * latents [1,F,C,h,w] model dtype (the pipeline's layout); scaled != 0: pipeline latents (multiplied by
 * 1/scaling_factor here), scaled == 0: already z = latents/scaling_factor (the argument of vae.decode);
 * out [1,out_channels,Fo,Ho,Wo] model dtype.
 * Buffers are (re)allocated when a larger geometry is seen for the first time, never otherwise. */
S2V_API int s2v_vae_decode(s2v_vae* vae, const void* latents, int32_t F, int32_t h, int32_t w, int32_t tiling, int32_t scaled,
                   void* out, s2v_stream stream);
/* VideoProcessor.postprocess_video(output_type="np") (video_processor.py:89-113, image_processor.py:227-240):
 * video [C,F,H,W] -> float32 [F,H,W,C], clamp(x/2 + 0.5, 0, 1) */
S2V_API int s2v_vae_postprocess(const void* video, int32_t C, int32_t F, int32_t H, int32_t W, float* out, int32_t dtype,
                        s2v_stream stream);
/* the same followed by export_to_video's frame conversion `(frame * 255).astype(np.uint8)` (utils/export_utils.py:175;
 * src/video_generate.py:65-66): video [C,F,H,W] -> uint8 [F,H,W,C], what the mp4 writer consumes (4x less D2H traffic) */
S2V_API int s2v_vae_postprocess_u8(const void* video, int32_t C, int32_t F, int32_t H, int32_t W, uint8_t* out, int32_t dtype,
                           s2v_stream stream);
/* Paste-back of masked video-to-video: s2v_vae_postprocess / s2v_vae_postprocess_u8 as a select per frame and pixel, for all C channels: of
 * `video` (the decoded video, `dtype`) where pixel_mask uint8 [F,H,W] (0 / 1: s2v_mask_to_latent's pixel_mask) is 1, of `keep` (the input video
 * [C,F,H,W], its own keep_dtype) where it is 0.  A kept pixel is exactly what the unmasked entry makes of the input video. */
S2V_API int s2v_vae_postprocess_masked(const void* video, const void* keep, int32_t keep_dtype, const uint8_t* pixel_mask, int32_t C, int32_t F,
                               int32_t H, int32_t W, float* out, int32_t dtype, s2v_stream stream);
S2V_API int s2v_vae_postprocess_u8_masked(const void* video, const void* keep, int32_t keep_dtype, const uint8_t* pixel_mask, int32_t C, int32_t F,
                                  int32_t H, int32_t W, uint8_t* out, int32_t dtype, s2v_stream stream);

/* ---- reference-image encode (the step in front of the denoise loop) ------------------------------------------
 * Replaces pipe.vae.encode(ref_image).latent_dist.sample() of src/video_generate.py:35-37
 * (AutoencoderKLCogVideoX.encode / _encode / tiled_encode, autoencoder_kl_cogvideox.py:1177-1229,1300-1372;
 * CogVideoXEncoder3D :755-814; CogVideoXDownsample3D downsampling.py:322-353; DiagonalGaussianDistribution
 * autoencoders/vae.py:767-790).  ONE frame here; s2v_vae_encode_video below takes a video.
 * s2v_vae_enc_create builds an s2v_vae handle that holds the ENCODER; its weights are loaded with s2v_vae_load_weight
 * under the reference's "encoder.*" state-dict keys, then s2v_vae_finalize; s2v_vae_destroy frees it.
 * cfg: same struct as the decoder (out_channels = image channels 3, latent_channels = 16). */
S2V_API int s2v_vae_enc_create(const s2v_vae_config* cfg, s2v_vae** out);
/* latent extent of s2v_vae_encode for an H x W image */
S2V_API int s2v_vae_encode_shape(s2v_vae* enc, int32_t H, int32_t W, int32_t tiling, int32_t* h, int32_t* w);
/* image [3,1,H,W] (model dtype, values in [-1,1]) -> moments [2*latent_channels,1,h,w] = the `parameters` of the
 * reference's DiagonalGaussianDistribution (mean | logvar); tiling != 0 follows tiled_encode when the image exceeds
 * (sample_height/2, sample_width/2). */
S2V_API int s2v_vae_encode(s2v_vae* enc, const void* image, int32_t H, int32_t W, int32_t tiling, void* moments, s2v_stream stream);
/* video encode (AutoencoderKLCogVideoX._encode / tiled_encode for more than one frame, the input of video-to-video,
 * pipeline_cogvideox_video2video.py:345-398): video [3,F,H,W] (model dtype, [-1,1]) -> moments [2*latent_channels,Fl,h,w],
 * Fl = (F - 1) / 4 + 1.  F = 1 or 8k + 1; other frame counts are refused.  Frame batches of 8 + F % 8, then 8, frames with the
 * causal convolutions' caches threaded through them; with tiling every spatial tile runs its own batches over all frames and the
 * latent-space blends apply to every latent frame.  F = 1 gives the bits of s2v_vae_encode. */
S2V_API int s2v_vae_encode_video_shape(s2v_vae* enc, int32_t F, int32_t H, int32_t W, int32_t tiling, int32_t* Fl, int32_t* h, int32_t* w);
S2V_API int s2v_vae_encode_video(s2v_vae* enc, const void* video, int32_t F, int32_t H, int32_t W, int32_t tiling, void* moments,
                                 s2v_stream stream);
/* DiagonalGaussianDistribution.sample with the caller's randn: out[c,i] = mean + exp(0.5 * clamp(logvar, -30, 20)) * noise,
 * every operation rounded to `dtype` like the reference's tensor ops; moments [2*C, n_spatial], noise / out [C, n_spatial] */
S2V_API int s2v_vae_gaussian_sample(const void* moments, const void* noise, int32_t latent_channels, int64_t n_spatial, void* out,
                            int32_t dtype, s2v_stream stream);

/* ---- prompt embeddings: T5 v1.1 encoder (the other caller-side step in front of the denoise loop) ----------------
 * Replaces `self.text_encoder(text_input_ids.to(device))[0]` of pipelines/cogvideo/pipeline_cogvideox.py:227 for the
 * T5EncoderModel src/inference.py:183-187 loads.  The arithmetic is transformers' models/t5/modeling_t5.py (third party,
 * not in the reference tree; pinned by tests/golden/t5_tiny.npz): T5LayerNorm, T5Attention (no scaling, relative-position
 * bias of block 0 added to every block's scores, softmax in fp32), T5DenseGatedActDense (gelu_new), no attention mask.
 * Weight names are the HF state-dict keys ("shared.weight", "encoder.block.3.layer.0.SelfAttention.q.weight",
 * "encoder.block.3.layer.1.DenseReluDense.wi_0.weight", "encoder.final_layer_norm.weight", ...). */
typedef struct s2v_t5 s2v_t5;
typedef struct s2v_t5_config {
    int32_t vocab_size;                        /* 32128 (+ added special tokens, src/inference.py:180-189) */
    int32_t d_model, d_kv, num_heads, d_ff;    /* 4096, 64, 64, 10240 */
    int32_t num_layers;                        /* 24 */
    int32_t relative_attention_num_buckets;    /* 32 */
    int32_t relative_attention_max_distance;   /* 128 */
    int32_t dtype;                             /* S2V_DTYPE_* */
    int32_t force_simple;                      /* 1 = generic kernels only (cross-check) */
    float layer_norm_epsilon;                  /* 1e-6 */
    int32_t reserved[5];
} s2v_t5_config;
S2V_API int s2v_t5_create(const s2v_t5_config* cfg, s2v_t5** out);
S2V_API void s2v_t5_destroy(s2v_t5* t5);
S2V_API int s2v_t5_load_weight(s2v_t5* t5, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim,
                       int32_t src_dtype, s2v_stream stream);
S2V_API int s2v_t5_finalize(s2v_t5* t5);
/* the same replica hand-off for the text encoder (9.4 GB in bf16) */
S2V_API int s2v_t5_weight_arena(s2v_t5* t5, void** dev_ptr, int64_t* bytes);
S2V_API int s2v_t5_mark_weights_loaded(s2v_t5* t5);
/* device address of the loaded block-0 relative_attention_bias table [num_buckets, num_heads] (model dtype) */
S2V_API int s2v_t5_rel_table(s2v_t5* t5, void** dev_ptr);
/* position_bias [num_heads, T, T] (model dtype) = T5Attention.compute_bias(T, T) of block 0, gathered by the host from
 * s2v_t5_rel_table with the implementation's own bucket function; sizes the workspace for (B, T) */
S2V_API int s2v_t5_set_position_bias(s2v_t5* t5, const void* bias_dev, int32_t B, int32_t T, s2v_stream stream);
/* input_ids int64 [B, T] -> last_hidden_state [B, T, d_model] (model dtype) */
S2V_API int s2v_t5_encode(s2v_t5* t5, const int64_t* input_ids_dev, int32_t B, int32_t T, void* out, s2v_stream stream);

/* the step cache's streaming kernels on their own (tools/step_cache_bench.py): sample b's n contiguous elements at x + b * x_bstride (elements)
 * against the dense cache [B][n]; op 0: cache = x; 1: cache = rnd(float(x) - float(cache)); 2: x = rnd(float(x) + float(cache)).  n, x_bstride
 * and the pointers in whole 16-byte vectors */
S2V_API int s2v_op_step_cache(int32_t op, void* x, int64_t x_bstride, void* cache, int32_t B, int64_t n, int32_t dtype, s2v_stream stream);
/* the temporal-window blend kernel on its own (one launch of s2v_denoise_step_windows): noise_pred [negative x wb | positive x wb] of [F][chw]
 * each in `dtype`, the forward's output on windows k0 .. k0 + wb - 1; acc fp32 [L][chw]; weights [F] and wsum [L] fp32 in DEVICE memory.  A
 * frame first covered by a window of this batch starts from +0 (its cell is not read); a frame last covered by one leaves divided by wsum */
S2V_API int s2v_op_window_blend(const void* noise_pred, float* acc, const float* weights, const float* wsum, float guidance, int32_t L, int32_t F,
                                int32_t stride, int32_t k0, int32_t wb, int32_t chw, int32_t dtype, s2v_stream stream);
/* the guidance rescale's statistics and finalize kernels on their own (two launches of an armed step, no log): noise_pred the planes of nvid
 * videos of n_vid elements each, [2, nvid n_vid] or [3, nvid n_vid], with `flags` as s2v_sched_step takes them (bit0 the pair, bit3 the triple --
 * exactly one of them; bit1 fp32 planes); guidance / guidance_subject (NULL for a pair) / phi: HOST arrays of nvid values.  Returns, on the HOST
 * and after synchronising `stream`, sums [nvid][4] fp64 (Sf, Sff, Sv, Svv) and factors [nvid] fp32 as the definition above states them.  The
 * scratch it needs is allocated and freed inside the call */
S2V_API int s2v_op_cfg_stats(const void* noise_pred, int32_t flags, int32_t nvid, int64_t n_vid, const float* guidance, const float* guidance_subject,
                             const float* phi, double* sums, float* factors, int32_t dtype, s2v_stream stream);
/* the attention-mass kernel on its own: qkv [B * Ntok][3 * H * 64] (q | k | v as s2v_op_attention takes them, 16-byte aligned; nothing past row
 * B * Ntok - 1 is read), query rows [q0, q0 + nq) of every sample, ranges_host n pairs (k0, k1) -> out [n][B][H][nq] fp32; accumulate != 0: out + mass
 * in one fp32 add.  An empty range gives exactly 0.  impl 0: v_mfma_f32_32x32x16 on bf16 / fp16 storage, q * 0.125 * log2 e rounded to the
 * storage type, exp2, v_rcp_f32; impl 1: the VALU on any dtype, q * 0.125, expf, a division.  Refused by name: n outside 1..4, a range outside
 * [0, Ntok] or with k1 < k0, q0 + nq > Ntok, impl 0 with fp32 */
S2V_API int s2v_op_attn_mass(const void* qkv, int32_t B, int32_t H, int32_t Ntok, int32_t q0, int32_t nq, const int32_t* ranges_host, int32_t n,
                     float* out, int32_t accumulate, int32_t dtype, int32_t impl, s2v_stream stream);
/* the head mean of s2v_attn_map_read on caller-owned sums: acc [n][B][H][nq] -> out [n][B][nq] = (sum over h = 0 .. H-1 in that order) * (1.0f / (H * count)) */
S2V_API int s2v_op_attn_mass_mean(const float* acc, int32_t n, int32_t B, int32_t H, int32_t nq, int64_t count, float* out, s2v_stream stream);

/* ---- operator-level entry points (used by the parity tests and micro-benchmarks) ------------------------- */
/* C[M,N] = A[M,K] . W[N,K]^T + bias, epilogue 0 = bias, 1 = bias + GELU(tanh); impl 0 = MFMA bf16, 1 = generic (VALU),
 * 3 = fp32 operands on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32; what the fp32 engine runs, bit-identical to impl 1; the launcher picks the
 *     tile; 30 .. 33 force 128 x 128 / 128 x 64 / 64 x 128 / 64 x 64, all with the same bits),
 * 4 = fp16 operands on v_mfma_f32_32x32x16_f16 (what the fp16 engine runs; M, N multiples of 128),
 * 2 = MFMA bf16 with K split over several workgroups per output tile, as the engine runs GEMMs with few tiles and a long
 * reduction (M, N multiples of 256; fails if the shape does not qualify; allocates its workspace, synchronous) */
S2V_API int s2v_op_linear(const void* A, const void* W, const void* bias, void* C, int32_t M, int32_t N, int32_t K,
                  int32_t epilogue, int32_t dtype, int32_t impl, s2v_stream stream);
/* One linear as a context runs it (api.hip linear()): the kernel plan of gemm.hip at this device's CU count -- split K, tile, the partial last
 * 256-row tile as a tail launch -- on the caller's operands, bf16 or fp16.  A [M rounded up to 256][lda] and W [N rounded up to 256][ldw]: the pad
 * rows are READ (any finite values; they reach no element m < M, n < N), K a multiple of 64, lda / ldw multiples of 8.  epilogue 0 = bias,
 * 1 = bias + GELU(tanh): C [M][ldc] out;  2 = gate + residual: C [M][ldc] is the residual, updated in place as C + rnd(gate * rnd(acc + bias)) with
 * the gate of row m taken from sample b = m / tok_per_batch, r = m % tok_per_batch: gate_txt for r < text_len, gate_ref (may be null: gate_vid)
 * for r < text_len + ref_len, gate_vid otherwise, each at + b * gate_stride elements;  3 = residual add: C = rnd(rnd(acc + bias) + R[m][n]), R
 * rows ldr apart.  tile 0 = the plan's choice, 1 / 2 force 256 x 128 / 128 x 128 tiles (GemmArgs::tile).  sk_tiles > 0 (bf16): a split-K workspace
 * of that many partial tiles is allocated and the plan may split K as it does in a context whose geometry carved one; the launch then runs twice
 * (epilogue 2: once) and fails unless every arrival counter is zero afterwards; synchronous.  tests/test_gpu_gemm_exact.py. */
S2V_API int s2v_op_linear_planned(const void* A, int32_t lda, const void* W, int32_t ldw, const void* bias, void* C, int32_t ldc, int32_t M, int32_t N,
                                  int32_t K, int32_t epilogue, int32_t dtype, const void* gate_txt, const void* gate_ref, const void* gate_vid,
                                  int32_t gate_stride, int32_t tok_per_batch, int32_t text_len, int32_t ref_len, const void* R, int32_t ldr,
                                  int32_t tile, int64_t sk_tiles, s2v_stream stream);
/* One adapted linear as the runtime adapter mode computes it (s2v_lora_attach): y = epilogue([x | T] . [W | rnd(scale * B)]^T + bias) with
 * T = rnd(x . A^T) from the down-projection kernel -- the attach-time packing, the down-projection and the K-extended GEMM that a context's
 * linear would launch for this shape, on the caller's operands.  x [M, K], W [N, K], bias [N] in `dtype` (bf16 or fp16); A [rank, K], B [N, rank]
 * fp32; K a multiple of 64, rank <= 128.  epilogue 0 = bias, 1 = bias + GELU(tanh): C [M, N] out;  2 = gate + residual: C is the residual
 * [M, N], updated in place as C + gate * (acc + bias) with every product and sum rounded as the block does, aux0 = gate [N];  4 = the fused
 * q/k-norm without rotary embedding: N = 3 * qk_D, per-head LayerNorm(64, eps 1e-6) on columns < 2 N / 3, aux0 = LayerNorm weights [2][64]
 * (q, k), aux1 = biases [2][64].  Allocates its scratch, synchronous.  tests/test_gpu_lora_runtime.py holds its error against fp64 to the error
 * of PEFT's Linear.forward evaluated in the same dtype. */
S2V_API int s2v_op_linear_lora(const void* x, const void* W, const void* bias, const float* A, const float* B, int32_t rank, float scale, void* C,
                               int32_t M, int32_t N, int32_t K, int32_t epilogue, const void* aux0, const void* aux1, int32_t dtype, s2v_stream stream);
/* qkv [B*Ntok (+64 rows of slack), 3*H*64] -> out [B*Ntok, H*64]; impl 0 = MFMA flash kernel (needs vt scratch
 * [B*H*64*ceil64(Ntok)] bf16, zero-filled by the caller), 1 = generic */
/* W8A8 linear on the fp8 matrix cores (BASELINE configs[4]: "fp8 (CDNA4 fp8 MFMA) weights"): A [M,K] and W [N,K] bf16 are
 * quantised per row to OCP e4m3 with fp32 scales amax/448 (per token / per output channel) into `scratch`
 * (>= M*K + N*K + 4*(M+N) bytes), multiplied with v_mfma_scale_f32_32x32x64_f8f6f4 and de-quantised in the epilogue:
 * C = epilogue(scale_a[m] * scale_w[n] * acc + bias), bf16.  The reference has no fp8 path (diffusers quantizers are
 * bitsandbytes-only): the contract is stated against this library's own bf16 path (tests/test_gpu_fp8.py).
 * M, N multiples of 256, K a multiple of 128; epilogue 0 = bias, 1 = bias + GELU(tanh). */
S2V_API int s2v_op_linear_fp8(const void* A, const void* W, const void* bias, void* C, int32_t M, int32_t N, int32_t K,
                              int32_t epilogue, void* scratch, int64_t scratch_bytes, s2v_stream stream);
/* FeedForward (attention.py:1237-1243: Linear D -> F, GELU(tanh), Linear F -> D) on the fp8 matrix cores as the fp8 engine runs it:
 * x [M, D], W1 [F, D], W2 [D, F] bf16, quantised per row to e4m3; mx = 1: GELU(h) leaves the first GEMM's epilogue as MX e4m3 (one
 * power-of-two scale per 32 columns, the block scales v_mfma_scale_f32_32x32x64_f8f6f4 takes per lane) and the second GEMM reads it
 * in place; mx = 0: bf16 h + a per-row quantisation pass.  M, D, F multiples of 256; allocates its scratch, synchronous.  No
 * reference arithmetic exists for fp8 (parity unpinned): tests/test_gpu_fp8.py states the contract against a torch emulation. */
S2V_API int s2v_op_ff_fp8(const void* x, const void* w1, const void* b1, const void* w2, const void* b2, void* out, int32_t M,
                          int32_t D, int32_t F, int32_t mx, s2v_stream stream);
/* One adapted linear as an fp8 context created with S2V_LORA_FP8_BRANCH computes it: s2v_op_linear_fp8 (same operands, quantisation, shapes and
 * epilogues) with the adapter branch beside it, C = epilogue(scale_a[m] * scale_w[n] * acc + T . rnd(scale * B)^T + bias), T = rnd(x . A^T) from
 * the bf16 rows of x.  A [rank, K], B [N, rank] fp32, rank <= 128.  scratch >= M*K + N*K + 4*(M+N) rounded up to 256, + 2*R*(K+N+M) bytes with
 * R = rank rounded up to 64.  scale = 0 or B = 0 returns the bytes of s2v_op_linear_fp8.  tests/test_gpu_lora_runtime_fp8.py. */
S2V_API int s2v_op_linear_fp8_lora(const void* x, const void* W, const void* bias, const float* A, const float* B, int32_t rank, float scale, void* C,
                                   int32_t M, int32_t N, int32_t K, int32_t epilogue, void* scratch, int64_t scratch_bytes, s2v_stream stream);
/* s2v_op_ff_fp8 with an adapter (A1 [rank, D], B1 [F, rank]; A2 [rank, F], B2 [D, rank]; fp32, one scale) on both linears.  FF1's branch reads
 * the bf16 rows of x; FF2's reads, mx = 1, the MX image of GELU(h) dequantised exactly, or, mx = 0, the bf16 h.  The caller's scratch
 * (4*M*F + M*D + 2*D*F + 2*R*(2*M + 2*D + 2*F) + 8*M + 4*(D + F) + 8192 bytes suffice) starts with the image bytes [M][F], then its block scales
 * [F / 128][M] dwords (dword (kt, m) at row (m & ~127) | (m & 31) << 2 | (m >> 5) & 3, byte b = the E8M0 scale of columns 128 kt + 32 b ..),
 * then, at the next multiple of 256 bytes, FF2's T [M][R] bf16 (R = rank rounded up to 64, pad columns zero).  Asynchronous. */
S2V_API int s2v_op_ff_fp8_lora(const void* x, const void* w1, const void* b1, const void* w2, const void* b2, const float* A1, const float* B1,
                               const float* A2, const float* B2, int32_t rank, float scale, void* out, int32_t M, int32_t D, int32_t F, int32_t mx,
                               void* scratch, int64_t scratch_bytes, s2v_stream stream);
/* out[b][r] = silu(emb[b]) . W[r] + bias[r] for the stacked AdaLN modulation linears of a step (every
 * CogVideoXLayerNormZero.linear and norm_out.linear on silu(temb), normalization.py / cogvideox_transformer_3d.py:122-186);
 * emb [B, temb_dim], W [rows, temb_dim], out [B, rows], B <= 4; impl 0 = the product dispatch, 1 = one wave per row */
S2V_API int s2v_op_mod_gemv(const void* emb, const void* W, const void* bias, void* out, int32_t B, int32_t temb_dim,
                            int64_t rows, int32_t dtype, int32_t impl, s2v_stream stream);
/* The HBM-bound row kernels between the GEMMs and the attention, one launch each as a context issues it (tests/test_gpu_norm_exact.py holds
 * them to expected bits).  Row pitches and mod_stride are in elements, cover D and keep every row 16-byte aligned; asynchronous.
 * s2v_op_ln_modulate (CogVideoXLayerNormZero): y[r] = rnd(rnd(LN(x[r]; w, b, eps) * rnd(1 + scale)) + shift) on rows [B * Ntok][D], D <= 4096 and
 * a multiple of 8; row r of sample b takes (shift, scale)_txt[b] for r < text_len, _ref[b] for the next ref_len rows when that set is given
 * (null: they are video rows), _vid[b] otherwise; the sets are [B][mod_stride].  q8 (bf16 only): the row leaves as e4m3 bytes [row][D] with
 * q8_scale[row] = amax / 448 (1 for a zero row) instead of y; q8_keep_y: y is written as well. */
S2V_API int s2v_op_ln_modulate(const void* x, int32_t ldx, void* y, int32_t ldy, const void* w, const void* b, float eps, const void* shift_vid,
                               const void* scale_vid, const void* shift_txt, const void* scale_txt, const void* shift_ref, const void* scale_ref,
                               int32_t mod_stride, int32_t B, int32_t Ntok, int32_t text_len, int32_t ref_len, int32_t D, void* q8, float* q8_scale,
                               int32_t q8_keep_y, int32_t dtype, s2v_stream stream);
/* norm_final then norm_out on the video rows: y[b * V + i] = rnd(rnd(LN(LN(x[b * Ntok + row0 + i]; w1, b1); w2, b2) * rnd(1 + scale[b])) + shift[b]),
 * i < V, row0 + V <= Ntok; shift / scale [B][mod_stride] */
S2V_API int s2v_op_tail_norm(const void* x, int32_t ldx, void* y, int32_t ldy, const void* w1, const void* b1, const void* w2, const void* b2,
                             float eps, const void* shift, const void* scale, int32_t mod_stride, int32_t B, int32_t Ntok, int32_t row0, int32_t V,
                             int32_t D, int32_t dtype, s2v_stream stream);
/* Per-head LayerNorm(64) of the q and k thirds of qkv [B * Ntok][ld_qkv] in place (columns < 2 * H * 64; weights and biases [64]), then on rows
 * r >= text_len of a sample the rotation of the pairs (2 i, 2 i + 1): (x0 cos[2i] - x1 sin[2i], x1 cos[2i+1] + x0 sin[2i+1]) with the fp32 tables
 * cos / sin [Ntok - text_len][64] (both null: no rotation).  The v third is not touched and no V^T is produced. */
S2V_API int s2v_op_qk_norm_rope(void* qkv, int32_t ld_qkv, int32_t B, int32_t H, int32_t Ntok, int32_t text_len, const void* nq_w, const void* nq_b,
                                const void* nk_w, const void* nk_b, float eps, const float* cos_tab, const float* sin_tab, int32_t dtype,
                                s2v_stream stream);
/* The v third of bf16 qkv [B * Ntok][ld_qkv] (columns 2 * H * 64 + h * 64 + d) -> vt [B][H][64][ntok_pad], token order [0-3, 8-11, 4-7, 12-15] inside
 * every 16 tokens, zeros from Ntok up to the next multiple of 64 -- positions beyond that multiple are NOT written (ntok_pad is that multiple in
 * every launch of a context).  vt_amax ([B * H] words): V^T as fp16, each (batch, head) times the power of two that puts its largest magnitude
 * into [2^14, 2^15); the word receives the bf16 bits of that magnitude; a head holding Inf / NaN is not scaled and Inf saturates to 65504. */
S2V_API int s2v_op_v_transpose(const void* qkv, int32_t ld_qkv, int32_t B, int32_t H, int32_t Ntok, void* vt, int32_t ntok_pad, uint32_t* vt_amax,
                               s2v_stream stream);
/* Census of the deferred-maximum slow path of the four-wave attention kernels since the last reset (device counters; the call synchronises):
 * slow = slow paths taken, total = (wave, KV tile) pairs run.  attn_p_format 1 lowers the threshold from 2^64 to 2^14; a caller whose data
 * take the slow path in more than a fraction of a percent of the pairs switches back with s2v_set_attn_p_format (the engine's "auto"
 * policy, engine.py, does that after the first step).  s2v_set_attn_p_format drops a captured step; it is re-captured at its next use. */
S2V_API int s2v_attn_slow_stats(s2v_ctx* ctx, uint64_t* slow, uint64_t* total, int32_t reset);
S2V_API int s2v_set_attn_p_format(s2v_ctx* ctx, int32_t attn_p_format);
S2V_API int s2v_op_attention(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok, int32_t dtype,
                     int32_t impl, s2v_stream stream);   /* impl: 0 product dispatch (bf16), 1 generic (VALU), 3 = 0 with attn_p_format 1, 4 = attn_q4h (fp16 P) at any length, 5 = fp32 / fp16 storage on the fp32 matrix pipe (what the fp32 engine runs), 6 = fp16 on v_mfma_f32_32x32x16_f16 (what the fp16 engine runs; vt scratch as impl 0).
                                                          * impl 3 / 4 keep the per-(batch, head) magnitude words of the fp16 V^T in ONE buffer per process, allocated on the
                                                          * device current at the first such call and never freed: such calls must stay on that device and be ordered
                                                          * against one another (one stream, or events); B * H <= 4096.  Contexts hold their own words. */
/* The same joint attention (F.scaled_dot_product_attention at attention_processor.py:2083-2087, head_dim 64, scale 1/8) as weight_format 2
 * runs it: q (times scale * log2 e) and k of the bf16 qkv rows [B*Ntok, 3*H*64] are quantised to MX e4m3 (32-element blocks along the
 * head dimension, E8M0 scales) into `scratch` and QK^T runs on v_mfma_scale_f32_32x32x64_f8f6f4; V^T (vt_scratch: B*H*64*rup(Ntok,64)
 * bf16), softmax and P.V as s2v_op_attention impl 0.  scratch >= B*H*(66*Ntok + 68*rup(Ntok,64)) + 1024 bytes; it holds, 256-byte
 * aligned and in this order, q8 [B][H][Ntok][64], q8s [B][H][Ntok][2], k8 [B][H][Npad][64], k8s [B][H][Npad/64][64] dwords (byte kb of
 * dword hi*32+r = scale of (key 32*kb+r, block hi)).  No reference arithmetic exists for fp8 (parity unpinned). */
S2V_API int s2v_op_attention_fp8qk(const void* qkv, void* vt_scratch, void* scratch, int64_t scratch_bytes, void* out, int32_t B,
                                   int32_t H, int32_t Ntok, s2v_stream stream);
/* The same with P and V^T in fp16 (attn_p_format 1 under weight_format 2): vt_scratch then holds fp16, each (batch, head) times a power of two
 * taken from its largest |V| (the kernel divides it out again); scratch >= the size above + 256 + 4*B*H bytes (the magnitude words follow the
 * images, 256-byte aligned). */
S2V_API int s2v_op_attention_fp8qk_p16(const void* qkv, void* vt_scratch, void* scratch, int64_t scratch_bytes, void* out, int32_t B,
                                       int32_t H, int32_t Ntok, s2v_stream stream);

#ifdef __cplusplus
}
#endif
#endif
