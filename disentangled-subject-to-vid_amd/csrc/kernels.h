// Internal launcher declarations (host side). Every launcher enqueues on `st` and returns 0 / <0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { S2V_F32 = 0, S2V_BF16 = 1, S2V_F16 = 2 };
// T = the storage type of `dtype`
#define S2V_DT_DISPATCH(dtype, ...)                                        \
    switch (dtype) {                                                       \
        case S2V_BF16: { using T = bf16_t; __VA_ARGS__; } break;           \
        case S2V_F16: { using T = f16_t; __VA_ARGS__; } break;             \
        default: { using T = float; __VA_ARGS__; } break;                  \
    }
enum { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_GATE_RES = 2 };

// C[m][n] = sum_k A[m][k] * W[n][k] (+ bias[n]) followed by an epilogue.
//   EPI_BIAS          : C = rnd(acc + bias)
//   EPI_BIAS_GELU     : C = rnd(gelu_tanh(rnd(acc + bias)))
//   EPI_BIAS_GATE_RES : X[m][n] = rnd(X[m][n] + rnd(gate(m)[n] * rnd(acc + bias)))   (C unused)
// gate(m): row m belongs to sample b = m / tok_per_batch; rows with (m % tok_per_batch) < text_len use
// gate_txt[b], the others (reference-image + video tokens) gate_vid[b]
// (reference: cogvideox_transformer_3d.py:165-167,182-184; normalization.py:484).
struct GemmArgs {
    const void* A; int lda;
    const void* W; int ldw;   // W is [N_pad, K], nn.Linear layout
    const void* bias;         // [N] or null
    void* C; int ldc;
    int M, N, K;
    void* X; int ldx;
    const void* gate_vid; const void* gate_txt; int gate_stride;
    int tok_per_batch; int text_len;
    // optional third gate for the reference-image rows [text_len, text_len + ref_len) of every sample (null: they take gate_vid,
    // which is what the shipped reference computes; set under lora_adaln_scope = 1, normalization.py:468-478)
    const void* gate_ref; int ref_len;
    // EPI_BIAS_ADD: C = rnd(rnd(acc + bias) + R[m][n])  (resnet skip, autoencoder_kl_cogvideox.py:318)
    const void* R; int ldr;
    // Implicit-GEMM convolution addressing of A (conv != 0).  A is a zero-bordered channels-last tensor
    // [frames][Hp][Wp][cin]; output row m = (f, y, x) of an [F][oH][oW] grid; k = (tap, ci) with tap = (dt, dy, dx),
    // dt in [0,kt), dy,dx in [0,3): A[m][k] = in[f + dt][y + dy][x + dx][ci].  kt = 3: causal conv (frames 0,1 of the
    // buffer hold the conv cache); kt = 1: per-frame 3x3 conv.  (CogVideoXCausalConv3d, autoencoder_kl_cogvideox.py:120-137)
    int conv, cin, Hp, Wp, oH, oW, kt;
    int cstride;        // conv mode: spatial stride of the output grid (0 or 1 = dense; 2 = CogVideoXDownsample3D, downsampling.py:322-353)
    int gm;             // 256-row kernel: row tiles per group of the tile order (0: chosen by the launcher)
    int tile;           // plain bf16 GEMMs: 0 = the launcher's choice (256 x 256 tiles where the shape fits them); 1 = 256 x 128 tiles, 2 = 128 x 128
                        // (few-tile GEMMs: more, smaller workgroups fill the CUs that a single partial round of 256 x 256 tiles leaves idle)
    int ablate;         // diagnostics only
    long long* clk;     // profile pass only: shader-clock stamp slot (common.h clk_stamp; gemm_g4 / g4t / g4f), else null
    int f16;            // launch_gemm_bf16: the 16-bit operands are fp16, not bf16 (set by launch_gemm_f16)
    int valu_only;      // fp32 only: stay on the VALU kernel gemm_simple_k (cfg.force_simple; the A/B reference of gemm_f32m, which returns the same bits)
    int a_rows_padded;  // plain mode: rows physically present behind A (>= M); the 256-row kernel needs ceil256(M)
    int m_begin;        // first output row of this launch (row-tail launches of a split GEMM; 128-row kernel only)
    int w_rows_padded;  // rows physically present behind W (>= N, zero or don't-care beyond N); 0 = exactly N
    // fp8 (OCP e4m3) operands, launch_gemm_fp8 only: A [M_pad][K] and W [N_pad][K] are bytes, lda / ldw in elements (= bytes);
    // C = rnd(a_scale[m] * w_scale[n] * acc + bias) ... : per-token and per-output-channel fp32 scales (weights.py / api.hip)
    const float* a_scale;
    const float* w_scale;
    // EPI_BIAS_QKNORM only: LayerNorm(64) weights / biases of q and k ([64] each), the PAIRED rotary table [positions][32 cos | 32 sin]
    // fp32 (value k = cos / sin of dims 2k and 2k+1; null: no rotary embedding), width of the q (= k = v) range, LayerNorm epsilon;
    // tok_per_batch and text_len above give the position of a row
    const void* qk_w[2]; const void* qk_b[2];
    const float* qk_cs;
    int qk_D; float qk_eps;
    // gemm_g4 only, split K (few output tiles, long K: the FF2 of the short-sequence geometries): splitk > 1 workgroups share an output
    // tile, each reduces K / splitk; sk_ws holds their fp32 partial tiles (tiles * splitk * 256 KiB), sk_cnt one arrival counter per
    // tile (zero before the launch, zero again after it).  The last workgroup to arrive adds the partials IN SPLIT ORDER (so the sum
    // does not depend on who was last) and runs the epilogue.
    int splitk; float* sk_ws; unsigned* sk_cnt;
    // fp8 GEMMs only, MX (block-scaled) activations: v_mfma_scale_f32_32x32x64_f8f6f4 takes one E8M0 scale per lane = per (row, 32
    // consecutive K elements), so a producer can quantise its output tile in place -- no row amax across workgroups.
    //   mx_out_q / mx_out_s (EPI_BIAS_GELU): the epilogue writes e4m3 bytes [M][N] and scale bytes [M][N / 32] (2^(s - 127), the
    //   smallest power of two with amax / scale <= 448) INSTEAD of the bf16 C;
    //   mx_a_s: A is such an image with its block scales; a_scale may then be null (= 1).
    //   Layout of the scales (round 4): K-TILE MAJOR -- [K / 128][mx_rows] dwords, dword (kt, m) = the four block scales of row m inside
    //   the 128 elements of K-tile kt (byte b = block 4 kt + b).  A GEMM's K-tile then finds the dwords of its 256 rows in ONE contiguous
    //   KiB (an LDS-DMA dword per lane over [M][K / 32] touched 64 cache lines per wave and K-tile: the MX loops ran at 3.3 k cycles per
    //   K-tile against 2.15 k for the unit-scale loop).  mx_rows = rows of that array (>= the padded M, a multiple of 128).
    //   Inside every 128-row half the rows are PERMUTED: row m sits at mx_perm_row(m) = (m & ~127) | (m & 31) << 2 | (m >> 5) & 3, so that
    //   the rows j * 32 + fr (j = 0..3) of the four A fragments of a lane are four consecutive dwords -- one 16-byte load.
    unsigned char* mx_out_q; unsigned char* mx_out_s;
    const unsigned char* mx_a_s;
    int mx_rows;
    // fp8 GEMMs only, runtime LoRA (lora_runtime_fp8): the adapter's up-projection rides behind the K loop as 16-bit matrix work,
    //   C = epilogue(a_scale[m] * w_scale[n] * acc + T . Bs^T + bias),   T = rnd(x . A^T) [M_pad][lora_ldt],   Bs = rnd(s * B) [N_pad][lora_r],
    // both bf16, lora_r a multiple of 16 (pad columns zero), rows present up to the padded 256-row tiles.  Output columns
    // [j * lora_seg, (j + 1) * lora_seg) read the columns [j * lora_r, (j + 1) * lora_r) of T (the fused QKV: q | k | v have an adapter
    // each; lora_seg = 0: one adapter, lora_seg % 64 == 0 otherwise).  lora_bs null: no branch -- the instantiation without it runs.
    const void* lora_t; int lora_ldt;
    const void* lora_bs; int lora_r, lora_seg;
};
// fp8 x fp8 -> bf16 GEMM on v_mfma_scale_f32_32x32x64_f8f6f4 (unit block scales; the per-row scales above in the epilogue): the
// 256 x 256 ping-pong schedule of gemm_bf16_pp64 on K-tiles of 128 bytes.  Plain mode only (no conv), K % 128 == 0, N_pad % 256 == 0.
int launch_gemm_fp8(const GemmArgs& a, int epi, hipStream_t st);
// rows [M][K] of bf16 (ld elements apart) -> e4m3 bytes [M][K] + scale[m] = amax(row) / 448 (dynamic per-row quantisation)
int launch_quant_rows_fp8(const void* src, int64_t ld, int64_t M, int K, void* dst, float* scale, hipStream_t st);
enum { EPI_BIAS_ADD = 3 };
// EPI_BIAS_QKNORM: the fused QKV projection.  C = rnd(acc + bias); then, on the 64-column heads of the q and k ranges (columns
// < 2 * qk_D), the per-head LayerNorm(64) + affine and the rotary embedding of attention_processor.py:2060-2080 /
// embeddings.py:759-778, with the same arithmetic and rounding points as qk_norm_rope_k (which it replaces on the MFMA path: one
// pass over 2/3 of the QKV buffer less per layer).  Rows are tokens: r = m % tok_per_batch, rotary for r >= text_len.
enum { EPI_BIAS_QKNORM = 4 };

__host__ __device__ __forceinline__ int64_t mx_perm_row(int64_t m) { return (m & ~(int64_t)127) | ((m & 31) << 2) | ((m >> 5) & 3); }
int launch_gemm_bf16(const GemmArgs& a, int epi, hipStream_t st);              // MFMA path, bf16 only
// any dtype, any shape.  fp32 calls that qualify (gemm_f32m_ok) run on the fp32 matrix pipe (gemm_f32m.hip) unless a.valu_only -- same bits
int launch_gemm_simple(const GemmArgs& a, int epi, int dtype, hipStream_t st);
// fp16 operands (the fp16 model dtype) on v_mfma_f32_32x32x16_f16: the 128 x 128 x 64 kernel of gemm.hip with its lane-local epilogue
bool gemm_f16_ok(const GemmArgs& a, int epi);
int launch_gemm_f16(const GemmArgs& a, int epi, hipStream_t st);
// gemm_f32m.hip: fp32 operands on v_mfma_f32_32x32x2_f32, bit-identical to gemm_simple_k<float>
bool gemm_f32m_ok(const GemmArgs& a);
int launch_gemm_f32m(const GemmArgs& a, int epi, hipStream_t st);
// gemm_g4.hip: 256 x 256 tiles, four waves, generated-asm K loop (plain operands; gemm_g4_ok says whether a call qualifies).  a.f16: the same
// loop on fp16 operands (v_mfma_f32_32x32x16_f16) with the fp16 form of the vector epilogue -- the fp16 model dtype's big linears
bool gemm_g4_ok(const GemmArgs& a, int epi);
int launch_gemm_g4(const GemmArgs& a, int epi, hipStream_t st);
// gemm_g4f.hip: the four-wave loop on e4m3 operands (launch_gemm_fp8 routes to it where gemm_g4f_ok)
bool gemm_g4f_ok(const GemmArgs& a, int epi);
int launch_gemm_g4f(const GemmArgs& a, int epi, hipStream_t st);
// gemm_g4t.hip: the same tiles as a persistent kernel whose epilogue is trickled through the next tile's K loop (gen_gemm_g4t.py);
// bias / bias + GELU epilogues on whole 256 x 256 tiles with at least two rounds of them on `ncu` CUs
bool gemm_g4t_ok(const GemmArgs& a, int epi, int ncu);
int launch_gemm_g4t(const GemmArgs& a, int epi, hipStream_t st);
// Few tiles and a long reduction (C1: the FF2 is 80 tiles of 120 K-tiles -- one K loop is 130 us however many CUs idle; the T5 encoder
// at M = 452: 32-96 tiles): split K over S workgroups per tile (GemmArgs::splitk), S the largest count <= 4 that still fits one round
// of `ncu` CUs and leaves an even number >= 16 of K-tiles per workgroup (below that the fp32 partial traffic costs what the shorter
// loop saves: measured on the C1 out-projection).  1 = do not split.  Workspace: S * tiles * 256 KiB of partials + tiles counters (zero).
int gemm_choose_splitk(int64_t tiles, int K, int64_t ncu);
// compute units of the current device, queried once per device (launch-path heuristics count tile ROUNDS in these; 256 if the query fails)
int device_cus();
// The kernel choice of the 16-bit and fp8 GEMMs (gemm.hip).  gemm_plan is pure -- no HIP call, the CU count is an argument -- so it runs
// without a device (tests/test_gemm_dispatch_cpu.py through s2v_diag_gemm_plan).  For an engine linear (api.hip linear(): plain operands
// with the rows padded to 256) it decides split K (sk_tiles = the partial tiles of the context's workspace, 0: none), GemmArgs::tile and
// whether the partial last row tile runs as a tail launch; convolutions and fp8 GEMMs run as given.  launch_gemm_bf16 / launch_gemm_fp8
// run the kernel it names for each launch.
enum GemmKernel { GEMM_NONE = 0, GEMM_128, GEMM_STAG, GEMM_PP64, GEMM_G4, GEMM_G4T, GEMM_W8, GEMM_Q4, GEMM_G4F, GEMM_PP64_FP8 };
struct GemmPlan {
    int splitk;  // GemmArgs::splitk of the launch (0: K is not split)
    int tile;    // GemmArgs::tile of the launches
    int m_main;  // rows of the main launch: M, or the whole 256-row tiles when the partial last one runs as the tail launch
    int main;    // GemmKernel of the main launch
    int tail;    // GemmKernel of the tail launch on rows [m_main, M) (m_begin = m_main, side stream); GEMM_NONE: no tail
};
GemmPlan gemm_plan(const GemmArgs& g, int epi, int ncu, int64_t sk_tiles);
// generic strided fp32 GEMM used at load time (LoRA merge): C[m,n] += alpha * sum_k A[m*sam+k*sak]*B[n*sbn+k*sbk]
int launch_gemm_strided_f32(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbn, int64_t sbk,
                            float* C, int64_t ldc, int M, int N, int K, float alpha, hipStream_t st);

// ---- runtime LoRA (lora.hip) ----------------------------------------------------
// out[m][n] = rnd(sum_k x[m][k] * A[n][k]), fp32 accumulation: the adapter's down-projection.  x [M][K] (rows ldx apart), A [N][K] (the
// layer's A stack, rows lda apart), out rows ldo apart -- in the engine `out` is column K of the buffer x lives in.
struct LoraDownArgs {
    const void* x; int ldx;
    const void* A; int lda;
    void* out; int ldo;
    int M, N, K;
    // launch_lora_down_mx only: the block scales of x (GemmArgs::mx_a_s: K-tile major dwords, rows permuted) and the rows of that array
    const unsigned char* mx_s; int mx_rows;
};
// mfma: the 16-bit model dtypes on v_mfma_f32_32x32x16_{bf16,f16} (N % 64 == 0, N <= 384, K % 64 == 0); otherwise the generic kernel
int launch_lora_down(const LoraDownArgs& a, int dtype, bool mfma, hipStream_t st);
// the same product with x given as an MX e4m3 image (bytes [M][K], ldx in bytes, block scales a.mx_s): every element is dequantised
// exactly -- e4m3(byte) * 2^(scale - 127) is a bf16 value -- and multiplied on v_mfma_f32_32x32x16_bf16; A and out are bf16.
// N % 64 == 0, N <= 128, K % 128 == 0
int launch_lora_down_mx(const LoraDownArgs& a, hipStream_t st);
// attach time: A [rank][K] fp32 -> `rows` rows of the stack (rows past rank zero); scale * B [N][rank] fp32 -> `cols` tail columns (past rank zero)
int launch_lora_pack_a(const float* A, int rank, int rows, int K, void* dst, int64_t ldd, int dtype, hipStream_t st);
int launch_lora_pack_b(const float* B, int rank, int cols, int N, float scale, void* dst, int64_t ldd, int dtype, hipStream_t st);

// ---- attention ---------------------------------------------------------------
// qkv: [B*Ntok (+pad), 3*D] rows = tokens; q at col h*64, k at col D+h*64, v at col 2D+h*64.
// out: [B*Ntok, D] (col h*64+d).  softmax(q k^T / 8) v, no mask  (attention_processor.py:2083-2087)
struct AttnArgs {
    const void* qkv; int ld_qkv;
    const void* vt;            // bf16 path only: V^T [B][H][64][ntok_pad] (kv-permuted inside 16-groups)
    int ntok_pad;
    void* out; int ld_out;
    int B, H, Ntok;
    float scale;               // 1/sqrt(64)
    // bf16 path, optional: nine zero-initialised ints owned by the caller (one set per concurrently running launch) and the CU count
    // -> the persistent, work-pulling launch (attention.hip: attn_pp_persist_k); null -> one workgroup per q-block
    int* queue; int num_cus;
    // fp8 engine, attn_q4 only: write the output as MX e4m3 [B*Ntok][ld_out] bytes + block scales (K-tile major, GemmArgs::mx_a_s:
    // [ld_out / 128][mx_rows] dwords) INSTEAD of the bf16 `out` (the out-projection reads it through GemmArgs::mx_a_s)
    unsigned char* mx_q; unsigned char* mx_s; int mx_rows;
    // fp8 QK^T (weight_format 2, attn_q4f): MX e4m3 images of q (pre-multiplied by scale * log2 e) and k, written by launch_qk_quant_mx:
    //   q8 [B][H][Ntok][64] bytes, q8s [B][H][Ntok] (byte 0 / 1 = E8M0 scale of head-dim block 0 / 1),
    //   k8 [B][H][ntok_pad][64] bytes (rows past Ntok zero), k8s [B][H][ntok_pad / 64][64] dwords: dword (hi * 32 + r) of a 64-key tile holds in
    //   byte kb the E8M0 scale of (key 32 kb + r, block hi) -- the scale VGPR of the QK^T MFMA, loaded as is
    const unsigned char* q8; const unsigned short* q8s; const unsigned char* k8; const unsigned* k8s;
    // attn_p_format 1 (attn_q4h / attn_q4fh): `vt` holds fp16 (launch_v_transpose(..., vt_amax)), P is built as fp16 pairs and summed by
    // packed fp16 adds, P.V runs on v_mfma_f32_32x32x16_f16; deferred maximum 2^14 instead of 2^64 (gen_attn_q4.py, P16).  attn_q4 forms only.
    int p16;
    // p16 with bf16 storage: [B * H] words written by launch_v_transpose -- bits of the largest |V| of each (batch, head); V^T holds V * 2^vt_f16_shift
    // of that word and the kernel's epilogue takes the power of two out again (exact; see vt_f16_shift)
    const unsigned* vt_amax;
    // optional census of the deferred-maximum slow path (attn_q4 forms): 256 slots of two counters, slot = workgroup & 255:
    // [2 s] += slow paths taken, [2 s + 1] += (wave, KV tile) pairs run.  The engine reads it to decide whether fp16 P pays on the data at hand.
    unsigned long long* stats;
    long long* clk;            // profile pass only: shader-clock stamp slot (common.h clk_stamp; the four-wave kernels), else null
    int order;                 // persistent four-wave launch: 0 = a head's q-blocks on one XCD (default), 1 = dealt over the XCDs (experiment, attn_qx_persist_k)
    int stagger;               // persistent four-wave launch: workgroup (blockIdx >> 3) = slot s of its XCD starts s * stagger * 64 cycles late (0 = together); see attn_qx_persist_k
    int valu_only;             // fp32 only: stay on attn_simple_k (cfg.force_simple) instead of the fp32-MFMA kernel attn_f32m_k
    // four-wave forms whose attn_plan splits: counters + partial slots (attn_kv_ws_bytes; the counters zero, which every launch restores).  The
    // engine carves it with the geometry; null = the launch takes the process-wide one, grown on demand (operator entries: never under capture)
    void* kv_ws; int64_t kv_ws_bytes;
};
// sequences up to this length run attn_pp (launch_attn_bf16), longer ones attn_q4 (profiles/r03_attn_short_sequences.txt: attn_pp 9 % ahead at
// 4000 tokens, attn_q4 2 % ahead at 6000, 7 % at 8192); the fp8 engine's MX output is attn_q4's at any length
#ifndef ATTN_PP_MAX_TOKENS
#define ATTN_PP_MAX_TOKENS 4608
#endif
// fp16 V^T of bf16 V (attn_p_format 1): fp16 has three exponent bits fewer than bf16, and V stored as it is would round everything under 2^-14 into
// subnormals and saturate above 65504.  Each (batch, head) is therefore stored times the power of two that puts its largest magnitude into
// [2^14, 2^15): nothing saturates (short of a largest magnitude of 2^115 and more, where the shift is clamped at -100 and v_transpose_k's clamp
// to +-65504 takes over), and values down to 2^-29 of the largest keep every bit.  amax_bits: bf16 bit pattern (sign cleared) of that magnitude;
// zero, inf and NaN leave V as it is.
#define VT_AMAX_WORDS 4096  // words the engine and the operator entry hold for AttnArgs::vt_amax (B * H of a launch must fit)
__host__ __device__ static inline int vt_f16_shift(unsigned amax_bits) {
    const int e = (int)((amax_bits >> 7) & 0xffu);
    if (e == 0 || e == 255) return 0;
    const int s = 14 - (e - 127);
    return s > 100 ? 100 : (s < -100 ? -100 : s);
}
static inline bool attn_runs_q4(int Ntok, bool mx_out) { return mx_out || Ntok > ATTN_PP_MAX_TOKENS; }
// KV split of the four-wave launch (attention_q4.hip).  A head's q-blocks cost the same, so B * H * nqb items leave the last round of a
// persistent launch mostly idle (C3: 7200 items on 256 workgroups = 28.125 rounds, run as 29; now 7008 whole items and 768 parts).  The trailing `split` q-blocks of every head are
// therefore cut BY KEY RANGE into S parts of contiguous KV tiles [t[s], t[s + 1]); a part runs the unchanged body over its tiles and leaves
// (unnormalised O, l, -m) in a workspace slot, and the last part to arrive merges the S slots in the order s = 0 .. S - 1 and runs the epilogue.
// attn_plan is the ONLY place that decides the split, and it sees the token count and the format alone: B, the head count, the CU count, the
// launch form and the entry point cannot enter, so a row's bits are a function of (Ntok, format, inputs) -- the bitwise B = 1 == half of B = 2,
// head-shard and per-item == persistent tests rest on that.  Pure host code (tests/test_attn_plan_cpu.py through s2v_diag_attn_plan).
enum { ATTN_FMT_Q4 = 0, ATTN_FMT_Q4H = 1, ATTN_FMT_Q4HH = 2, ATTN_FMT_Q4F = 3, ATTN_FMT_Q4FH = 4, ATTN_FMT_COUNT = 5 };
#ifndef ATTN_KV_PARTS
#define ATTN_KV_PARTS 4         // S: parts of a split q-block (4 and 8 measured: profiles/r19_attn_kv_split.txt)
#endif
#ifndef ATTN_KV_SPLIT_BLOCKS
#define ATTN_KV_SPLIT_BLOCKS 2  // trailing q-blocks of a head that are split (1 and 2 measured)
#endif
#define ATTN_KV_MIN_TILES 8     // shortest part: the body pre-stages K tiles 0 .. 3 and V^T tiles 0 .. 1 and walks its last five tiles in phase B
#define ATTN_KV_SLOT_BYTES (4 * 2 * 32 * 64 * 4 + 2 * 4 * 2 * 64 * 4)  // a part's slot: O^T fp32 [wave][j][register][lane], then l and -m [wave][j][lane]
struct AttnPlan {
    int whole;                 // q-blocks per head that run as one item over all KV tiles
    int split;                 // trailing q-blocks per head cut by key range (0: no split; then S = 1)
    int S;                     // parts per split q-block
    int t[ATTN_KV_PARTS + 1];  // part s = KV tiles [t[s], t[s + 1]); t[0] = 0, t[S] = ceil(Ntok / 64)
};
// the head of the plan: whole / split / S.  __host__ __device__: the kernels recompute it from (Ntok, format) where they need it instead of
// carrying it across the body, which leaves them no registers to spare
__host__ __device__ static inline void attn_plan_head(int Ntok, int format, int& whole, int& split, int& S) {
    const int nqb = (Ntok + 255) / 256, nt = (Ntok + 63) / 64;
    whole = nqb; split = 0; S = 1;
    // short sequences run attn_pp; the fp8-QK^T formats keep whole items (their block-scale ring is not offset by a part's first tile)
    if (Ntok <= ATTN_PP_MAX_TOKENS || format == ATTN_FMT_Q4F || format == ATTN_FMT_Q4FH || format < 0 || format >= ATTN_FMT_COUNT) return;
    int s = nt / ATTN_KV_MIN_TILES;
    if (s > ATTN_KV_PARTS) s = ATTN_KV_PARTS;
    const int sp = nqb < ATTN_KV_SPLIT_BLOCKS ? nqb : ATTN_KV_SPLIT_BLOCKS;
    if (s < 2 || sp < 1) return;
    whole = nqb - sp; split = sp; S = s;
}
// first KV tile of part s of S over nt tiles (s = S: nt): the first nt % S parts are one tile longer
__host__ __device__ static inline int attn_part_tile(int nt, int S, int s) { return s * (nt / S) + (s < nt % S ? s : nt % S); }
static inline AttnPlan attn_plan(int Ntok, int format) {
    AttnPlan p{};
    attn_plan_head(Ntok, format, p.whole, p.split, p.S);
    for (int s = 0; s <= p.S; ++s) p.t[s] = attn_part_tile((Ntok + 63) / 64, p.S, s);
    return p;
}
// bytes of AttnArgs::kv_ws for a launch of B * H <= ATTN_KV_MAX_BH heads: a head of fixed size -- 8 sub-item queue counters, then one arrival
// counter per split q-block, all zero between launches -- then B * H * split * S slots; 0 when the plan does not split
#define ATTN_KV_MAX_BH 4096
#define ATTN_KV_WS_HEAD ((8 + ATTN_KV_MAX_BH * ATTN_KV_SPLIT_BLOCKS) * 4 + 224)  // a multiple of 256
static inline int64_t attn_kv_ws_bytes(const AttnPlan& p, int64_t BH) {
    return p.split == 0 ? 0 : ATTN_KV_WS_HEAD + BH * p.split * p.S * (int64_t)ATTN_KV_SLOT_BYTES;
}
// q / k of the (normalised, rotated) QKV buffer -> the MX e4m3 images above (elementwise.hip)
int launch_qk_quant_mx(const void* qkv, int ld_qkv, int B, int H, int Ntok, int ntok_pad, float q_prescale, unsigned char* q8, unsigned short* q8s,
                       unsigned char* k8, unsigned* k8s, hipStream_t st);
// the same images from the RAW q / k of the projection: per-head LayerNorm + rotary (qk_norm_rope_k's arithmetic) folded into the quantisation pass;
// a.vt is ignored (V^T stays launch_v_transpose's); bf16 only (elementwise.hip)
struct QkNormRopeArgs;
int launch_qk_norm_quant_mx(const QkNormRopeArgs& a, float q_prescale, unsigned char* q8, unsigned short* q8s, unsigned char* k8, unsigned* k8s, hipStream_t st);
// attn_q4 with QK^T on the scaled fp8 MFMA (attention_q4.hip); needs a.q8 / q8s / k8 / k8s and a.vt
int launch_attn_q4f(const AttnArgs& a, bool persistent, hipStream_t st);
// attn_q4 with P / V^T in fp16 (AttnArgs::p16 = 1)
int launch_attn_q4h(const AttnArgs& a, bool persistent, hipStream_t st);
int launch_attn_bf16(const AttnArgs& a, hipStream_t st);
// generic kernel, any dtype; fp32 and fp16 calls run attn_f32m (attention_f32m.hip: QK^T and P.V on v_mfma_f32_32x32x2_f32) unless a.valu_only
int launch_attn_simple(const AttnArgs& a, int dtype, hipStream_t st);
int launch_attn_f32m(const AttnArgs& a, int dtype, hipStream_t st);
// fp16 storage on v_mfma_f32_32x32x16_f16 (the lock-step kernel of attention.hip): what the fp16 engine runs; needs a.vt (fp16 V^T)
int launch_attn_f16(const AttnArgs& a, hipStream_t st);
// the four-wave asm kernel with fp16 q / k / V^T / P (attention_q4.hip, attn_q4hh); launch_attn_f16 routes long sequences to it
int launch_attn_q4hh(const AttnArgs& a, bool persistent, hipStream_t st);  // dtype S2V_F32 or S2V_F16 (storage; the arithmetic is fp32 either way)
// four-wave form of the bf16 kernel (attention_q4.hip); persistent needs a.queue / a.num_cus
int launch_attn_q4(const AttnArgs& a, bool persistent, hipStream_t st);
// eight waves x 32 rows running the same fine-grained stream, two waves per SIMD
int launch_attn_q8(const AttnArgs& a, bool persistent, hipStream_t st);

// ---- attention steering: a logit bias on key ranges (include/s2v_hip.h, "Attention steering") --------------------
//   out_i = sum_j softmax_j(s_ij + beta_b(i, j)) v_j,  s_ij = q_i . k_j / 8,
//   beta_b(i, j) = ln w_r  when key j lies in range r = [k0[r], k1[r]), bit b of sample_mask[r] is set and query row i lies in [q0, q1); else 0.
// The record as the kernels read it from DEVICE memory with uniform loads (it is data, not a launch argument: new weights re-capture nothing).
// Ranges disjoint and ascending inside [0, Ntok), 2^-16 <= w <= 2^16 (attn_steer_make refuses anything else by name).
#define ATTN_STEER_MAX_RANGES 4
struct AttnSteerRec {
    int n, q0, q1, pad;
    int k0[ATTN_STEER_MAX_RANGES], k1[ATTN_STEER_MAX_RANGES];
    float log2w[ATTN_STEER_MAX_RANGES];   // what the exp2-domain kernel (attn_pp) adds to its scores
    float lnw[ATTN_STEER_MAX_RANGES];     // what the generic kernel (attn_simple_k, expf) adds: ln w rounded once, not log2 w times a rounded ln 2
    unsigned sample_mask[ATTN_STEER_MAX_RANGES];
};
// host: check n ranges (k0, k1, w, sample_mask) and the query range against Ntok and fill the record; `who` prefixes the error
int attn_steer_make(const char* who, int n, const int* k0, const int* k1, const float* w, const unsigned* sample_mask, int q0, int q1, int Ntok,
                    AttnSteerRec* out);
// attn_pp<STEER> at ANY length (bf16; persistent under launch_attn_bf16's rule), and the steered attn_simple_k (any dtype; the fp32 engine's steered
// layers and the cross-check).  rec_dev: the record in device memory.  a.mx_q and a.p16 are refused: attn_pp writes bf16 and reads bf16 V^T only
int launch_attn_bf16_steer(const AttnArgs& a, const AttnSteerRec* rec_dev, hipStream_t st);
int launch_attn_simple_steer(const AttnArgs& a, const AttnSteerRec* rec_dev, int dtype, hipStream_t st);

// ---- steering maps: the same bias with a weight per query row (include/s2v_hip.h, "Steering maps") ----------------
//   beta_b(i, j) = ln W_p[i - q0]  when key j lies in range r = [k0[r], k1[r]), p = plane[r][b] >= 0 and q0 <= i < q1; else 0.
// The record as the kernels read it from DEVICE memory (data, not a launch argument), 4-byte words, nqb = ceil(Ntok / 256), V = q1 - q0 >= 1:
//   the header below (AttnSteerMapRec, ATTN_STEER_MAP_HDR words)
//   [off_log2 ..)   log2 W_p[v], fp32 [n_planes][V]: what attn_pp<MAP> adds (the expression that fills AttnSteerRec::log2w)
//   [off_ln ..)     ln W_p[v], fp32 [n_planes][V]: what the generic kernel adds (the expression that fills AttnSteerRec::lnw)
//   [off_live ..)   wave liveness, int32 [ATTN_STEER_MAP_BATCH][8 nqb]: bit r of entry (b, 8 q + w) is set iff plane[r][b] >= 0 and some row of
//                   [256 q + 32 w, +32) inside [q0, q1) has W_p != 1 -- a wave reads its entry with a uniform load and looks at its live ranges only
// The offsets are in words from the record's start and leave room for the allocation's plane capacity, so a record with fewer planes fits in place.
#define ATTN_STEER_MAP_MAX_PLANES 16
#define ATTN_STEER_MAP_BATCH 8
struct AttnSteerMapRec {
    int n, q0, q1, n_planes;
    int k0[ATTN_STEER_MAX_RANGES], k1[ATTN_STEER_MAX_RANGES];
    signed char plane[ATTN_STEER_MAX_RANGES][ATTN_STEER_MAP_BATCH];
    int off_log2, off_ln, off_live, nqb;
};
#define ATTN_STEER_MAP_HDR ((int)(sizeof(AttnSteerMapRec) / 4))
// the words of a record at Ntok tokens, V query rows and room for cap_planes planes
inline size_t attn_steer_map_words(int Ntok, int V, int cap_planes) {
    return (size_t)ATTN_STEER_MAP_HDR + 2 * (size_t)cap_planes * V + (size_t)ATTN_STEER_MAP_BATCH * 8 * ((Ntok + 255) / 256);
}
// host: the liveness table alone, [ATTN_STEER_MAP_BATCH][8 nqb] (exported as s2v_attn_steer_map_wave_flags for the CPU test against brute force)
void attn_steer_map_wave_flags(int n, int q0, int q1, int Ntok, const signed char* plane /* [4][8] */, const float* planes /* [.][q1 - q0] */, int* out);
// host: check everything (ranges as attn_steer_make; 1 <= n_planes <= 16; plane indices inside [-1, n_planes) and -1 on samples >= B; every weight
// finite inside [2^-16, 2^16], the error naming plane and cell) and build the record with room for cap_planes >= n_planes planes
int attn_steer_map_make(const char* who, int n, const int* k0, const int* k1, const signed char* plane /* [4][8] */, int n_planes, const float* planes,
                        int q0, int q1, int Ntok, int B, int cap_planes, std::vector<int>* out);
// attn_pp<MAP> at ANY length (bf16; persistent under launch_attn_bf16's rule) and the mapped attn_simple_k (any dtype); as the STEER launches
int launch_attn_bf16_steer_map(const AttnArgs& a, const AttnSteerMapRec* rec_dev, hipStream_t st, bool force_persist = false);
int launch_attn_simple_steer_map(const AttnArgs& a, const AttnSteerMapRec* rec_dev, int dtype, hipStream_t st);

// ---- local attention in time: video rows attend a window of frames (include/s2v_hip.h, "Local attention") ------------
//   out_i = sum_{j in vis(i)} softmax_{j in vis(i)}(s_ij) v_j,  s_ij = q_i . k_j / 8,  vis(i) = [0, P) union [lo_i, hi_i)
// with one P and one row table (lo_i, hi_i) for every sample and head; 1 <= P <= Ntok, P <= lo_i <= hi_i <= Ntok (lo_i == hi_i: the prefix only).
// The record as the kernels read it from DEVICE memory (data, not a launch argument: a new table re-captures nothing), all int32, nqb =
// ceil(Ntok / 256):
//   [0 .. 4)                 header  P, Ntok, nqb, 0
//   [4 .. 4 + 4 nqb)         per 256-row work item  np, w0, w1, np + (w1 - w0): it visits the key tiles [0, np) and [w0, w1), w0 >= np
//   [.. + 16 nqb)            per 32-row wave  lo_max, hi_min over its rows below Ntok (a wave with none: P, Ntok)
//   [.. + 256 nqb) twice     lo_i, then hi_i, padded to 256 nqb rows with dense rows (P, Ntok)
// attn_local_make (host) checks the table, refusing every bound by name, and reduces the item and wave tables.
#define ATTN_LOCAL_HDR 4
static inline size_t attn_local_ints(int Ntok) { return (size_t)ATTN_LOCAL_HDR + (size_t)((Ntok + 255) / 256) * (4 + 16 + 512); }
#include <vector>
int attn_local_make(const char* who, int P, int Ntok, const int* lo, const int* hi, std::vector<int>* out);
// attn_pp<LOCAL> at ANY length (bf16; persistent under launch_attn_bf16's rule), and the local attn_simple_k (any dtype; the fp32 engine's local
// layers and the cross-check).  rec_dev: the record in device memory, made for a.Ntok.  a.mx_q and a.p16 are refused as for steering
int launch_attn_bf16_local(const AttnArgs& a, const int* rec_dev, hipStream_t st);
int launch_attn_simple_local(const AttnArgs& a, const int* rec_dev, int dtype, hipStream_t st);

// ---- local attention in space and time: a window of frames and of patch rows (include/s2v_hip.h, "Local attention in space and time") ------------
//   vis(i) = [0, P) union { j : lo_i <= j < hi_i and olo_i <= (j - P) mod S < ohi_i }
// with one P, one period S (the rows of a latent frame) and one row table (lo_i, hi_i, olo_i, ohi_i) for every sample and head; 1 <= P <= Ntok,
// P <= lo_i <= hi_i <= Ntok, 0 <= olo_i <= ohi_i <= S, 64 <= S (a 64-key tile then holds at most one frame boundary).
// The record as the kernels read it from DEVICE memory (data, not a launch argument), all int32, nqb = ceil(Ntok / 256), nt = ceil(Ntok / 64):
//   [0 .. 8)                    header  P, Ntok, nqb, S, nt, 0, 0, 0
//   [8 .. 8 + 8 nqb)            per 256-row work item  n (the tiles it visits, >= 1), 0 ...
//   [.. + 256 nqb) four times   lo_i, hi_i - lo_i, olo_i, ohi_i - olo_i, padded to 256 nqb rows with dense rows (P, Ntok - P, 0, S)
//   [.. + 8 nt nqb)             per work item nt entries of 8, the first n in use: entry j = tile(j), o(j), whole(j), tile(j + 2), tile(j + 4),
//                               tile(j + 1), tile(j + 3), 0 with tile(x) the x-th visited tile, x clamped to n - 1 (what the pipeline stages ahead
//                               of iteration j, so that no DMA issue waits on a load of its own); o(j) = (64 tile(j) - P) mod S, the frame offset
//                               of the tile's first key; whole(j) bit w: every key of the tile below Ntok is seen by every row below Ntok of wave w
// The visited tiles of an item are the prefix tiles [0, ceil(P / 64)) and, ascending, every later tile that holds a key some row of the item sees.
// attn_box_make (host) checks the table, refusing every bound by name, and builds the lists and the whole bits: the kernel reduces nothing.
#define ATTN_BOX_HDR 8
static inline size_t attn_box_ints(int Ntok) {
    const size_t nqb = (size_t)((Ntok + 255) / 256), nt = (size_t)((Ntok + 63) / 64);
    return (size_t)ATTN_BOX_HDR + nqb * (8 + 1024 + 8 * nt);
}
int attn_box_make(const char* who, int P, int S, int Ntok, const int* lo, const int* hi, const int* olo, const int* ohi, std::vector<int>* out);
// attn_pp<BOX> at ANY length (bf16; persistent under launch_attn_bf16's rule), and the box attn_simple_k (any dtype); as the local launches above
int launch_attn_bf16_box(const AttnArgs& a, const int* rec_dev, hipStream_t st);
int launch_attn_simple_box(const AttnArgs& a, const int* rec_dev, int dtype, hipStream_t st);

// ---- elementwise / normalisation ------------------------------------------------
// LayerNorm(eps, affine w,b) then (1+scale)*y+shift with per-row-range modulation sets.
// rows: [B*Ntok, D]; text rows use (shift_txt, scale_txt), other rows (shift_vid, scale_vid); all [B][mod_stride].
struct LnModArgs {
    const void* x; int ldx; void* y; int ldy;
    const void* w; const void* b; float eps;
    const void* shift_vid; const void* scale_vid; const void* shift_txt; const void* scale_txt; int mod_stride;
    int B, Ntok, text_len, D;
    const void* shift_ref; const void* scale_ref; int ref_len;  // optional set for rows [text_len, text_len + ref_len); null: vid
    // fp8 linears (bf16 storage only): when q8 is set the modulated row is NOT stored as bf16 but quantised on the spot exactly as
    // quant_rows_fp8_k would quantise its bf16 image -- e4m3 bytes [row][D] and scale[row] = amax / 448 -- for the projection that
    // consumes it (one read + one write pass over the activations less per LayerNorm)
    void* q8; float* q8_scale;
    int q8_keep_y;  // with q8: the bf16 rows are stored to y as well (the fp8 engine's runtime LoRA reads them for its down-projection)
};
int launch_ln_modulate(const LnModArgs& a, int dtype, hipStream_t st);
// which kernel launch_ln_modulate runs for rows x D of `dtype`, and with how many rounds of 64 lanes x 16 bytes (NR; -1: row too long): pure host
// arithmetic, the launcher's own choice (the diagnostics build exports it as s2v_diag_ln_plan).  lds_rows: from this many rows on bf16 rows take
// ln_modulate_lds_k (0 = never); the product's value is LN_LDS_ROWS
enum { LN_KERNEL_REG = 0, LN_KERNEL_LDS = 1 };
#define LN_LDS_ROWS 16384  // at least four workgroups of sixteen rows per CU
struct LnPlan { int kernel, nr; };
LnPlan ln_modulate_plan(int rows, int D, int dtype, int lds_rows);

// per-head LayerNorm(64, eps 1e-6, affine) on q,k (in place in qkv) + interleaved-pair RoPE on rows >= text_len,
// optional V^T production (bf16 path).  cos/sin: [Ntok - text_len, 64] fp32 (ref rows then video rows), null => no RoPE.
struct QkNormRopeArgs {
    void* qkv; int ld_qkv; int B, H, Ntok, text_len;
    const void* nq_w; const void* nq_b; const void* nk_w; const void* nk_b; float eps;
    const float* cos; const float* sin;
    void* vt; int ntok_pad;   // null => skip
    int vt_f16;               // V^T as fp16 (AttnArgs::p16)
    unsigned* vt_amax;        // vt_f16: AttnArgs::vt_amax, [B * H] words
};
int launch_qk_norm_rope(const QkNormRopeArgs& a, int dtype, hipStream_t st);
// bf16 V [B*Ntok, ld] (cols 2D + h*64 + d) -> V^T [B][H][64][ntok_pad] in the k-slot order attn_bf16 consumes
// vt_amax non-null: V^T as fp16, each (batch, head) scaled by 2^vt_f16_shift of its largest magnitude, which is left in vt_amax[b * H + h]
int launch_v_transpose(const void* qkv, int ld_qkv, int B, int H, int Ntok, void* vt, int ntok_pad, hipStream_t st, unsigned* vt_amax = nullptr);

// timestep sinusoid -> Linear -> SiLU -> Linear  (embeddings.py:27-78, 864-876)
int launch_time_embed(const float* t_dev, int B, int D, const void* w1, const void* b1, const void* w2, const void* b2,
                      int temb_dim, void* tmp /*[B,temb]*/, void* emb_out /*[B,temb]*/, int dtype, hipStream_t st);
// out[j][b][:] = W_j . silu(emb[b]) + bias_j for a batch of stacked linears: W [rows_total, temb], bias [rows_total]
// (a batch over GEMV_MAX_B runs in chunks of at most GEMV_MAX_B samples, each sample's sum the chain it is alone)
#define GEMV_MAX_B 4
int launch_mod_gemv(const void* emb, int B, int temb_dim, const void* W, const void* bias, int64_t rows_total,
                    void* out /*[B][rows_total]*/, int dtype, hipStream_t st, bool rowwise = false);

// latents [Bn, F, C, H, W] -> patches [Bn*F*(H/2)*(W/2), C*4] with feature order (c, py, px);
// lat_bstride = elements between samples (0 => every sample reads the same latent: the CFG pair); n_lat > 0: sample b reads latent
// b mod n_lat (the CFG pairs of n_lat videos, [negative x n_lat | positive x n_lat], straight from the [n_lat] latents)
int launch_patchify(const void* lat, int64_t lat_bstride, int Bn, int F, int C, int H, int W, void* out, int dtype,
                    hipStream_t st, int n_lat = 0);
// y [B*V, C*4] (feature c*4+py*2+px) -> out [B, F, C, H, W]; rows of y start at y_row0 with batch stride y_bstride rows
int launch_unpatchify(const void* y, int ldy, int64_t y_bstride, void* out, int B, int F, int C, int H, int W, int dtype,
                      hipStream_t st);
// Ulysses packs / unpacks (ulysses.hip): for every segment k = (ko, ki) of nseg = (nseg / nseg_inner) x nseg_inner and row i < rows,
// width16 16-byte pieces move from src + ko * src_seg_outer + ki * src_seg_inner + smap(i) * src_ld to the same place under dst's strides;
// smap / dmap = the row maps when given (identity otherwise), a negative map entry skips the row.  Byte offsets and strides, all 16-aligned.
struct ShardCopyArgs {
    const char* src; char* dst;
    int rows, width16;
    int64_t src_ld, dst_ld;
    const int* src_map; const int* dst_map;
    int nseg, nseg_inner;
    int64_t src_seg_outer, src_seg_inner, dst_seg_outer, dst_seg_inner;
};
int launch_shard_copy(const ShardCopyArgs& a, hipStream_t st);
// The O exchange of the fp8 engine carries MX e4m3 (AttnArgs::mx_q / mx_s): the bytes are whole 16-byte pieces (launch_shard_copy), the E8M0 block
// scales are dwords of a K-tile-major array (GemmArgs::mx_a_s: dword (kt, m) at kt * mx_rows + mx_perm_row(m)).  For every segment k < nseg, row
// i < rows and K-tile kt < nkt, one dword moves from src + k * src_seg + kt * src_kt + row(smap(i)) * src_row to the same place under dst's strides,
// row(m) = mx_perm_row(m) on a side with perm set, m otherwise; smap / dmap as for launch_shard_copy.  Offsets and strides in dwords.
struct ShardScaleArgs {
    const unsigned* src; unsigned* dst;
    int rows, nkt, nseg;
    const int* src_map; const int* dst_map;
    int64_t src_row, src_kt, src_seg, dst_row, dst_kt, dst_seg;
    int src_perm, dst_perm;
};
int launch_shard_scales(const ShardScaleArgs& a, hipStream_t st);
// dst[r][:] = rnd(src[r][:] (+ add[r][:]))
int launch_copy_rows(const void* src, int lds_, const void* add, int ldadd, void* dst, int ldd, int rows, int D,
                     int dtype, hipStream_t st);
// step cache (include/s2v_hip.h): sample b's n contiguous elements at x + b * x_bstride against the dense cache [B][n]
//   SC_KEEP: cache = x (and keep2 = x when non-null)   SC_SUB: cache = rnd(x - cache)   SC_ADD: x = rnd(x + cache)
enum { SC_KEEP = 0, SC_SUB = 1, SC_ADD = 2 };
int launch_step_cache(int op, void* x, int64_t x_bstride, void* cache, void* keep2, int B, int64_t n, int dtype, hipStream_t st);
// final: y = LN2(LN1(x)) * (1+scale[b]) + shift[b]   on video rows  (cogvideox_transformer_3d.py:536-542)
struct TailNormArgs {
    const void* x; int ldx; void* y; int ldy;
    const void* w1; const void* b1; const void* w2; const void* b2; float eps;
    const void* shift; const void* scale; int mod_stride;
    int B, Ntok, row0, V, D;
};
int launch_tail_norm(const TailNormArgs& a, int dtype, hipStream_t st);

// CFG + scheduler step (custom_cogvideox_pipe.py:266-296; scheduling_{ddim,dpm}_cogvideox.py)
// Per-step scalars live in DEVICE memory so one captured hipGraph serves every step.
//   x0 = rnd(c_x0_x * x) - c_x0_v * v
//   kind 0 (DDIM)          : out = rnd(a_t * x) + b_t * x0
//   kind 1 (DPM first/last): out = (rnd(m1 * x) - m2 * x0) + rnd(mn * noise)
//   kind 2 (DPM multistep) : d = m3 * x0 - m4 * x0_old ; out = (rnd(m1 * x) - m2 * d) + rnd(mn * noise)
// nvid videos per launch, video v = blockIdx.y with its own coefficient set coef[v] (kind and guidance included): the set is chosen per
// workgroup, so its load stays uniform and no workgroup runs across two videos.
struct SchedCoef {
    int kind; float guidance;
    float c_x0_x, c_x0_v, a_t, b_t, m1, m2, m3, m4, mn;
    float guidance_subject;   // the triple combine's subject scale (cfg = SCHED_CFG_TRIPLE); the pair paths never read it
};
// Subject guidance: three predictions per video, u (negative text, null reference), r (negative text, the reference), f (positive text, the
// reference), combined as v = (u + guidance_subject * (r - u)) + guidance * (f - r) in fp32, every operation rounding on its own and in this
// association.  With the u plane holding the r plane's bits r - u = +0, so v is the pair's r + guidance * (f - r) bit for bit whatever the scale.
enum { SCHED_CFG_TRIPLE = 2 };
struct SchedArgs {
    const void* noise_pred;   // [2, n] model dtype (uncond, cond), [1, n] when !cfg, or [3, n] (u, r, f) when cfg == SCHED_CFG_TRIPLE; n = nvid * n_vid, every plane n elements on
    const void* latents_in;   // [n] model dtype: nvid videos of n_vid elements
    void* latents_out;        // [n] model dtype (may alias latents_in)
    float* x0_hist;           // [n] fp32: read as x0_old (kind 2), overwritten with this step's x0 (may be null for DDIM)
    const void* noise;        // [n] model dtype, DPM only
    int64_t n; int cfg;       // 0, 1 or SCHED_CFG_TRIPLE
    int nvid; int64_t n_vid;  // videos in this launch and the elements of one (n = nvid * n_vid)
    const SchedCoef* coef;    // device pointer to nvid consecutive sets, or null => use cval (nvid = 1)
    SchedCoef cval;
    int np_f32;               // noise_pred is fp32 (the scheduler-object seam: model_output after .float())
    int out_f32;              // latents_out is fp32 and un-rounded (scheduler.step's return value)
};
int launch_sched_step(const SchedArgs& a, int dtype, hipStream_t st, const float* factor = nullptr);   // factor: the RESCALE form (below)
// Masked video-to-video (pipeline_stable_diffusion_inpaint.py:1271-1285, the 4-channel branch, as a select): after the step has produced
// `prev` rounded to T, an element whose latent cell has mask 0 is overwritten -- with add_noise(z0, noise0) at the video's NEXT timestep
// (add_noise_k's arithmetic: rnd(rnd(sqrt_a * z0) + rnd(sqrt_1ma * noise0))), or on the video's last step with z0's own bits.  x0_hist
// keeps the unblended x0.  The records sit beside the coefficient sets in device memory, so the captured graph serves every step.
// The plane holds LEVELS 0..255 (unsigned bytes) and a cell is kept iff level <= keep_max, the video's threshold of this step: a 0 / 1 mask is
// the case keep_max = 0, and a change map (differential diffusion: pipeline_stable_diffusion_xl_differential_img2img.py:1316-1347, whose
// `map` is 1 - level / 255) lowers keep_max step by step, so a cell of level L is released at the step its level asks for.  Every step is
// still a select: no latent is ever multiplied by the map.
struct SchedBlend {
    float sqrt_a, sqrt_1ma;   // Scheduler.add_noise_scalars(t_next, T): already taken in T by the host
    int last;                 // the video's last step: kept elements are z0, bit for bit (coefficients (1, 0) would turn -0 into +0)
    int keep_max;             // 0..255: cells whose level is <= keep_max are kept
};
struct SchedMaskArgs : SchedArgs {     // latents_out is T (out_f32 is refused)
    const void* z0;            // [n] model dtype: the clean input latents, scaled
    const void* noise0;        // [n] model dtype: the noise that started the loop
    const unsigned char* mask; // [nvid][F * hw]: levels, kept where <= keep_max (a mask: 1 repaint, 0 keep); one plane for all channels of a video [F][C][hw]
    int chw, hw;               // C * H * W and H * W of the latent: element j of a video is frame j / chw, cell j % hw of the plane
    int mask_vid;              // F * H * W: the cells of one video's plane
    const SchedBlend* blend;   // device pointer to nvid consecutive records, or null => use bval (nvid = 1)
    SchedBlend bval;
};
int launch_sched_step_masked(const SchedMaskArgs& a, int dtype, hipStream_t st, const float* factor = nullptr);
// Guidance rescale (include/s2v_hip.h has the definition and the order of the sums).  Three launches on one stream: cfg_stats_k, one workgroup per
// (chunk of CFG_STATS_CHUNK elements, video) writing the fp64 quadruple (sum f, sum f^2, sum v, sum v^2) of its chunk, v formed by the step
// kernel's own combine; cfg_finalize_k, adding a video's quadruples in chunk order, deriving the fp32 factor and appending it to the log; and
// the RESCALE form of sched_step_k, whose arguments are the step's with the device factors behind them: v' = v * factor[video], one more rounding.
enum { CFG_STATS_CHUNK = 4096, CFG_LOG_STEPS = 1024, CFG_LOG_COLS = 4 };   // CFG_LOG_COLS = S2V_MAX_BATCH / 2
struct SchedRescaleArgs : SchedArgs { const float* factor; };           // [nvid] fp32, device
struct SchedMaskRescaleArgs : SchedMaskArgs { const float* factor; };
struct CfgStatsArgs {
    const void* noise_pred;   // [2, n] or [3, n] as SchedArgs::noise_pred; model dtype, or fp32 with np_f32
    int64_t n; int cfg;       // 1 or SCHED_CFG_TRIPLE
    int nvid; int64_t n_vid;
    const SchedCoef* coef;    // device pointer to nvid consecutive sets (guidance, guidance_subject), or null => cval (nvid = 1)
    SchedCoef cval;
    int np_f32;
    double* partials;         // [nvid][cfg_stats_chunks(n_vid)][4] fp64, device
};
struct CfgFinalArgs {
    const double* partials; int chunks;
    int nvid; int64_t n_vid;
    const float* phi;         // [nvid] fp32, device
    double* sums;             // [nvid][4] fp64, device: sum f, sum f^2, sum v, sum v^2
    float* factors;           // [nvid] fp32, device
    float* log;               // [CFG_LOG_STEPS][CFG_LOG_COLS] fp32, device, or null: row *log_count takes the factors (0 past nvid) while it is < CFG_LOG_STEPS
    unsigned* log_count;      // device: advanced by every launch
};
int cfg_stats_chunks(int64_t n_vid);
int launch_cfg_stats(const CfgStatsArgs& a, int dtype, hipStream_t st);
int launch_cfg_finalize(const CfgFinalArgs& a, hipStream_t st);
// Temporal windows (include/s2v_hip.h): a long latent of L frames [L][chw] is denoised as W = (L - F) / s + 1 windows of F frames, window k over
// frames [k s, k s + F), and the windows' predictions are averaged where they overlap.  One launch takes the forward of the wb windows
// k0 .. k0 + wb - 1, noise_pred [negative x wb | positive x wb] of [F][chw] each, and adds them into the fp32 plane:
//   v = u + g * (c - u)                      the pair combine of sched_step_k, same association
//   acc[k s + j] = acc[k s + j] + w[j] * v   windows in ascending k, every operation rounding on its own
// A frame whose first covering window is in this launch starts from +0 and its plane cell is not read; a frame whose last covering window is
// in this launch leaves as acc / wsum[frame] (IEEE division), so after the launch of window W - 1 the plane is the averaged prediction, ready
// for launch_sched_step with np_f32 = 1, cfg = 0.  The launches of a step run k0 = 0, wb, 2 wb, ... in order on one stream.
struct WindowBlendArgs {
    const void* noise_pred;   // [2 wb][F][chw] model dtype: the forward's output on the batch's windows
    float* acc;               // [L][chw] fp32
    const float* w;           // [F] fp32 device: the weight of window frame j
    const float* wsum;        // [L] fp32 device: the sum of the weights that cover a frame, accumulated in window order
    const SchedCoef* coef;    // device pointer to the step's coefficient set (its guidance is g), or null => gval
    float gval;
    int L, F, s, W;           // frames of the long latent and of a window, the stride between window starts, the number of windows
    int k0, wb;               // this launch's windows
    int chw;                  // C * H * W: the elements of a frame
};
int launch_window_blend(const WindowBlendArgs& a, int dtype, hipStream_t st);
// pixel mask [F][H][W] (mdtype: S2V_F32 / S2V_BF16 / S2V_F16 binarised at 0.5, or S2V_MASK_U8: non-zero) -> latent mask uint8 [Fl][H/8][W/8],
// a cell 1 if ANY pixel it covers is 1: the 8 x 8 block of pixel frame 0 (latent frame 0) or of pixel frames 4j-3 .. 4j (latent frame j >= 1),
// the causal grouping of the VAE encode; Fl = (F - 1) / 4 + 1.  pixel_out (may be null): the binarised pixel mask, uint8 [F][H][W]
#define S2V_MASK_U8 3
int launch_mask_to_latent(const void* mask, int mdtype, int F, int H, int W, unsigned char* latent_out, unsigned char* pixel_out, hipStream_t st);
// change map [F][H][W] -> latent levels uint8 [Fl][H/8][W/8]: every value becomes a level 0..255 (S2V_MASK_U8: the byte itself; S2V_F32 / S2V_BF16 /
// S2V_F16: floor(clamp(v, 0, 1) * 255 + 0.5) in fp32, one multiply and one add, no fma; NaN -> 0) and a cell takes the MAXIMUM level of the block
// launch_mask_to_latent reduces with "any".  pixel_out (may be null): level > 0 as uint8 0 / 1 [F][H][W], what the masked post-processes take
int launch_map_to_latent(const void* map, int mdtype, int F, int H, int W, unsigned char* level_out, unsigned char* pixel_out, hipStream_t st);
int launch_add_noise(const void* x, const void* noise, int64_t n, float sqrt_a, float sqrt_1ma, void* out, int dtype, hipStream_t st);
// dst[i] = (Tdst) src[i]
int launch_convert(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, hipStream_t st);
// strided 2-D convert-copy: dst[r*ldd + c] = src[r*lds + c]
int launch_convert2d(const void* src, int src_dtype, int64_t lds_, void* dst, int dst_dtype, int64_t ldd, int64_t rows,
                     int64_t cols, hipStream_t st);

// Attention mass (attn_mass.hip): the softmax weight a query of qkv [B * Ntok][ld_qkv] (q | k | v, head_dim 64, scores q . k / 8 over the
// sample's own Ntok keys) puts on n <= 4 key ranges [k0_r, k1_r) -> out [n][B][H][nq] fp32 for the query rows [q0, q0 + nq) of every sample.
// accumulate: out + mass in one fp32 add by the owning thread.  impl 0: v_mfma_f32_32x32x16 (bf16 / fp16 storage; q * 0.125 * log2 e rounded
// to the storage type, exp2, v_rcp_f32); impl 1: the VALU (any dtype; q * 0.125, expf, a division)
#define AM_MAX_RANGES 4
struct AttnMassArgs {
    const void* qkv; int ld_qkv;
    int B, H, Ntok;
    int q0, nq;
    int n; int k0[AM_MAX_RANGES], k1[AM_MAX_RANGES];
    float* out; int accumulate;
};
int launch_attn_mass(const AttnMassArgs& a, int dtype, int impl, hipStream_t st);
// head mean of raw sums acc [n][B][H][nq] -> out [n][B][nq]: (acc[.][.][0][i] + ... + acc[.][.][H-1][i], in that order) * (1.0f / (H * count))
int launch_attn_mass_mean(const float* acc, int n, int B, int H, int nq, int64_t count, float* out, hipStream_t st);
