// Joint [text | ref-image | video] self-attention, head_dim 64, no mask (replaces F.scaled_dot_product_attention at
// attention_processor.py:2083-2087): the four-wave, one-wave-per-SIMD form.  Compiled with -fno-slp-vectorize (build.py): the SLP
// vectoriser merges element accesses of neighbouring accumulators into 32-wide vectors, which keeps SROA from promoting them.
#define S2V_HOST
#include "common.h"
#include "kernels.h"
#include <type_traits>

#define KV_TILE 64
__device__ __forceinline__ float max3f(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// XCD-aware order of the work items (as attention.hip): XCD x owns a contiguous range of q-blocks
__device__ __forceinline__ void attn_xcd_range(int total, int x, int& first, int& cnt) {
    const int q = total >> 3, r = total & 7;
    first = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    cnt = q + (x < r ? 1 : 0);
}

// ---------------------------------------------------------------------------------------------------
// attn_q4: FOUR waves, one per SIMD, 64 query rows per wave (two 32-row blocks j = 0, 1), the whole 512-entry register file.
// A workgroup is the same 256-row work item as attn_pp_item (attention.hip).  What changes against the eight-wave ping-pong:
//   * no SIMD partner: the wave fills the shadow of its OWN MFMAs.  A 32x32x16 MFMA occupies the matrix pipe for 32 cycles and
//     leaves room for about five single-issue instructions behind it (MI355X_MICROARCH, per-instruction constants); the
//     eight-wave form gave the softmax wave one VALU per 16 cycles beside its partner's MFMA stream;
//   * a K / V^T fragment read from LDS feeds TWO MFMAs (both 32-row blocks): 16 ds_read_b128 per 32 MFMA instead of 32;
//   * one barrier per KV tile instead of two.
// Per KV tile and wave: 32 MFMA (1024 matrix-pipe cycles) and 64 exp2 + 64 row-sum adds + 32 v_cvt_pk + 16 fragment reads +
// 4 LDS-DMA pieces + the check = about six fillers per MFMA, each placed by hand.
// Software pipeline (iteration t, S = scores, P = exp2(S - m)):
//   segment 1: 16 MFMA  S(t+1) = K(t+1).Q^T  -> st[(t+1)&1]   | fillers: second half of P(t) (keys 32-63) -> pk[.][2,3],
//                                                               V^T(t) fragments, K(t+4) DMA
//   check    : row sums of tile t against 2^13 (deferred maximum, as attn_pp_item)
//   segment 2: 16 MFMA  O += V^T(t).P(t)                       | fillers: first half of P(t+1) (keys 0-31) -> pk[.][0,1] (written
//                                                               behind the MFMAs that read the old values), K(t+2) fragments,
//                                                               V^T(t+2) DMA, l += row sums of t; vmcnt(4) + barrier
// The raw scores of a tile stay in their st buffer until S(t+2) overwrites them, so the slow path (true row maximum, rescale,
// exp2 redone) has them at the check; it also shifts S(t+1), which segment 1 computed against the old maximum.
// Everything from "tiles staged, Q loaded" to "O and l complete" is ONE generated asm statement (csrc/gen_attn_q4.py ->
// attn_q4_body.inc; register map, phases and the reasons in its header): this function stages the first tiles, loads Q and, after
// the asm, normalises and stores O.  Hazards the assembler does not see: a VALU reads an MFMA result at least four MFMAs after its
// issue, the rare paths and the end of the body start with s_nop 15 x 2, fragment reads are awaited with one s_waitcnt lgkmcnt(0)
// per segment.
// LDS: ring of 4 slots x [K tile 8 KiB | V^T tile 8 KiB]; a wave stages pieces w and w + 4 (8 rows each) of every tile.
//   RAW  K(t+4), V(t+2) are issued in iteration t and awaited (vmcnt(4): everything but this iteration's four) at the end of
//        iteration t+1, one barrier before their first readers (K(t+4): segment 2 of t+2; V(t+2): segment 1 of t+2).
//   WAR  K(t+4) replaces K(t) (last read in segment 2 of t-2), V(t+2) replaces V(t-2) (last read in segment 1 of t-2).
#include "attn_q4_regs.h"
typedef __attribute__((ext_vector_type(32))) float f32x32;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(32))) unsigned int u32x32;
typedef __attribute__((ext_vector_type(8))) unsigned int u32x8;
#ifdef S2V_DIAG
__device__ unsigned long long g_qx_slow[2];
extern "C" __attribute__((visibility("default"))) int s2v_attn_slow_read(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qx_slow), 16) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_qx_slow), z, 16) != hipSuccess) return -1;
    }
    return 0;
}
#endif
// The KV split of a launch (kernels.h attn_plan).  The launcher sets AttnArgs::kv_ws exactly when the plan splits; the kernels recompute the
// head of the plan from (Ntok, format) WHERE they use it -- before the body, after it, at the queue -- from a token count the compiler cannot see
// through (attn_opaque): the body statement owns all but a few registers, and a plan carried across it does not fit beside the operands.
// kv_ws = [8 queue counters of the sub-items, one per XCD | arrival counter of split q-block (b * H + h) * split + i | ... ATTN_KV_WS_HEAD |
// slot ((b * H + h) * split + i) * S + s, ATTN_KV_SLOT_BYTES each].
struct AttnKv { int whole, split, S; };
__device__ __forceinline__ int attn_opaque(int x) {
    asm volatile("" : "+s"(x));
    return x;
}
template <int FMT>
__device__ __forceinline__ AttnKv attn_kv_of(const AttnArgs& a) {
    const int ntok = attn_opaque(a.Ntok);
    AttnKv kv{(ntok + 255) / 256, 0, 1};
    if (FMT >= 0 && a.kv_ws != nullptr) attn_plan_head(ntok, FMT, kv.whole, kv.split, kv.S);
    return kv;
}
// a work item of the list [whole items | sub-items]: q-block qb of head bh over all KV tiles (part < 0), or over the tiles of part `part`
struct AttnItem { int bh, qb, part; };
__device__ __forceinline__ AttnItem attn_item_of(const AttnKv& kv, int total_whole, int item) {
    AttnItem it;
    if (item < total_whole) {
        it.bh = item / kv.whole; it.qb = item - it.bh * kv.whole; it.part = -1;
    } else {
        const int u = item - total_whole, per = kv.split * kv.S;
        it.bh = u / per;
        const int r = u - it.bh * per, i = r / kv.S;
        it.qb = kv.whole + i; it.part = r - i * kv.S;
    }
    return it;
}

// normalise the 32 rows of row block j by 1 / l_tot and store them: the epilogue of a whole item and of the merge of a split q-block
template <bool P16, bool H16>
__device__ __forceinline__ void attn_qx_store(const AttnArgs& a, int b, int h, const f32x32& OTj, float l_tot, int q_row, int hi) {
    float inv = 1.0f / l_tot;
    if constexpr (P16 && !H16) inv *= __uint_as_float((unsigned)(127 - vt_f16_shift(a.vt_amax[b * a.H + h])) << 23);  // V^T holds V * 2^shift
    u32x2 og[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const int db = g >> 2, rq = g & 3;
        if constexpr (H16) {
            og[g].x = pack2h(OTj[16 * db + rq * 4 + 0] * inv, OTj[16 * db + rq * 4 + 1] * inv);
            og[g].y = pack2h(OTj[16 * db + rq * 4 + 2] * inv, OTj[16 * db + rq * 4 + 3] * inv);
        } else {
            og[g].x = pack2bf(OTj[16 * db + rq * 4 + 0] * inv, OTj[16 * db + rq * 4 + 1] * inv);
            og[g].y = pack2bf(OTj[16 * db + rq * 4 + 2] * inv, OTj[16 * db + rq * 4 + 3] * inv);
        }
    }
    u32x4 vv[4];  // the lane's 8-column groups: columns 16 u + 8 hi .. + 7 of the head, u = 0 .. 3
#pragma unroll
    for (int g = 0; g < 8; g += 2) {
        const auto rx = __builtin_amdgcn_permlane32_swap(og[g].x, og[g + 1].x, false, false);
        const auto ry = __builtin_amdgcn_permlane32_swap(og[g].y, og[g + 1].y, false, false);
        vv[g >> 1] = u32x4{rx[0], ry[0], rx[1], ry[1]};
    }
    const size_t orow = (size_t)(b * a.Ntok + min(q_row, a.Ntok - 1));
    if (a.mx_q == nullptr) {
        bf16_t* o = (bf16_t*)a.out + orow * a.ld_out + h * 64 + hi * 8;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q_row < a.Ntok) *(u32x4*)(o + 16 * u) = vv[u];
    } else {
        // fp8 engine: the out-projection's A operand as MX e4m3 (GemmArgs::mx_a_s) -- a head is two 32-column blocks, each held by
        // the row's two lanes (16 values each): block amax by v_pk_max_u16 + one cross-half exchange, scale = the smallest power
        // of two with amax / scale <= 448, conversion by v_cvt_scalef32_pk_fp8_bf16 (as the FF1 epilogue, gemm_epi.h)
        typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
        unsigned ebs = 0;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            u16x2_t pm = {0, 0};
#pragma unroll
            for (int u = 2 * blk; u < 2 * blk + 2; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) pm = __builtin_elementwise_max(pm, __builtin_bit_cast(u16x2_t, vv[u][e] & 0x7fff7fffu));
            unsigned amb = max((unsigned)pm[0], (unsigned)pm[1]) << 16;
            const auto sw = __builtin_amdgcn_permlane32_swap(amb, amb, false, false);
            amb = max(sw[0], sw[1]);
            unsigned eb = (__float_as_uint(__uint_as_float(amb) * (1.0f / 448.0f)) + 0x7fffffu) >> 23;
            eb = min(max(eb, 1u), 254u);
            ebs |= eb << (8 * blk);
            const float bscale = __uint_as_float(eb << 23);
#pragma unroll
            for (int u = 2 * blk; u < 2 * blk + 2; ++u) {
                unsigned w0 = 0, w1 = 0;
                asm volatile("v_cvt_scalef32_pk_fp8_bf16 %0, %1, %2" : "+v"(w0) : "v"(vv[u][0]), "v"(bscale));
                asm volatile("v_cvt_scalef32_pk_fp8_bf16 %0, %1, %2 op_sel:[0,0,1]" : "+v"(w0) : "v"(vv[u][1]), "v"(bscale));
                asm volatile("v_cvt_scalef32_pk_fp8_bf16 %0, %1, %2" : "+v"(w1) : "v"(vv[u][2]), "v"(bscale));
                asm volatile("v_cvt_scalef32_pk_fp8_bf16 %0, %1, %2 op_sel:[0,0,1]" : "+v"(w1) : "v"(vv[u][3]), "v"(bscale));
                if (q_row < a.Ntok) *(u32x2*)(a.mx_q + orow * a.ld_out + h * 64 + 16 * u + hi * 8) = u32x2{w0, w1};
            }
        }
        if (hi == 0 && q_row < a.Ntok) *(unsigned short*)(a.mx_s + ((size_t)(h >> 1) * a.mx_rows + mx_perm_row((int64_t)orow)) * 4 + (h & 1) * 2) = (unsigned short)ebs;  // K-tile major: head h = blocks 2 h, 2 h + 1 of K-tile h / 2
    }
}

// Merge of a split q-block, run by the workgroup whose part arrived last: every wave merges its own 64 rows from the S slots, ALL of them read
// from memory in the order s = 0 .. S - 1 (its own included), so the sums do not depend on who was last.  With m_s the reference exponent of
// part s (what its exp2 were taken against) and M = max m_s:  O = sum_s 2^(m_s - M) O_s,  l = sum_s 2^(m_s - M) l_s.  A part whose weight
// underflows contributes exactly 0 (its O_s is not multiplied: 0 * inf); equal exponents give weight 1 without a subtraction (inf - inf).
// The slots are read by agent-scope loads: written through by their producers on other XCDs, never served from this XCD's L2.
template <bool P16, bool H16>
__device__ __forceinline__ void attn_qx_merge(const AttnArgs& a, int S, const float* slot0, int b, int h, int wave, int lane, int q_row0) {
    const int hi = lane >> 5;
    constexpr int SLOT = ATTN_KV_SLOT_BYTES / 4;
    auto ld = [](const float* p) __attribute__((always_inline)) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
        const int wj = wave * 2 + j;
        float nmin = INFINITY;  // -M
        for (int s = 0; s < S; ++s) nmin = fminf(nmin, ld(slot0 + (size_t)s * SLOT + 16384 + 512 + wj * 64 + lane));
        f32x32 acc;
#pragma unroll
        for (int e = 0; e < 32; ++e) acc[e] = 0.f;
        float l = 0.f;
#pragma unroll 1
        for (int s = 0; s < S; ++s) {
            const float* sl = slot0 + (size_t)s * SLOT;
            const float nm = ld(sl + 16384 + 512 + wj * 64 + lane);
            const float w = nm == nmin ? 1.0f : __builtin_amdgcn_exp2f(nmin - nm);  // 2^(m_s - M), in [0, 1]
            const float ls = ld(sl + 16384 + wj * 64 + lane);
            l = __builtin_fmaf(w, w == 0.f ? 0.f : ls, l);
#pragma unroll
            for (int e = 0; e < 32; ++e) {
                const float o = ld(sl + (wj * 32 + e) * 64 + lane);
                acc[e] = __builtin_fmaf(w, w == 0.f ? 0.f : o, acc[e]);
            }
        }
        attn_qx_store<P16, H16>(a, b, h, acc, l, q_row0 + 32 * j, hi);
    }
}

// JB = 32-row blocks per wave: 2 = attn_q4 (four waves x 64 rows, one per SIMD), 1 = attn_q8 (eight waves x 32 rows, two per SIMD, the
// same fine-grained stream in both: gen_attn_q4.py)
// F8 (JB = 2 only, attn_q4f): q and k are read as MX e4m3 images (AttnArgs::q8 / k8 + block scales, made by qk_quant_mx_k) and S^T = K.Q^T runs
// on v_mfma_scale_f32_32x32x64_f8f6f4 -- 4 MFMA of 64 cycles per KV tile instead of 16 of 32; V^T, P.V, softmax and the epilogue are the bf16
// kernel's.  No reference code for it (the reference has no fp8 path): parity unpinned, selected only by weight_format 2.
// P16 (JB = 2 only, attn_q4h / attn_q4fh): P and V^T in fp16, row sums by packed fp16 adds, deferred maximum 2^14 (gen_attn_q4.py, P16); the
// code around the body is the same -- the format lives in the V^T buffer (AttnArgs::p16) and in the generated instructions.
// H16 (JB = 2, with P16, not F8: attn_q4hh): the fp16 model dtype -- q, k and the output are fp16 as well; the body is attn_q4h's with its QK^T MFMAs on fp16 (string
// macro Q4H_QK16 around the #include), and the code around it converts q and packs O as fp16.
template <int JB, bool F8 = false, bool P16 = false, bool H16 = false>
__device__ __forceinline__ void attn_qx_item(const AttnArgs& a, int item, char* smem, unsigned& slow_acc, unsigned& tile_acc) {
    constexpr int FMT = JB != 2 ? -1 : F8 ? (P16 ? ATTN_FMT_Q4FH : ATTN_FMT_Q4F) : H16 ? ATTN_FMT_Q4HH : P16 ? ATTN_FMT_Q4H : ATTN_FMT_Q4;
    const AttnKv kv0 = attn_kv_of<FMT>(a);
    const AttnItem it = attn_item_of(kv0, a.B * a.H * kv0.whole, item);
    static_assert((!F8 && !P16) || JB == 2, "the fp8 QK^T and fp16 P bodies exist for the four-wave form only");
    static_assert(!H16 || (P16 && !F8), "fp16 q / k come with fp16 P and bf16-free MFMAs only");
    constexpr int NW = 8 / JB;  // waves per work item
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, hi = lane >> 5;
    const int bh = it.bh, qb = it.qb;
    const int b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * 64;
    // a part of a split q-block runs the body over KV tiles [t0, t0 + nt) as if they were the whole sequence: the K / V^T sources start at
    // tile t0, and the key count the tail mask sees is what is left from there (the fp8-QK^T forms never split: attn_plan)
    const bool part = JB == 2 && !F8 && it.part >= 0;
    const int nt_all = (a.Ntok + KV_TILE - 1) / KV_TILE;
    const int t0 = part ? attn_part_tile(nt_all, kv0.S, it.part) : 0;
    const int nt = part ? attn_part_tile(nt_all, kv0.S, it.part + 1) - t0 : nt_all;
    const int ntok_kv = a.Ntok - KV_TILE * t0;

    const bf16_t* qkv = (const bf16_t*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    const char* Kg = (const char*)(qkv + D + h * 64) + (size_t)t0 * ((size_t)KV_TILE * a.ld_qkv * 2);  // (F8: the e4m3 image, below)
    const char* VTg = (const char*)((const bf16_t*)a.vt + (size_t)(b * a.H + h) * 64 * a.ntok_pad) + (size_t)t0 * (KV_TILE * 2);
    const unsigned lds0 = lds_base_u32(smem);

    // staging: a tile is eight pieces of 8 rows x 128 B; wave w stages piece w (and w + 4 when there are four waves), lane = (row,
    // 16-B chunk), chunk XOR on the SOURCE address ((row + 32) has the same XOR term: the second piece is the lane offset + 32 rows)
    const int srow = wave * 8 + (lane >> 3);
    const int sc = (lane & 7) ^ ((srow >> 1) & 7);
    u32x8 vin;  // [0..3] fragment address of k-step kk in slot 0 (the 32-row half and the slot are immediates), [4..7] staging offsets
    u32x4 kin = {0, 0, 0, 0};  // F8: [0 / 1] LDS address of chunks hi / 2 + hi of key fr in slot 0, [2] the lane's dword of a tile's block scales
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) vin[kk] = lds0 + fr * 128 + (((kk * 2 + hi) ^ ((fr >> 1) & 7)) << 4);
    if constexpr (F8) {
        // e4m3 K tile: 64 keys x 64 B; wave w stages keys 16 w .. 16 w + 15 (one 1-KiB piece), lane = (key, 16-byte position), the chunk XOR
        // ((key >> 2) & 3) on the SOURCE address; a lane's MFMA operand of a 32-key half = chunks hi and 2 + hi of key fr
        Kg = (const char*)a.k8 + (size_t)(b * a.H + h) * a.ntok_pad * 64;
        const int krow = wave * 16 + (lane >> 2);
        kin[0] = lds0 + fr * 64 + (((0 + hi) ^ ((fr >> 2) & 3)) << 4);
        kin[1] = lds0 + fr * 64 + (((2 + hi) ^ ((fr >> 2) & 3)) << 4);
        kin[2] = (unsigned)lane * 4;
        vin[4] = (unsigned)(krow * 64 + (((lane & 3) ^ ((krow >> 2) & 3)) << 4));
        vin[5] = 0;
    } else {
        vin[4] = (unsigned)(2 * (srow * a.ld_qkv + sc * 8));
        vin[5] = vin[4] + 64u * a.ld_qkv;
    }
    vin[6] = (unsigned)(2 * (srow * a.ntok_pad + sc * 8));
    vin[7] = vin[6] + 64u * a.ntok_pad;
    const unsigned k_tile_stride = F8 ? 4096u : (unsigned)KV_TILE * a.ld_qkv * 2;
    const unsigned m0w = lds0 + wave * 1024;  // LDS address of this wave's first piece in slot 0
    // tiles past the end are clamped (re-staged into a dead slot): every wave issues the same number of DMAs in every iteration
    auto k_src = [&](int t) __attribute__((always_inline)) { return Kg + (size_t)min(t, nt - 1) * k_tile_stride; };
    auto v_src = [&](int t) __attribute__((always_inline)) { return VTg + (size_t)min(t, nt - 1) * (KV_TILE * 2); };
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < (F8 ? 1 : JB); ++p) glds16_saddr_m0(k_src(i), vin[4 + p], m0w + i * 16384 + p * 4096);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int p = 0; p < JB; ++p) glds16_saddr_m0(v_src(i), vin[6 + p], m0w + i * 16384 + 8192 + p * 4096);

    // Q fragments of the wave's row blocks, pre-multiplied by scale * log2(e) and rounded to bf16 once (as attn_pp_item); word 16 j + 4 kk
    const float c0 = a.scale * 1.4426950408889634f;
    typedef __attribute__((ext_vector_type((F8 ? 8 : 16) * JB))) unsigned int qf_t;
    qf_t qf;
    int q_row[JB];
    u32x4 ks_ring = {0, 0, 0, 0};  // F8: block scales of K tiles 0 .. 2 (the body loads tile t + 3 in iteration t)
    u32x2 qs = {0, 0};             // F8: block scale of (query row of block j, 32-element block hi) in byte 0
    const char* ksb = nullptr;
#pragma unroll
    for (int j = 0; j < JB; ++j) {
        q_row[j] = qb * 256 + wave * (32 * JB) + j * 32 + fr;
        const int q_ld = min(q_row[j], a.Ntok - 1);
        if constexpr (F8) {  // the image already carries scale * log2(e) (qk_quant_mx_k)
            const size_t qr = (size_t)(b * a.H + h) * a.Ntok + q_ld;
            const u32x4 lo = *(const u32x4*)(a.q8 + qr * 64 + hi * 16), hi4 = *(const u32x4*)(a.q8 + qr * 64 + 32 + hi * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e) { qf[8 * j + e] = lo[e]; qf[8 * j + 4 + e] = hi4[e]; }
            qs[j] = ((unsigned)a.q8s[qr] >> (8 * hi)) & 0xffu;
        } else {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const bf16x8 q = *(const bf16x8*)(qkv + (size_t)q_ld * a.ld_qkv + h * 64 + kk * 16 + hi * 8);
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    if constexpr (H16) {
                        const f16x8 qh = __builtin_bit_cast(f16x8, q);
                        qf[16 * j + 4 * kk + (e >> 1)] = pack2h((float)qh[e] * c0, (float)qh[e + 1] * c0);
                    } else {
                        qf[16 * j + 4 * kk + (e >> 1)] = pack2bf((float)q[e] * c0, (float)q[e + 1] * c0);
                    }
                }
            }
        }
    }
    if constexpr (F8) {
        ksb = (const char*)(a.k8s + (size_t)(b * a.H + h) * (a.ntok_pad / 64) * 64);
#pragma unroll
        for (int i = 0; i < 3; ++i) ks_ring[i] = *(const unsigned*)(ksb + (size_t)min(i, nt - 1) * 256 + lane * 4);
    }
    u32x4 ptr, sin;  // sources of the next K / V^T tile to stage (64-bit each); nt, K tile stride, Ntok, LDS address of the wave's first piece
    {
        const unsigned long long kp = (unsigned long long)k_src(4), vp = (unsigned long long)v_src(2);
        ptr[0] = __builtin_amdgcn_readfirstlane((unsigned)kp); ptr[1] = __builtin_amdgcn_readfirstlane((unsigned)(kp >> 32));
        ptr[2] = __builtin_amdgcn_readfirstlane((unsigned)vp); ptr[3] = __builtin_amdgcn_readfirstlane((unsigned)(vp >> 32));
        sin[0] = (unsigned)nt; sin[1] = k_tile_stride; sin[2] = (unsigned)ntok_kv; sin[3] = m0w;
    }
    f32x32 OT[JB];  // ot(j, db)[e] = OT[j][16 db + e]
    f32x2 LR;
    float NM[JB];   // -m of the lane's row of block j: the exponent OT and LR are relative to (used by the parts of a split q-block)
    unsigned slow_cnt;  // slow paths this wave took (diagnostics)

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (F8) {
        u32x2 ksbp;
        ksbp[0] = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)ksb);
        ksbp[1] = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)ksb >> 32));
        if constexpr (P16) {
            asm volatile(
#include "attn_q4fh_body.inc"
                : "=" Q4FH_OT0(OT[0]), "=" Q4FH_OT1(OT[JB - 1]), "=" Q4FH_LRUN(LR), "=" Q4FH_NEGM0(NM[0]), "=" Q4FH_NEGM1(NM[JB - 1]), "+" Q4FH_PTR(ptr), "=" Q4FH_CNT(slow_cnt), "+" Q4FH_KS(ks_ring)
                : Q4FH_QF(qf), Q4FH_VIN(vin), Q4FH_SIN(sin), Q4FH_QS(qs), Q4FH_KIN(kin), Q4FH_KSB(ksbp)
                : Q4FH_CLOBBERS);
        } else {
            asm volatile(
#include "attn_q4f_body.inc"
                : "=" Q4F_OT0(OT[0]), "=" Q4F_OT1(OT[JB - 1]), "=" Q4F_LRUN(LR), "=" Q4F_NEGM0(NM[0]), "=" Q4F_NEGM1(NM[JB - 1]), "+" Q4F_PTR(ptr), "=" Q4F_CNT(slow_cnt), "+" Q4F_KS(ks_ring)
                : Q4F_QF(qf), Q4F_VIN(vin), Q4F_SIN(sin), Q4F_QS(qs), Q4F_KIN(kin), Q4F_KSB(ksbp)
                : Q4F_CLOBBERS);
        }
    } else if constexpr (H16) {
#define Q4H_QK16 "f16"
        asm volatile(
#include "attn_q4h_body.inc"
            : "=" Q4H_OT0(OT[0]), "=" Q4H_OT1(OT[JB - 1]), "=" Q4H_LRUN(LR), "=" Q4H_NEGM0(NM[0]), "=" Q4H_NEGM1(NM[JB - 1]), "+" Q4H_PTR(ptr), "=" Q4H_CNT(slow_cnt)
            : Q4H_QF(qf), Q4H_VIN(vin), Q4H_SIN(sin)
            : Q4H_CLOBBERS);
#undef Q4H_QK16
    } else if constexpr (P16) {
#define Q4H_QK16 "bf16"
        asm volatile(
#include "attn_q4h_body.inc"
            : "=" Q4H_OT0(OT[0]), "=" Q4H_OT1(OT[JB - 1]), "=" Q4H_LRUN(LR), "=" Q4H_NEGM0(NM[0]), "=" Q4H_NEGM1(NM[JB - 1]), "+" Q4H_PTR(ptr), "=" Q4H_CNT(slow_cnt)
            : Q4H_QF(qf), Q4H_VIN(vin), Q4H_SIN(sin)
            : Q4H_CLOBBERS);
#undef Q4H_QK16
    } else if constexpr (JB == 2) {
        asm volatile(
#include "attn_q4_body.inc"
            : "=" Q4_OT0(OT[0]), "=" Q4_OT1(OT[JB - 1]), "=" Q4_LRUN(LR), "=" Q4_NEGM0(NM[0]), "=" Q4_NEGM1(NM[JB - 1]), "+" Q4_PTR(ptr), "=" Q4_CNT(slow_cnt)
            : Q4_QF(qf), Q4_VIN(vin), Q4_SIN(sin)
            : Q4_CLOBBERS);
    } else {
        asm volatile(
#include "attn_q8_body.inc"
            : "=" Q8_OT0(OT[0]), "=" Q8_LRUN(LR), "=" Q8_NEGM0(NM[0]), "+" Q8_PTR(ptr), "=" Q8_CNT(slow_cnt)
            : Q8_QF(qf), Q8_VIN(vin), Q8_SIN(sin)
            : Q8_CLOBBERS);
    }

    slow_acc += slow_cnt;   // census of this wave over its items (AttnArgs::stats), reported once per kernel
    tile_acc += (unsigned)nt;
#ifdef S2V_DIAG
    if (lane == 0) {  // slow-path census of tools/attn_harness: (wave, tile) pairs that took the slow path / that ran
        atomicAdd(&g_qx_slow[0], (unsigned long long)slow_cnt);
        atomicAdd(&g_qx_slow[1], (unsigned long long)nt);
    }
#endif
    if constexpr (JB == 2 && !F8) {
        if (part) {
            // a part of a split q-block: (O^T unnormalised, l, -m) -> its slot in the register layout, written through to device scope; the
            // workgroup whose part arrives last (agent-scope fetch-add, as the split-K hand-over of gemm_g4) merges the S slots.  Nobody waits.
            const AttnKv kv = attn_kv_of<FMT>(a);  // recomputed: see AttnKv
            const int blk = bh * kv.split + (qb - kv.whole);
            unsigned* cnt = (unsigned*)a.kv_ws + 8 + blk;
            float* slot0 = (float*)((char*)a.kv_ws + ATTN_KV_WS_HEAD) + (size_t)blk * kv.S * (ATTN_KV_SLOT_BYTES / 4);
            float* sl = slot0 + (size_t)it.part * (ATTN_KV_SLOT_BYTES / 4);
            auto stw = [](float* p, float v) __attribute__((always_inline)) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                const int wj = wave * 2 + j;
#pragma unroll
                for (int e = 0; e < 32; ++e) stw(sl + (wj * 32 + e) * 64 + lane, OT[j][e]);
                stw(sl + 16384 + wj * 64 + lane, LR[j] + __shfl_xor(LR[j], 32, 64));
                stw(sl + 16384 + 512 + wj * 64 + lane, NM[j]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the slot is in memory before the arrival is counted
            __syncthreads();
            unsigned* flag = (unsigned*)smem;  // every wave is past the body: the ring is free
            if (tid == 0) *flag = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const bool last = *flag == (unsigned)(kv.S - 1);
            __syncthreads();  // flag is read by everyone before the next item stages into the ring
            if (!last) return;
            if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the next launch finds zero
            attn_qx_merge<P16, H16>(a, kv.S, slot0, b, h, wave, lane, q_row[0]);
            return;
        }
    }
    // epilogue: as attn_pp_item, once per row block
#pragma unroll
    for (int j = 0; j < JB; ++j) attn_qx_store<P16, H16>(a, b, h, OT[j], LR[j] + __shfl_xor(LR[j], 32, 64), q_row[j], hi);
}
// one pair of atomics per wave and KERNEL (the persistent launch: 1024 per launch, on 256 distinct slots)
__device__ __forceinline__ void attn_report(const AttnArgs& a, unsigned slow, unsigned tiles) {
    if (a.stats != nullptr && (threadIdx.x & 63) == 0) {
        unsigned long long* s = a.stats + 2 * (blockIdx.x & 255);
        atomicAdd(s, (unsigned long long)slow);
        atomicAdd(s + 1, (unsigned long long)tiles);
    }
}
// Both launch forms run the same item list [whole items | sub-items]: B * H * whole whole items (q-block qb < whole of head bh: item bh * whole + qb),
// then the B * H * split * S parts of the split q-blocks (attn_item_of).
template <int JB, bool F8 = false, bool P16 = false, bool H16 = false>
__global__ __launch_bounds__(64 * (8 / JB), 1) void attn_qx_k(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [4 slots][K tile | VT tile]
    int first, cnt;
    clk_stamp(a.clk, gridDim.x >> 1, 0);
    attn_xcd_range((int)gridDim.x, blockIdx.x & 7, first, cnt);
    unsigned slow = 0, tiles = 0;
    attn_qx_item<JB, F8, P16, H16>(a, first + (int)(blockIdx.x >> 3), smem, slow, tiles);
    attn_report(a, slow, tiles);
    clk_stamp(a.clk, gridDim.x >> 1, 1);
}
template <int JB, bool F8 = false, bool P16 = false, bool H16 = false>
__global__ __launch_bounds__(64 * (8 / JB), 1) void attn_qx_persist_k(const AttnArgs a, int* __restrict__ queue) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_item;
    const int xcd = blockIdx.x & 7;
    constexpr int FMT = JB != 2 ? -1 : F8 ? (P16 ? ATTN_FMT_Q4FH : ATTN_FMT_Q4F) : H16 ? ATTN_FMT_Q4HH : P16 ? ATTN_FMT_Q4H : ATTN_FMT_Q4;
    unsigned slow = 0, tiles = 0;
    clk_stamp(a.clk, 0, 0);  // persistent: workgroup 0 pulls work until the queues are empty
    // Start stagger (round 5, configs[4] locality experiment): the 32 workgroups of an XCD walk consecutive q-blocks of one head, i.e. the SAME
    // K / V^T tiles, and every item costs the same -- started together they request each tile within the latency of its first miss.  With
    // a.stagger > 0 slot s of the XCD starts s * stagger * 64 cycles late, once per launch: a convoy in which the leader misses in L2 and the
    // followers find the tile there.  0 = start together (the default; profiles/r05_attn_stagger.txt for what it measured: slower).  The
    // diagnostics build only: the product kernel carries neither this knob nor the a.order experiment below.
#ifdef S2V_DIAG
    if (a.stagger > 0) {
        const int slot = (int)(blockIdx.x >> 3);
        for (int i = 0; i < slot * a.stagger; i += 64) __builtin_amdgcn_s_sleep(64);
        if ((slot * a.stagger) & 63) __builtin_amdgcn_s_sleep(1);
    }
#endif
    for (;;) {
        if (threadIdx.x == 0) {
            // long items first, short items last: every whole item (the own XCD's, then stolen ones) before any sub-item (the own XCD's share first)
            const AttnKv kv = attn_kv_of<FMT>(a);  // recomputed per item: see AttnKv
            const int nqb = kv.whole, total = a.B * a.H * nqb, nsub = a.B * a.H * kv.split * kv.S;  // whole q-blocks per head, whole items, sub-items
            int* subq = (int*)a.kv_ws;
            int wg = -1;
            for (int k = 0; k < 8 && wg < 0; ++k) {
                const int y = (xcd + k) & 7;
                int first, cnt;
                // a.order 0: XCD y owns a contiguous range of items (a head's q-blocks stay on one XCD); 1 (experiment, round 5): a head's q-blocks
                // are dealt round-robin over the XCDs (q-block qb on XCD qb & 7), so all 32 workgroups of an XCD are on the SAME head at any time
#ifdef S2V_DIAG
                const bool dealt = a.order != 0;
#else
                constexpr bool dealt = false;
#endif
                const int per = dealt ? (nqb > y ? (nqb - y + 7) >> 3 : 0) : 0;
                if (dealt) { first = 0; cnt = (total / nqb) * per; }
                else attn_xcd_range(total, y, first, cnt);
                if (__hip_atomic_load(&queue[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= cnt) continue;
                const int i = atomicAdd(&queue[y], 1);
                if (i < cnt) {
#ifdef S2V_DIAG
                    if (dealt) { const int bh = i / per, j = i - bh * per; wg = bh * nqb + y + 8 * j; }
                    else
#endif
                        wg = first + i;
                }
            }
            for (int k = 0; k < 8 && wg < 0 && nsub > 0; ++k) {
                const int y = (xcd + k) & 7;
                int first, cnt;
                attn_xcd_range(nsub, y, first, cnt);  // contiguous: the parts of a head's split q-blocks stay on the XCD that ran most of the head
                if (__hip_atomic_load(&subq[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= cnt) continue;
                const int i = atomicAdd(&subq[y], 1);
                if (i < cnt) wg = total + first + i;
            }
            s_item = wg;
        }
        __syncthreads();
        const int wg = s_item;
        __syncthreads();
        if (wg < 0) break;
        attn_qx_item<JB, F8, P16, H16>(a, wg, smem, slow, tiles);
    }
    attn_report(a, slow, tiles);
    clk_stamp(a.clk, 0, 1);
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&queue[8], 1) == (int)gridDim.x - 1) {
            for (int i = 0; i < 9; ++i) __hip_atomic_store(&queue[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int i = 0; i < 8 && a.kv_ws != nullptr; ++i) __hip_atomic_store((int*)a.kv_ws + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
        }
    }
}

#ifdef S2V_DIAG
// operator-level A/B and the "rows of whole q-blocks keep their bits" test: 1 = every four-wave launch runs whole items only.  The product
// library carries no such knob.
static int g_attn_kv_nosplit = 0;
extern "C" __attribute__((visibility("default"))) int s2v_diag_attn_kv_nosplit(int on) { g_attn_kv_nosplit = on; return 0; }
// attn_plan without a device (tests/test_attn_plan_cpu.py): format = ATTN_FMT_*; out = [whole, split, S, ATTN_KV_MIN_TILES, t[0] .. t[ATTN_KV_PARTS]]
// (4 + ATTN_KV_PARTS + 1 ints, -1 past t[S]).  The arguments of attn_plan are these two and nothing else.
extern "C" __attribute__((visibility("default"))) int s2v_diag_attn_plan(int32_t Ntok, int32_t format, int32_t* out) {
    S2V_REQUIRE(out && Ntok > 0, "s2v_diag_attn_plan: bad argument");
    const AttnPlan p = attn_plan(Ntok, format);
    out[0] = p.whole; out[1] = p.split; out[2] = p.S; out[3] = ATTN_KV_MIN_TILES;
    for (int s = 0; s <= ATTN_KV_PARTS; ++s) out[4 + s] = s <= p.S ? p.t[s] : -1;
    return 0;
}
#endif

// the process-wide split workspace of launches whose caller brought none (operator entries; as their magnitude words: one per process, on the
// device of the first such call, never under capture -- growing it allocates)
static void* g_kv_ws = nullptr;
static int64_t g_kv_ws_bytes = 0;
static int attn_kv_process_ws(int64_t need, void** ws) {
    if (g_kv_ws_bytes < need) {
        if (g_kv_ws) { S2V_CHECK_HIP(hipDeviceSynchronize()); S2V_CHECK_HIP(hipFree(g_kv_ws)); g_kv_ws = nullptr; g_kv_ws_bytes = 0; }
        S2V_CHECK_HIP(hipMalloc(&g_kv_ws, need));
        S2V_CHECK_HIP(hipMemset(g_kv_ws, 0, ATTN_KV_WS_HEAD));
        g_kv_ws_bytes = need;
    }
    *ws = g_kv_ws;
    return 0;
}
#ifdef S2V_DIAG
// the counters of the process-wide workspace after the launches so far (synchronises): how many of its sub-item queue and arrival counters are
// not zero -- every launch must leave all of them at zero; bytes = the size it has grown to (0: no launch has split yet)
extern "C" __attribute__((visibility("default"))) int s2v_diag_attn_kv_counters(int32_t* nonzero, int64_t* bytes) {
    S2V_REQUIRE(nonzero && bytes, "s2v_diag_attn_kv_counters: null argument");
    *nonzero = 0; *bytes = g_kv_ws_bytes;
    if (!g_kv_ws) return 0;
    static int32_t head[ATTN_KV_WS_HEAD / 4];
    S2V_CHECK_HIP(hipDeviceSynchronize());
    S2V_CHECK_HIP(hipMemcpy(head, g_kv_ws, ATTN_KV_WS_HEAD, hipMemcpyDeviceToHost));
    for (int i = 0; i < ATTN_KV_WS_HEAD / 4; ++i) *nonzero += head[i] != 0;
    return 0;
}
#endif

template <int JB, bool F8 = false, bool P16 = false, bool H16 = false>
static int launch_attn_qx(const AttnArgs& a_in, bool persistent, hipStream_t st) {
    // 256 query rows per item in both forms; attn_plan alone decides which q-blocks are cut by key range (never for the eight-wave form)
    constexpr int fmt = JB != 2 ? -1 : F8 ? (P16 ? ATTN_FMT_Q4FH : ATTN_FMT_Q4F) : H16 ? ATTN_FMT_Q4HH : P16 ? ATTN_FMT_Q4H : ATTN_FMT_Q4;
    AttnArgs a = a_in;
    AttnPlan p = attn_plan(a.Ntok, fmt);
#ifdef S2V_DIAG
    if (g_attn_kv_nosplit) p = attn_plan(a.Ntok, -1);
#endif
    const int64_t BH = (int64_t)a.B * a.H;
    if (p.split) {
        S2V_REQUIRE(BH <= ATTN_KV_MAX_BH, "attn_q4: B * heads too large for the KV-split counters");
        const int64_t need = attn_kv_ws_bytes(p, BH);
        if (a.kv_ws) S2V_REQUIRE(a.kv_ws_bytes >= need, "attn_q4: AttnArgs::kv_ws is smaller than attn_kv_ws_bytes of this launch");
        else S2V_TRY(attn_kv_process_ws(need, &a.kv_ws));
    } else {
        a.kv_ws = nullptr;  // the kernels read "no split" from it
    }
    const int total = p.whole * a.B * a.H;  // whole items
    const int nsub = (int)BH * p.split * p.S;
    const size_t lds = 65536;
    const dim3 blk(64 * (8 / JB));
    if (persistent && a.queue != nullptr && a.num_cus >= 8) {
        const void* fn = (const void*)attn_qx_persist_k<JB, F8, P16, H16>;
        S2V_TRY(ensure_lds_attr(fn, 65536));
        int* queue = a.queue;
        void* args[] = {(void*)&a, (void*)&queue};
        S2V_CHECK_HIP(hipLaunchKernel(fn, dim3((a.num_cus / 8) * 8), blk, args, lds, st));
        return 0;
    }
    const void* fn = (const void*)attn_qx_k<JB, F8, P16, H16>;
    S2V_TRY(ensure_lds_attr(fn, 65536));
    void* args[] = {(void*)&a};
    S2V_CHECK_HIP(hipLaunchKernel(fn, dim3(total + nsub), blk, args, lds, st));
    return 0;
}
int launch_attn_q4(const AttnArgs& a, bool persistent, hipStream_t st) { return launch_attn_qx<2>(a, persistent, st); }
int launch_attn_q8(const AttnArgs& a, bool persistent, hipStream_t st) { return launch_attn_qx<1>(a, persistent, st); }
int launch_attn_q4f(const AttnArgs& a, bool persistent, hipStream_t st) {
    S2V_REQUIRE(a.q8 && a.k8 && a.q8s && a.k8s && a.vt, "attn_q4f: the MX images of q / k (launch_qk_quant_mx) and V^T are required");
    S2V_REQUIRE(!a.p16 || a.vt_amax, "attn_q4f: fp16 P needs the magnitude words of the fp16 V^T (launch_v_transpose(..., vt_amax))");
    return a.p16 ? launch_attn_qx<2, true, true>(a, persistent, st) : launch_attn_qx<2, true>(a, persistent, st);
}
// fp16 model dtype: qkv / out fp16, a.vt = fp16 V^T (the transpose pass moves the bits); the four-wave kernel with fp16 q, k, P
int launch_attn_q4hh(const AttnArgs& a, bool persistent, hipStream_t st) {
    S2V_REQUIRE(a.vt && a.mx_q == nullptr, "attn_q4hh: the fp16 V^T is required (and no MX output)");
    return launch_attn_qx<2, false, true, true>(a, persistent, st);
}
int launch_attn_q4h(const AttnArgs& a, bool persistent, hipStream_t st) {
    S2V_REQUIRE(a.p16 && a.vt && a.vt_amax, "attn_q4h: the fp16 V^T and its magnitude words (launch_v_transpose(..., vt_amax)) are required");
    return launch_attn_qx<2, false, true>(a, persistent, st);
}
