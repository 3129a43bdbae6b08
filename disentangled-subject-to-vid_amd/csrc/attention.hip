// Joint [text | ref-image | video] self-attention, head_dim 64, no mask
// (replaces F.scaled_dot_product_attention at attention_processor.py:2083-2087).
//
//  The bf16 product kernel is attn_q4 (attention_q4.hip: four waves, one per SIMD, generated asm): launch_attn_bf16 below dispatches to
//     it -- one workgroup per 256-row q-block (op-level launches) or one persistent workgroup per CU pulling q-blocks from per-XCD
//     queues (the engine's launches).  What follows in this file is compiled into the DIAGNOSTICS library only, as A/B references:
//  attn_pp_k / attn_pp_persist_k : the round-2 product kernel, flash-attention forward on v_mfma_f32_32x32x16_bf16, eight waves in a
//     two-group ping-pong (below); same launch forms; 5-6 % slower than attn_q4 on the same box (profiles/r03_attn_harness.txt).
//     block = 8 waves x 32 query rows; KV tile = 64 keys; K tile [64 kv][64 d] and V^T tile [64 d][64 kv] are staged with
//     LDS-DMA (global_load_lds) into a ring of XOR-swizzled LDS slots (same image as gemm.hip).
//     QK^T is issued swapped (S^T = K . Q^T) so every lane owns ONE query row: row max / row sum / rescale are
//     lane-local (one cross-half exchange per tile).  P^T feeds the PV MFMA straight from the S^T accumulator
//     registers: the MFMA k-slot <-> key assignment is free, so V^T is stored in HBM with the keys of every
//     16-group permuted [0-3, 8-11, 4-7, 12-15] (done by qk_norm_rope) and no lane exchange is needed.
//     O^T = V^T . P^T accumulates with the query again on the lane axis.
//     Softmax in the exp2 domain: Q is pre-multiplied by scale * log2(e) and the S^T accumulators start at -m_run (a
//     loop-carried register block), so p = exp2(MFMA result) with no per-score fma.
//  attn_pp_steer_k / attn_pp_steer_persist_k : attn_pp_item<ACCT, STEER = true> in the same two launch forms -- attention steering, a logit bias
//     log2 w on up to four key ranges (kernels.h AttnSteerRec; include/s2v_hip.h "Attention steering"); what a steered layer of a bf16 engine
//     runs at every length.  attn_simple_steer_k<T>: the same bias in the generic kernel (fp32 engines, and the cross-check).
//  attn_pp_steer_map_k / attn_pp_steer_map_persist_k : attn_pp_item<.., MAP = true> -- steering maps, the same bias with a weight per query row
//     (log2 W_p[row - q0], kernels.h AttnSteerMapRec) and a liveness bit per wave and range from the host; attn_simple_steer_map_k<T>: the generic twin.
//  attn_pp_local_k / attn_pp_local_persist_k : attn_pp_item<ACCT, STEER, LOCAL = true> in the same two launch forms -- local attention in time:
//     row i sees the keys [0, P) and [lo_i, hi_i); an item visits only the key tiles some row of it sees (kernels.h "local attention";
//     include/s2v_hip.h "Local attention"); what a local layer of a bf16 engine runs at every length.  attn_simple_local_k<T>: the same mask
//     in the generic kernel (fp32 engines, and the cross-check).
//  attn_pp_box_k / attn_pp_box_persist_k : attn_pp_item<ACCT, STEER, LOCAL, BOX = true> in the same two launch forms -- local attention in space and
//     time: row i sees [0, P) and the keys of [lo_i, hi_i) whose offset in their frame lies in [olo_i, ohi_i); an item visits the tiles of a list the
//     host made (kernels.h "local attention in space and time"; include/s2v_hip.h).  attn_simple_box_k<T>: the same mask in the generic kernel.
//  attn_bf16_k (S2V_DIAG builds only): the round-1 lock-step kernel with a per-tile row maximum, kept as the A/B reference.
//  attn_simple_k<T> : one wave per query row, fp32 math, any dtype (CPU-reference-parity mode / cross-check).
#define S2V_HOST
#include "common.h"
#include "kernels.h"
#include <type_traits>

#define KV_TILE 64
#define Q_BLOCK 128
#define ATT_TILE_BYTES (64 * 64 * 2)  // 8 KiB
#ifndef ATTN_PP_MAX_TOKENS
#define ATTN_PP_MAX_TOKENS 4608  // launch_attn_bf16: sequences up to this length run attn_pp, longer ones attn_q4 (profiles/r03_attn_short_sequences.txt:
                                 // attn_pp 9 % ahead at 4000 tokens, attn_q4 2 % ahead at 6000, 6 % at 19126)
#endif

// v_max3_f32 written out so that the max tree keeps the order it is given (the scores are never NaN: no canonicalisation)
__device__ __forceinline__ float max3f(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// ---- the lock-step kernel: A/B reference in bf16 (diagnostics library), the fp16 model dtype's attention in the product (T16 = f16_t) ----
template <int NT>
__device__ __forceinline__ void stage64(const bf16_t* __restrict__ g, size_t ld, char* lds, int tid) {
    // 64 rows x 128 B; 512 chunks of 16 B; 512 / NT rounds of NT threads.  The address is written as
    // (wave-uniform tile base) + zext(32-bit lane offset) so the LDS-DMA can take the saddr + voffset form
    const int wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 512 / NT; ++i) {
        const int gi = i * NT + tid;
        const int row = gi >> 3;
        const int cp = gi & 7;
        const int c = cp ^ ((row >> 1) & 7);
        const unsigned off = (unsigned)(2 * ((unsigned)row * (unsigned)ld + c * 8));
        const char* src = (const char*)g + (size_t)off;
        char* dst = lds + (i * NT + wave * 64) * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
}
template <int NW>
__device__ __forceinline__ void stage_kv(const bf16_t* __restrict__ kg, size_t ldk, const bf16_t* __restrict__ vg, size_t ldv,
                                         char* lds, int tid) {
    stage64<NW * 64>(kg, ldk, lds, tid);
    stage64<NW * 64>(vg, ldv, lds + ATT_TILE_BYTES, tid);
}
__device__ __forceinline__ bf16x8 frag64(const char* tile, int row, int cl) {
    return *(const bf16x8*)(tile + row * 128 + ((cl ^ ((row >> 1) & 7)) << 4));
}

// round-1 lock-step kernel (A/B reference of tools/attn_harness); ABL is unused.
// T16 = f16_t (round 5): the attention of the fp16 model dtype (src/inference.py:191) -- q, k, V^T and P in fp16 on v_mfma_f32_32x32x16_f16, output
// fp16.  This kernel takes a true per-tile row maximum, so p <= 1 and nothing can leave the fp16 range; staging, swizzle and fragment reads move
// 16-bit elements whatever they encode.  ~1 PFLOP/s at C3 in bf16 (9.2-9.4 ms, profiles/r02_attn_harness.txt): not the tuned asm kernel, but an
// order of magnitude above the fp32-pipe kernel the fp16 dtype started on.
template <int ABL, int NW = 8, typename T16 = bf16_t>
__global__ __launch_bounds__(NW * 64, 2) void attn_bf16_k(const AttnArgs a, int nqb) {
    constexpr bool H16 = std::is_same<T16, f16_t>::value;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][K tile | VT tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, hi = lane >> 5;

    // XCD-aware order: all q-blocks of one (b,h) run on one XCD so its K/V stay in that XCD's L2
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int qq = nwg >> 3, rr = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    const int wg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
    const int bh = wg / nqb, qb = wg - bh * nqb;
    const int b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * 64;

    const bf16_t* qkv = (const bf16_t*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    const bf16_t* Kg = qkv + D + h * 64;
    const bf16_t* VTg = (const bf16_t*)a.vt + (size_t)(b * a.H + h) * 64 * a.ntok_pad;

    // Q fragments (B operand of S^T = K.Q^T): lane (q = fr, hi) holds Q[q][16kk + 8hi .. +8], pre-multiplied by
    // scale * log2(e) and rounded to bf16 once (the reference's math path rounds its scaled q and k to bf16 as well), so the
    // MFMA result is already the exp2 argument
    const int q_row = qb * (NW * 32) + wave * 32 + fr;
    const int q_ld = min(q_row, a.Ntok - 1);
    const float c0 = a.scale * 1.4426950408889634f;
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        qf[kk] = *(const bf16x8*)(qkv + (size_t)q_ld * a.ld_qkv + h * 64 + kk * 16 + hi * 8);
        if constexpr (H16) {
            f16x8 qh = __builtin_bit_cast(f16x8, qf[kk]);
#pragma unroll
            for (int e = 0; e < 8; ++e) qh[e] = (_Float16)((float)qh[e] * c0);
            qf[kk] = __builtin_bit_cast(bf16x8, qh);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[kk][e] = (__bf16)((float)qf[kk][e] * c0);
        }
    }
    auto mfma16 = [](bf16x8 x, bf16x8 y, f32x16 acc) __attribute__((always_inline)) {
        if constexpr (H16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, x), __builtin_bit_cast(f16x8, y), acc, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, acc, 0, 0, 0);
    };

    f32x16 ot[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) ot[i][e] = 0.f;
    // the S^T accumulators START at -m_run: this 16-register block is loop-carried and only rewritten when a row maximum
    // grows, so in the steady state a score costs exp2 + add (+ half a cvt_pk) and no fma
    f32x16 negm16;
#pragma unroll
    for (int e = 0; e < 16; ++e) negm16[e] = 0.f;
    float m_run = 0.f, l_run = 0.f;

    const int nt = (a.Ntok + KV_TILE - 1) / KV_TILE;
    stage_kv<NW>(Kg, a.ld_qkv, VTg, a.ntok_pad, smem, tid);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const int cur = t & 1;
        const int kv0 = t * KV_TILE;
        if (t + 1 < nt) {
            char* nb = smem + (cur ^ 1) * 2 * ATT_TILE_BYTES;
            stage_kv<NW>(Kg + (size_t)(kv0 + KV_TILE) * a.ld_qkv, a.ld_qkv, VTg + kv0 + KV_TILE, a.ntok_pad, nb, tid);
        }
        const char* tK = smem + cur * 2 * ATT_TILE_BYTES;
        const char* tV = tK + ATT_TILE_BYTES;

        // S^T[kv][q] - m_run for two 32-key blocks
        f32x16 st[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            st[kb] = mfma16(frag64(tK, kb * 32 + fr, hi), qf[0], negm16);
#pragma unroll
            for (int kk = 1; kk < 4; ++kk) st[kb] = mfma16(frag64(tK, kb * 32 + fr, kk * 2 + hi), qf[kk], st[kb]);
        }
        if (kv0 + KV_TILE > a.Ntok) {  // tail tile: mask keys >= Ntok
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int kv = kv0 + kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hi;
                    if (kv >= a.Ntok) st[kb][e] = -INFINITY;
                }
        }
        float mx = st[0][0];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (ABL != 3) mx = fmaxf(mx, st[kb][e]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // (row max of this tile) - m_run
        // The first tile adopts its own maximum (m_run starts at 0); later tiles only raise it, and the branch is skipped
        // exactly when no row of the wave grew (alpha == 1 for every lane).
        if (t == 0 || __any(mx > 0.f)) {
            const float d = (t == 0) ? mx : fmaxf(mx, 0.f);
            // t == 0: O and l are still zero, and exp2(-d) would overflow to inf (0 * inf = NaN) for scores below -128
            const float alpha = (t == 0) ? 1.0f : __builtin_amdgcn_exp2f(-d);
            m_run += d;
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) ot[i][e] *= alpha;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) st[kb][e] -= d;
#pragma unroll
            for (int e = 0; e < 16; ++e) negm16[e] = -m_run;
        }
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = (ABL == 1) ? st[kb][e] : __builtin_amdgcn_exp2f(st[kb][e]);
                st[kb][e] = p;
                if (ABL != 2) psum += p;
            }
        l_run += psum;

        // O^T[d][q] += V^T[d][kv] . P^T[kv][q]; k-step s covers keys 16s..16s+15 of the tile
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kb = s >> 1, r0 = (s & 1) * 8;
            bf16x8 pf;
            if constexpr (H16) {
                f16x8 ph;
#pragma unroll
                for (int e = 0; e < 8; ++e) ph[e] = (_Float16)st[kb][r0 + e];
                pf = __builtin_bit_cast(bf16x8, ph);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = (__bf16)st[kb][r0 + e];
            }
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                bf16x8 vf = frag64(tV, db * 32 + fr, s * 2 + hi);
                ot[db] = mfma16(vf, pf, ot[db]);
            }
        }
        __syncthreads();
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (q_row < a.Ntok) {
        bf16_t* o = (bf16_t*)a.out + (size_t)(b * a.Ntok + q_row) * a.ld_out + h * 64;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int d = db * 32 + 8 * rq + 4 * hi;
                u32x2 p;
                if constexpr (H16) {
                    p.x = pack2h(ot[db][rq * 4 + 0] * inv, ot[db][rq * 4 + 1] * inv);
                    p.y = pack2h(ot[db][rq * 4 + 2] * inv, ot[db][rq * 4 + 3] * inv);
                } else {
                    p.x = pack2bf(ot[db][rq * 4 + 0] * inv, ot[db][rq * 4 + 1] * inv);
                    p.y = pack2bf(ot[db][rq * 4 + 2] * inv, ot[db][rq * 4 + 3] * inv);
                }
                *(u32x2*)(o + d) = p;
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// attn_pp_k: 8-wave PING-PONG flash attention.  Waves w and w + 4 share a SIMD; group A = waves 0-3, group B = waves 4-7, one
// barrier interval apart.  Every interval one group is in its MATRIX segment M(t+1) (QK^T of tile t+1, P.V of tile t) while
// its SIMD partner is in its SOFTMAX segment S(t).
//
// What shapes the split (tools/probes/valu_rate.hip, MI355X): a wave issues plain VALU every 4.9 cycles and v_exp_f32 every 8.9
// on its own, but beside a partner that streams v_mfma_f32_32x32x16_bf16 back to back the SIMD grants the partner one VALU
// per 16 cycles (exp2 or not, any priority, either wave older); (exp2, exp2, add, add) per MFMA is the densest partner stream
// that still fits (33 cycles per MFMA), and the MFMA wave can place two plain VALU of its own behind each MFMA.  Head
// dimension 64 needs 32 exp2 per 16 MFMA, so the softmax is cut down to what those slots hold:
//   * NO per-tile row maximum.  The running maximum is adopted from the first tile; afterwards a tile only checks its row
//     SUMS (psum > 2^13, wave-wide vote) and takes the slow path -- true row max, rescale of O and l, exp2 again -- when some
//     p exceeded ~2^8 (deferred maximum: p stays far inside the fp32 / bf16 range, the result is the same up to rounding);
//   * S(t): 32 exp2 + 32 row-sum adds as 16 (exp2, exp2, add, add) groups, the vote, the wait for this wave's LDS-DMA;
//   * M(t+1): per MFMA one fragment read; the 16 v_cvt_pk (bf16 packing of P) behind the 8 QK^T MFMAs, the K fragments of
//     tile t+2 behind the 8 P.V MFMAs, and the wave's two LDS-DMA pieces AFTER its last MFMA (an LDS-DMA instruction keeps its
//     wave from issuing for 60-100 cycles: between MFMAs that is a bubble of the matrix pipe, after them it is barrier slack).
// Phases (one per barrier): A runs M(t) in phase 2t and S(t) in phase 2t+1, B one phase later.
// LDS ring of 4 slots x [K tile 8 KiB | V^T tile 8 KiB]; in M(t+1) every wave issues ONE K piece (8 rows) of tile t+4 and ONE
// V^T piece of tile t+2 and waits for them (vmcnt(0)) at the end of S(t+1):
//   RAW  K(t+4): A's pieces land by the end of phase 2t+3, B's by 2t+4; first read (fragment prefetch in M(t+3)) in phase 2t+6.
//        V(t+2): first read in M(t+3) = phase 2t+6.
//   WAR  K(t+4) replaces K(t), last read in phase 2t-1 (B's M(t-1) prefetch; K(0) and K(1): M(0), phases 0-1); first write in
//        phase 2t+2.  V(t+2) replaces V(t-2), last read by B's M(t-1) in phase 2t-1.
// Measured at C3 (B 2, H 48, N 19126; tools/attn_harness): 8.1 ms against 9.2-9.4 for the lock-step kernel; variants that
// lost the A/B (kept out of the tree): row sums with v_pk_add_f32 (+5 %), no s_setprio in M (+6 %), LDS-DMA between the P.V
// MFMAs (+3 %) or in S (+4 %), dedicated loader waves (three waves per SIMD force 168 registers and drop the fragment
// prefetch: +2 %), bounded scores with no maximum at all and the row sums on the matrix pipe (20 MFMA per tile: -1.5 %, not
// worth its precondition).
// (attn_pp below: the bf16 short-sequence kernel, see launch_attn_bf16)
__device__ long long g_attn_dbg[64];  // ACCT: per-wave s_memtime totals of block 100
__device__ long long g_attn_blk[2 * 8192];  // ACCT: s_memrealtime at entry / exit of every workgroup (timeline of a launch)
#ifdef S2V_DIAG
extern "C" __attribute__((visibility("default"))) int s2v_attn_debug_read_blocks(long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_attn_blk), sizeof(long long) * 2 * 8192) == hipSuccess ? 0 : -1; }
extern "C" __attribute__((visibility("default"))) int s2v_attn_debug_read(long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_attn_dbg), sizeof(long long) * 64) == hipSuccess ? 0 : -1; }
#endif
// one work item = the 256 query rows (wg % nqb) of (sample, head) wg / nqb; all eight waves enter and leave it together
// STEER (attention steering, kernels.h AttnSteerRec): the scores of the keys of up to four ranges get log2 w added on the query rows [q0, q1) of
// the samples in the range's mask -- before the tail mask and before everything the softmax segment does (the sum vote, the slow path's
// maximum, exp2), so the deferred maximum sees the biased scores.  A key is an accumulator row and a query a lane, so a KV tile is classified
// wave-uniformly against the ranges: outside every range it runs the un-steered code; wholly inside one, 32 adds of one per-lane value;
// straddling an edge, compares on the key index the tail mask computes (at most eight such tiles at any length).  The query range is the
// per-lane factor (the addend is 0.0f on the other lanes).  A wave with no row in [q0, q1), and every wave of a sample outside the masks,
// takes the un-steered path on every tile: those rows equal the un-steered launch bit for bit.  So do the rows outside [q0, q1) of a wave
// that has rows inside, UNLESS a steered lane of that wave votes the wave into a slow path past tile 0 that the un-steered launch does not take
// (or the reverse): the slow path re-sums the tile's p in another order, within rounding of the fast sum.  STEER = false: nothing below changes.
// LOCAL (local attention in time, kernels.h "local attention"): row i sees the keys [0, P) and [lo_i, hi_i).  The item visits the prefix tiles
// [0, np) and the tiles [w0, w1) of the envelope of its 256 rows (merged by the host where they touch): loop iteration j is tile
// j < np ? j : j + (w0 - np).  Everything that is a position in the pipeline goes by the ITERATION -- the ring slot, the DMA clamp, the
// fragment prefetch of t + 1 / t + 2, the t == 0 tests, the loop bound; everything that is a position in the sequence goes by the TILE --
// kv0, the global addresses, the tail mask.  Per wave and tile, in scalar code: a tile every key of which every row of the wave sees runs
// the untouched code; any other visited tile sets the scores of the keys a lane's own row does not see to -inf, before everything the softmax
// segment does.  P >= 1 makes key 0 visible to every row, so iteration 0 (always tile 0) holds a finite score for every lane.
// BOX (local attention in space and time, kernels.h): row i sees [0, P) and the keys j of [lo_i, hi_i) with olo_i <= (j - P) mod S < ohi_i.  The
// item visits the tiles of its list in the record: loop iteration j is tile(j), and entry j also names the tiles of the iterations j + 1 .. j + 4
// (clamped by the host), which is all the DMA of iteration j issues -- so the entry of iteration j + 1 is fetched at the top of iteration j and
// waited for where the softmax segment ends, and no DMA issue waits on a load of its own entry.  ITERATION and TILE divide as for LOCAL.  Per
// wave and tile the host's whole bit picks the untouched code; any other visited tile masks per lane, on the key index and on the key's offset
// in its frame: the tile's first offset from the entry plus the key's position, less S once where it passes S (S >= 64: at most once per tile).
typedef __attribute__((ext_vector_type(8))) int i32x8;
// MAP (steering maps, kernels.h AttnSteerMapRec): STEER with the lane's addend read from a table -- log2 W_p[row - q0] of the plane p = plane[r][b] of
// each range, at most four values a lane, loaded once per work item and picked by selects in the rolled range loop (0.0f outside [q0, q1), which
// holds every row at or past Ntok; the index is clamped, so no lane reads past a plane).  Tile classification is STEER's.  The ranges a wave looks
// at come from the host's liveness table (one uniform load): a range none of whose planes' weights on the wave's rows differs from 1 is not live,
// its envelope does not count, and a wave with no live range runs the un-steered code on every tile.
template <bool ACCT, bool STEER = false, bool LOCAL = false, bool BOX = false, bool MAP = false>
__device__ __forceinline__ void attn_pp_item(const AttnArgs& a, int nqb, int wg, char* smem, const AttnSteerRec* __restrict__ sr = nullptr,
                                             const int* __restrict__ lr = nullptr, const AttnSteerMapRec* __restrict__ mr = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int fr = lane & 31, hi = lane >> 5;
    if (ACCT && tid == 0 && wg < 8192) g_attn_blk[2 * wg] = (long long)__builtin_amdgcn_s_memrealtime();
    const int bh = wg / nqb, qb = wg - bh * nqb;
    const int b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * 64;

    const bf16_t* qkv = (const bf16_t*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    const char* Kg = (const char*)(qkv + D + h * 64);
    const char* VTg = (const char*)((const bf16_t*)a.vt + (size_t)(b * a.H + h) * 64 * a.ntok_pad);
    int nt = (a.Ntok + KV_TILE - 1) / KV_TILE;   // LOCAL: the number of loop iterations (visited tiles) of this item
    int l_np = 0, l_gap = 0, l_P = 0, l_lomax = 0, l_himin = 0, lo_lane = 0, hi_lane = 0;
    if constexpr (LOCAL) {
        const int qbu = __builtin_amdgcn_readfirstlane(qb);
        const int nq = lr[2];
        const int* it = lr + ATTN_LOCAL_HDR + 4 * qbu;                       // (np, w0, w1, -)
        const int* wv = lr + ATTN_LOCAL_HDR + 4 * nq + 2 * (qbu * 8 + wave); // (lo_max, hi_min) of the wave's 32 rows
        const int* rw = lr + ATTN_LOCAL_HDR + 20 * nq + qbu * 256 + wave * 32 + fr;
        l_P = lr[0];
        l_np = it[0]; l_gap = it[1] - it[0]; nt = it[0] + (it[2] - it[1]);
        l_lomax = wv[0]; l_himin = wv[1];
        lo_lane = rw[0]; hi_lane = rw[256 * nq];   // the lane's own row's window (rows past Ntok are stored dense)
    }
    // BOX: cur = the entry of the iteration that is running, nxt = of the next one; the lane's own row as (lo, hi - lo, olo, ohi - olo)
    i32x8 cur = {0, 0, 0, 0, 0, 0, 0, 0}, nxt = {0, 0, 0, 0, 0, 0, 0, 0};
    const int* b_lst = nullptr;
    int b_S = 0, b_lo = 0, b_olo = 0;
    unsigned b_len = 0, b_olen = 0;
    if constexpr (BOX) {
        const int qbu = __builtin_amdgcn_readfirstlane(qb);
        const int nq = lr[2], ntl = lr[4];
        const int* rw = lr + ATTN_BOX_HDR + 8 * nq + qbu * 256 + wave * 32 + fr;
        l_P = lr[0]; b_S = lr[3];
        nt = lr[ATTN_BOX_HDR + 8 * qbu];
        b_lst = lr + ATTN_BOX_HDR + 1032 * nq + 8 * ntl * qbu;
        cur = *(const i32x8*)b_lst;
        b_lo = rw[0]; b_len = (unsigned)rw[256 * nq]; b_olo = rw[512 * nq]; b_olen = (unsigned)rw[768 * nq];
    }
    auto tix = [&](int j) -> int {  // iteration -> tile
        if constexpr (LOCAL) return j < l_np ? j : j + l_gap;
        else return j;
    };

    // staging: this wave's piece = rows wave*8 .. +7 of a tile, lane = (row, 16-B chunk), chunk XOR on the SOURCE address;
    // global address = wave-uniform tile base (SGPR pair) + per-lane 32-bit offset
    const int srow = wave * 8 + (lane >> 3);
    const int sc = (lane & 7) ^ ((srow >> 1) & 7);
    const unsigned offK = (unsigned)(2 * (srow * a.ld_qkv + sc * 8));
    const unsigned offV = (unsigned)(2 * (srow * a.ntok_pad + sc * 8));
    const size_t k_tile_stride = (size_t)KV_TILE * a.ld_qkv * 2;
    auto dma_k = [&](int t) {  // tiles past the end are clamped (re-staged into a dead slot) so that every wave issues the same count
        const int tc = tix(min(t, nt - 1));
        glds16_saddr(Kg + (size_t)tc * k_tile_stride, offK, smem + (t & 3) * 16384 + wave * 1024);
    };
    auto dma_v = [&](int t) {
        const int tc = tix(min(t, nt - 1));
        glds16_saddr(VTg + (size_t)tc * (KV_TILE * 2), offV, smem + (t & 3) * 16384 + 8192 + wave * 1024);
    };
    // BOX: the same two issues with the tile taken from the entry (clamped by the host), the ring slot from the iteration
    auto dma_k_box = [&](int t, int tile) { glds16_saddr(Kg + (size_t)tile * k_tile_stride, offK, smem + (t & 3) * 16384 + wave * 1024); };
    auto dma_v_box = [&](int t, int tile) { glds16_saddr(VTg + (size_t)tile * (KV_TILE * 2), offV, smem + (t & 3) * 16384 + 8192 + wave * 1024); };
    if constexpr (BOX) {
        dma_k_box(0, cur[0]); dma_v_box(0, cur[0]); dma_k_box(1, cur[5]); dma_v_box(1, cur[5]); dma_k_box(2, cur[3]); dma_k_box(3, cur[6]);
    } else {
        dma_k(0); dma_v(0); dma_k(1); dma_v(1); dma_k(2); dma_k(3);
    }

    // Q fragments (B operand of S^T = K.Q^T): lane (q = fr, hi) holds Q[q][16kk + 8hi .. +8], pre-multiplied by
    // scale * log2(e) and rounded to bf16 once (the reference's math path rounds its scaled q and k to bf16 as well), so the
    // MFMA result is already the exp2 argument
    const int q_row = qb * 256 + wave * 32 + fr;
    const int q_ld = min(q_row, a.Ntok - 1);
    const float c0 = a.scale * 1.4426950408889634f;
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        qf[kk] = *(const bf16x8*)(qkv + (size_t)q_ld * a.ld_qkv + h * 64 + kk * 16 + hi * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[kk][e] = (__bf16)((float)qf[kk][e] * c0);
    }

    // STEER: this item's view of the record, wave-uniform (scalar registers): the ranges that apply to this sample and wave as a bit set, and their
    // envelope [s_lo, s_hi) -- a tile outside it never looks at the record (both 0 when no range applies)
    unsigned s_on = 0;
    int s_lo = 0, s_hi = 0;
    bool inq = false;
    if constexpr (STEER) {
        const int bu = __builtin_amdgcn_readfirstlane(b);
        const int wq0 = __builtin_amdgcn_readfirstlane(qb) * 256 + wave * 32;
        const int sq0 = sr->q0, sq1 = sr->q1, sn = min(sr->n, ATTN_STEER_MAX_RANGES);
        if (wq0 < sq1 && wq0 + 32 > sq0) {
            for (int r = sn - 1; r >= 0; --r)
                if ((sr->sample_mask[r] >> bu) & 1u) {
                    if (!s_on) s_hi = sr->k1[r];
                    s_lo = sr->k0[r];
                    s_on |= 1u << r;
                }
        }
        inq = q_row >= sq0 && q_row < sq1;
    }
    // MAP: the live ranges of this sample and wave from the host's table, their envelope, and the lane's own row's addend for each of them
    float m_ad0 = 0.f, m_ad1 = 0.f, m_ad2 = 0.f, m_ad3 = 0.f;
    if constexpr (MAP) {
        const int bu = min(__builtin_amdgcn_readfirstlane(b), ATTN_STEER_MAP_BATCH - 1);
        const int qbu = min(__builtin_amdgcn_readfirstlane(qb), mr->nqb - 1);
        const int* mw = (const int*)mr;
        s_on = (unsigned)mw[mr->off_live + (bu * mr->nqb + qbu) * 8 + wave] & 15u;
        bool top = true;
        for (int r = ATTN_STEER_MAX_RANGES - 1; r >= 0; --r)
            if ((s_on >> r) & 1u) {
                if (top) s_hi = mr->k1[r];
                top = false;
                s_lo = mr->k0[r];
            }
        const int sq0 = mr->q0, vq = mr->q1 - sq0;
        inq = q_row >= sq0 && q_row < mr->q1;
        const float* lp = (const float*)mr + mr->off_log2 + min(max(q_row - sq0, 0), vq - 1);
        const int* pw = (const int*)mr->plane;   // plane[r][b] as bytes of two words per range: a scalar load and a bit-field extract
        auto addend = [&](int r) -> float {
            const int p = (int)(signed char)(pw[2 * r + (bu >> 2)] >> (8 * (bu & 3)));
            const float v = lp[max(p, 0) * vq];
            return (inq && ((s_on >> r) & 1u)) ? v : 0.f;
        };
        m_ad0 = addend(0); m_ad1 = addend(1); m_ad2 = addend(2); m_ad3 = addend(3);
    }

    // the S^T accumulators START at -m_run: this 16-register block is loop-carried and only rewritten on the slow path
    f32x16 ot[2], st[2], negm16;
#pragma unroll
    for (int e = 0; e < 16; ++e) { ot[0][e] = 0.f; ot[1][e] = 0.f; negm16[e] = 0.f; }
    float l_run = 0.f;
    bf16x8 pk[4], kf[8], vf[8];
    f32x16 pp[2];  // exp2 results of the tile in flight between S(t) and M(t+1)

    // fragment byte offsets inside a tile: K (kk, kb) and V^T (s, db) use the same (row, chunk) pattern
    int foff[4][2];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int row = kb * 32 + fr, cl = kk * 2 + hi;
            foff[kk][kb] = row * 128 + ((cl ^ ((row >> 1) & 7)) << 4);
        }
    auto k_frag = [&](int t, int i) -> bf16x8 { return *(const bf16x8*)(smem + (t & 3) * 16384 + foff[i >> 1][i & 1]); };
    auto v_frag = [&](int t, int i) -> bf16x8 { return *(const bf16x8*)(smem + (t & 3) * 16384 + 8192 + foff[i >> 1][i & 1]); };
    auto fence = [&]() { __builtin_amdgcn_sched_barrier(0); };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (grp) __builtin_amdgcn_s_barrier();  // group B runs one phase behind
    fence();
    // M(0): QK^T of tile 0 and the K fragments of tile 1
#pragma unroll
    for (int i = 0; i < 8; ++i) kf[i] = k_frag(0, i);
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[i], qf[i >> 1], i < 2 ? negm16 : st[i & 1], 0, 0, 0);
    fence();
#pragma unroll
    for (int i = 0; i < 8; ++i) kf[i] = k_frag(min(1, nt - 1), i);
    fence();
    __builtin_amdgcn_s_barrier();
    fence();

    long long tacc[6] = {0, 0, 0, 0, 0, 0};
    auto now = [&]() -> long long { return ACCT ? (long long)__builtin_amdgcn_s_memtime() : 0; };
    const long long tl0 = now();
    for (int t = 0; t < nt; ++t) {
        // ---- softmax segment S(t)
        const long long u0 = now();
        int kv0;
        if constexpr (BOX) {
            kv0 = cur[0] * KV_TILE;
            // the entry of iteration t + 1, in flight across this segment (asm: the load is issued HERE and waited for below, by hand).
            // INVARIANT the compiler is not told: the eight SGPRs of nxt are NOT valid between this asm and the lgkmcnt(0) asm below (its waitcnt
            // insertion does not see a load issued from inline asm).  Nothing in between may name nxt: the only reads are `cur = nxt` at the
            // loop's end.  A copy or spill of nxt ahead of the wait would read stale registers -- when this code or the compiler changes,
            // check in the disassembly of attn_pp_box_k and attn_pp_box_persist_k that the destination octet is first read after the wait.
            const int* ep = b_lst + 8 * min(t + 1, nt - 1);
            asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=&s"(nxt) : "s"(ep));
        } else {
            kv0 = tix(t) * KV_TILE;
        }
        if constexpr (STEER) {
            if (kv0 < s_hi && kv0 + KV_TILE > s_lo) {
#pragma nounroll
                for (int r = 0; r < ATTN_STEER_MAX_RANGES; ++r) {
                    if (!((s_on >> r) & 1u)) continue;
                    const int lo = max(sr->k0[r], kv0), up = min(sr->k1[r], kv0 + KV_TILE);
                    if (lo >= up) continue;  // the tile holds no key of range r
                    const float bl = inq ? sr->log2w[r] : 0.f;
                    if (up - lo == KV_TILE) {  // interior tile
#pragma unroll
                        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                            for (int e = 0; e < 16; ++e) st[kb][e] += bl;
                    } else {  // an edge of the range inside the tile: the key index of the tail mask, as an offset from the range's first key
                        const unsigned len = (unsigned)(up - lo);
                        const int kvb = kv0 - lo + 4 * hi;
#pragma unroll
                        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                            for (int e = 0; e < 16; ++e)
                                if ((unsigned)(kvb + kb * 32 + (e & 3) + 8 * (e >> 2)) < len) st[kb][e] += bl;
                    }
                }
            }
        }
        if constexpr (MAP) {
            if (kv0 < s_hi && kv0 + KV_TILE > s_lo) {
#pragma nounroll
                for (int r = 0; r < ATTN_STEER_MAX_RANGES; ++r) {
                    if (!((s_on >> r) & 1u)) continue;
                    const int lo = max(mr->k0[r], kv0), up = min(mr->k1[r], kv0 + KV_TILE);
                    if (lo >= up) continue;  // the tile holds no key of range r
                    const float bl = r == 0 ? m_ad0 : r == 1 ? m_ad1 : r == 2 ? m_ad2 : m_ad3;
                    if (up - lo == KV_TILE) {  // interior tile
#pragma unroll
                        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                            for (int e = 0; e < 16; ++e) st[kb][e] += bl;
                    } else {  // an edge of the range inside the tile, as STEER
                        const unsigned len = (unsigned)(up - lo);
                        const int kvb = kv0 - lo + 4 * hi;
#pragma unroll
                        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                            for (int e = 0; e < 16; ++e)
                                if ((unsigned)(kvb + kb * 32 + (e & 3) + 8 * (e >> 2)) < len) st[kb][e] += bl;
                    }
                }
            }
        }
        if constexpr (LOCAL) {
            // whole: every key of the tile below Ntok is seen by every row of the wave -- inside the prefix, or inside [lo_max, hi_min) (reaching
            // down through the prefix when lo_max == P: every row's window then starts where the prefix ends)
            const int kend = min(kv0 + KV_TILE, a.Ntok);
            const bool whole = kend <= l_P || (kend <= l_himin && (kv0 >= l_lomax || l_lomax <= l_P));
            if (!whole) {
                const unsigned len = (unsigned)(hi_lane - lo_lane);
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int kv = kv0 + kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hi;
                        if (!(kv < l_P || (unsigned)(kv - lo_lane) < len)) st[kb][e] = -INFINITY;
                    }
            }
        }
        if constexpr (BOX) {
            if (!((cur[2] >> wave) & 1)) {   // not whole for this wave (the host's bit)
                const int kvb = kv0 + 4 * hi;
                const unsigned ob = (unsigned)(cur[1] + 4 * hi);
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int kp = kb * 32 + (e & 3) + 8 * (e >> 2);
                        const int kv = kvb + kp;
                        const unsigned o = min(ob + (unsigned)kp, ob + (unsigned)kp - (unsigned)b_S);
                        // bitwise on purpose: the short-circuit form compiles to a branch per key
                        const bool seen = (kv < l_P) | (((unsigned)(kv - b_lo) < b_len) & (o - (unsigned)b_olo < b_olen));
                        st[kb][e] = seen ? st[kb][e] : -INFINITY;
                    }
            }
        }
        if (kv0 + KV_TILE > a.Ntok) {  // tail tile: mask keys >= Ntok
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int kv = kv0 + kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hi;
                    if (kv >= a.Ntok) st[kb][e] = -INFINITY;
                }
        }
        float ps0 = 0.f, ps1 = 0.f;
        // 16 groups of (exp2, exp2, add, add): the adds of a group consume the exp2 results of the group before.  Written as
        // asm so that neither the SLP vectoriser (it packs the adds) nor the scheduler reorders the stream.
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int kb = g >> 3, e = (g & 7) * 2;
            asm volatile("v_exp_f32 %0, %1" : "=v"(pp[kb][e]) : "v"(st[kb][e]));
            asm volatile("v_exp_f32 %0, %1" : "=v"(pp[kb][e + 1]) : "v"(st[kb][e + 1]));
            if (g > 0) {
                const int gp = g - 1, kbp = gp >> 3, ep = (gp & 7) * 2;
                asm volatile("v_add_f32 %0, %0, %1" : "+v"(ps0) : "v"(pp[kbp][ep]));
                asm volatile("v_add_f32 %0, %0, %1" : "+v"(ps1) : "v"(pp[kbp][ep + 1]));
            }
        }
        ps0 += pp[1][14];
        ps1 += pp[1][15];
        float psum = ps0 + ps1;
        // Deferred maximum: the slow path runs for the first tile (adopts its maximum; its first exp2 pass may overflow, the
        // vote is NaN-safe) and whenever some p of the wave grew past ~2^8: m_run rises to the true maximum, everything at
        // the old scale is rescaled once, and the tile's exp2 is redone at the new scale.
        if (t == 0 || __any(!(psum <= 18446744073709551616.f))) {
            float m0 = max3f(st[0][0], st[0][1], st[0][2]), m1 = max3f(st[1][0], st[1][1], st[1][2]);
#pragma unroll
            for (int e = 3; e < 15; e += 2) { m0 = max3f(m0, st[0][e], st[0][e + 1]); m1 = max3f(m1, st[1][e], st[1][e + 1]); }
            const float mxp = max3f(m0, m1, fmaxf(st[0][15], st[1][15]));
            // cross-half exchange without LDS: sw[0] = lower half's value in both halves, sw[1] = upper half's
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mxp), __float_as_uint(mxp), false, false);
            const float mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
            const float d = (t == 0) ? mx : fmaxf(mx, 0.f);
            // t == 0: O and l are still zero, and exp2(-d) would overflow to inf (0 * inf = NaN) for scores below -128
            const float alpha = (t == 0) ? 1.0f : __builtin_amdgcn_exp2f(-d);
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) ot[i][e] *= alpha;
#pragma unroll
            for (int e = 0; e < 16; ++e) negm16[e] -= d;  // -(m + d) == (-m) - d exactly
            psum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    pp[kb][e] = __builtin_amdgcn_exp2f(st[kb][e] - d);
                    psum += pp[kb][e];
                }
        }
        l_run += psum;
        asm volatile("" : "+v"(l_run));
        fence();
        const long long u1 = now();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (BOX) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(nxt)::"memory");   // the next entry has landed (the K fragments are due here anyway)
        const long long u2 = now();
        __builtin_amdgcn_s_barrier();
        const long long u3 = now();
        fence();

        // ---- matrix segment M(t+1), in issue order, one fenced step per MFMA.
        // QK^T of tile t+1 (clamped: the last one is computed twice and dropped): K fragments were prefetched; behind each MFMA
        // the V^T fragment of tile t for the matching P.V step and two v_cvt_pk of P.
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            st[i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[i], qf[i >> 1], i < 2 ? negm16 : st[i & 1], 0, 0, 0);
            vf[i] = v_frag(t, i);
            // P values 4i .. 4i+3: pk[s] element e = pp[s >> 1][(s & 1) * 8 + e]
            const int s = i >> 1, kb = s >> 1, r0 = (s & 1) * 8 + (i & 1) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) pk[s][(i & 1) * 4 + e] = (__bf16)pp[kb][r0 + e];
            fence();
        }
        // P.V of tile t; behind the MFMAs the K fragments of tile t+2
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ot[i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[i], pk[i >> 1], ot[i & 1], 0, 0, 0);
            kf[i] = k_frag(min(t + 2, nt - 1), i);
            fence();
        }
        if constexpr (BOX) {
            dma_k_box(t + 4, cur[4]);
            dma_v_box(t + 2, cur[3]);
            cur = nxt;
        } else {
            dma_k(t + 4);
            dma_v(t + 2);
        }
        __builtin_amdgcn_s_setprio(0);
        fence();
        const long long u4 = now();
        __builtin_amdgcn_s_barrier();
        const long long u5 = now();
        fence();
        if (ACCT) {
            tacc[0] += u1 - u0;  // softmax segment
            tacc[1] += u2 - u1;  // vmcnt(0)
            tacc[2] += u3 - u2;  // barrier after S
            tacc[3] += u4 - u3;  // matrix segment
            tacc[4] += u5 - u4;  // barrier after M
        }
    }
    if (ACCT) {
        tacc[5] = now() - tl0;
        if (wg == 100 && lane == 0)
            for (int e = 0; e < 6; ++e) g_attn_dbg[wave * 8 + e] = tacc[e];
    }
    if (!grp) __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    // A lane holds dims 8g + 4hi .. + 3 of its row for the eight groups g: one half-wave exchange per pair of groups (g, g + 1)
    // gives the lower half 16 contiguous bytes of group g and the upper half those of group g + 1 -> 4 x 16-B stores per lane
    // instead of 8 x 8-B (the store tail of a block is issue-bound)
    u32x2 og[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const int db = g >> 2, rq = g & 3;
        og[g].x = pack2bf(ot[db][rq * 4 + 0] * inv, ot[db][rq * 4 + 1] * inv);
        og[g].y = pack2bf(ot[db][rq * 4 + 2] * inv, ot[db][rq * 4 + 3] * inv);
    }
    bf16_t* o = (bf16_t*)a.out + (size_t)(b * a.Ntok + min(q_row, a.Ntok - 1)) * a.ld_out + h * 64 + hi * 8;
#pragma unroll
    for (int g = 0; g < 8; g += 2) {
        const auto rx = __builtin_amdgcn_permlane32_swap(og[g].x, og[g + 1].x, false, false);
        const auto ry = __builtin_amdgcn_permlane32_swap(og[g].y, og[g + 1].y, false, false);
        u32x4 v = {rx[0], ry[0], rx[1], ry[1]};
        if (q_row < a.Ntok) *(u32x4*)(o + 8 * g) = v;
    }
    if (ACCT && tid == 0 && wg < 8192) g_attn_blk[2 * wg + 1] = (long long)__builtin_amdgcn_s_memrealtime();
}

// XCD-aware order of the work items: XCD x owns a contiguous range, so all q-blocks of one (sample, head) run on one XCD and its
// K / V stay in that XCD's L2
__device__ __forceinline__ void attn_xcd_range(int total, int x, int& first, int& cnt) {
    const int q = total >> 3, r = total & 7;
    first = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    cnt = q + (x < r ? 1 : 0);
}
// one workgroup per work item (the op-level entry point: no per-launch state)
template <bool ACCT>
__global__ __launch_bounds__(512, 2) void attn_pp_k(const AttnArgs a, int nqb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [4 slots][K tile | VT tile]
    int first, cnt;
    attn_xcd_range((int)gridDim.x, blockIdx.x & 7, first, cnt);
    attn_pp_item<ACCT>(a, nqb, first + (int)(blockIdx.x >> 3), smem);
}
// the STEER = true instantiation of the same launch form: the record comes as one more pointer argument
__global__ __launch_bounds__(512, 2) void attn_pp_steer_k(const AttnArgs a, int nqb, const AttnSteerRec* __restrict__ sr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int first, cnt;
    attn_xcd_range((int)gridDim.x, blockIdx.x & 7, first, cnt);
    attn_pp_item<false, true>(a, nqb, first + (int)(blockIdx.x >> 3), smem, sr);
}
// the LOCAL = true instantiation of the same launch form: the record (kernels.h "local attention") comes as one more pointer argument
__global__ __launch_bounds__(512, 2) void attn_pp_local_k(const AttnArgs a, int nqb, const int* __restrict__ lr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int first, cnt;
    attn_xcd_range((int)gridDim.x, blockIdx.x & 7, first, cnt);
    attn_pp_item<false, false, true>(a, nqb, first + (int)(blockIdx.x >> 3), smem, nullptr, lr);
}
// the BOX = true instantiation of the same launch form: the record (kernels.h "local attention in space and time") as the one pointer argument
__global__ __launch_bounds__(512, 2) void attn_pp_box_k(const AttnArgs a, int nqb, const int* __restrict__ lr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int first, cnt;
    attn_xcd_range((int)gridDim.x, blockIdx.x & 7, first, cnt);
    attn_pp_item<false, false, false, true>(a, nqb, first + (int)(blockIdx.x >> 3), smem, nullptr, lr);
}
// the MAP = true instantiation of the same launch form: the map record (kernels.h AttnSteerMapRec) as the one pointer argument
__global__ __launch_bounds__(512, 2) void attn_pp_steer_map_k(const AttnArgs a, int nqb, const AttnSteerMapRec* __restrict__ mr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int first, cnt;
    attn_xcd_range((int)gridDim.x, blockIdx.x & 7, first, cnt);
    attn_pp_item<false, false, false, false, true>(a, nqb, first + (int)(blockIdx.x >> 3), smem, nullptr, nullptr, mr);
}
// PERSISTENT form (the engine's launches): one workgroup per CU pulls items from its XCD's queue and, when that is empty, from the
// other XCDs' queues.  The hardware hands every XCD exactly 1/8 of a grid, but the XCDs of one launch run a few percent apart in
// clock: with static shares the launch ended 95-100 % apart per XCD plus a last round of 32 items on 256 slots (4.6 % of the
// slot-time idle, tools/attn_harness timeline); pulled work ends within one item.  queue[0..7]: next item of XCD x, queue[8]:
// workgroups done -- the last one to leave zeroes the nine counters for the next launch (they must be zero at the first).
// TWIN: attn_pp_steer_persist_k, attn_pp_local_persist_k, attn_pp_box_persist_k and attn_pp_steer_map_persist_k below repeat this loop word for word (a shared function changed this kernel's
// schedule): a change to the queue protocol here is made there as well.
template <bool ACCT>
__global__ __launch_bounds__(512, 2) void attn_pp_persist_k(const AttnArgs a, int nqb, int total, int* __restrict__ queue) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_item;
    const int xcd = blockIdx.x & 7;
    for (;;) {
        if (threadIdx.x == 0) {
            int wg = -1;
            for (int k = 0; k < 8 && wg < 0; ++k) {
                const int y = (xcd + k) & 7;
                int first, cnt;
                attn_xcd_range(total, y, first, cnt);
                if (__hip_atomic_load(&queue[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= cnt) continue;  // drained: do not hammer it
                const int i = atomicAdd(&queue[y], 1);
                if (i < cnt) wg = first + i;
            }
            s_item = wg;
        }
        __syncthreads();  // also fences the previous item's LDS traffic from the next item's prologue
        const int wg = s_item;
        __syncthreads();
        if (wg < 0) break;
        attn_pp_item<ACCT>(a, nqb, wg, smem);
    }
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&queue[8], 1) == (int)gridDim.x - 1) {
            for (int i = 0; i < 9; ++i) __hip_atomic_store(&queue[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
        }
    }
}
// the STEER = true instantiation of the persistent form: the same loop (kept as a twin so that the kernel above keeps its code to the instruction)
__global__ __launch_bounds__(512, 2) void attn_pp_steer_persist_k(const AttnArgs a, int nqb, int total, int* __restrict__ queue, const AttnSteerRec* __restrict__ sr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_item;
    const int xcd = blockIdx.x & 7;
    for (;;) {
        if (threadIdx.x == 0) {
            int wg = -1;
            for (int k = 0; k < 8 && wg < 0; ++k) {
                const int y = (xcd + k) & 7;
                int first, cnt;
                attn_xcd_range(total, y, first, cnt);
                if (__hip_atomic_load(&queue[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= cnt) continue;  // drained: do not hammer it
                const int i = atomicAdd(&queue[y], 1);
                if (i < cnt) wg = first + i;
            }
            s_item = wg;
        }
        __syncthreads();  // also fences the previous item's LDS traffic from the next item's prologue
        const int wg = s_item;
        __syncthreads();
        if (wg < 0) break;
        attn_pp_item<false, true>(a, nqb, wg, smem, sr);
    }
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&queue[8], 1) == (int)gridDim.x - 1) {
            for (int i = 0; i < 9; ++i) __hip_atomic_store(&queue[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
        }
    }
}
// the LOCAL = true instantiation of the persistent form: the same loop once more (a twin, as above); its items are of unequal length, which the
// pulled queue evens out
__global__ __launch_bounds__(512, 2) void attn_pp_local_persist_k(const AttnArgs a, int nqb, int total, int* __restrict__ queue, const int* __restrict__ lr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_item;
    const int xcd = blockIdx.x & 7;
    for (;;) {
        if (threadIdx.x == 0) {
            int wg = -1;
            for (int k = 0; k < 8 && wg < 0; ++k) {
                const int y = (xcd + k) & 7;
                int first, cnt;
                attn_xcd_range(total, y, first, cnt);
                if (__hip_atomic_load(&queue[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= cnt) continue;  // drained: do not hammer it
                const int i = atomicAdd(&queue[y], 1);
                if (i < cnt) wg = first + i;
            }
            s_item = wg;
        }
        __syncthreads();  // also fences the previous item's LDS traffic from the next item's prologue
        const int wg = s_item;
        __syncthreads();
        if (wg < 0) break;
        attn_pp_item<false, false, true>(a, nqb, wg, smem, nullptr, lr);
    }
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&queue[8], 1) == (int)gridDim.x - 1) {
            for (int i = 0; i < 9; ++i) __hip_atomic_store(&queue[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
        }
    }
}
// the BOX = true instantiation of the persistent form: the same loop a fourth time (a twin, as above)
__global__ __launch_bounds__(512, 2) void attn_pp_box_persist_k(const AttnArgs a, int nqb, int total, int* __restrict__ queue, const int* __restrict__ lr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_item;
    const int xcd = blockIdx.x & 7;
    for (;;) {
        if (threadIdx.x == 0) {
            int wg = -1;
            for (int k = 0; k < 8 && wg < 0; ++k) {
                const int y = (xcd + k) & 7;
                int first, cnt;
                attn_xcd_range(total, y, first, cnt);
                if (__hip_atomic_load(&queue[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= cnt) continue;  // drained: do not hammer it
                const int i = atomicAdd(&queue[y], 1);
                if (i < cnt) wg = first + i;
            }
            s_item = wg;
        }
        __syncthreads();  // also fences the previous item's LDS traffic from the next item's prologue
        const int wg = s_item;
        __syncthreads();
        if (wg < 0) break;
        attn_pp_item<false, false, false, true>(a, nqb, wg, smem, nullptr, lr);
    }
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&queue[8], 1) == (int)gridDim.x - 1) {
            for (int i = 0; i < 9; ++i) __hip_atomic_store(&queue[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
        }
    }
}

// the MAP = true instantiation of the persistent form: the same loop a fifth time (a twin, as above)
__global__ __launch_bounds__(512, 2) void attn_pp_steer_map_persist_k(const AttnArgs a, int nqb, int total, int* __restrict__ queue, const AttnSteerMapRec* __restrict__ mr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_item;
    const int xcd = blockIdx.x & 7;
    for (;;) {
        if (threadIdx.x == 0) {
            int wg = -1;
            for (int k = 0; k < 8 && wg < 0; ++k) {
                const int y = (xcd + k) & 7;
                int first, cnt;
                attn_xcd_range(total, y, first, cnt);
                if (__hip_atomic_load(&queue[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= cnt) continue;  // drained: do not hammer it
                const int i = atomicAdd(&queue[y], 1);
                if (i < cnt) wg = first + i;
            }
            s_item = wg;
        }
        __syncthreads();  // also fences the previous item's LDS traffic from the next item's prologue
        const int wg = s_item;
        __syncthreads();
        if (wg < 0) break;
        attn_pp_item<false, false, false, false, true>(a, nqb, wg, smem, nullptr, nullptr, mr);
    }
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&queue[8], 1) == (int)gridDim.x - 1) {
            for (int i = 0; i < 9; ++i) __hip_atomic_store(&queue[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
        }
    }
}

#ifdef S2V_DIAG
int g_attn_variant = 0;  // see launch_attn_bf16
extern "C" __attribute__((visibility("default"))) int s2v_set_attn_variant(int v) { g_attn_variant = v; return 0; }
static int* g_attn_queue = nullptr;  // harness: a queue for op-level launches (variants 4, 5 = persistent product / accounting kernel)
static int g_attn_ncu = 0;
extern "C" __attribute__((visibility("default"))) int s2v_set_attn_queue(int* q, int ncu) { g_attn_queue = q; g_attn_ncu = ncu; return 0; }
#endif

int launch_attn_bf16(const AttnArgs& a_in, hipStream_t st) {
    AttnArgs a = a_in;
    S2V_REQUIRE(a.vt != nullptr, "attn_bf16: V^T buffer missing");
    S2V_REQUIRE(a.ld_qkv % 8 == 0 && a.ntok_pad % 64 == 0, "attn_bf16: bad leading dims");
    S2V_REQUIRE(a.ntok_pad >= ((a.Ntok + 63) / 64) * 64, "attn_bf16: ntok_pad too small");
    const int nqb8 = (a.Ntok + 255) / 256;  // 256 query rows per work item
    const int total = nqb8 * a.B * a.H;
#ifdef S2V_DIAG
    // variants: 0 = product (attn_q4; persistent when the caller brought a queue), 3 = product, one workgroup per item,
    //   4 = product, persistent on the harness queue (0 / 3 / 4: attn_pp up to ATTN_PP_MAX_TOKENS, attn_q4 beyond), 6 / 7 = attn_q4 per item /
    //   persistent at any length, 8 / 9 = attn_q8 (the same stream, eight
    //   waves x 32 rows), 10 / 11 = attn_pp (round-2 kernel) per item / persistent, 1 / 5 = attn_pp with stall accounting, 2 = round-1 kernel
    const int v = g_attn_variant;
    if ((v == 4 || v == 5 || v == 7 || v == 9 || v == 11) && !a.queue) { a.queue = g_attn_queue; a.num_cus = g_attn_ncu; }
    if (v == 3 || v == 6 || v == 8 || v == 10 || v == 1 || v == 2) a.queue = nullptr;
    if (v == 8 || v == 9) return launch_attn_q8(a, v == 9, st);
    if (v == 6 || v == 7) return launch_attn_q4(a, v == 7 && a.queue != nullptr, st);  // attn_q4 whatever the sequence length
    if (v == 1 || v == 2 || v == 5 || v == 10 || v == 11) {
        S2V_REQUIRE(a.mx_q == nullptr, "attn_bf16: the MX output of the fp8 engine is attn_q4 / attn_q8's (reference variants write bf16 only)");
        const dim3 g8(total), b8(512);
        const void* fn = (v == 1) ? (const void*)attn_pp_k<true> : (const void*)attn_pp_k<false>;
        size_t lds = 65536;
        if (v == 2) { fn = (const void*)attn_bf16_k<0, 8>; lds = 4 * ATT_TILE_BYTES; }
        if ((v == 5 || v == 11) && a.queue != nullptr) {
            fn = (v == 5) ? (const void*)attn_pp_persist_k<true> : (const void*)attn_pp_persist_k<false>;
            S2V_TRY(ensure_lds_attr(fn, 65536));
            int* queue = a.queue;
            void* args[] = {(void*)&a, (void*)&nqb8, (void*)&total, (void*)&queue};
            S2V_CHECK_HIP(hipLaunchKernel(fn, dim3((a.num_cus / 8) * 8), b8, args, lds, st));
            return 0;
        }
        S2V_TRY(ensure_lds_attr(fn, 65536));
        void* args[] = {(void*)&a, (void*)&nqb8};
        S2V_CHECK_HIP(hipLaunchKernel(fn, g8, b8, args, lds, st));
        return 0;
    }
#endif
    // persistent (work-pulling) launch when the caller owns a queue and there is more than two rounds of work; else one workgroup per item
    const bool persist = a.queue != nullptr && total > 2 * a.num_cus && a.num_cus >= 8;
    // Short sequences run the eight-wave ping-pong kernel (attn_pp, round 2's product kernel): attn_q4's one-statement body pays a long
    // prologue (first-tile maxima, fragment pipeline fill) and walks its last five KV tiles through the rare-path handler, which is
    // nothing at 299 tiles (C3: attn_q4 5-6 % ahead) and a quarter of the iterations at 20 (C1 step 12.01 -> 11.27 ms on one box, DESIGN section 3;
    // tools/attn_small_probe.py).  Same deferred-maximum rule (2^64), results within bf16 rounding of attn_q4's, not bit-identical.
    if (a.p16) {
        S2V_REQUIRE(attn_runs_q4(a.Ntok, a.mx_q != nullptr), "attn_bf16: fp16 P / V^T is the four-wave kernel's; short sequences run attn_pp on bf16 V^T");
        return launch_attn_q4h(a, persist, st);
    }
    if (a.mx_q == nullptr && a.Ntok <= ATTN_PP_MAX_TOKENS) {
        const void* fn = persist ? (const void*)attn_pp_persist_k<false> : (const void*)attn_pp_k<false>;
        S2V_TRY(ensure_lds_attr(fn, 65536));
        if (persist) {
            int* queue = a.queue;
            void* args[] = {(void*)&a, (void*)&nqb8, (void*)&total, (void*)&queue};
            S2V_CHECK_HIP(hipLaunchKernel(fn, dim3((a.num_cus / 8) * 8), dim3(512), args, 65536, st));
        } else {
            void* args[] = {(void*)&a, (void*)&nqb8};
            S2V_CHECK_HIP(hipLaunchKernel(fn, dim3(total), dim3(512), args, 65536, st));
        }
        return 0;
    }
    return launch_attn_q4(a, persist, st);
}

// a steered layer of a bf16 engine (and s2v_op_attention_steer impl 0): attn_pp<STEER> at every length, persistent under the rule above
int launch_attn_bf16_steer(const AttnArgs& a, const AttnSteerRec* rec_dev, hipStream_t st) {
    S2V_REQUIRE(rec_dev != nullptr, "attn_bf16_steer: steer record missing");
    S2V_REQUIRE(a.vt != nullptr, "attn_bf16_steer: V^T buffer missing");
    S2V_REQUIRE(a.mx_q == nullptr && !a.p16, "attn_bf16_steer: attn_pp writes bf16 and reads bf16 V^T (no MX output, no attn_p_format 1)");
    S2V_REQUIRE(a.ld_qkv % 8 == 0 && a.ntok_pad % 64 == 0, "attn_bf16_steer: bad leading dims");
    S2V_REQUIRE(a.ntok_pad >= ((a.Ntok + 63) / 64) * 64, "attn_bf16_steer: ntok_pad too small");
    S2V_REQUIRE(a.B >= 1 && a.B <= 32, "attn_bf16_steer: the sample masks hold 32 samples");
    int nqb8 = (a.Ntok + 255) / 256;
    int total = nqb8 * a.B * a.H;
    const bool persist = a.queue != nullptr && total > 2 * a.num_cus && a.num_cus >= 8;
    const void* fn = persist ? (const void*)attn_pp_steer_persist_k : (const void*)attn_pp_steer_k;
    S2V_TRY(ensure_lds_attr(fn, 65536));
    AttnArgs av = a;
    if (persist) {
        int* queue = a.queue;
        void* args[] = {(void*)&av, (void*)&nqb8, (void*)&total, (void*)&queue, (void*)&rec_dev};
        S2V_CHECK_HIP(hipLaunchKernel(fn, dim3((a.num_cus / 8) * 8), dim3(512), args, 65536, st));
    } else {
        void* args[] = {(void*)&av, (void*)&nqb8, (void*)&rec_dev};
        S2V_CHECK_HIP(hipLaunchKernel(fn, dim3(total), dim3(512), args, 65536, st));
    }
    return 0;
}

// a local layer of a bf16 engine (and s2v_op_attention_local impl 0): attn_pp<LOCAL> at every length, persistent under the rule above
int launch_attn_bf16_local(const AttnArgs& a, const int* rec_dev, hipStream_t st) {
    S2V_REQUIRE(rec_dev != nullptr, "attn_bf16_local: local-attention record missing");
    S2V_REQUIRE(a.vt != nullptr, "attn_bf16_local: V^T buffer missing");
    S2V_REQUIRE(a.mx_q == nullptr && !a.p16, "attn_bf16_local: attn_pp writes bf16 and reads bf16 V^T (no MX output, no attn_p_format 1)");
    S2V_REQUIRE(a.ld_qkv % 8 == 0 && a.ntok_pad % 64 == 0, "attn_bf16_local: bad leading dims");
    S2V_REQUIRE(a.ntok_pad >= ((a.Ntok + 63) / 64) * 64, "attn_bf16_local: ntok_pad too small");
    int nqb8 = (a.Ntok + 255) / 256;
    int total = nqb8 * a.B * a.H;
    const bool persist = a.queue != nullptr && total > 2 * a.num_cus && a.num_cus >= 8;
    const void* fn = persist ? (const void*)attn_pp_local_persist_k : (const void*)attn_pp_local_k;
    S2V_TRY(ensure_lds_attr(fn, 65536));
    AttnArgs av = a;
    if (persist) {
        int* queue = a.queue;
        void* args[] = {(void*)&av, (void*)&nqb8, (void*)&total, (void*)&queue, (void*)&rec_dev};
        S2V_CHECK_HIP(hipLaunchKernel(fn, dim3((a.num_cus / 8) * 8), dim3(512), args, 65536, st));
    } else {
        void* args[] = {(void*)&av, (void*)&nqb8, (void*)&rec_dev};
        S2V_CHECK_HIP(hipLaunchKernel(fn, dim3(total), dim3(512), args, 65536, st));
    }
    return 0;
}

// host: the record (kernels.h "local attention") from P and the row table, every bound refused by name; the item and wave tables are reduced
// here, once per table, not by the kernel
int attn_local_make(const char* who, int P, int Ntok, const int* lo, const int* hi, std::vector<int>* out) {
    static thread_local char msg[256];
#define LOCAL_REQUIRE(cond, ...) do { if (!(cond)) { snprintf(msg, sizeof(msg), __VA_ARGS__); S2V_REQUIRE(false, msg); } } while (0)
    LOCAL_REQUIRE(Ntok >= 1, "%s: Ntok = %d must be at least 1", who, Ntok);
    LOCAL_REQUIRE(lo && hi, "%s: null row table", who);
    LOCAL_REQUIRE(P >= 1 && P <= Ntok, "%s: the prefix P = %d must lie inside [1, Ntok = %d] (key 0 is visible to every row)", who, P, Ntok);
    for (int i = 0; i < Ntok; ++i)
        LOCAL_REQUIRE(P <= lo[i] && lo[i] <= hi[i] && hi[i] <= Ntok, "%s: row %d has the window [%d, %d): P = %d <= lo <= hi <= Ntok = %d is required", who, i,
                      lo[i], hi[i], P, Ntok);
#undef LOCAL_REQUIRE
    const int nqb = (Ntok + 255) / 256, npre = (P + KV_TILE - 1) / KV_TILE;
    std::vector<int>& r = *out;
    r.assign(attn_local_ints(Ntok), 0);
    r[0] = P; r[1] = Ntok; r[2] = nqb;
    int* item = r.data() + ATTN_LOCAL_HDR;
    int* wave = item + 4 * nqb;
    int* rlo = wave + 16 * nqb;
    int* rhi = rlo + 256 * nqb;
    for (int i = 0; i < 256 * nqb; ++i) { rlo[i] = i < Ntok ? lo[i] : P; rhi[i] = i < Ntok ? hi[i] : Ntok; }   // rows past Ntok: dense
    for (int q = 0; q < nqb; ++q) {
        int e0 = Ntok, e1 = 0;   // the envelope of the non-empty windows of the item's rows
        for (int w = 0; w < 8; ++w) {
            int lm = P, hm = Ntok;
            bool any = false;
            for (int i = q * 256 + w * 32; i < std::min(q * 256 + w * 32 + 32, Ntok); ++i) {
                lm = any ? std::max(lm, lo[i]) : lo[i];
                hm = any ? std::min(hm, hi[i]) : hi[i];
                any = true;
                if (lo[i] < hi[i]) { e0 = std::min(e0, lo[i]); e1 = std::max(e1, hi[i]); }
            }
            wave[2 * (q * 8 + w)] = lm; wave[2 * (q * 8 + w) + 1] = hm;
        }
        int np = npre, w0 = npre, w1 = npre;
        if (e0 < e1) {
            w0 = e0 / KV_TILE; w1 = (e1 + KV_TILE - 1) / KV_TILE;
            if (w0 <= np) { np = std::max(np, w1); w0 = w1 = np; }   // the runs touch or overlap: one run
        }
        item[4 * q] = np; item[4 * q + 1] = w0; item[4 * q + 2] = w1; item[4 * q + 3] = np + (w1 - w0);
    }
    return 0;
}

// a box layer of a bf16 engine (and s2v_op_attention_box impl 0): attn_pp<BOX> at every length, persistent under the rule above
int launch_attn_bf16_box(const AttnArgs& a, const int* rec_dev, hipStream_t st) {
    S2V_REQUIRE(rec_dev != nullptr, "attn_bf16_box: local-attention record missing");
    S2V_REQUIRE(a.vt != nullptr, "attn_bf16_box: V^T buffer missing");
    S2V_REQUIRE(a.mx_q == nullptr && !a.p16, "attn_bf16_box: attn_pp writes bf16 and reads bf16 V^T (no MX output, no attn_p_format 1)");
    S2V_REQUIRE(a.ld_qkv % 8 == 0 && a.ntok_pad % 64 == 0, "attn_bf16_box: bad leading dims");
    S2V_REQUIRE(a.ntok_pad >= ((a.Ntok + 63) / 64) * 64, "attn_bf16_box: ntok_pad too small");
    int nqb8 = (a.Ntok + 255) / 256;
    int total = nqb8 * a.B * a.H;
    const bool persist = a.queue != nullptr && total > 2 * a.num_cus && a.num_cus >= 8;
    const void* fn = persist ? (const void*)attn_pp_box_persist_k : (const void*)attn_pp_box_k;
    S2V_TRY(ensure_lds_attr(fn, 65536));
    AttnArgs av = a;
    if (persist) {
        int* queue = a.queue;
        void* args[] = {(void*)&av, (void*)&nqb8, (void*)&total, (void*)&queue, (void*)&rec_dev};
        S2V_CHECK_HIP(hipLaunchKernel(fn, dim3((a.num_cus / 8) * 8), dim3(512), args, 65536, st));
    } else {
        void* args[] = {(void*)&av, (void*)&nqb8, (void*)&rec_dev};
        S2V_CHECK_HIP(hipLaunchKernel(fn, dim3(total), dim3(512), args, 65536, st));
    }
    return 0;
}

// host: the record (kernels.h "local attention in space and time") from P, S and the row table, every bound refused by name; the visit lists
// and the whole bits are made here, once per table, from each row's count of visible keys per tile
int attn_box_make(const char* who, int P, int S, int Ntok, const int* lo, const int* hi, const int* olo, const int* ohi, std::vector<int>* out) {
    static thread_local char msg[256];
#define BOX_REQUIRE(cond, ...) do { if (!(cond)) { snprintf(msg, sizeof(msg), __VA_ARGS__); S2V_REQUIRE(false, msg); } } while (0)
    BOX_REQUIRE(Ntok >= 1, "%s: Ntok = %d must be at least 1", who, Ntok);
    BOX_REQUIRE(lo && hi && olo && ohi, "%s: null row table", who);
    BOX_REQUIRE(P >= 1 && P <= Ntok, "%s: the prefix P = %d must lie inside [1, Ntok = %d] (key 0 is visible to every row)", who, P, Ntok);
    BOX_REQUIRE(S >= KV_TILE, "%s: the period S = %d must be at least 64 (a 64-key tile holds at most one frame boundary)", who, S);
    for (int i = 0; i < Ntok; ++i) {
        BOX_REQUIRE(P <= lo[i] && lo[i] <= hi[i] && hi[i] <= Ntok, "%s: row %d has the window [%d, %d): P = %d <= lo <= hi <= Ntok = %d is required", who, i,
                    lo[i], hi[i], P, Ntok);
        BOX_REQUIRE(0 <= olo[i] && olo[i] <= ohi[i] && ohi[i] <= S, "%s: row %d has the offsets [%d, %d): 0 <= olo <= ohi <= S = %d is required", who, i,
                    olo[i], ohi[i], S);
    }
#undef BOX_REQUIRE
    const int nqb = (Ntok + 255) / 256, nt = (Ntok + KV_TILE - 1) / KV_TILE, npre = (P + KV_TILE - 1) / KV_TILE;
    std::vector<int>& r = *out;
    r.assign(attn_box_ints(Ntok), 0);
    r[0] = P; r[1] = Ntok; r[2] = nqb; r[3] = S; r[4] = nt;
    int* item = r.data() + ATTN_BOX_HDR;
    int* rows = item + 8 * nqb;
    int* list = rows + 1024 * nqb;
    for (int i = 0; i < 256 * nqb; ++i) {   // rows past Ntok: dense
        const bool in = i < Ntok;
        rows[i] = in ? lo[i] : P;
        rows[256 * nqb + i] = in ? hi[i] - lo[i] : Ntok - P;
        rows[512 * nqb + i] = in ? olo[i] : 0;
        rows[768 * nqb + i] = in ? ohi[i] - olo[i] : S;
    }
    // per row only the tiles it sees are touched (the prefix range, then its box in each frame, ascending and disjoint): cnt[t] = the keys of tile t
    // the row sees, with the tiles listed in `hit` and cleared again; nfull[t] = the rows of the wave that see every key of tile t below Ntok
    std::vector<int> cnt((size_t)nt, 0), any((size_t)nt), full((size_t)nt), nfull((size_t)nt, 0), hit, whit, seen;
    auto add = [&](int a, int b) {   // the keys [a, b) are visible to the row
        for (int t = a / KV_TILE; a < b; ++t) {
            const int e = std::min(b, (t + 1) * KV_TILE);
            if (cnt[t] == 0) hit.push_back(t);
            cnt[t] += e - a;
            a = e;
        }
    };
    for (int q = 0; q < nqb; ++q) {
        std::fill(any.begin(), any.end(), 0);
        std::fill(full.begin(), full.end(), 0);
        for (int w = 0; w < 8; ++w) {
            const int i0 = q * 256 + w * 32, i1 = std::min(i0 + 32, Ntok);
            if (i0 >= i1) {   // a wave with no row below Ntok: its rows are stored dense
                for (int t = 0; t < nt; ++t) full[t] |= 1 << w;
                continue;
            }
            whit.clear();
            for (int i = i0; i < i1; ++i) {
                hit.clear();
                add(0, P);
                if (lo[i] < hi[i] && olo[i] < ohi[i])
                    for (long long base = P + (long long)((lo[i] - P) / S) * S; base < hi[i]; base += S)
                        add((int)std::max<long long>(base + olo[i], lo[i]), (int)std::min<long long>(base + ohi[i], hi[i]));
                for (int t : hit) {
                    any[t] = 1;
                    if (cnt[t] == std::min(KV_TILE, Ntok - t * KV_TILE)) {
                        if (nfull[t] == 0) whit.push_back(t);
                        ++nfull[t];
                    }
                    cnt[t] = 0;
                }
            }
            for (int t : whit) {
                if (nfull[t] == i1 - i0) full[t] |= 1 << w;
                nfull[t] = 0;
            }
        }
        seen.clear();
        for (int t = 0; t < nt; ++t)
            if (t < npre || any[t]) seen.push_back(t);
        const int n = (int)seen.size();   // >= 1: P >= 1 puts tile 0 first
        item[8 * q] = n;
        auto tile = [&](int x) { return seen[std::min(x, n - 1)]; };
        for (int j = 0; j < n; ++j) {
            int* e = list + ((size_t)q * nt + j) * 8;
            const int t = seen[j];
            e[0] = t;
            e[1] = (int)((((long long)t * KV_TILE - P) % S + S) % S);
            e[2] = full[t];
            e[3] = tile(j + 2); e[4] = tile(j + 4); e[5] = tile(j + 1); e[6] = tile(j + 3);
        }
    }
    return 0;
}

// host: the record from n ranges, refused by name when a range, a weight or the query range is wrong
int attn_steer_make(const char* who, int n, const int* k0, const int* k1, const float* w, const unsigned* sample_mask, int q0, int q1, int Ntok,
                    AttnSteerRec* out) {
    static thread_local char msg[256];
#define STEER_REQUIRE(cond, ...) do { if (!(cond)) { snprintf(msg, sizeof(msg), __VA_ARGS__); S2V_REQUIRE(false, msg); } } while (0)
    STEER_REQUIRE(n >= 0 && n <= ATTN_STEER_MAX_RANGES, "%s: 0..4 key ranges are accepted (n = %d)", who, n);
    STEER_REQUIRE(n == 0 || (k0 && k1 && w && sample_mask), "%s: null range array", who);
    STEER_REQUIRE(q0 >= 0 && q0 <= q1 && q1 <= Ntok, "%s: the query range [%d, %d) must lie inside [0, Ntok = %d)", who, q0, q1, Ntok);
    AttnSteerRec r{};
    r.n = n; r.q0 = q0; r.q1 = q1;
    for (int i = 0; i < n; ++i) {
        STEER_REQUIRE(k0[i] >= 0 && k0[i] < k1[i] && k1[i] <= Ntok, "%s: key range %d = [%d, %d) must be non-empty and inside [0, Ntok = %d)", who, i, k0[i], k1[i], Ntok);
        STEER_REQUIRE(i == 0 || k0[i] >= k1[i - 1], "%s: key range %d = [%d, %d) overlaps or precedes range %d (ranges are disjoint and ascending)", who, i, k0[i], k1[i], i - 1);
        STEER_REQUIRE(w[i] == w[i] && w[i] >= 1.52587890625e-05f && w[i] <= 65536.0f, "%s: weight %d = %g must be finite and inside [2^-16, 2^16] (no w = 0)", who, i, (double)w[i]);
        r.k0[i] = k0[i]; r.k1[i] = k1[i]; r.sample_mask[i] = sample_mask[i];
        r.log2w[i] = (float)log2((double)w[i]);
        r.lnw[i] = (float)log((double)w[i]);
    }
#undef STEER_REQUIRE
    *out = r;
    return 0;
}

// a mapped layer of a bf16 engine (and s2v_op_attention_steer_map impl 0): attn_pp<MAP> at every length, persistent under the rule above, or at
// any item count with force_persist (s2v_op_attention_steer_map impl 2: the persistent twin at a test's size; idle workgroups find no item and leave)
int launch_attn_bf16_steer_map(const AttnArgs& a, const AttnSteerMapRec* rec_dev, hipStream_t st, bool force_persist) {
    S2V_REQUIRE(rec_dev != nullptr, "attn_bf16_steer_map: map record missing");
    S2V_REQUIRE(a.vt != nullptr, "attn_bf16_steer_map: V^T buffer missing");
    S2V_REQUIRE(a.mx_q == nullptr && !a.p16, "attn_bf16_steer_map: attn_pp writes bf16 and reads bf16 V^T (no MX output, no attn_p_format 1)");
    S2V_REQUIRE(a.ld_qkv % 8 == 0 && a.ntok_pad % 64 == 0, "attn_bf16_steer_map: bad leading dims");
    S2V_REQUIRE(a.ntok_pad >= ((a.Ntok + 63) / 64) * 64, "attn_bf16_steer_map: ntok_pad too small");
    S2V_REQUIRE(a.B >= 1 && a.B <= ATTN_STEER_MAP_BATCH, "attn_bf16_steer_map: a plane index is held for 8 samples");
    int nqb8 = (a.Ntok + 255) / 256;
    int total = nqb8 * a.B * a.H;
    const bool persist = a.queue != nullptr && a.num_cus >= 8 && (force_persist || total > 2 * a.num_cus);
    const void* fn = persist ? (const void*)attn_pp_steer_map_persist_k : (const void*)attn_pp_steer_map_k;
    S2V_TRY(ensure_lds_attr(fn, 65536));
    AttnArgs av = a;
    if (persist) {
        int* queue = a.queue;
        void* args[] = {(void*)&av, (void*)&nqb8, (void*)&total, (void*)&queue, (void*)&rec_dev};
        S2V_CHECK_HIP(hipLaunchKernel(fn, dim3((a.num_cus / 8) * 8), dim3(512), args, 65536, st));
    } else {
        void* args[] = {(void*)&av, (void*)&nqb8, (void*)&rec_dev};
        S2V_CHECK_HIP(hipLaunchKernel(fn, dim3(total), dim3(512), args, 65536, st));
    }
    return 0;
}

// host: the wave liveness table of a map record (kernels.h AttnSteerMapRec), from the weights themselves: w != 1, not log2 w != 0
void attn_steer_map_wave_flags(int n, int q0, int q1, int Ntok, const signed char* plane, const float* planes, int* out) {
    const int nqb = (Ntok + 255) / 256, V = q1 - q0;
    for (int b = 0; b < ATTN_STEER_MAP_BATCH; ++b)
        for (int w = 0; w < 8 * nqb; ++w) {
            int bits = 0;
            const int i0 = std::max(w * 32, q0), i1 = std::min(std::min(w * 32 + 32, q1), Ntok);
            for (int r = 0; r < n; ++r) {
                const int p = plane[r * ATTN_STEER_MAP_BATCH + b];
                if (p < 0) continue;
                for (int i = i0; i < i1; ++i)
                    if (planes[(size_t)p * V + (i - q0)] != 1.0f) { bits |= 1 << r; break; }
            }
            out[(size_t)b * 8 * nqb + w] = bits;
        }
}

int attn_steer_map_make(const char* who, int n, const int* k0, const int* k1, const signed char* plane, int n_planes, const float* planes,
                        int q0, int q1, int Ntok, int B, int cap_planes, std::vector<int>* out) {
    static thread_local char msg[256];
#define MAP_REQUIRE(cond, ...) do { if (!(cond)) { snprintf(msg, sizeof(msg), __VA_ARGS__); S2V_REQUIRE(false, msg); } } while (0)
    MAP_REQUIRE(n >= 0 && n <= ATTN_STEER_MAX_RANGES, "%s: 0..4 key ranges are accepted (n = %d)", who, n);
    MAP_REQUIRE(n == 0 || (k0 && k1 && plane), "%s: null range array", who);
    MAP_REQUIRE(B >= 1 && B <= ATTN_STEER_MAP_BATCH, "%s: 1 <= B <= 8 samples (a plane index is held per range and sample; B = %d)", who, B);
    MAP_REQUIRE(q0 >= 0 && q0 < q1 && q1 <= Ntok, "%s: the query range [%d, %d) must be non-empty and lie inside [0, Ntok = %d) (a plane holds q1 - q0 weights)", who, q0,
                q1, Ntok);
    MAP_REQUIRE(n_planes >= 1 && n_planes <= ATTN_STEER_MAP_MAX_PLANES, "%s: 1..16 planes are accepted (n_planes = %d)", who, n_planes);
    MAP_REQUIRE(cap_planes >= n_planes && cap_planes <= ATTN_STEER_MAP_MAX_PLANES, "%s: the allocation holds %d planes, the record has %d", who, cap_planes, n_planes);
    MAP_REQUIRE(planes != nullptr, "%s: null plane pointer", who);
    for (int i = 0; i < n; ++i) {
        MAP_REQUIRE(k0[i] >= 0 && k0[i] < k1[i] && k1[i] <= Ntok, "%s: key range %d = [%d, %d) must be non-empty and inside [0, Ntok = %d)", who, i, k0[i], k1[i], Ntok);
        MAP_REQUIRE(i == 0 || k0[i] >= k1[i - 1], "%s: key range %d = [%d, %d) overlaps or precedes range %d (ranges are disjoint and ascending)", who, i, k0[i], k1[i], i - 1);
        for (int b = 0; b < ATTN_STEER_MAP_BATCH; ++b) {
            const int p = plane[i * ATTN_STEER_MAP_BATCH + b];
            MAP_REQUIRE(p >= -1 && p < n_planes, "%s: plane index %d of range %d, sample %d lies outside [-1, n_planes = %d)", who, p, i, b, n_planes);
            MAP_REQUIRE(b < B || p == -1, "%s: range %d names plane %d on sample %d, at or beyond B = %d (such entries are -1)", who, i, p, b, B);
        }
    }
    const int V = q1 - q0;
    for (int p = 0; p < n_planes; ++p)
        for (int v = 0; v < V; ++v) {
            const float w = planes[(size_t)p * V + v];
            MAP_REQUIRE(w == w && w >= 1.52587890625e-05f && w <= 65536.0f, "%s: plane %d, cell %d: weight %g must be finite and inside [2^-16, 2^16] (no w = 0)", who, p, v,
                        (double)w);
        }
#undef MAP_REQUIRE
    std::vector<int>& r = *out;
    r.assign(attn_steer_map_words(Ntok, V, cap_planes), 0);
    AttnSteerMapRec h{};
    h.n = n; h.q0 = q0; h.q1 = q1; h.n_planes = n_planes;
    for (int i = 0; i < ATTN_STEER_MAX_RANGES; ++i)
        for (int b = 0; b < ATTN_STEER_MAP_BATCH; ++b) h.plane[i][b] = -1;
    for (int i = 0; i < n; ++i) {
        h.k0[i] = k0[i]; h.k1[i] = k1[i];
        for (int b = 0; b < ATTN_STEER_MAP_BATCH; ++b) h.plane[i][b] = plane[i * ATTN_STEER_MAP_BATCH + b];
    }
    h.nqb = (Ntok + 255) / 256;
    h.off_log2 = ATTN_STEER_MAP_HDR;
    h.off_ln = h.off_log2 + cap_planes * V;
    h.off_live = h.off_ln + cap_planes * V;
    *(AttnSteerMapRec*)r.data() = h;
    float* l2 = (float*)r.data() + h.off_log2;
    float* ln = (float*)r.data() + h.off_ln;
    for (size_t i = 0; i < (size_t)n_planes * V; ++i) {   // the expressions of attn_steer_make: a constant plane is the scalar record's bits
        l2[i] = (float)log2((double)planes[i]);
        ln[i] = (float)log((double)planes[i]);
    }
    attn_steer_map_wave_flags(n, q0, q1, Ntok, &h.plane[0][0], planes, r.data() + h.off_live);
    return 0;
}
// the liveness table for a test against brute force: out is [8][8 ceil(Ntok / 256)] int32; no check beyond null pointers (the caller's record is valid)
extern "C" __attribute__((visibility("default"))) int s2v_attn_steer_map_wave_flags(int n, int q0, int q1, int Ntok, const signed char* plane,
                                                                                    const float* planes, int* out) {
    S2V_REQUIRE(plane && planes && out && n >= 0 && n <= ATTN_STEER_MAX_RANGES && q0 >= 0 && q0 < q1 && q1 <= Ntok, "s2v_attn_steer_map_wave_flags: bad argument");
    attn_steer_map_wave_flags(n, q0, q1, Ntok, plane, planes, out);
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// TWIN: attn_simple_steer_k below repeats this body with the bias added to the score (a shared function changed this kernel's code): a change
// here is made there as well.
template <typename T>
__global__ __launch_bounds__(256) void attn_simple_k(const AttnArgs a) {
    __shared__ float sq[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
    const int D = a.H * 64;
    const bool active = q < a.Ntok;
    const T* base = (const T*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    const int ql = active ? q : a.Ntok - 1;
    sq[wave][lane] = ET<T>::ld(base + (size_t)ql * a.ld_qkv + h * 64 + lane) * a.scale;
    __syncthreads();
    float m = -INFINITY, l = 0.f, o = 0.f;
    for (int kv0 = 0; kv0 < a.Ntok; kv0 += 64) {
        const int kv = kv0 + lane;
        float s = -INFINITY;
        if (kv < a.Ntok) {
            const T* kp = base + (size_t)kv * a.ld_qkv + D + h * 64;
            float acc = 0.f;
#pragma unroll 8
            for (int d = 0; d < 64; ++d) acc = fmaf(sq[wave][d], ET<T>::ld(kp + d), acc);
            s = acc;
        }
        const float mx = wave_max(s);
        const float mn = fmaxf(m, mx);
        const float alpha = expf(m - mn);
        const float p = expf(s - mn);
        l = l * alpha + wave_sum(p);
        o *= alpha;
        m = mn;
        const int nv = min(64, a.Ntok - kv0);
        for (int j = 0; j < nv; ++j) {
            const float pj = __shfl(p, j, 64);
            o = fmaf(pj, ET<T>::ld(base + (size_t)(kv0 + j) * a.ld_qkv + 2 * D + h * 64 + lane), o);
        }
    }
    if (active) ET<T>::st((T*)a.out + (size_t)(b * a.Ntok + q) * a.ld_out + h * 64 + lane, o / l);
}
// the steered form of attn_simple_k (a twin, so that the kernel above keeps its code): beta = ln w of the key's range (AttnSteerRec::lnw) is added
// to the score of an in-range key before the maximum and expf, on the query rows and samples the record names.  Speed is no goal here: fp32 is
// the parity mode, and this form is the second implementation the steered MFMA kernel is checked against.
template <typename T>
__global__ __launch_bounds__(256) void attn_simple_steer_k(const AttnArgs a, const AttnSteerRec* __restrict__ sr) {
    __shared__ float sq[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
    const int D = a.H * 64;
    const bool active = q < a.Ntok;
    const T* base = (const T*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    const int ql = active ? q : a.Ntok - 1;
    sq[wave][lane] = ET<T>::ld(base + (size_t)ql * a.ld_qkv + h * 64 + lane) * a.scale;
    __syncthreads();
    const bool steer_row = q >= sr->q0 && q < sr->q1;
    float m = -INFINITY, l = 0.f, o = 0.f;
    for (int kv0 = 0; kv0 < a.Ntok; kv0 += 64) {
        const int kv = kv0 + lane;
        float s = -INFINITY;
        if (kv < a.Ntok) {
            const T* kp = base + (size_t)kv * a.ld_qkv + D + h * 64;
            float acc = 0.f;
#pragma unroll 8
            for (int d = 0; d < 64; ++d) acc = fmaf(sq[wave][d], ET<T>::ld(kp + d), acc);
            s = acc;
            if (steer_row) {
#pragma unroll
                for (int r = 0; r < ATTN_STEER_MAX_RANGES; ++r)
                    if (r < sr->n && kv >= sr->k0[r] && kv < sr->k1[r] && ((sr->sample_mask[r] >> b) & 1u)) s += sr->lnw[r];
            }
        }
        const float mx = wave_max(s);
        const float mn = fmaxf(m, mx);
        const float alpha = expf(m - mn);
        const float p = expf(s - mn);
        l = l * alpha + wave_sum(p);
        o *= alpha;
        m = mn;
        const int nv = min(64, a.Ntok - kv0);
        for (int j = 0; j < nv; ++j) {
            const float pj = __shfl(p, j, 64);
            o = fmaf(pj, ET<T>::ld(base + (size_t)(kv0 + j) * a.ld_qkv + 2 * D + h * 64 + lane), o);
        }
    }
    if (active) ET<T>::st((T*)a.out + (size_t)(b * a.Ntok + q) * a.ld_out + h * 64 + lane, o / l);
}

// fp16 model dtype: qkv / out fp16, a.vt = V^T [B][H][64][ntok_pad] fp16 in the k-slot order (launch_v_transpose moves 16-bit elements: the bf16
// pass serves fp16 input unchanged)
int launch_attn_f16(const AttnArgs& a, hipStream_t st) {
    S2V_REQUIRE(a.vt != nullptr && a.ntok_pad % 64 == 0 && a.ld_qkv % 8 == 0, "attn_f16: V^T scratch / padding / leading dimension");
    // long sequences: the four-wave generated-asm kernel (fp16 q / k / P: attn_q4hh), persistent when the caller brought a queue; short ones
    // (where attn_q4's long pipeline does not pay, as in bf16) the lock-step kernel below
    if (a.Ntok > ATTN_PP_MAX_TOKENS) return launch_attn_q4hh(a, a.queue != nullptr && a.num_cus >= 8, st);
    const int nqb = (a.Ntok + 255) / 256, total = nqb * a.B * a.H;
    hipLaunchKernelGGL((attn_bf16_k<0, 8, f16_t>), dim3(total), dim3(512), 4 * ATT_TILE_BYTES, st, a, nqb);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_attn_simple(const AttnArgs& a, int dtype, hipStream_t st) {
    if ((dtype == S2V_F32 || dtype == S2V_F16) && !a.valu_only) return launch_attn_f32m(a, dtype, st);
    dim3 grid((a.Ntok + 3) / 4, a.H, a.B);
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(attn_simple_k<T>, grid, dim3(256), 0, st, a))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_attn_simple_steer(const AttnArgs& a, const AttnSteerRec* rec_dev, int dtype, hipStream_t st) {
    S2V_REQUIRE(rec_dev != nullptr, "attn_simple_steer: steer record missing");
    S2V_REQUIRE(a.B >= 1 && a.B <= 32, "attn_simple_steer: the sample masks hold 32 samples");
    dim3 grid((a.Ntok + 3) / 4, a.H, a.B);
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(attn_simple_steer_k<T>, grid, dim3(256), 0, st, a, rec_dev))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// the mapped form of attn_simple_steer_k (steering maps, kernels.h AttnSteerMapRec; a twin again): beta = ln W_p[q - q0] of the key's range and the
// sample's plane.  It reads no liveness table: a weight of 1 adds ln 1 = 0.0f.
template <typename T>
__global__ __launch_bounds__(256) void attn_simple_steer_map_k(const AttnArgs a, const AttnSteerMapRec* __restrict__ mr) {
    __shared__ float sq[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
    const int D = a.H * 64;
    const bool active = q < a.Ntok;
    const T* base = (const T*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    const int ql = active ? q : a.Ntok - 1;
    sq[wave][lane] = ET<T>::ld(base + (size_t)ql * a.ld_qkv + h * 64 + lane) * a.scale;
    __syncthreads();
    const bool steer_row = q >= mr->q0 && q < mr->q1;
    const int vq = mr->q1 - mr->q0;
    const float* lp = (const float*)mr + mr->off_ln + min(max(q - mr->q0, 0), vq - 1);
    const int bs = min(b, ATTN_STEER_MAP_BATCH - 1);
    float m = -INFINITY, l = 0.f, o = 0.f;
    for (int kv0 = 0; kv0 < a.Ntok; kv0 += 64) {
        const int kv = kv0 + lane;
        float s = -INFINITY;
        if (kv < a.Ntok) {
            const T* kp = base + (size_t)kv * a.ld_qkv + D + h * 64;
            float acc = 0.f;
#pragma unroll 8
            for (int d = 0; d < 64; ++d) acc = fmaf(sq[wave][d], ET<T>::ld(kp + d), acc);
            s = acc;
            if (steer_row) {
#pragma unroll
                for (int r = 0; r < ATTN_STEER_MAX_RANGES; ++r) {
                    const int p = mr->plane[r][bs];
                    if (r < mr->n && kv >= mr->k0[r] && kv < mr->k1[r] && p >= 0) s += lp[p * vq];
                }
            }
        }
        const float mx = wave_max(s);
        const float mn = fmaxf(m, mx);
        const float alpha = expf(m - mn);
        const float p = expf(s - mn);
        l = l * alpha + wave_sum(p);
        o *= alpha;
        m = mn;
        const int nv = min(64, a.Ntok - kv0);
        for (int j = 0; j < nv; ++j) {
            const float pj = __shfl(p, j, 64);
            o = fmaf(pj, ET<T>::ld(base + (size_t)(kv0 + j) * a.ld_qkv + 2 * D + h * 64 + lane), o);
        }
    }
    if (active) ET<T>::st((T*)a.out + (size_t)(b * a.Ntok + q) * a.ld_out + h * 64 + lane, o / l);
}

int launch_attn_simple_steer_map(const AttnArgs& a, const AttnSteerMapRec* rec_dev, int dtype, hipStream_t st) {
    S2V_REQUIRE(rec_dev != nullptr, "attn_simple_steer_map: map record missing");
    S2V_REQUIRE(a.B >= 1 && a.B <= ATTN_STEER_MAP_BATCH, "attn_simple_steer_map: a plane index is held for 8 samples");
    dim3 grid((a.Ntok + 3) / 4, a.H, a.B);
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(attn_simple_steer_map_k<T>, grid, dim3(256), 0, st, a, rec_dev))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// the local form of attn_simple_k (a twin once more, so that the kernel above keeps its code): a key the row does not see gets the score -inf before
// the maximum and expf, and a 64-key tile the row sees nothing of is skipped.  Tile 0 holds key 0, which every row sees (P >= 1), so the running
// maximum is finite from the first tile on.  Speed is no goal here: it is what an fp32 engine runs on a local layer, and the second implementation
// the MFMA kernel is checked against.
template <typename T>
__global__ __launch_bounds__(256) void attn_simple_local_k(const AttnArgs a, const int* __restrict__ lr) {
    __shared__ float sq[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
    const int D = a.H * 64;
    const bool active = q < a.Ntok;
    const T* base = (const T*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    const int ql = active ? q : a.Ntok - 1;
    sq[wave][lane] = ET<T>::ld(base + (size_t)ql * a.ld_qkv + h * 64 + lane) * a.scale;
    __syncthreads();
    const int P = lr[0], nq = lr[2];
    const int lo = lr[ATTN_LOCAL_HDR + 20 * nq + ql], up = lr[ATTN_LOCAL_HDR + 276 * nq + ql];
    float m = -INFINITY, l = 0.f, o = 0.f;
    for (int kv0 = 0; kv0 < a.Ntok; kv0 += 64) {
        if (!(kv0 < P || (kv0 < up && kv0 + 64 > lo))) continue;  // the row sees no key of this tile
        const int kv = kv0 + lane;
        float s = -INFINITY;
        if (kv < a.Ntok && (kv < P || (unsigned)(kv - lo) < (unsigned)(up - lo))) {
            const T* kp = base + (size_t)kv * a.ld_qkv + D + h * 64;
            float acc = 0.f;
#pragma unroll 8
            for (int d = 0; d < 64; ++d) acc = fmaf(sq[wave][d], ET<T>::ld(kp + d), acc);
            s = acc;
        }
        const float mx = wave_max(s);
        const float mn = fmaxf(m, mx);
        const float alpha = expf(m - mn);
        const float p = expf(s - mn);
        l = l * alpha + wave_sum(p);
        o *= alpha;
        m = mn;
        const int nv = min(64, a.Ntok - kv0);
        for (int j = 0; j < nv; ++j) {
            const float pj = __shfl(p, j, 64);
            o = fmaf(pj, ET<T>::ld(base + (size_t)(kv0 + j) * a.ld_qkv + 2 * D + h * 64 + lane), o);
        }
    }
    if (active) ET<T>::st((T*)a.out + (size_t)(b * a.Ntok + q) * a.ld_out + h * 64 + lane, o / l);
}

int launch_attn_simple_local(const AttnArgs& a, const int* rec_dev, int dtype, hipStream_t st) {
    S2V_REQUIRE(rec_dev != nullptr, "attn_simple_local: local-attention record missing");
    dim3 grid((a.Ntok + 3) / 4, a.H, a.B);
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(attn_simple_local_k<T>, grid, dim3(256), 0, st, a, rec_dev))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// the box form of attn_simple_k (a twin once more): a key the row does not see -- outside the prefix and outside the box of frames and frame offsets --
// gets the score -inf before the maximum and expf, and a 64-key tile the row sees nothing of is skipped.  Tile 0 holds key 0, which every row
// sees (P >= 1).  It is what an fp32 engine runs on a box layer, and the second implementation the MFMA kernel is checked against.
template <typename T>
__global__ __launch_bounds__(256) void attn_simple_box_k(const AttnArgs a, const int* __restrict__ lr) {
    __shared__ float sq[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
    const int D = a.H * 64;
    const bool active = q < a.Ntok;
    const T* base = (const T*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    const int ql = active ? q : a.Ntok - 1;
    sq[wave][lane] = ET<T>::ld(base + (size_t)ql * a.ld_qkv + h * 64 + lane) * a.scale;
    __syncthreads();
    const int P = lr[0], nq = lr[2], S = lr[3];
    const int* rw = lr + ATTN_BOX_HDR + 8 * nq + ql;
    const int lo = rw[0], olo = rw[512 * nq];
    const unsigned len = (unsigned)rw[256 * nq], olen = (unsigned)rw[768 * nq];
    float m = -INFINITY, l = 0.f, o = 0.f;
    for (int kv0 = 0; kv0 < a.Ntok; kv0 += 64) {
        const int kv = kv0 + lane;
        const bool vis = kv < a.Ntok && (kv < P || ((unsigned)(kv - lo) < len && (unsigned)((kv - P) % S - olo) < olen));
        if (!__any(vis)) continue;  // the row sees no key of this tile
        float s = -INFINITY;
        if (vis) {
            const T* kp = base + (size_t)kv * a.ld_qkv + D + h * 64;
            float acc = 0.f;
#pragma unroll 8
            for (int d = 0; d < 64; ++d) acc = fmaf(sq[wave][d], ET<T>::ld(kp + d), acc);
            s = acc;
        }
        const float mx = wave_max(s);
        const float mn = fmaxf(m, mx);
        const float alpha = expf(m - mn);
        const float p = expf(s - mn);
        l = l * alpha + wave_sum(p);
        o *= alpha;
        m = mn;
        const int nv = min(64, a.Ntok - kv0);
        for (int j = 0; j < nv; ++j) {
            const float pj = __shfl(p, j, 64);
            o = fmaf(pj, ET<T>::ld(base + (size_t)(kv0 + j) * a.ld_qkv + 2 * D + h * 64 + lane), o);
        }
    }
    if (active) ET<T>::st((T*)a.out + (size_t)(b * a.Ntok + q) * a.ld_out + h * 64 + lane, o / l);
}

int launch_attn_simple_box(const AttnArgs& a, const int* rec_dev, int dtype, hipStream_t st) {
    S2V_REQUIRE(rec_dev != nullptr, "attn_simple_box: local-attention record missing");
    dim3 grid((a.Ntok + 3) / 4, a.H, a.B);
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(attn_simple_box_k<T>, grid, dim3(256), 0, st, a, rec_dev))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}
