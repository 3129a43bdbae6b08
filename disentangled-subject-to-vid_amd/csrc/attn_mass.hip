// Attention mass: how much of a query's softmax weight falls on up to four key ranges -- flash attention without V.
//   s_ij = q_i . k_j / 8 over the sample's own Ntok keys,  mass_r(b, h, i) = sum_{j in [k0_r, k1_r)} softmax_j(s_i.)   (fp32)
// The engine runs it on c->QKV right after a block's attention (s2v_attn_map_arm), where q and k are normed and rotated: range 0 is the
// reference-image stream, so the mass of a video query says where in the video the subject lands (include/s2v_hip.h, "Attention map").
//
// attn_mass_mfma_k (impl 0, bf16 / fp16 storage): one workgroup = 4 waves x 32 query rows of one (sample, head); KV tiles of 64 keys,
// double-buffered in LDS as they sit in memory ([key][64 d], rows 144 bytes apart).  The tile is computed TRANSPOSED,
//   S^T[key][q] = sum_d K[key][d] Qs[q][d]     2 x 4 v_mfma_f32_32x32x16: A = 8 consecutive d of key row (lane & 31), B = the same d of the
//                                              wave's query (lane & 31), held in 16 registers for the whole launch
// so a lane owns ONE query column and 16 of a sub-tile's 32 keys (register e: key (e & 3) + 8 (e >> 2) + 4 (lane >> 5); the other 16 sit in
// lane ^ 32): maximum, sum over all keys and sums per range are in-register reductions plus one v_permlane32_swap -- no LDS transpose, no P
// tile.  Qs = q * 0.125 * log2 e rounded to the storage type, as the product attention kernels round it, and exp2.  A range test is a
// compare of the key index per register, and only in the tiles a range boundary cuts: a tile wholly inside a range adds the tile sum, one
// wholly outside adds nothing.
//
// attn_mass_simple_k (impl 1, any dtype): one wave per (query, head, sample) on the VALU -- q * 0.125, an fmaf chain over the head
// dimension, expf, a true division.  What an fp32 engine runs (the parity mode against the CPU oracle), and the second implementation.
//
// Both write out[r][b][h][i - q0]; accumulate: out + mass in ONE fp32 add by the thread that owns the element (no atomics, and this file is
// built without fma contraction, so two accumulated launches are the fp32 sum of two plain ones bit for bit).
#define S2V_HOST
#include "common.h"
#include "kernels.h"
#include <type_traits>

#define AM_QROWS 128  // query rows per workgroup
#define AM_KTILE 64   // keys per KV tile
#define AM_PITCH 72   // 16-bit elements per key row of the LDS image (64 + 8)

template <bool H16>
__global__ __launch_bounds__(256) void attn_mass_mfma_k(const AttnMassArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short sK[2][AM_KTILE][AM_PITCH];
    using T = typename std::conditional<H16, f16_t, bf16_t>::type;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, hi = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int D = a.H * 64;
    const T* base = (const T*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    const int q = a.q0 + blockIdx.x * AM_QROWS + wave * 32 + fr;
    const int ql = min(q, a.Ntok - 1);   // a ragged last query tile loads a real row and stores nothing
    // B operand of k-step s: Qs[q][16 s + 8 hi + j], j = 0..7
    u32x4 qf[4];
    {
        const T* qp = base + (size_t)ql * a.ld_qkv + h * 64 + 8 * hi;
        const float c0 = 0.125f * 1.4426950408889634f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float v[8];
            Vec16<T>::ld(qp + 16 * s, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (H16) qf[s][j] = pack2h(v[2 * j] * c0, v[2 * j + 1] * c0);
                else qf[s][j] = pack2bf(v[2 * j] * c0, v[2 * j + 1] * c0);
            }
        }
    }
    // staging of a KV tile: 64 keys x 128 bytes = 512 chunks of 16 bytes, two per thread
    const int skey = tid >> 2, sc = tid & 3;
    u32x4 rk[2];
    auto gload = [&](int kv0) {
        const int key = min(kv0 + skey, a.Ntok - 1);   // never past the sample's last row: the tail is masked below
        const T* kp = base + (size_t)key * a.ld_qkv + D + h * 64;
        rk[0] = *(const u32x4*)(kp + sc * 8);
        rk[1] = *(const u32x4*)(kp + (sc + 4) * 8);
    };
    auto lstore = [&](int buf) {
        *(u32x4*)&sK[buf][skey][sc * 8] = rk[0];
        *(u32x4*)&sK[buf][skey][(sc + 4) * 8] = rk[1];
    };
    auto mfma = [](const u32x4& x, const u32x4& y, const f32x16& acc) -> f32x16 {
        if constexpr (H16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, x), __builtin_bit_cast(f16x8, y), acc, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, y), acc, 0, 0, 0);
    };
    float m = -INFINITY, l = 0.f;   // running maximum of the query row; this lane's share of the sum over all keys
    float rs[AM_MAX_RANGES];        // ... and of the sum over each range
#pragma unroll
    for (int r = 0; r < AM_MAX_RANGES; ++r) rs[r] = 0.f;

    const int ntile = (a.Ntok + AM_KTILE - 1) / AM_KTILE;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
        const int buf = t & 1, kv0 = t * AM_KTILE;
        if (t + 1 < ntile) gload(kv0 + AM_KTILE);
        f32x16 s[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[u][e] = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) s[u] = mfma(*(const u32x4*)&sK[buf][32 * u + fr][16 * i + 8 * hi], qf[i], s[u]);
        }
        // register e of sub-tile u: key kv0 + 32 u + (e & 3) + 8 (e >> 2) + 4 hi
        const int kb = kv0 + 4 * hi;
        if (kv0 + AM_KTILE > a.Ntok) {   // the ragged last tile: masked before the maximum
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (kb + 32 * u + (e & 3) + 8 * (e >> 2) >= a.Ntok) s[u][e] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[u][e]);
        {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        const float mn = fmaxf(m, mx);   // finite: every tile holds at least one real key
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s[u][e] = __builtin_amdgcn_exp2f(s[u][e] - mn);
                ps += s[u][e];
            }
        l = l * alpha + ps;
#pragma unroll
        for (int r = 0; r < AM_MAX_RANGES; ++r) {
            if (r >= a.n) break;
            const int k0 = a.k0[r], k1 = a.k1[r];
            if (k1 <= kv0 || k0 >= kv0 + AM_KTILE || k0 >= k1) {   // the tile holds no key of the range
                rs[r] *= alpha;
            } else if (k0 <= kv0 && k1 >= min(kv0 + AM_KTILE, a.Ntok)) {   // every real key of the tile (masked ones are exact zeros)
                rs[r] = rs[r] * alpha + ps;
            } else {   // a boundary runs through the tile: the key index of every register, in the order of ps
                float pr = 0.f;
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int key = kb + 32 * u + (e & 3) + 8 * (e >> 2);
                        pr += (key >= k0 && key < k1) ? s[u][e] : 0.f;
                    }
                rs[r] = rs[r] * alpha + pr;
            }
        }
        if (t + 1 < ntile) lstore(buf ^ 1);
        __syncthreads();
    }
    {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
        l = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    const float rl = __builtin_amdgcn_rcpf(l);
#pragma unroll
    for (int r = 0; r < AM_MAX_RANGES; ++r) {
        if (r >= a.n) break;
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(rs[r]), __float_as_uint(rs[r]), false, false);
        const float mass = (__uint_as_float(sw[0]) + __uint_as_float(sw[1])) * rl;
        if (hi == 0 && q < a.q0 + a.nq) {
            float* op = a.out + (((size_t)r * a.B + b) * a.H + h) * a.nq + (q - a.q0);
            *op = a.accumulate ? *op + mass : mass;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64) void attn_mass_simple_k(const AttnMassArgs a) {
    __shared__ float sq[64];
    const int lane = threadIdx.x;
    const int q = a.q0 + blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int D = a.H * 64;
    const T* base = (const T*)a.qkv + (size_t)b * a.Ntok * a.ld_qkv;
    sq[lane] = ET<T>::ld(base + (size_t)q * a.ld_qkv + h * 64 + lane) * 0.125f;
    __syncthreads();
    // every lane runs an online softmax over its keys j = lane, lane + 64, ...; the lanes meet at the end
    float m = -INFINITY, l = 0.f, rs[AM_MAX_RANGES];
#pragma unroll
    for (int r = 0; r < AM_MAX_RANGES; ++r) rs[r] = 0.f;
    for (int j = lane; j < a.Ntok; j += 64) {
        const T* kp = base + (size_t)j * a.ld_qkv + D + h * 64;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 64; c += Vec16<T>::N) {
            float kv[Vec16<T>::N];
            Vec16<T>::ld(kp + c, kv);
#pragma unroll
            for (int e = 0; e < Vec16<T>::N; ++e) s = fmaf(sq[c + e], kv[e], s);
        }
        const float mn = fmaxf(m, s);
        const float alpha = expf(m - mn), p = expf(s - mn);
        m = mn;
        l = l * alpha + p;
#pragma unroll
        for (int r = 0; r < AM_MAX_RANGES; ++r)
            if (r < a.n) rs[r] = rs[r] * alpha + ((j >= a.k0[r] && j < a.k1[r]) ? p : 0.f);
    }
    const float M = wave_max(m);
    const float w = l > 0.f ? expf(m - M) : 0.f;   // a lane without keys (Ntok < 64) brings nothing
    l = wave_sum(l * w);
#pragma unroll
    for (int r = 0; r < AM_MAX_RANGES; ++r) {
        if (r >= a.n) break;
        const float mass = wave_sum(rs[r] * w) / l;
        if (lane == 0) {
            float* op = a.out + (((size_t)r * a.B + b) * a.H + h) * a.nq + (q - a.q0);
            *op = a.accumulate ? *op + mass : mass;
        }
    }
}

int launch_attn_mass(const AttnMassArgs& a, int dtype, int impl, hipStream_t st) {
    S2V_REQUIRE(a.qkv && a.out, "attn_mass: null argument");
    S2V_REQUIRE(a.B >= 1 && a.B <= 65535 && a.H >= 1 && a.H <= 65535 && a.Ntok >= 1, "attn_mass: bad shape");
    S2V_REQUIRE(a.n >= 1 && a.n <= AM_MAX_RANGES, "attn_mass: the number of key ranges must be 1..4");
    for (int r = 0; r < a.n; ++r)
        S2V_REQUIRE(a.k0[r] >= 0 && a.k0[r] <= a.k1[r] && a.k1[r] <= a.Ntok, "attn_mass: a key range must satisfy 0 <= k0 <= k1 <= Ntok");
    S2V_REQUIRE(a.q0 >= 0 && a.nq >= 1 && (int64_t)a.q0 + a.nq <= a.Ntok, "attn_mass: the query rows [q0, q0 + nq) must lie inside the sample (q0 + nq <= Ntok)");
    S2V_REQUIRE(impl == 0 || impl == 1, "attn_mass: impl is 0 (matrix pipe) or 1 (generic)");
    S2V_REQUIRE(dtype == S2V_F32 || dtype == S2V_BF16 || dtype == S2V_F16, "attn_mass: dtype must be f32, bf16 or f16");
    if (impl == 0) {
        S2V_REQUIRE(dtype != S2V_F32, "attn_mass: impl 0 (matrix pipe) runs bf16 / fp16 storage; fp32 runs impl 1");
        S2V_REQUIRE(a.ld_qkv % 8 == 0 && ((uintptr_t)a.qkv & 15) == 0, "attn_mass: impl 0 needs qkv 16-byte aligned with a leading dimension that is a multiple of 8");
        const dim3 grid((a.nq + AM_QROWS - 1) / AM_QROWS, a.H, a.B);
        if (dtype == S2V_F16) hipLaunchKernelGGL(attn_mass_mfma_k<true>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(attn_mass_mfma_k<false>, grid, dim3(256), 0, st, a);
    } else {
        S2V_REQUIRE(a.ld_qkv % 8 == 0 && ((uintptr_t)a.qkv & 15) == 0, "attn_mass: qkv must be 16-byte aligned with a leading dimension that is a multiple of 8");
        const dim3 grid(a.nq, a.H, a.B);
        if (dtype == S2V_F32) hipLaunchKernelGGL(attn_mass_simple_k<float>, grid, dim3(64), 0, st, a);
        else if (dtype == S2V_BF16) hipLaunchKernelGGL(attn_mass_simple_k<bf16_t>, grid, dim3(64), 0, st, a);
        else hipLaunchKernelGGL(attn_mass_simple_k<f16_t>, grid, dim3(64), 0, st, a);
    }
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// mean[nb][i] = (sum over h = 0 .. H-1, in that order, of acc[nb][h][i]) * inv
__global__ __launch_bounds__(256) void attn_mass_mean_k(const float* __restrict__ acc, float* __restrict__ out, int64_t total, int H, int nq, float inv) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int64_t nb = idx / nq, i = idx - nb * nq;
    const float* p = acc + nb * H * nq + i;
    float s = 0.f;
    for (int h = 0; h < H; ++h) s += p[(int64_t)h * nq];
    out[idx] = s * inv;
}

int launch_attn_mass_mean(const float* acc, int n, int B, int H, int nq, int64_t count, float* out, hipStream_t st) {
    S2V_REQUIRE(acc && out && n >= 1 && B >= 1 && H >= 1 && nq >= 1 && count >= 1, "attn_mass_mean: null argument, an empty shape or a count below 1");
    const int64_t total = (int64_t)n * B * nq;
    S2V_REQUIRE((total + 255) / 256 <= 0x7fffffff, "attn_mass_mean: too many elements");
    const float inv = 1.0f / (float)((int64_t)H * count);
    hipLaunchKernelGGL(attn_mass_mean_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, acc, out, total, H, nq, inv);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}
