// HBM-bound kernels of the denoise step: AdaLN-Zero modulate, per-head QK LayerNorm + RoPE, V^T production,
// timestep / modulation GEMVs, patchify / unpatchify, tail norms, CFG + scheduler step.
// Every kernel is templated on the storage type T (float for the fp32 CPU-parity mode, bf16 otherwise); math is
// fp32 and results pass through ET<T>::rnd at the points where the reference materialises a tensor in the model
// dtype, so the bf16 path rounds where the reference's bf16 CPU run rounds.
#define S2V_HOST
#include "common.h"
#include "kernels.h"
#include <cstdlib>
#include <type_traits>

// ---------------------------------------------------------------------------------------------------
// Row LayerNorm helpers: one wave per row, row cached in registers (D <= 4096, D % (16/sizeof(T)) == 0)
// NR = rounds of 64 lanes x 16 bytes that cover the row (compile time: 6 for D = 3072 in bf16).  Every load is UNCONDITIONAL on a
// clamped address and the lane mask is applied to the value: with a per-chunk bounds branch the compiler closed each load with its
// own s_waitcnt vmcnt(0), i.e. a wave fetched its row in NR dependent memory round trips (3.1 TB/s on the C3 step).
#define LN_MAX_FLOATS 64
template <typename T, int NR>
__device__ __forceinline__ void row_load(const T* x, int D, int lane, float* v) {
    constexpr int VN = Vec16<T>::N;
    const int chunks = D / VN;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = lane + 64 * i;
        const bool ok = c < chunks;
        Vec16<T>::ld(x + (ok ? c : 0) * VN, v + i * VN);
#pragma unroll
        for (int e = 0; e < VN; ++e) v[i * VN + e] = ok ? v[i * VN + e] : 0.f;
    }
}
// normalise the register-resident row in place: v = rnd((v-mean)*rstd*w + b)
template <typename T, int NR>
__device__ __forceinline__ void row_layernorm(float* v, int D, int lane, const T* w, const T* b, float eps) {
    constexpr int VN = Vec16<T>::N;
    const int chunks = D / VN;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NR * VN; ++i) s += v[i];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const bool ok = lane + 64 * i < chunks;
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            const float d = v[i * VN + e] - mean;
            q += ok ? d * d : 0.f;
        }
    }
    const float var = wave_sum(q) / (float)D;
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = lane + 64 * i;
        const bool ok = c < chunks;
        const int cc = ok ? c : 0;
        float wv[VN], bv[VN];
        Vec16<T>::ld(w + cc * VN, wv);
        Vec16<T>::ld(b + cc * VN, bv);
#pragma unroll
        for (int e = 0; e < VN; ++e) v[i * VN + e] = ok ? ET<T>::rnd((v[i * VN + e] - mean) * rstd * wv[e] + bv[e]) : 0.f;  // lanes past the row stay 0 (tail_norm normalises twice)
    }
}
// v = rnd(rnd(v * rnd(1+scale)) + shift), then store
template <typename T, int NR>
__device__ __forceinline__ void row_modulate_store(float* v, int D, int lane, const T* shift, const T* scale, T* y) {
    constexpr int VN = Vec16<T>::N;
    const int chunks = D / VN;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = lane + 64 * i;
        const bool ok = c < chunks;
        const int cc = ok ? c : 0;
        float sc[VN], sh[VN], o[VN];
        Vec16<T>::ld(scale + cc * VN, sc);
        Vec16<T>::ld(shift + cc * VN, sh);
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            const float s1 = ET<T>::rnd(1.0f + sc[e]);
            const float p = ET<T>::rnd(v[i * VN + e] * s1);
            o[e] = p + sh[e];
        }
        if (ok) Vec16<T>::st(y + c * VN, o);
    }
}
// the same modulation, then per-row e4m3 quantisation of the bf16-rounded result instead of the bf16 store (bf16 rows only): the
// arithmetic of quant_rows_fp8_k on values that never leave the registers
template <int NR>
__device__ __forceinline__ void row_modulate_quant_store(float* v, int D, int lane, const bf16_t* shift, const bf16_t* scale, unsigned char* q,
                                                         float* qscale, bf16_t* y = nullptr /* LnModArgs::q8_keep_y: the bf16 row as well */) {
    const int chunks = D / 8;
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = lane + 64 * i;
        const bool ok = c < chunks;
        const int cc = ok ? c : 0;
        float sc[8], sh[8];
        Vec16<bf16_t>::ld(scale + cc * 8, sc);
        Vec16<bf16_t>::ld(shift + cc * 8, sh);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float s1 = ET<bf16_t>::rnd(1.0f + sc[e]);
            const float p = ET<bf16_t>::rnd(v[i * 8 + e] * s1);
            const float o = ok ? ET<bf16_t>::rnd(p + sh[e]) : 0.f;  // the value the bf16 store would have held
            v[i * 8 + e] = o;
            amax = fmaxf(amax, fabsf(o));
        }
    }
    amax = wave_max(amax);
    const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
    const float inv = 1.0f / sc;
    if (lane == 0) *qscale = sc;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = lane + 64 * i;
        int w0 = 0, w1 = 0;
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[i * 8 + 0] * inv, v[i * 8 + 1] * inv, w0, false);
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[i * 8 + 2] * inv, v[i * 8 + 3] * inv, w0, true);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[i * 8 + 4] * inv, v[i * 8 + 5] * inv, w1, false);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[i * 8 + 6] * inv, v[i * 8 + 7] * inv, w1, true);
        if (c < chunks) *(u32x2*)(q + c * 8) = u32x2{(unsigned)w0, (unsigned)w1};
        if (y != nullptr && c < chunks) Vec16<bf16_t>::st(y + c * 8, v + i * 8);
    }
}
// The same three steps with the parameter vectors (LayerNorm weight / bias, modulation scale / shift) REQUESTED WITH THE ROW: as written
// above the compiler issues each parameter chunk where it is used -- behind the two wave reductions, one chunk at a time -- so a wave
// paid up to 2 NR dependent L2 round trips after its row had arrived (C1: 13.5 us for a 9.6 MB pass).  row_params issues all 4 NR loads
// behind the row's own (clamped addresses, values of lanes past the row are never used); a scheduling barrier keeps them there.
template <typename T, int NR>
struct RowParams { typename Vec16<T>::raw_t w[NR], b[NR], sc[NR], sh[NR]; };
template <typename T, int NR>
__device__ __forceinline__ void row_params(RowParams<T, NR>& p, int D, int lane, const T* w, const T* b, const T* scale, const T* shift) {
    constexpr int VN = Vec16<T>::N;
    const int chunks = D / VN;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = lane + 64 * i;
        const int cc = c < chunks ? c : 0;
        p.w[i] = Vec16<T>::ldraw(w + cc * VN);
        p.b[i] = Vec16<T>::ldraw(b + cc * VN);
        p.sc[i] = Vec16<T>::ldraw(scale + cc * VN);
        p.sh[i] = Vec16<T>::ldraw(shift + cc * VN);
    }
    __builtin_amdgcn_sched_barrier(0);
}
template <typename T, int NR>
__device__ __forceinline__ void row_layernorm_p(float* v, int D, int lane, const RowParams<T, NR>& p, float eps) {
    constexpr int VN = Vec16<T>::N;
    const int chunks = D / VN;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NR * VN; ++i) s += v[i];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const bool ok = lane + 64 * i < chunks;
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            const float d = v[i * VN + e] - mean;
            q += ok ? d * d : 0.f;
        }
    }
    const float var = wave_sum(q) / (float)D;
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const bool ok = lane + 64 * i < chunks;
        float wv[VN], bv[VN];
        Vec16<T>::dec(p.w[i], wv);
        Vec16<T>::dec(p.b[i], bv);
#pragma unroll
        for (int e = 0; e < VN; ++e) v[i * VN + e] = ok ? ET<T>::rnd((v[i * VN + e] - mean) * rstd * wv[e] + bv[e]) : 0.f;
    }
}
template <typename T, int NR>
__device__ __forceinline__ void row_modulate_store_p(float* v, int D, int lane, const RowParams<T, NR>& p, T* y) {
    constexpr int VN = Vec16<T>::N;
    const int chunks = D / VN;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = lane + 64 * i;
        float sc[VN], sh[VN], o[VN];
        Vec16<T>::dec(p.sc[i], sc);
        Vec16<T>::dec(p.sh[i], sh);
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            const float s1 = ET<T>::rnd(1.0f + sc[e]);
            const float pr = ET<T>::rnd(v[i * VN + e] * s1);
            o[e] = pr + sh[e];
        }
        if (c < chunks) Vec16<T>::st(y + c * VN, o);
    }
}

// rounds needed for D elements of T, rounded up to an instantiated count
template <typename T> static int ln_rounds(int D) {
    const int need = (D / Vec16<T>::N + 63) / 64;
    for (int r : {1, 2, 3, 4, 6, 8, 12, 16})
        if (r >= need) return r;
    return -1;
}
#define S2V_LN_DISPATCH_NR(T, nr, ...)                                                \
    switch (nr) {                                                                     \
        case 1: { constexpr int NR = 1; __VA_ARGS__; } break;                                \
        case 2: { constexpr int NR = 2; __VA_ARGS__; } break;                                \
        case 3: { constexpr int NR = 3; __VA_ARGS__; } break;                                \
        case 4: { constexpr int NR = 4; __VA_ARGS__; } break;                                \
        case 6: { constexpr int NR = 6; __VA_ARGS__; } break;                                \
        case 8: { constexpr int NR = 8; __VA_ARGS__; } break;                                \
        case 12: if constexpr (sizeof(T) == 4) { constexpr int NR = 12; __VA_ARGS__; } break; \
        case 16: if constexpr (sizeof(T) == 4) { constexpr int NR = 16; __VA_ARGS__; } break; \
        default: return s2v_fail(__FILE__, __LINE__, "layer norm: row too long", -1); \
    }
#define S2V_LN_DISPATCH(T, D, ...) S2V_LN_DISPATCH_NR(T, ln_rounds<T>(D), __VA_ARGS__)

// CogVideoXLayerNormZero.forward (normalization.py:467-484): LN(x)*(1+scale)+shift, three token ranges
template <typename T, int NR>
__global__ __launch_bounds__(256) void ln_modulate_k(const LnModArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.B * a.Ntok) return;
    const int b = row / a.Ntok, r = row - b * a.Ntok;
    const bool txt = r < a.text_len;
    const bool ref = a.shift_ref != nullptr && !txt && r < a.text_len + a.ref_len;
    const T* shift = (const T*)(txt ? a.shift_txt : ref ? a.shift_ref : a.shift_vid) + (size_t)b * a.mod_stride;
    const T* scale = (const T*)(txt ? a.scale_txt : ref ? a.scale_ref : a.scale_vid) + (size_t)b * a.mod_stride;
    float v[NR * Vec16<T>::N];
    if constexpr (std::is_same<T, bf16_t>::value) {
        if (a.q8 != nullptr) {  // fp8 engine: per-row e4m3 image instead of the bf16 store
            row_load<T, NR>((const T*)a.x + (size_t)row * a.ldx, a.D, lane, v);
            row_layernorm<T, NR>(v, a.D, lane, (const T*)a.w, (const T*)a.b, a.eps);
            row_modulate_quant_store<NR>(v, a.D, lane, shift, scale, (unsigned char*)a.q8 + (size_t)row * a.D, a.q8_scale + row,
                                         a.q8_keep_y ? (bf16_t*)a.y + (size_t)row * a.ldy : nullptr);
            return;
        }
    }
    // the row and all four parameter vectors in flight together (row_params), then the same arithmetic as row_layernorm / row_modulate_store
    typename Vec16<T>::raw_t xr[NR];
    {
        constexpr int VN = Vec16<T>::N;
        const int chunks = a.D / VN;
        const T* x = (const T*)a.x + (size_t)row * a.ldx;
#pragma unroll
        for (int i = 0; i < NR; ++i) xr[i] = Vec16<T>::ldraw(x + (lane + 64 * i < chunks ? lane + 64 * i : 0) * VN);
        RowParams<T, NR> prm;
        row_params<T, NR>(prm, a.D, lane, (const T*)a.w, (const T*)a.b, scale, shift);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            Vec16<T>::dec(xr[i], v + i * VN);
            const bool ok = lane + 64 * i < chunks;
#pragma unroll
            for (int e = 0; e < VN; ++e) v[i * VN + e] = ok ? v[i * VN + e] : 0.f;
        }
        row_layernorm_p<T, NR>(v, a.D, lane, prm, a.eps);
        row_modulate_store_p<T, NR>(v, a.D, lane, prm, (T*)a.y + (size_t)row * a.ldy);
    }
}
// The same rows with the four parameter vectors (LayerNorm weight / bias, modulation scale / shift) staged ONCE per workgroup in LDS: ln_modulate_k
// keeps them in registers per row (96 of its 179 VGPRs at D = 3072: two waves per SIMD, 24 KiB of L1 / L2 reads per 6-KiB row); here a workgroup of
// four waves handles 4 x RPW consecutive rows, reads the parameters from LDS where they are used and keeps ~100 registers.  The rows of a workgroup
// share their parameter set unless a text / reference / video or sample boundary falls inside it: those workgroups read the parameters from global
// memory per row, as before.  Arithmetic is row_layernorm / row_modulate_store's, i.e. ln_modulate_k's.
template <typename T, int NR, int RPW>
__global__ __launch_bounds__(256) void ln_modulate_lds_k(const LnModArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ln_smem[];
    constexpr int VN = Vec16<T>::N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = a.B * a.Ntok, r0 = blockIdx.x * (4 * RPW), rl = min(r0 + 4 * RPW, rows) - 1;
    auto params_of = [&](int row, const T*& shift, const T*& scale) {
        const int b = row / a.Ntok, r = row - b * a.Ntok;
        const bool txt = r < a.text_len;
        const bool ref = a.shift_ref != nullptr && !txt && r < a.text_len + a.ref_len;
        shift = (const T*)(txt ? a.shift_txt : ref ? a.shift_ref : a.shift_vid) + (size_t)b * a.mod_stride;
        scale = (const T*)(txt ? a.scale_txt : ref ? a.scale_ref : a.scale_vid) + (size_t)b * a.mod_stride;
    };
    const T *sh0, *sc0, *sh1, *sc1;
    params_of(r0, sh0, sc0);
    params_of(rl, sh1, sc1);
    const bool uniform = sh0 == sh1 && sc0 == sc1;   // parameter sets are contiguous row ranges: equal ends = one set
    T* lw = (T*)ln_smem;
    T *lb = lw + a.D, *lsc = lb + a.D, *lsh = lsc + a.D;
    if (uniform) {
        const int chunks = a.D / VN;
        for (int c = threadIdx.x; c < chunks; c += 256) {
            *(typename Vec16<T>::raw_t*)(lw + c * VN) = Vec16<T>::ldraw((const T*)a.w + c * VN);
            *(typename Vec16<T>::raw_t*)(lb + c * VN) = Vec16<T>::ldraw((const T*)a.b + c * VN);
            *(typename Vec16<T>::raw_t*)(lsc + c * VN) = Vec16<T>::ldraw(sc0 + c * VN);
            *(typename Vec16<T>::raw_t*)(lsh + c * VN) = Vec16<T>::ldraw(sh0 + c * VN);
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int k = 0; k < RPW; ++k) {
        const int row = r0 + k * 4 + wave;
        if (row >= rows) break;
        const T *pw = lw, *pb = lb, *psc = lsc, *psh = lsh;
        if (!uniform) { pw = (const T*)a.w; pb = (const T*)a.b; params_of(row, psh, psc); }
        float v[NR * VN];
        row_load<T, NR>((const T*)a.x + (size_t)row * a.ldx, a.D, lane, v);
        row_layernorm<T, NR>(v, a.D, lane, pw, pb, a.eps);
        if constexpr (std::is_same<T, bf16_t>::value) {
            if (a.q8 != nullptr) {
                row_modulate_quant_store<NR>(v, a.D, lane, psh, psc, (unsigned char*)a.q8 + (size_t)row * a.D, a.q8_scale + row,
                                             a.q8_keep_y ? (bf16_t*)a.y + (size_t)row * a.ldy : nullptr);
                continue;
            }
        }
        row_modulate_store<T, NR>(v, a.D, lane, psh, psc, (T*)a.y + (size_t)row * a.ldy);
    }
}
// many rows (at least four workgroups of sixteen rows per CU): parameters staged in LDS per workgroup (bf16 only)
LnPlan ln_modulate_plan(int rows, int D, int dtype, int lds_rows) {
    LnPlan p;
    p.kernel = dtype == S2V_BF16 && lds_rows > 0 && rows >= lds_rows ? LN_KERNEL_LDS : LN_KERNEL_REG;
    p.nr = dtype == S2V_BF16 ? ln_rounds<bf16_t>(D) : dtype == S2V_F16 ? ln_rounds<f16_t>(D) : ln_rounds<float>(D);
    if (dtype != S2V_F32 && p.nr > 8) p.nr = -1;  // 12 and 16 rounds are instantiated for fp32 only
    return p;
}
static int ln_lds_rows() {
#ifdef S2V_DIAG
    if (const char* e = getenv("S2V_LN_LDS_ROWS")) return atoi(e);  // tools/ln_lds_probe.py (diagnostics library): 0 = never
#endif
    return LN_LDS_ROWS;
}
#ifdef S2V_DIAG
// ln_modulate_plan without a device: out = {kernel (LN_KERNEL_*), NR}; lds_rows < 0: the launcher's own threshold (S2V_LN_LDS_ROWS included)
extern "C" __attribute__((visibility("default"))) int s2v_diag_ln_plan(int32_t rows, int32_t D, int32_t dtype, int32_t lds_rows, int32_t* out) {
    S2V_REQUIRE(out && rows > 0 && D > 0 && (dtype == S2V_F32 || dtype == S2V_BF16 || dtype == S2V_F16), "s2v_diag_ln_plan: bad argument");
    const LnPlan p = ln_modulate_plan(rows, D, dtype, lds_rows < 0 ? ln_lds_rows() : lds_rows);
    out[0] = p.kernel; out[1] = p.nr;
    return 0;
}
#endif
int launch_ln_modulate(const LnModArgs& a, int dtype, hipStream_t st) {
    S2V_REQUIRE(a.D <= 4096 && a.D % 8 == 0, "ln_modulate: D must be <= 4096 and a multiple of 8");
    S2V_REQUIRE(a.q8 == nullptr || (dtype == S2V_BF16 && a.q8_scale != nullptr), "ln_modulate: the fp8 output needs bf16 rows and a scale vector");
    const int rows = a.B * a.Ntok;
    dim3 grid((rows + 3) / 4);
    const LnPlan pl = ln_modulate_plan(rows, a.D, dtype, ln_lds_rows());
    if (pl.kernel == LN_KERNEL_LDS) {
        constexpr int RPW = 4;
        dim3 g16((rows + 4 * RPW - 1) / (4 * RPW));
        const size_t lds = (size_t)4 * a.D * 2;
        S2V_LN_DISPATCH_NR(bf16_t, pl.nr, hipLaunchKernelGGL((ln_modulate_lds_k<bf16_t, NR, RPW>), g16, dim3(256), lds, st, a))
        S2V_CHECK_HIP(hipGetLastError());
        return 0;
    }
    if (dtype == S2V_BF16) {
        S2V_LN_DISPATCH_NR(bf16_t, pl.nr, hipLaunchKernelGGL((ln_modulate_k<bf16_t, NR>), grid, dim3(256), 0, st, a))
    } else if (dtype == S2V_F16) {
        S2V_LN_DISPATCH_NR(f16_t, pl.nr, hipLaunchKernelGGL((ln_modulate_k<f16_t, NR>), grid, dim3(256), 0, st, a))
    } else {
        S2V_LN_DISPATCH_NR(float, pl.nr, hipLaunchKernelGGL((ln_modulate_k<float, NR>), grid, dim3(256), 0, st, a))
    }
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// norm_final -> norm_out (AdaLayerNorm, shift first) on the video rows (cogvideox_transformer_3d.py:536-542)
template <typename T, int NR>
__global__ __launch_bounds__(256) void tail_norm_k(const TailNormArgs a) {
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= a.B * a.V) return;
    const int b = idx / a.V, vr = idx - b * a.V;
    const size_t xrow = (size_t)b * a.Ntok + a.row0 + vr;
    float v[NR * Vec16<T>::N];
    row_load<T, NR>((const T*)a.x + xrow * a.ldx, a.D, lane, v);
    row_layernorm<T, NR>(v, a.D, lane, (const T*)a.w1, (const T*)a.b1, a.eps);
    row_layernorm<T, NR>(v, a.D, lane, (const T*)a.w2, (const T*)a.b2, a.eps);
    const T* shift = (const T*)a.shift + (size_t)b * a.mod_stride;
    const T* scale = (const T*)a.scale + (size_t)b * a.mod_stride;
    row_modulate_store<T, NR>(v, a.D, lane, shift, scale, (T*)a.y + (size_t)idx * a.ldy);
}
int launch_tail_norm(const TailNormArgs& a, int dtype, hipStream_t st) {
    S2V_REQUIRE(a.D <= 4096 && a.D % 8 == 0, "tail_norm: D must be <= 4096 and a multiple of 8");
    dim3 grid((a.B * a.V + 3) / 4);
    if (dtype == S2V_BF16) {
        S2V_LN_DISPATCH(bf16_t, a.D, hipLaunchKernelGGL((tail_norm_k<bf16_t, NR>), grid, dim3(256), 0, st, a))
    } else if (dtype == S2V_F16) {
        S2V_LN_DISPATCH(f16_t, a.D, hipLaunchKernelGGL((tail_norm_k<f16_t, NR>), grid, dim3(256), 0, st, a))
    } else {
        S2V_LN_DISPATCH(float, a.D, hipLaunchKernelGGL((tail_norm_k<float, NR>), grid, dim3(256), 0, st, a))
    }
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// per-head LN(64) on q and k + RoPE (attention_processor.py:2060-2080, embeddings.py:759-778).
// 8 lanes per 64-wide head vector (8 contiguous elements per lane); one thread-task = (row, q|k, head, octet)
// Grid: x = row, y = 256-task slices of the row's 2 * H * 8 tasks (no division by the task count); the rotary tables of the row are
// requested together with its q / k chunk (clamped address for text rows), so a thread pays ONE memory latency, not two.
template <typename T>
__global__ __launch_bounds__(256) void qk_norm_rope_k(const QkNormRopeArgs a) {
    const int D = a.H * 64;
    const int row = blockIdx.x;
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= 2 * a.H * 8) return;  // whole 8-lane groups exit together
    const int which = t >= a.H * 8;  // 0 = q, 1 = k
    const int hh = (t >> 3) - which * a.H;
    const int oct = t & 7;
    T* p = (T*)a.qkv + (size_t)row * a.ld_qkv + which * D + hh * 64 + oct * 8;
    const int r = row % a.Ntok;
    const bool rope = a.cos != nullptr && r >= a.text_len;
    const size_t tab = (size_t)(rope ? r - a.text_len : 0) * 64 + oct * 8;
    float v[8], cs[8], sn[8], wv[8], bv[8];
    if constexpr (sizeof(T) == 2) {
        Vec16<T>::ld(p, v);
    } else {
        Vec16<T>::ld(p, v);
        Vec16<T>::ld(p + 4, v + 4);
    }
    if (a.cos != nullptr) {
        Vec16<float>::ld(a.cos + tab, cs);
        Vec16<float>::ld(a.cos + tab + 4, cs + 4);
        Vec16<float>::ld(a.sin + tab, sn);
        Vec16<float>::ld(a.sin + tab + 4, sn + 4);
    }
    const T* w = (const T*)(which ? a.nk_w : a.nq_w) + oct * 8;
    const T* bb = (const T*)(which ? a.nk_b : a.nq_b) + oct * 8;
    if constexpr (sizeof(T) == 2) {
        Vec16<T>::ld(w, wv);
        Vec16<T>::ld(bb, bv);
    } else {
        Vec16<T>::ld(w, wv);
        Vec16<T>::ld(w + 4, wv + 4);
        Vec16<T>::ld(bb, bv);
        Vec16<T>::ld(bb + 4, bv + 4);
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
    s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
    const float mean = s * (1.0f / 64.0f);
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float d = v[e] - mean; q += d * d; }
    q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64); q += __shfl_xor(q, 4, 64);
    const float rstd = 1.0f / sqrtf(q * (1.0f / 64.0f) + a.eps);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = ET<T>::rnd((v[e] - mean) * rstd * wv[e] + bv[e]);
    if (rope) {
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            const float x0 = v[e], x1 = v[e + 1];
            v[e] = ET<T>::rnd(x0 * cs[e] + (-x1) * sn[e]);
            v[e + 1] = ET<T>::rnd(x1 * cs[e + 1] + x0 * sn[e + 1]);
        }
    }
    if constexpr (sizeof(T) == 2) {
        Vec16<T>::st(p, v);
    } else {
        Vec16<T>::st(p, v);
        Vec16<T>::st(p + 4, v + 4);
    }
}

// V [B*Ntok, .] (cols 2D + h*64 + d) -> V^T [B][H][64][ntok_pad]; inside every aligned 16-token group the
// tokens are stored in the order [0-3, 8-11, 4-7, 12-15] (bits 2 and 3 of the token index swapped) which is the
// k-slot order the PV MFMA of attn_bf16_k consumes.  64 tokens x 64 dims per block through LDS.
// vamax non-null: the values are written as fp16 (attn_q4h: P.V on the fp16 MFMA), times 2^vt_f16_shift(vamax[b * H + h]) (kernels.h): the head's
// largest magnitude lands in [2^14, 2^15), so V does not saturate (below a largest magnitude of 2^115: vt_f16_shift's clamp) and every value down to 2^-29 of the largest converts exactly (below, it
// rounds into the fp16 subnormals).  Inf / NaN in V switch the scaling off; an infinity is then SATURATED to +-65504 -- in V^T it would turn the
// whole head-dim column into NaN through 0 * inf in P.V, which no slow-path census would notice.
__global__ __launch_bounds__(256) void v_amax_k(const bf16_t* qkv, int ld_qkv, int H, int Ntok, unsigned* vamax) {
    const int n0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
    const int D = H * 64;
    unsigned m = 0;
    for (int i = threadIdx.x; i < 64 * 8; i += 256) {
        const int n = n0 + (i >> 3), cc = (i & 7) * 8;
        if (n < Ntok) {
            const u32x4 val = *(const u32x4*)(qkv + (size_t)(b * Ntok + n) * ld_qkv + 2 * D + h * 64 + cc);
#pragma unroll
            for (int e = 0; e < 4; ++e) m = max(m, max(val[e] & 0x7fffu, (val[e] >> 16) & 0x7fffu));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(vamax + b * H + h, m);
}
__global__ __launch_bounds__(256) void v_transpose_k(const bf16_t* qkv, int ld_qkv, int B, int H, int Ntok, bf16_t* vt,
                                                     int ntok_pad, const unsigned* vamax) {
    __shared__ bf16_t tile[64][64 + 2];
    const int n0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
    const int D = H * 64;
    const int tid = threadIdx.x;
    const bool to_f16 = vamax != nullptr;
    const float vscale = to_f16 ? __uint_as_float((unsigned)(127 + vt_f16_shift(vamax[b * H + h])) << 23) : 1.0f;
    // load: 64 rows x 128 B, 8 lanes x 16 B per row
    for (int i = tid; i < 64 * 8; i += 256) {
        const int rr = i >> 3, cc = (i & 7) * 8;
        const int n = n0 + rr;
        u32x4 val = {0, 0, 0, 0};
        if (n < Ntok) val = *(const u32x4*)(qkv + (size_t)(b * Ntok + n) * ld_qkv + 2 * D + h * 64 + cc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            tile[rr][cc + 2 * e] = (bf16_t)(val[e] & 0xffff);
            tile[rr][cc + 2 * e + 1] = (bf16_t)(val[e] >> 16);
        }
    }
    __syncthreads();
    bf16_t* dst = vt + (size_t)(b * H + h) * 64 * ntok_pad;
    for (int i = tid; i < 64 * 64; i += 256) {
        const int d = i >> 6, pos = i & 63;
        const int tok = (pos & ~12) | ((pos & 4) << 1) | ((pos & 8) >> 1);  // token stored at this position
        if (n0 + tok < Ntok) {
            bf16_t v = tile[tok][d];
            if (to_f16) {
                float f = __uint_as_float((unsigned)v << 16) * vscale;
                f = f != f ? f : fminf(fmaxf(f, -65504.0f), 65504.0f);  // NaN stays NaN (it is one in bf16 too); +-inf and > 65504 saturate
                v = __builtin_bit_cast(unsigned short, (_Float16)f);
            }
            dst[(size_t)d * ntok_pad + n0 + pos] = v;
        }
        else if (n0 + pos < ntok_pad) dst[(size_t)d * ntok_pad + n0 + pos] = 0;
    }
}

// q / k of the normalised, rotated QKV buffer -> MX e4m3 images for the fp8 QK^T of attn_q4f (AttnArgs::q8 ... k8s; weight_format 2; no
// reference code: the reference has no fp8 path).  A block = 64 tokens of one head of q or k; a thread = 16 head-dim elements, two threads = one
// 32-element MX block: x = bf16 value (q: times scale * log2 e, in fp32), amax over the block, E8M0 scale = the smallest power of two with
// amax / scale <= 448, byte = rne_e4m3(x / scale).  Rows [Ntok, ntok_pad) of k are written as zeros with unit scales.
__global__ __launch_bounds__(256) void qk_quant_mx_k(const bf16_t* qkv, int ld_qkv, int H, int Ntok, int ntok_pad, float q_prescale,
                                                      unsigned char* q8, unsigned short* q8s, unsigned char* k8, unsigned* k8s) {
    const int tile = blockIdx.x, h = blockIdx.y, b = blockIdx.z >> 1, is_k = blockIdx.z & 1;
    const int tid = threadIdx.x, kr = tid >> 2, qt = tid & 3, blk = qt >> 1;
    const int n = tile * 64 + kr;
    if (!is_k && n >= Ntok) return;
    const int D = H * 64;
    float x[16];
    if (n < Ntok) {
        const bf16_t* src = qkv + (size_t)(b * Ntok + n) * ld_qkv + is_k * D + h * 64 + qt * 16;
        const u32x4 v0 = *(const u32x4*)src, v1 = *(const u32x4*)(src + 8);
        const float c = is_k ? 1.0f : q_prescale;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[2 * e] = __uint_as_float(v0[e] << 16) * c; x[2 * e + 1] = __uint_as_float(v0[e] & 0xffff0000u) * c;
            x[8 + 2 * e] = __uint_as_float(v1[e] << 16) * c; x[8 + 2 * e + 1] = __uint_as_float(v1[e] & 0xffff0000u) * c;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) x[e] = 0.f;
    }
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(x[e]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    unsigned eb = (__float_as_uint(amax * (1.0f / 448.0f)) + 0x7fffffu) >> 23;
    eb = n < Ntok ? min(max(eb, 1u), 253u) : 127u;
    const float inv = __uint_as_float((254u - eb) << 23);
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        int r = 0;
        r = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w] * inv, x[4 * w + 1] * inv, r, false);
        r = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w + 2] * inv, x[4 * w + 3] * inv, r, true);
        o[w] = (unsigned)r;
    }
    const size_t bh = (size_t)b * H + h;
    if (is_k) {
        *(u32x4*)(k8 + (bh * ntok_pad + n) * 64 + qt * 16) = o;
        if ((qt & 1) == 0)
            ((unsigned char*)k8s)[((bh * (ntok_pad / 64) + tile) * 64 + blk * 32 + (kr & 31)) * 4 + (kr >> 5)] = (unsigned char)eb;
    } else {
        *(u32x4*)(q8 + (bh * Ntok + n) * 64 + qt * 16) = o;
        if ((qt & 1) == 0) ((unsigned char*)q8s)[(bh * Ntok + n) * 2 + blk] = (unsigned char)eb;
    }
}
int launch_qk_quant_mx(const void* qkv, int ld_qkv, int B, int H, int Ntok, int ntok_pad, float q_prescale, unsigned char* q8, unsigned short* q8s,
                       unsigned char* k8, unsigned* k8s, hipStream_t st) {
    S2V_REQUIRE(ntok_pad % 64 == 0 && ntok_pad >= Ntok, "qk_quant_mx: ntok_pad must be a multiple of 64 covering Ntok");
    hipLaunchKernelGGL(qk_quant_mx_k, dim3(ntok_pad / 64, H, 2 * B), dim3(256), 0, st, (const bf16_t*)qkv, ld_qkv, H, Ntok, ntok_pad, q_prescale, q8,
                       q8s, k8, k8s);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// The fp8-QK^T engine's q / k pass with the per-head LayerNorm + rotary embedding folded in (round 5): the RAW q / k of the QKV projection (plain
// bias epilogue) -> qk_norm_rope_k's arithmetic with its rounding points (the same bits as the stand-alone kernel and as the projection's fused
// EPI_BIAS_QKNORM epilogue: octet sums in element order, the 8-lane butterfly -- here one in-lane add of the thread's two octets and two shuffles --,
// correctly rounded sqrt / reciprocal, (d * rstd) * w + b rounded to bf16, the rotary pair on the rounded values) -> qk_quant_mx_k's MX e4m3 images.
// The attention kernel reads q and k ONLY through these images (attn_q4f), so the normalised bf16 q / k are never written: the pass moves the bytes
// the quantisation pass moved anyway, and the projection's epilogue -- exposed VALU work behind a K loop half as long as the bf16 one -- goes back
// to bias + rounding.  Thread = 16 head-dim elements (octets 2 qt, 2 qt + 1) of a (token, head); grid as qk_quant_mx_k.
__global__ __launch_bounds__(256) void qk_norm_quant_mx_k(const QkNormRopeArgs a, float q_prescale, unsigned char* q8, unsigned short* q8s, unsigned char* k8,
                                                           unsigned* k8s, int hg) {
    // a block = 64 tokens x hg heads of q or k: the rotary values and the LayerNorm parameters of a thread (its token, its 16 head-dim elements) are the
    // same for every head, so they are fetched once per hg heads (one head per block read four times the q / k bytes in table values)
    const int tile = blockIdx.x, h0 = blockIdx.y * hg, b = blockIdx.z >> 1, is_k = blockIdx.z & 1;
    const int tid = threadIdx.x, kr = tid >> 2, qt = tid & 3, blk = qt >> 1;
    const int n = tile * 64 + kr;
    const int H = a.H, Ntok = a.Ntok, ntok_pad = a.ntok_pad;
    if (!is_k && n >= Ntok) return;  // the four threads of a row leave together
    const int D = H * 64;
    const bool live = n < Ntok;
    const bool rope = live && a.cos != nullptr && n >= a.text_len;
    float cs[16], sn[16], wv[16], bv[16];
    if (live) {
        const size_t tab = (size_t)(rope ? n - a.text_len : 0) * 64 + qt * 16;
        if (a.cos != nullptr) {
#pragma unroll
            for (int e = 0; e < 16; e += 4) {
                Vec16<float>::ld(a.cos + tab + e, cs + e);
                Vec16<float>::ld(a.sin + tab + e, sn + e);
            }
        }
        const bf16_t* w = (const bf16_t*)(is_k ? a.nk_w : a.nq_w) + qt * 16;
        const bf16_t* bb = (const bf16_t*)(is_k ? a.nk_b : a.nq_b) + qt * 16;
        Vec16<bf16_t>::ld(w, wv); Vec16<bf16_t>::ld(w + 8, wv + 8);
        Vec16<bf16_t>::ld(bb, bv); Vec16<bf16_t>::ld(bb + 8, bv + 8);
    }
    const float c = is_k ? 1.0f : q_prescale;
#pragma unroll 1
    for (int h = h0; h < h0 + hg; ++h) {
        float x[16];
        if (live) {
            const bf16_t* src = (const bf16_t*)a.qkv + (size_t)(b * Ntok + n) * a.ld_qkv + is_k * D + h * 64 + qt * 16;
            Vec16<bf16_t>::ld(src, x);
            Vec16<bf16_t>::ld(src + 8, x + 8);
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { s0 += x[e]; s1 += x[8 + e]; }
            float s = s0 + s1;
            s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64);
            const float mean = s * (1.0f / 64.0f);
            float q0 = 0.f, q1 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d0 = x[e] - mean, d1 = x[8 + e] - mean;
                q0 += d0 * d0; q1 += d1 * d1;
            }
            float q = q0 + q1;
            q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64);
            const float rstd = 1.0f / sqrtf(q * (1.0f / 64.0f) + a.eps);
#pragma unroll
            for (int e = 0; e < 16; ++e) x[e] = ET<bf16_t>::rnd((x[e] - mean) * rstd * wv[e] + bv[e]);
            if (rope) {
#pragma unroll
                for (int e = 0; e < 16; e += 2) {
                    const float x0 = x[e], x1 = x[e + 1];
                    x[e] = ET<bf16_t>::rnd(x0 * cs[e] + (-x1) * sn[e]);
                    x[e + 1] = ET<bf16_t>::rnd(x1 * cs[e + 1] + x0 * sn[e + 1]);
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) x[e] *= c;
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) x[e] = 0.f;
        }
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(x[e]));
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
        unsigned eb = (__float_as_uint(amax * (1.0f / 448.0f)) + 0x7fffffu) >> 23;
        eb = live ? min(max(eb, 1u), 253u) : 127u;
        const float inv = __uint_as_float((254u - eb) << 23);
        u32x4 o;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            int r = 0;
            r = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w] * inv, x[4 * w + 1] * inv, r, false);
            r = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w + 2] * inv, x[4 * w + 3] * inv, r, true);
            o[w] = (unsigned)r;
        }
        const size_t bh = (size_t)b * H + h;
        if (is_k) {
            *(u32x4*)(k8 + (bh * ntok_pad + n) * 64 + qt * 16) = o;
            if ((qt & 1) == 0)
                ((unsigned char*)k8s)[((bh * (ntok_pad / 64) + tile) * 64 + blk * 32 + (kr & 31)) * 4 + (kr >> 5)] = (unsigned char)eb;
        } else {
            *(u32x4*)(q8 + (bh * Ntok + n) * 64 + qt * 16) = o;
            if ((qt & 1) == 0) ((unsigned char*)q8s)[(bh * Ntok + n) * 2 + blk] = (unsigned char)eb;
        }
    }
}
int launch_qk_norm_quant_mx(const QkNormRopeArgs& a, float q_prescale, unsigned char* q8, unsigned short* q8s, unsigned char* k8, unsigned* k8s, hipStream_t st) {
    S2V_REQUIRE(a.ntok_pad % 64 == 0 && a.ntok_pad >= a.Ntok, "qk_norm_quant_mx: ntok_pad must be a multiple of 64 covering Ntok");
    S2V_REQUIRE(a.nq_w && a.nq_b && a.nk_w && a.nk_b && (a.cos == nullptr) == (a.sin == nullptr), "qk_norm_quant_mx: LayerNorm parameters / rotary tables");
    const int hg = a.H % 4 == 0 ? 4 : a.H % 2 == 0 ? 2 : 1;
    hipLaunchKernelGGL(qk_norm_quant_mx_k, dim3(a.ntok_pad / 64, a.H / hg, 2 * a.B), dim3(256), 0, st, a, q_prescale, q8, q8s, k8, k8s, hg);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_qk_norm_rope(const QkNormRopeArgs& a, int dtype, hipStream_t st) {
    dim3 grid((unsigned)(a.B * a.Ntok), (unsigned)((2 * a.H * 8 + 255) / 256));
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(qk_norm_rope_k<T>, grid, dim3(256), 0, st, a))
    S2V_CHECK_HIP(hipGetLastError());
    if (a.vt != nullptr) {
        S2V_REQUIRE(dtype == S2V_BF16 || (dtype == S2V_F16 && !a.vt_f16), "V^T is produced for 16-bit storage only (fp16 rows are moved as they are)");
        S2V_REQUIRE(!a.vt_f16 || a.vt_amax, "an fp16 V^T needs the per-head magnitude words (QkNormRopeArgs::vt_amax)");
        S2V_TRY(launch_v_transpose(a.qkv, a.ld_qkv, a.B, a.H, a.Ntok, a.vt, a.ntok_pad, st, a.vt_f16 ? a.vt_amax : nullptr));
    }
    return 0;
}
int launch_v_transpose(const void* qkv, int ld_qkv, int B, int H, int Ntok, void* vt, int ntok_pad, hipStream_t st, unsigned* vt_amax) {
    dim3 g2((Ntok + 63) / 64, H, B);
    if (vt_amax != nullptr) {
        S2V_CHECK_HIP(hipMemsetAsync(vt_amax, 0, sizeof(unsigned) * B * H, st));
        hipLaunchKernelGGL(v_amax_k, g2, dim3(256), 0, st, (const bf16_t*)qkv, ld_qkv, H, Ntok, vt_amax);
        S2V_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(v_transpose_k, g2, dim3(256), 0, st, (const bf16_t*)qkv, ld_qkv, B, H, Ntok, (bf16_t*)vt, ntok_pad, (const unsigned*)vt_amax);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// timestep sinusoid [cos | sin] (flip_sin_to_cos=True, shift 0), fp32 math then cast (embeddings.py:56-73)
template <typename T>
__global__ void timestep_sincos_k(const float* t, int B, int D, T* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, j = i - b * D;
    const int half = D / 2;
    const int f = j < half ? j : j - half;
    const float expo = -logf(10000.0f) * (float)f / (float)half;
    const float arg = t[b] * expf(expo);
    ET<T>::st(out + i, j < half ? cosf(arg) : sinf(arg));
}

// out[b][row] = rnd(sum_k f(in[b][k]) * W[row][k] + bias[row]); f = rnd(silu(.)) when PRE_SILU. One wave per row.
template <typename T, bool PRE_SILU>
__global__ __launch_bounds__(256) void gemv_rows_k(const T* in, int B, int K, const T* W, const T* bias, int64_t rows,
                                                   T* out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    constexpr int VN = Vec16<T>::N;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const T* w = W + row * K;
    for (int k = lane * VN; k < K; k += 64 * VN) {
        float wv[VN];
        Vec16<T>::ld(w + k, wv);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < B) {
                float xv[VN];
                Vec16<T>::ld(in + (size_t)b * K + k, xv);
#pragma unroll
                for (int e = 0; e < VN; ++e) {
                    float x = xv[e];
                    if (PRE_SILU) x = ET<T>::rnd(silu_f(x));
                    acc[b] = fmaf(x, wv[e], acc[b]);
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (b < B) {
            const float s = wave_sum(acc[b]);
            if (lane == 0) ET<T>::st(out + (size_t)b * rows + row, s + (bias ? ET<T>::ld(bias + row) : 0.f));
        }
    }
}
// The same sums in the same order (bit-identical), shaped for the weight stream: K = KC * 64 * (16-byte vector) exactly, so a lane
// owns KC fixed chunks of every row; it applies f to its slice of the B input vectors ONCE (the one-wave-per-row kernel re-evaluated
// silu for every row: 16 exp per 16 bytes of weights, which held the step's modulation GEMV at 1.1 TB/s) and then streams GEMV_R rows
// with all their loads in flight.
constexpr int GEMV_R = 8;
template <typename T, bool PRE_SILU, int KC, int BN>
__global__ __launch_bounds__(256) void gemv_rows_reg_k(const T* in, const T* W, const T* bias, int64_t rows, T* out) {
    constexpr int VN = Vec16<T>::N, K = KC * 64 * VN;
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GEMV_R;
    if (row0 >= rows) return;
    float x[BN][KC][VN];
#pragma unroll
    for (int b = 0; b < BN; ++b)
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            Vec16<T>::ld(in + (size_t)b * K + (c * 64 + lane) * VN, x[b][c]);
            if (PRE_SILU)
#pragma unroll
                for (int e = 0; e < VN; ++e) x[b][c][e] = ET<T>::rnd(silu_f(x[b][c][e]));
        }
    const int nr = (int)min((int64_t)GEMV_R, rows - row0);
    float wv[GEMV_R][KC][VN];
#pragma unroll
    for (int r = 0; r < GEMV_R; ++r) {
        const T* w = W + (row0 + min(r, nr - 1)) * K;
#pragma unroll
        for (int c = 0; c < KC; ++c) Vec16<T>::ld(w + (c * 64 + lane) * VN, wv[r][c]);
    }
#pragma unroll
    for (int r = 0; r < GEMV_R; ++r) {
        float acc[BN];
#pragma unroll
        for (int b = 0; b < BN; ++b) {
            acc[b] = 0.f;
#pragma unroll
            for (int c = 0; c < KC; ++c)
#pragma unroll
                for (int e = 0; e < VN; ++e) acc[b] = fmaf(x[b][c][e], wv[r][c][e], acc[b]);
            acc[b] = wave_sum(acc[b]);
        }
        if (lane == 0 && r < nr) {
            const float bv = bias ? ET<T>::ld(bias + row0 + r) : 0.f;
#pragma unroll
            for (int b = 0; b < BN; ++b) ET<T>::st(out + (size_t)b * rows + row0 + r, acc[b] + bv);
        }
    }
}
template <typename T, bool PRE_SILU, int KC>
static int gemv_rows_reg(const void* in, int B, const void* W, const void* bias, int64_t rows, void* out, hipStream_t st) {
    dim3 grid((unsigned)((rows + 4 * GEMV_R - 1) / (4 * GEMV_R)));
#define S2V_GEMV_B(BN)                                                                                                     \
    case BN:                                                                                                               \
        hipLaunchKernelGGL((gemv_rows_reg_k<T, PRE_SILU, KC, BN>), grid, dim3(256), 0, st, (const T*)in, (const T*)W,      \
                           (const T*)bias, rows, (T*)out);                                                                 \
        break;
    switch (B) {
        S2V_GEMV_B(1) S2V_GEMV_B(2) S2V_GEMV_B(3) S2V_GEMV_B(4)
        default: return s2v_fail(__FILE__, __LINE__, "gemv_rows: batch must be <= 4", -1);
    }
#undef S2V_GEMV_B
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
static int gemv_rows(const void* in, int B, int K, const void* W, const void* bias, int64_t rows, void* out,
                     bool pre_silu, hipStream_t st, bool rowwise = false) {
    S2V_REQUIRE(K % Vec16<T>::N == 0, "gemv_rows: K must be a multiple of the 16-byte vector width");
    if (B > GEMV_MAX_B) {  // the kernels hold GEMV_MAX_B accumulators per row: more samples run as chunks, in [b][K] -> out [b][rows]
        for (int b0 = 0; b0 < B; b0 += GEMV_MAX_B)
            S2V_TRY(gemv_rows<T>((const T*)in + (size_t)b0 * K, std::min(GEMV_MAX_B, B - b0), K, W, bias, rows, (T*)out + (size_t)b0 * rows,
                                 pre_silu, st, rowwise));
        return 0;
    }
    if (pre_silu && rows >= 4096 && !rowwise) {  // the modulation stack (K = time_embed_dim): one or two chunks per lane
        if (K == 64 * Vec16<T>::N) return gemv_rows_reg<T, true, 1>(in, B, W, bias, rows, out, st);
        if (K == 128 * Vec16<T>::N) return gemv_rows_reg<T, true, 2>(in, B, W, bias, rows, out, st);
    }
    dim3 grid((unsigned)((rows + 3) / 4));
    if (pre_silu)
        hipLaunchKernelGGL((gemv_rows_k<T, true>), grid, dim3(256), 0, st, (const T*)in, B, K, (const T*)W,
                           (const T*)bias, rows, (T*)out);
    else
        hipLaunchKernelGGL((gemv_rows_k<T, false>), grid, dim3(256), 0, st, (const T*)in, B, K, (const T*)W,
                           (const T*)bias, rows, (T*)out);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_time_embed(const float* t_dev, int B, int D, const void* w1, const void* b1, const void* w2, const void* b2,
                      int temb_dim, void* tmp, void* emb_out, int dtype, hipStream_t st) {
    // tmp holds [B, D] sinusoid followed by [B, temb] hidden
    const int n = B * D;
    S2V_DT_DISPATCH(dtype, {
        T* sc = (T*)tmp;
        T* h1 = sc + n;
        hipLaunchKernelGGL(timestep_sincos_k<T>, dim3((n + 255) / 256), dim3(256), 0, st, t_dev, B, D, sc);
        S2V_CHECK_HIP(hipGetLastError());
        S2V_TRY(gemv_rows<T>(sc, B, D, w1, b1, temb_dim, h1, false, st));
        S2V_TRY(gemv_rows<T>(h1, B, temb_dim, w2, b2, temb_dim, emb_out, true, st));
    })
    return 0;
}

int launch_mod_gemv(const void* emb, int B, int temb_dim, const void* W, const void* bias, int64_t rows_total,
                    void* out, int dtype, hipStream_t st, bool rowwise) {
    S2V_DT_DISPATCH(dtype, return gemv_rows<T>(emb, B, temb_dim, W, bias, rows_total, out, true, st, rowwise))
    return 0;
}

// ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ void patchify_k(const T* lat, int64_t lat_bstride, int n_lat, int Bn, int F, int C, int H, int W, T* out) {
    // out[(((b*F + f)*hp + y)*wp + x)][c*4 + py*2 + px] = lat[b][f][c][2y+py][2x+px]
    // (the im2col operand of the 2x2 stride-2 patch conv, embeddings.py:414-419)
    const int hp = H / 2, wp = W / 2, K = C * 4;
    const int64_t total = (int64_t)Bn * F * hp * wp * K;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % K);
    const int64_t tok = i / K;
    const int x = (int)(tok % wp);
    const int y = (int)((tok / wp) % hp);
    const int f = (int)((tok / ((int64_t)wp * hp)) % F);
    const int64_t b = tok / ((int64_t)wp * hp * F);
    const int64_t bl = n_lat > 0 ? b % n_lat : b;  // n_lat videos shared by Bn samples
    const int c = k >> 2, py = (k >> 1) & 1, px = k & 1;
    out[i] = lat[bl * lat_bstride + (((int64_t)f * C + c) * H + 2 * y + py) * W + 2 * x + px];
}
int launch_patchify(const void* lat, int64_t lat_bstride, int Bn, int F, int C, int H, int W, void* out, int dtype,
                    hipStream_t st, int n_lat) {
    const int64_t total = (int64_t)Bn * F * (H / 2) * (W / 2) * C * 4;
    dim3 grid((unsigned)((total + 255) / 256));
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(patchify_k<T>, grid, dim3(256), 0, st, (const T*)lat, lat_bstride, n_lat, Bn, F, C, H, W, (T*)out))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
__global__ void unpatchify_k(const T* y, int ldy, int64_t y_bstride, T* out, int B, int F, int C, int H, int W) {
    // out[b][f][c][yy][xx] = y[b*y_bstride + (f*hp + yy/2)*wp + xx/2][c*4 + (yy&1)*2 + (xx&1)]
    // (cogvideox_transformer_3d.py:549-551)
    const int hp = H / 2, wp = W / 2;
    const int64_t total = (int64_t)B * F * C * H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int xx = (int)(i % W);
    const int yy = (int)((i / W) % H);
    const int c = (int)((i / ((int64_t)W * H)) % C);
    const int f = (int)((i / ((int64_t)W * H * C)) % F);
    const int b = (int)(i / ((int64_t)W * H * C * F));
    const int64_t row = (int64_t)b * y_bstride + ((int64_t)f * hp + yy / 2) * wp + xx / 2;
    out[i] = y[row * ldy + c * 4 + (yy & 1) * 2 + (xx & 1)];
}
int launch_unpatchify(const void* y, int ldy, int64_t y_bstride, void* out, int B, int F, int C, int H, int W, int dtype,
                      hipStream_t st) {
    const int64_t total = (int64_t)B * F * C * H * W;
    dim3 grid((unsigned)((total + 255) / 256));
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(unpatchify_k<T>, grid, dim3(256), 0, st, (const T*)y, ldy, y_bstride, (T*)out, B, F, C, H, W))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
__global__ void copy_rows_k(const T* src, int lds_, const T* add, int ldadd, T* dst, int ldd, int rows, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * D) return;
    const int r = (int)(i / D), c = (int)(i - (int64_t)r * D);
    float v = ET<T>::ld(src + (size_t)r * lds_ + c);
    if (add) v += ET<T>::ld(add + (size_t)r * ldadd + c);
    ET<T>::st(dst + (size_t)r * ldd + c, v);
}
int launch_copy_rows(const void* src, int lds_, const void* add, int ldadd, void* dst, int ldd, int rows, int D,
                     int dtype, hipStream_t st) {
    const int64_t total = (int64_t)rows * D;
    if (total == 0) return 0;
    dim3 grid((unsigned)((total + 255) / 256));
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(copy_rows_k<T>, grid, dim3(256), 0, st, (const T*)src, lds_, (const T*)add, ldadd, (T*)dst, ldd, rows, D))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// CFG + scheduler step (custom_cogvideox_pipe.py:266-296; scheduling_ddim_cogvideox.py:364-394;
// scheduling_dpm_cogvideox.py:391-434).  Coefficients that multiply a model-dtype tensor (c_x0_x, a_t, m1, mn)
// arrive already rounded to the model dtype by the host: torch rounds a 0-dim fp64 scalar to the tensor dtype
// before the multiply (pinned by tests/golden/sched_*.npz).  __f*_rn keep the reference's separate roundings
// (no fma contraction), so the fp32 arithmetic is bit-identical to the CPU reference.
// A = SchedArgs: the step.  A = SchedMaskArgs: the step, then the masked video-to-video select on its rounded result (kernels.h): a cell is
// kept iff its level is <= the record's keep_max (a 0 / 1 mask: keep_max = 0; a change map: the video's threshold of this step).  The
// SchedArgs instantiation is the kernel it was before the masked form existed, kernel arguments included.
// TRIPLE (subject guidance, kernels.h): noise_pred is [3, n] = [u | r | f] and v = (u + g_subject * (r - u)) + g_text * (f - r), five roundings in
// that association.  A compile-time policy: the two pair instantiations hold no branch for it and take the arguments they took.
// The combine alone, element i of the planes: the guided prediction v as the step kernel uses it and as the statistics kernel of the guidance
// rescale sums it (cfg_stats_k below) -- one function, so the two cannot drift
template <typename T, bool TRIPLE, typename A>
__device__ __forceinline__ float cfg_combine(const A& a, int64_t i, const SchedCoef& k) {
#pragma clang fp contract(off)  // hipcc defaults to -ffp-contract=fast and __fmul_rn is a plain multiply in HIP
    float v;
    if constexpr (TRIPLE) {
        float u, r, f;
        if (a.np_f32) {
            const float* np = (const float*)a.noise_pred;
            u = np[i]; r = np[a.n + i]; f = np[2 * a.n + i];
        } else {
            const T* np = (const T*)a.noise_pred;
            u = ET<T>::ld(np + i); r = ET<T>::ld(np + a.n + i); f = ET<T>::ld(np + 2 * a.n + i);
        }
        const float s = __fadd_rn(u, __fmul_rn(k.guidance_subject, __fsub_rn(r, u)));
        v = __fadd_rn(s, __fmul_rn(k.guidance, __fsub_rn(f, r)));
    } else if (a.np_f32) {
        const float* np = (const float*)a.noise_pred;
        v = a.cfg ? __fadd_rn(np[i], __fmul_rn(k.guidance, __fsub_rn(np[a.n + i], np[i]))) : np[i];
    } else {
        const T* np = (const T*)a.noise_pred;
        if (a.cfg) {
            const float u = ET<T>::ld(np + i), c = ET<T>::ld(np + a.n + i);
            v = __fadd_rn(u, __fmul_rn(k.guidance, __fsub_rn(c, u)));
        } else {
            v = ET<T>::ld(np + i);
        }
    }
    return v;
}
// RESCALE (guidance rescale, kernels.h): A carries the device factors of the videos, and v' = v * factor[video] is one more separately rounded
// multiply ahead of the scheduler arithmetic.  A compile-time policy that the argument type carries (SchedRescaleArgs / SchedMaskRescaleArgs): the
// instantiations on SchedArgs / SchedMaskArgs keep their names and arguments and hold no load or multiply for it.
template <typename T, typename A, bool TRIPLE = false>
__global__ void sched_step_k(const A a) {
#pragma clang fp contract(off)  // hipcc defaults to -ffp-contract=fast and __fmul_rn is a plain multiply in HIP
    constexpr bool RESCALE = std::is_same<A, SchedRescaleArgs>::value || std::is_same<A, SchedMaskRescaleArgs>::value;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // within video blockIdx.y
    if (j >= a.n_vid) return;
    const int64_t i = (int64_t)blockIdx.y * a.n_vid + j;
    const SchedCoef k = a.coef ? a.coef[blockIdx.y] : a.cval;
    float v = cfg_combine<T, TRIPLE>(a, i, k);
    if constexpr (RESCALE) v = __fmul_rn(v, a.factor[blockIdx.y]);
    const float x = ET<T>::ld((const T*)a.latents_in + i);
    const float x0 = __fsub_rn(ET<T>::rnd(__fmul_rn(x, k.c_x0_x)), __fmul_rn(k.c_x0_v, v));
    float prev;
    if (k.kind == 0) {
        prev = __fadd_rn(ET<T>::rnd(__fmul_rn(k.a_t, x)), __fmul_rn(k.b_t, x0));
    } else {
        float d = x0;
        if (k.kind == 2) d = __fsub_rn(__fmul_rn(k.m3, x0), __fmul_rn(k.m4, a.x0_hist[i]));
        const float nz = ET<T>::ld((const T*)a.noise + i);
        prev = __fadd_rn(__fsub_rn(ET<T>::rnd(__fmul_rn(k.m1, x)), __fmul_rn(k.m2, d)), ET<T>::rnd(__fmul_rn(k.mn, nz)));
    }
    if (a.x0_hist) a.x0_hist[i] = x0;
    if constexpr (std::is_base_of<SchedMaskArgs, A>::value) {
        // the channel does not enter: element j of a video [F][C][hw] sits in cell j % hw of frame j / chw of the video's mask plane
        // (32-bit divisions: the launch requires a video of fewer than 2^31 elements)
        const unsigned ju = (unsigned)j, chw = (unsigned)a.chw, hw = (unsigned)a.hw;
        const int64_t cell = (int64_t)blockIdx.y * a.mask_vid + (ju / chw) * hw + ju % hw;
        T* out = (T*)a.latents_out + i;
        // the plane holds levels 0..255 as unsigned bytes; the record is the workgroup's own (uniform), loaded before the branch.  A 0 / 1 mask
        // with keep_max = 0 is the test `mask != 0`
        const SchedBlend bl = a.blend ? a.blend[blockIdx.y] : a.bval;
        if ((int)a.mask[cell] > bl.keep_max) { ET<T>::st(out, prev); return; }
        const T* z0 = (const T*)a.z0 + i;
        if (bl.last) { *out = *z0; return; }   // the bits of z0, -0 included
        const float s = ET<T>::rnd(__fmul_rn(bl.sqrt_a, ET<T>::ld(z0)));                       // add_noise_k's arithmetic
        const float e = ET<T>::rnd(__fmul_rn(bl.sqrt_1ma, ET<T>::ld((const T*)a.noise0 + i)));
        ET<T>::st(out, __fadd_rn(s, e));
    } else {
        if (a.out_f32) ((float*)a.latents_out)[i] = prev;
        else ET<T>::st((T*)a.latents_out + i, prev);
    }
}
static int sched_step_checks(const SchedArgs& a) {
    S2V_REQUIRE(a.nvid >= 1 && a.n_vid >= 1 && (int64_t)a.nvid * a.n_vid == a.n, "sched_step: n must be nvid videos of n_vid elements");
    S2V_REQUIRE(a.coef || a.nvid == 1, "sched_step: several videos take their coefficient sets from device memory");
    S2V_REQUIRE(a.cfg == 0 || a.cfg == 1 || a.cfg == SCHED_CFG_TRIPLE, "sched_step: cfg is 0 (one prediction), 1 (the CFG pair) or SCHED_CFG_TRIPLE (the subject-guidance triple)");
    return 0;
}
int launch_sched_step(const SchedArgs& a, int dtype, hipStream_t st, const float* factor) {
    S2V_TRY(sched_step_checks(a));
    dim3 grid((unsigned)((a.n_vid + 255) / 256), (unsigned)a.nvid);
    if (factor) {   // the RESCALE form: the same arguments with the videos' factors behind them
        SchedRescaleArgs r{};
        static_cast<SchedArgs&>(r) = a; r.factor = factor;
        if (a.cfg == SCHED_CFG_TRIPLE) { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((sched_step_k<T, SchedRescaleArgs, true>), grid, dim3(256), 0, st, r)) }
        else { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((sched_step_k<T, SchedRescaleArgs>), grid, dim3(256), 0, st, r)) }
    }
    else if (a.cfg == SCHED_CFG_TRIPLE) { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((sched_step_k<T, SchedArgs, true>), grid, dim3(256), 0, st, a)) }
    else { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((sched_step_k<T, SchedArgs>), grid, dim3(256), 0, st, a)) }
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}
int launch_sched_step_masked(const SchedMaskArgs& a, int dtype, hipStream_t st, const float* factor) {
    S2V_TRY(sched_step_checks(a));
    S2V_REQUIRE(a.z0 && a.noise0 && a.mask, "sched_step_masked: z0, noise0 and the latent mask are required");
    S2V_REQUIRE(a.blend || a.nvid == 1, "sched_step_masked: several videos take their blend records from device memory");
    S2V_REQUIRE(!a.out_f32, "sched_step_masked: the blend runs on the latents rounded to the model dtype (no fp32 output)");    S2V_REQUIRE(a.hw >= 1 && a.chw >= a.hw && a.chw % a.hw == 0 && a.n_vid % a.chw == 0,
                "sched_step_masked: a video is [F][C][H * W] elements over a mask plane of [F][H * W] cells");
    S2V_REQUIRE(a.n_vid < ((int64_t)1 << 31) && a.mask_vid == a.n_vid / a.chw * a.hw, "sched_step_masked: a video of fewer than 2^31 elements, mask_vid = F * H * W cells");
    dim3 grid((unsigned)((a.n_vid + 255) / 256), (unsigned)a.nvid);
    if (factor) {
        SchedMaskRescaleArgs r{};
        static_cast<SchedMaskArgs&>(r) = a; r.factor = factor;
        if (a.cfg == SCHED_CFG_TRIPLE) { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((sched_step_k<T, SchedMaskRescaleArgs, true>), grid, dim3(256), 0, st, r)) }
        else { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((sched_step_k<T, SchedMaskRescaleArgs>), grid, dim3(256), 0, st, r)) }
    }
    else if (a.cfg == SCHED_CFG_TRIPLE) { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((sched_step_k<T, SchedMaskArgs, true>), grid, dim3(256), 0, st, a)) }
    else { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((sched_step_k<T, SchedMaskArgs>), grid, dim3(256), 0, st, a)) }
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Guidance rescale (kernels.h; include/s2v_hip.h has the definition): the statistics of a video's text-conditioned prediction f and of its guided
// prediction v, ahead of the step kernel that multiplies v by the video's factor.
// cfg_stats_k: workgroup (chunk c, video blockIdx.y) owns the elements [c * CFG_STATS_CHUNK, min(n_vid, (c + 1) * CFG_STATS_CHUNK)) of its video.
// Thread t adds its elements c * CFG_STATS_CHUNK + t + 256 r, r = 0, 1, ... ascending, into four fp64 accumulators that start from +0 (f, f * f,
// v, v * v: the fp32 values widened first, so every square is exact); the 256 thread sums then meet in LDS in the halving tree
// acc[t] += acc[t + s], s = 128, 64, ..., 1, and thread 0 stores the chunk's quadruple.  Nothing depends on the grid or on timing: no atomics.
template <typename T, bool TRIPLE>
__global__ __launch_bounds__(256) void cfg_stats_k(const CfgStatsArgs a) {
#pragma clang fp contract(off)  // every fp64 add and multiply rounds on its own, as the restatements do
    __shared__ double red[4][256];
    const int t = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * CFG_STATS_CHUNK;
    const int64_t hi = lo + CFG_STATS_CHUNK < a.n_vid ? lo + CFG_STATS_CHUNK : a.n_vid;
    const SchedCoef k = a.coef ? a.coef[blockIdx.y] : a.cval;
    double sf = 0.0, sff = 0.0, sv = 0.0, svv = 0.0;
    for (int64_t j = lo + t; j < hi; j += 256) {
        const int64_t i = (int64_t)blockIdx.y * a.n_vid + j;
        const int64_t fi = (TRIPLE ? 2 : 1) * a.n + i;   // the positive half of a pair, the f plane of a triple
        const double f = a.np_f32 ? (double)((const float*)a.noise_pred)[fi] : (double)ET<T>::ld((const T*)a.noise_pred + fi);
        const double v = (double)cfg_combine<T, TRIPLE>(a, i, k);
        sf = sf + f; sff = sff + f * f; sv = sv + v; svv = svv + v * v;
    }
    red[0][t] = sf; red[1][t] = sff; red[2][t] = sv; red[3][t] = svv;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s)
            for (int q = 0; q < 4; ++q) red[q][t] = red[q][t] + red[q][t + s];
        __syncthreads();
    }
    if (t < 4) a.partials[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + t] = red[t][0];
}
// cfg_finalize_k: one workgroup; thread k < nvid adds video k's chunk quadruples in ascending chunk order (from +0), stores the four sums and
// derives the factor in fp64 (include/s2v_hip.h); threads 0 .. CFG_LOG_COLS - 1 append the row of factors (0 past nvid) to the log at the
// device-side count, which thread 0 then advances with a plain store -- the launches of a stream are ordered, and a graph replay logs too.
__global__ __launch_bounds__(64) void cfg_finalize_k(const CfgFinalArgs a) {
#pragma clang fp contract(off)
    const int k = threadIdx.x;
    float factor = 0.f;
    if (k < a.nvid) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        const double* p = a.partials + (int64_t)k * a.chunks * 4;
        for (int c = 0; c < a.chunks; ++c)
            for (int q = 0; q < 4; ++q) s[q] = s[q] + p[c * 4 + q];
        for (int q = 0; q < 4; ++q) a.sums[k * 4 + q] = s[q];
        const double phi = (double)a.phi[k], n = (double)a.n_vid;
        factor = 1.0f;
        if (phi != 0.0 && a.n_vid >= 2) {
            const double std_f = sqrt((s[1] - s[0] * s[0] / n) / (n - 1.0));
            const double std_v = sqrt((s[3] - s[2] * s[2] / n) / (n - 1.0));
            if (isfinite(std_v) && std_v != 0.0) {
                const double q = std_f / std_v;
                if (isfinite(q)) factor = (float)(phi * q + (1.0 - phi));
            }
        }
        a.factors[k] = factor;
    }
    if (a.log) {
        const unsigned step = *a.log_count;
        if (k < CFG_LOG_COLS && step < CFG_LOG_STEPS) a.log[step * CFG_LOG_COLS + k] = factor;
        __syncthreads();
        if (k == 0) *a.log_count = step + 1;
    }
}
int cfg_stats_chunks(int64_t n_vid) { return (int)((n_vid + CFG_STATS_CHUNK - 1) / CFG_STATS_CHUNK); }
int launch_cfg_stats(const CfgStatsArgs& a, int dtype, hipStream_t st) {
    S2V_REQUIRE(a.noise_pred && a.partials, "cfg_stats: null argument");
    S2V_REQUIRE(a.nvid >= 1 && a.n_vid >= 1 && (int64_t)a.nvid * a.n_vid == a.n, "cfg_stats: n must be nvid videos of n_vid elements");
    S2V_REQUIRE(a.coef || a.nvid == 1, "cfg_stats: several videos take their coefficient sets from device memory");
    S2V_REQUIRE(a.cfg == 1 || a.cfg == SCHED_CFG_TRIPLE, "cfg_stats: cfg is 1 (the CFG pair) or SCHED_CFG_TRIPLE (the subject-guidance triple): one prediction has no guided form");
    dim3 grid((unsigned)cfg_stats_chunks(a.n_vid), (unsigned)a.nvid);
    if (a.cfg == SCHED_CFG_TRIPLE) { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((cfg_stats_k<T, true>), grid, dim3(256), 0, st, a)) }
    else { S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL((cfg_stats_k<T, false>), grid, dim3(256), 0, st, a)) }
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}
int launch_cfg_finalize(const CfgFinalArgs& a, hipStream_t st) {
    S2V_REQUIRE(a.partials && a.phi && a.sums && a.factors, "cfg_finalize: null argument");
    S2V_REQUIRE(a.nvid >= 1 && a.nvid <= CFG_LOG_COLS && a.n_vid >= 1 && a.chunks == cfg_stats_chunks(a.n_vid), "cfg_finalize: 1..4 videos of n_vid elements in the chunks of cfg_stats");
    S2V_REQUIRE(!a.log == !a.log_count, "cfg_finalize: the log and its count go together");
    hipLaunchKernelGGL(cfg_finalize_k, dim3(1), dim3(64), 0, st, a);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Temporal windows: the blend of one forward's windows into the fp32 plane of the long latent (kernels.h).  A GATHER: one thread owns one
// element of the plane inside the frames [k0 s, (k0 + wb - 1) s + F) this launch covers, and adds the contributions of the batch's windows
// that cover its frame in ascending k.  The windows of a batch overlap, so a thread per window element would race on the plane, and atomics
// would lose the order of the additions, which the bits depend on.
// Frame f is covered by the windows k_first .. k_last, k_first = 0 for f < F, else (f - F) / s + 1, and k_last = min(W - 1, f / s).  Both
// ends are decided PER FRAME, not per launch: the thread starts from +0 without reading the plane when k_first is in this batch (so the plane
// never needs clearing between steps), and divides by wsum[f] on the way out when k_last is in this batch -- every frame is divided by the
// batch that covers it last, no launch runs over frames it has nothing to add to.  The batches of a step are stream-ordered launches.
template <typename T>
__global__ void window_blend_k(const WindowBlendArgs a) {
#pragma clang fp contract(off)  // as sched_step_k: every operation rounds on its own
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned chw = (unsigned)a.chw;
    if (i >= (int64_t)((a.wb - 1) * a.s + a.F) * chw) return;
    // 32-bit divisions: the launch requires a plane of fewer than 2^31 elements
    const unsigned iu = (unsigned)i, e = iu % chw;
    const int f = a.k0 * a.s + (int)(iu / chw);
    const int k_first = f < a.F ? 0 : (f - a.F) / a.s + 1, k_last = min(a.W - 1, f / a.s);
    const int ka = max(k_first, a.k0), kb = min(k_last, a.k0 + a.wb - 1);
    const float g = a.coef ? a.coef->guidance : a.gval;
    float* cell = a.acc + (int64_t)f * chw + e;
    float acc = k_first >= a.k0 ? 0.f : *cell;
    const int64_t win = (int64_t)a.F * chw;
    const T* np = (const T*)a.noise_pred;
    for (int k = ka; k <= kb; ++k) {
        const int j = f - k * a.s;   // the frame's place in window k: 0 <= j < F by the bounds of k
        const int64_t o = (k - a.k0) * win + (int64_t)j * chw + e;
        const float u = ET<T>::ld(np + o), c = ET<T>::ld(np + a.wb * win + o);
        const float v = __fadd_rn(u, __fmul_rn(g, __fsub_rn(c, u)));
        acc = __fadd_rn(acc, __fmul_rn(a.w[j], v));
    }
    if (k_last <= a.k0 + a.wb - 1) acc = __fdiv_rn(acc, a.wsum[f]);
    *cell = acc;
}
int launch_window_blend(const WindowBlendArgs& a, int dtype, hipStream_t st) {
    S2V_REQUIRE(a.noise_pred && a.acc && a.w && a.wsum, "window_blend: null argument");
    S2V_REQUIRE(a.F >= 1 && a.s >= 1 && a.s <= a.F && a.L >= a.F && (a.L - a.F) % a.s == 0 && a.W == (a.L - a.F) / a.s + 1,
                "window_blend: W = (L - F) / s + 1 windows of F frames, 1 <= s <= F, must tile the L frames exactly");
    S2V_REQUIRE(a.k0 >= 0 && a.wb >= 1 && a.k0 + a.wb <= a.W, "window_blend: the batch's windows k0 .. k0 + wb - 1 must lie inside 0 .. W - 1");
    S2V_REQUIRE(a.chw >= 1 && (int64_t)a.L * a.chw < ((int64_t)1 << 31), "window_blend: a plane of fewer than 2^31 elements");
    const int64_t n = (int64_t)((a.wb - 1) * a.s + a.F) * a.chw;
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(window_blend_k<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// The pixel mask of masked video-to-video -> the latent mask (kernels.h).  One thread per latent cell: its 8 x 8 pixels of 1 or 4 frames,
// a row of 8 mask values per load; with pixel_out the binarised rows are written on the way (8 bytes per store).
template <typename M> struct MaskRow;   // the 8 mask values at p, binarised: byte k of the result is 0 or 1
// byte != 0 -> 1: the high bit of (b & 0x7f) + 0x7f is set when the low seven bits are non-zero, b's own high bit covers the rest
__device__ __forceinline__ unsigned long long nonzero_bytes(unsigned long long v) {
    return ((((v & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | v) >> 7) & 0x0101010101010101ull;
}
template <> struct MaskRow<unsigned char> {
    static __device__ __forceinline__ unsigned long long ld(const unsigned char* p) { return nonzero_bytes(*(const unsigned long long*)p); }
};
template <> struct MaskRow<float> {
    static __device__ __forceinline__ unsigned long long ld(const float* p) {
        float v[8];
        Vec16<float>::ld(p, v);
        Vec16<float>::ld(p + 4, v + 4);
        unsigned long long r = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) r |= (unsigned long long)(v[k] >= 0.5f) << (8 * k);
        return r;
    }
};
template <typename M> struct MaskRow {   // bf16_t / f16_t: eight values in one 16-byte load
    static __device__ __forceinline__ unsigned long long ld(const M* p) {
        float v[8];
        Vec16<M>::ld(p, v);
        unsigned long long r = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) r |= (unsigned long long)(v[k] >= 0.5f) << (8 * k);
        return r;
    }
};
template <typename M>
__global__ void mask_to_latent_k(const M* mask, int F, int H, int W, unsigned char* lat, unsigned char* pix) {
    const int h = H / 8, w = W / 8, Fl = (F - 1) / 4 + 1;
    const int64_t total = (int64_t)Fl * h * w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % w), y = (int)((i / w) % h), fl = (int)(i / ((int64_t)w * h));
        const int f0 = fl == 0 ? 0 : 4 * fl - 3, f1 = fl == 0 ? 0 : 4 * fl;   // pixel frames f0 .. f1 (F = 4 (Fl - 1) + 1: all inside)
        unsigned long long any = 0;
        for (int f = f0; f <= f1; ++f)
            for (int r = 0; r < 8; ++r) {
                const int64_t p = ((int64_t)f * H + 8 * y + r) * W + 8 * x;
                const unsigned long long row = MaskRow<M>::ld(mask + p);
                any |= row;
                if (pix) *(unsigned long long*)(pix + p) = row;
            }
        lat[i] = any != 0;
    }
}
int launch_mask_to_latent(const void* mask, int mdtype, int F, int H, int W, unsigned char* latent_out, unsigned char* pixel_out, hipStream_t st) {
    S2V_REQUIRE(mask && latent_out, "mask_to_latent: null argument");
    S2V_REQUIRE(F >= 1 && (F - 1) % 4 == 0 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0,
                "mask_to_latent: F = 4k + 1 frames of H x W pixels, both multiples of 8");
    S2V_REQUIRE(mdtype == S2V_F32 || mdtype == S2V_BF16 || mdtype == S2V_F16 || mdtype == S2V_MASK_U8, "mask_to_latent: unknown mask dtype");
    const int64_t total = (int64_t)((F - 1) / 4 + 1) * (H / 8) * (W / 8);
    const dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 16));
    if (mdtype == S2V_MASK_U8) {
        hipLaunchKernelGGL(mask_to_latent_k<unsigned char>, grid, dim3(256), 0, st, (const unsigned char*)mask, F, H, W, latent_out, pixel_out);
    } else {
        S2V_DT_DISPATCH(mdtype, hipLaunchKernelGGL(mask_to_latent_k<T>, grid, dim3(256), 0, st, (const T*)mask, F, H, W, latent_out, pixel_out))
    }
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// The change map of video-to-video -> the latent levels (kernels.h).  mask_to_latent_k's walk -- one thread per latent cell, its 8 x 8 pixels
// of 1 or 4 frames, a row of 8 map values per load -- with every value quantised to a level 0..255 and the running MAXIMUM in place of "any";
// with pixel_out the rows of `level > 0` are written on the way (8 bytes per store).
// float maps: level = floor(clamp(v, 0, 1) * 255 + 0.5) in fp32, the multiply and the add rounded separately; NaN -> 0 (no compare holds)
__device__ __forceinline__ unsigned long long quantise_row(const float* v) {
#pragma clang fp contract(off)  // hipcc defaults to -ffp-contract=fast
    unsigned long long r = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float c = v[k] > 0.f ? (v[k] < 1.f ? v[k] : 1.f) : 0.f;
        r |= (unsigned long long)(unsigned)__fadd_rn(__fmul_rn(c, 255.f), 0.5f) << (8 * k);   // 0.5 <= the sum <= 255.5: truncation is floor
    }
    return r;
}
template <typename M> struct MapRow;   // the 8 map values at p as levels: byte k of the result is 0..255
template <> struct MapRow<unsigned char> {
    static __device__ __forceinline__ unsigned long long ld(const unsigned char* p) { return *(const unsigned long long*)p; }
};
template <> struct MapRow<float> {
    static __device__ __forceinline__ unsigned long long ld(const float* p) {
        float v[8];
        Vec16<float>::ld(p, v);
        Vec16<float>::ld(p + 4, v + 4);
        return quantise_row(v);
    }
};
template <typename M> struct MapRow {   // bf16_t / f16_t: eight values in one 16-byte load
    static __device__ __forceinline__ unsigned long long ld(const M* p) {
        float v[8];
        Vec16<M>::ld(p, v);
        return quantise_row(v);
    }
};
template <typename M>
__global__ void map_to_latent_k(const M* map, int F, int H, int W, unsigned char* lat, unsigned char* pix) {
    const int h = H / 8, w = W / 8, Fl = (F - 1) / 4 + 1;
    const int64_t total = (int64_t)Fl * h * w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % w), y = (int)((i / w) % h), fl = (int)(i / ((int64_t)w * h));
        const int f0 = fl == 0 ? 0 : 4 * fl - 3, f1 = fl == 0 ? 0 : 4 * fl;   // pixel frames f0 .. f1 (F = 4 (Fl - 1) + 1: all inside)
        unsigned level = 0;
        for (int f = f0; f <= f1; ++f)
            for (int r = 0; r < 8; ++r) {
                const int64_t p = ((int64_t)f * H + 8 * y + r) * W + 8 * x;
                const unsigned long long row = MapRow<M>::ld(map + p);
#pragma unroll
                for (int k = 0; k < 8; ++k) level = max(level, (unsigned)(row >> (8 * k)) & 0xffu);
                if (pix) *(unsigned long long*)(pix + p) = nonzero_bytes(row);
            }
        lat[i] = (unsigned char)level;
    }
}
int launch_map_to_latent(const void* map, int mdtype, int F, int H, int W, unsigned char* level_out, unsigned char* pixel_out, hipStream_t st) {
    S2V_REQUIRE(map && level_out, "map_to_latent: null argument");
    S2V_REQUIRE(F >= 1 && (F - 1) % 4 == 0 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0,
                "map_to_latent: F = 4k + 1 frames of H x W pixels, both multiples of 8");
    S2V_REQUIRE(mdtype == S2V_F32 || mdtype == S2V_BF16 || mdtype == S2V_F16 || mdtype == S2V_MASK_U8, "map_to_latent: unknown map dtype");
    const int64_t total = (int64_t)((F - 1) / 4 + 1) * (H / 8) * (W / 8);
    const dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 16));
    if (mdtype == S2V_MASK_U8) {
        hipLaunchKernelGGL(map_to_latent_k<unsigned char>, grid, dim3(256), 0, st, (const unsigned char*)map, F, H, W, level_out, pixel_out);
    } else {
        S2V_DT_DISPATCH(mdtype, hipLaunchKernelGGL(map_to_latent_k<T>, grid, dim3(256), 0, st, (const T*)map, F, H, W, level_out, pixel_out))
    }
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// scheduler.add_noise (scheduling_ddim_cogvideox.py:405-431, scheduling_dpm_cogvideox.py:442) of the video-to-video start
// (pipeline_cogvideox_video2video.py:389): out = sqrt_a * x + sqrt_1ma * noise.  The host hands sqrt(alphas_cumprod[t]) and
// sqrt(1 - alphas_cumprod[t]) already taken in T as torch takes them; both products and the sum round to T like torch's elementwise ops.
// No fma contraction.
template <typename T>
__global__ void add_noise_k(const T* x, const T* noise, int64_t n, float sqrt_a, float sqrt_1ma, T* out) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float a = ET<T>::rnd(__fmul_rn(sqrt_a, ET<T>::ld(x + i)));
        const float b = ET<T>::rnd(__fmul_rn(sqrt_1ma, ET<T>::ld(noise + i)));
        ET<T>::st(out + i, __fadd_rn(a, b));
    }
}
int launch_add_noise(const void* x, const void* noise, int64_t n, float sqrt_a, float sqrt_1ma, void* out, int dtype, hipStream_t st) {
    const int64_t g = std::min<int64_t>((n + 255) / 256, 1 << 20);
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(add_noise_k<T>, dim3((unsigned)(g < 1 ? 1 : g)), dim3(256), 0, st, (const T*)x,
                       (const T*)noise, n, sqrt_a, sqrt_1ma, (T*)out))
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
template <typename TS, typename TD>
__global__ void convert2d_k(const TS* src, int64_t lds_, TD* dst, int64_t ldd, int64_t rows, int64_t cols) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int64_t r = i / cols, c = i - r * cols;
    ET<TD>::st(dst + r * ldd + c, ET<TS>::ld(src + r * lds_ + c));
}
int launch_convert2d(const void* src, int sdt, int64_t lds_, void* dst, int ddt, int64_t ldd, int64_t rows, int64_t cols,
                     hipStream_t st) {
    const int64_t total = rows * cols;
    if (total == 0) return 0;
    dim3 grid((unsigned)((total + 255) / 256));
#define CV(TS, TD) hipLaunchKernelGGL((convert2d_k<TS, TD>), grid, dim3(256), 0, st, (const TS*)src, lds_, (TD*)dst, ldd, rows, cols)
    S2V_REQUIRE(sdt >= 0 && sdt <= 2 && ddt >= 0 && ddt <= 2, "convert: unknown dtype");
    switch (sdt * 3 + ddt) {
        case S2V_F32 * 3 + S2V_F32: CV(float, float); break;
        case S2V_F32 * 3 + S2V_BF16: CV(float, bf16_t); break;
        case S2V_F32 * 3 + S2V_F16: CV(float, f16_t); break;
        case S2V_BF16 * 3 + S2V_F32: CV(bf16_t, float); break;
        case S2V_BF16 * 3 + S2V_BF16: CV(bf16_t, bf16_t); break;
        case S2V_BF16 * 3 + S2V_F16: CV(bf16_t, f16_t); break;
        case S2V_F16 * 3 + S2V_F32: CV(f16_t, float); break;
        case S2V_F16 * 3 + S2V_BF16: CV(f16_t, bf16_t); break;
        default: CV(f16_t, f16_t); break;
    }
#undef CV
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}
int launch_convert(const void* src, int sdt, void* dst, int ddt, int64_t n, hipStream_t st) {
    return launch_convert2d(src, sdt, n, dst, ddt, n, 1, n, st);
}

// ---------------------------------------------------------------------------------------------------
// Dynamic per-row fp8 quantisation (W8A8, BASELINE configs[4]): one wave per row, two passes over a row that stays in L2 / registers:
// amax -> scale = amax / 448 (the largest e4m3 magnitude) -> q = rne_e4m3(x / scale).  Also quantises the weights at load time (a
// weight row = an output channel).  Rows are padded to the caller's tile by zero scales / zero bytes outside [0, M).
__global__ __launch_bounds__(256) void quant_rows_fp8_k(const bf16_t* src, int64_t ld, int64_t M, int K, unsigned char* dst, float* scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const bf16_t* x = src + row * ld;
    float amax = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        const u32x4 v = *(const u32x4*)(x + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            amax = fmaxf(amax, fabsf(__uint_as_float(v[e] << 16)));
            amax = fmaxf(amax, fabsf(__uint_as_float(v[e] & 0xffff0000u)));
        }
    }
    amax = wave_max(amax);
    const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
    const float inv = 1.0f / sc;
    if (lane == 0) scale[row] = sc;
    unsigned char* q = dst + row * (int64_t)K;
    for (int k = lane * 8; k < K; k += 512) {
        const u32x4 v = *(const u32x4*)(x + k);
        u32x2 o;
        int w0 = 0, w1 = 0;
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(v[0] << 16) * inv, __uint_as_float(v[0] & 0xffff0000u) * inv, w0, false);
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(v[1] << 16) * inv, __uint_as_float(v[1] & 0xffff0000u) * inv, w0, true);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(v[2] << 16) * inv, __uint_as_float(v[2] & 0xffff0000u) * inv, w1, false);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(v[3] << 16) * inv, __uint_as_float(v[3] & 0xffff0000u) * inv, w1, true);
        o.x = (unsigned)w0; o.y = (unsigned)w1;
        *(u32x2*)(q + k) = o;
    }
}
int launch_quant_rows_fp8(const void* src, int64_t ld, int64_t M, int K, void* dst, float* scale, hipStream_t st) {
    S2V_REQUIRE(K % 8 == 0 && ld % 8 == 0, "quant_rows_fp8: K and the row stride must be multiples of 8");
    if (M <= 0) return 0;
    hipLaunchKernelGGL(quant_rows_fp8_k, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, (const bf16_t*)src, ld, M, K, (unsigned char*)dst, scale);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Step cache (include/s2v_hip.h): the video rows of the packed residual buffer -- sample b's n = V * D elements start at x + b * x_bstride
// and are contiguous, rows being D apart -- against the dense cache [B][n].  Streaming kernels: every lane moves 16 bytes per operand and
// round, blockIdx.y is the sample, the grid strides over the sample's n / Vec16<T>::N vectors (any count: no multiple of the block is assumed).
//   SC_KEEP: cache = x (and keep2 = x when given)      SC_SUB: cache = rnd(float(x) - float(cache))      SC_ADD: x = rnd(float(x) + float(cache))
// The sums are single fp32 operations rounded once to T (round to nearest even); this translation unit is built without fma contraction.
template <typename T, int OP>
__global__ __launch_bounds__(256) void step_cache_k(T* x, int64_t x_bstride, T* cache, T* keep2, int64_t nvec) {
    constexpr int VN = Vec16<T>::N;
    T* xs = x + (int64_t)blockIdx.y * x_bstride;
    T* cs = cache + (int64_t)blockIdx.y * nvec * VN;
    T* ks = keep2 ? keep2 + (int64_t)blockIdx.y * nvec * VN : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        if (OP == SC_KEEP) {
            const typename Vec16<T>::raw_t v = Vec16<T>::ldraw(xs + i * VN);
            *(typename Vec16<T>::raw_t*)(cs + i * VN) = v;
            if (ks) *(typename Vec16<T>::raw_t*)(ks + i * VN) = v;
        } else {
            float a[VN], d[VN], o[VN];
            Vec16<T>::ld(xs + i * VN, a);
            Vec16<T>::ld(cs + i * VN, d);
#pragma unroll
            for (int e = 0; e < VN; ++e) o[e] = OP == SC_SUB ? a[e] - d[e] : a[e] + d[e];
            Vec16<T>::st(OP == SC_SUB ? cs + i * VN : xs + i * VN, o);
        }
    }
}
int launch_step_cache(int op, void* x, int64_t x_bstride, void* cache, void* keep2, int B, int64_t n, int dtype, hipStream_t st) {
    const int esz = dtype == S2V_F32 ? 4 : 2, vn = 16 / esz;
    S2V_REQUIRE(op == SC_KEEP || op == SC_SUB || op == SC_ADD, "step_cache: unknown operation");
    S2V_REQUIRE(n % vn == 0 && x_bstride % vn == 0 && ((uintptr_t)x | (uintptr_t)cache | (uintptr_t)keep2) % 16 == 0,
                "step_cache: the rows must be whole 16-byte vectors on 16-byte boundaries");
    if (B <= 0 || n <= 0) return 0;
    const int64_t nvec = n / vn;
    // at most ~2048 workgroups in all (eight per CU); the rest of a sample is taken by the grid stride
    const int64_t cap = std::max<int64_t>(1, 2048 / B);
    dim3 grid((unsigned)std::min<int64_t>((nvec + 255) / 256, cap), (unsigned)B);
#define S2V_SC_OP(OP) hipLaunchKernelGGL((step_cache_k<T, OP>), grid, dim3(256), 0, st, (T*)x, x_bstride, (T*)cache, (T*)keep2, nvec)
    S2V_DT_DISPATCH(dtype, {
        if (op == SC_KEEP) S2V_SC_OP(SC_KEEP);
        else if (op == SC_SUB) S2V_SC_OP(SC_SUB);
        else S2V_SC_OP(SC_ADD);
    })
#undef S2V_SC_OP
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}
