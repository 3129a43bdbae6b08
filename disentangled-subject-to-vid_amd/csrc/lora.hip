// Runtime LoRA (include/s2v_hip.h, s2v_lora_*): the adapter branch of an adapted linear rides in the base GEMM as a K extension,
//     y = epilogue([x | T] . [W | Bs]^T + b),   T = rnd(x . A^T),   Bs = rnd(s * B),
// so the only new work per step is the down-projection T = x . A^T.  It is a skinny GEMM (N <= 384 output columns against K = 3072 or
// 12 288) whose cost is reading x once: one workgroup owns 128 rows and ALL N columns, x streams from HBM exactly once and the A stack
// (<= 2.4 MB) is re-read from cache by every workgroup.  T is rounded to the model dtype (the point where PEFT rounds lora_A's output)
// and stored into the columns [K, K + N) of the buffer x itself lives in (the buffer's row pitch has room for them).
// The attach-time kernels (A -> stack, s * B -> weight tail) are plain HIP below.
#define S2V_HOST
#include "common.h"
#include "kernels.h"
#include <type_traits>

// ---- down-projection on v_mfma_f32_32x32x16_{bf16,f16} --------------------------------------------------------------------------------
// 512 threads = 8 waves: wave (wm, wn) owns rows [32 wm, 32 wm + 32) of the 128-row block and the column half wn (N / 2 columns =
// N / 64 tiles of 32, at most NTW = 6 for the fused QKV's N = 384: 96 accumulator registers, 180 VGPRs, one workgroup per CU).  K runs in chunks of 64: the 128 x 64 piece of x and the N x 64 piece of A
// sit in LDS as 128-byte rows whose 16-byte chunks are XOR-swizzled with (row >> 1) & 7 (the layout of gemm_bf16_128: conflict-free
// ds_read_b128 fragments); the next chunk's global loads are in flight in registers while the current one is multiplied.
#define LD_BM 128
#define LD_BK 64
#define LD_NMAX 384
#define LD_THREADS 512
#define LD_LDS(n) ((LD_BM + (n)) * LD_BK * 2)   // 64 KiB at N = 384, 32 KiB at N = 128

template <typename T16>
__device__ __forceinline__ f32x16 lora_mfma(bf16x8 x, bf16x8 y, f32x16 acc) {
    if constexpr (std::is_same<T16, f16_t>::value) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, x), __builtin_bit_cast(f16x8, y), acc, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, acc, 0, 0, 0);
}

__device__ __forceinline__ int lora_swz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

template <typename T16, int NTW>
__global__ __launch_bounds__(LD_THREADS, 2) void lora_down_mfma_k(const LoraDownArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* tX = smem;                       // [128][64] of x
    char* tA = smem + LD_BM * LD_BK * 2;   // [N][64] of the A stack
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 3, wn = wave >> 2;
    const int fr = lane & 31, hi = lane >> 5;
    const int m0 = blockIdx.x * LD_BM;
    const int ntw = a.N >> 6;              // 32-column tiles per wave (N % 64 == 0, N <= 64 NTW)
    const char* X = (const char*)a.x;
    const char* A = (const char*)a.A;

    // global pieces of a K chunk: 16 bytes each; x: 128 rows x 8, A: N rows x 8.  Piece p -> row p >> 3, chunk p & 7
    u32x4 rx[2], ra[NTW];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = i * LD_THREADS + tid, row = p >> 3, ch = p & 7;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (m0 + row < a.M) v = *(const u32x4*)(X + 2 * ((int64_t)(m0 + row) * a.ldx + k0 + ch * 8));
            rx[i] = v;
        }
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int p = i * LD_THREADS + tid, row = p >> 3, ch = p & 7;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (row < a.N) v = *(const u32x4*)(A + 2 * ((int64_t)row * a.lda + k0 + ch * 8));
            ra[i] = v;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = i * LD_THREADS + tid;
            *(u32x4*)(tX + lora_swz(p >> 3, p & 7)) = rx[i];
        }
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int p = i * LD_THREADS + tid;
            if ((p >> 3) < a.N) *(u32x4*)(tA + lora_swz(p >> 3, p & 7)) = ra[i];
        }
    };

    f32x16 acc[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    const int nt = a.K / LD_BK;
    fetch(0);
    for (int t = 0; t < nt; ++t) {
        commit();
        __syncthreads();
        if (t + 1 < nt) fetch((t + 1) * LD_BK);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bf16x8 xf = *(const bf16x8*)(tX + lora_swz(wm * 32 + fr, kk * 2 + hi));
#pragma unroll
            for (int i = 0; i < NTW; ++i) {
                if (i < ntw) {
                    const bf16x8 af = *(const bf16x8*)(tA + lora_swz((wn * ntw + i) * 32 + fr, kk * 2 + hi));
                    acc[i] = lora_mfma<T16>(af, xf, acc[i]);   // D[i = column of T][j = row of x]
                }
            }
        }
        __syncthreads();
    }
    // lane: row m = fr of the wave's 32, columns (reg & 3) + 8 * (reg >> 2) + 4 * hi of the tile: four consecutive columns per quad
    const int m = m0 + wm * 32 + fr;
    if (m >= a.M) return;
    T16* out = (T16*)a.out + (int64_t)m * a.ldo;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        if (i < ntw) {
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int n = (wn * ntw + i) * 32 + 8 * rq + 4 * hi;
                u32x2 w;
                if constexpr (std::is_same<T16, f16_t>::value) {
                    w[0] = pack2h(acc[i][rq * 4 + 0], acc[i][rq * 4 + 1]);
                    w[1] = pack2h(acc[i][rq * 4 + 2], acc[i][rq * 4 + 3]);
                } else {
                    w[0] = pack2bf(acc[i][rq * 4 + 0], acc[i][rq * 4 + 1]);
                    w[1] = pack2bf(acc[i][rq * 4 + 2], acc[i][rq * 4 + 3]);
                }
                *(u32x2*)(out + n) = w;
            }
        }
    }
}

// ---- generic form (fp32 model dtype, force_simple): one thread per output, fp32 accumulation in K order ----------------------------------
template <typename T>
__global__ void lora_down_simple_k(const LoraDownArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.M * a.N) return;
    const int m = (int)(i / a.N), n = (int)(i - (int64_t)m * a.N);
    const T* x = (const T*)a.x + (int64_t)m * a.ldx;
    const T* w = (const T*)a.A + (int64_t)n * a.lda;
    float acc = 0.f;
    for (int k = 0; k < a.K; ++k) acc = fmaf(ET<T>::ld(x + k), ET<T>::ld(w + k), acc);
    ET<T>::st((T*)a.out + (int64_t)m * a.ldo + n, acc);
}

int launch_lora_down(const LoraDownArgs& a, int dtype, bool mfma, hipStream_t st) {
    S2V_REQUIRE(a.x && a.A && a.out && a.M > 0 && a.N > 0 && a.K > 0, "lora_down: bad argument");
    if (mfma && dtype != S2V_F32) {
        S2V_REQUIRE(a.N % 64 == 0 && a.N <= LD_NMAX && a.K % LD_BK == 0 && a.ldx % 8 == 0 && a.lda % 8 == 0 && a.ldo % 4 == 0,
                    "lora_down: the MFMA kernel needs N % 64 == 0, N <= 384, K % 64 == 0 and 16-byte aligned rows");
        const int grid = (a.M + LD_BM - 1) / LD_BM, lds = LD_LDS(a.N);
#define LORA_DOWN_LAUNCH(T16, NTW)                                                                  \
    do {                                                                                            \
        S2V_TRY(ensure_lds_attr((const void*)lora_down_mfma_k<T16, NTW>, LD_LDS(64 * NTW)));        \
        hipLaunchKernelGGL((lora_down_mfma_k<T16, NTW>), dim3(grid), dim3(LD_THREADS), lds, st, a); \
    } while (0)
        if (dtype == S2V_F16) LORA_DOWN_LAUNCH(f16_t, 6);
        else LORA_DOWN_LAUNCH(bf16_t, 6);
#undef LORA_DOWN_LAUNCH
    } else {
        const int64_t n = (int64_t)a.M * a.N;
        S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(lora_down_simple_k<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a));
    }
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- down-projection from an MX e4m3 image (the fp8 engine: attention output -> out-projection, GELU(FF1) -> FF2) ------------------------------
// The same tiling and the same v_mfma_f32_32x32x16_bf16 as lora_down_mfma_k, but x arrives as one byte per element plus one E8M0 scale per
// (row, 32 elements) in the K-tile-major layout of GemmArgs::mx_a_s -- dword (kt, mx_perm_row(m)), byte b = block 4 kt + b -- so the kernel reads
// half the bytes of the bf16 one.  A thread owns 16 consecutive elements of a row per K chunk (half an MX block: one scale byte), converts them
// with v_cvt_pk_f32_fp8, multiplies by 2^(scale - 127) and packs bf16 pairs: e4m3 has four significant bits, so every product is a bf16 value and
// the operand the MFMA sees is the image dequantised exactly.  N <= 128 (one adapter's padded rank): two 32-column tiles per wave at most.
template <int NTW>
__global__ __launch_bounds__(LD_THREADS, 2) void lora_down_mx_k(const LoraDownArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* tX = smem;                       // [128][64] of x, bf16
    char* tA = smem + LD_BM * LD_BK * 2;   // [N][64] of the A stack
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 3, wn = wave >> 2;
    const int fr = lane & 31, hi = lane >> 5;
    const int m0 = blockIdx.x * LD_BM;
    const int ntw = a.N >> 6;
    const unsigned char* X = (const unsigned char*)a.x;
    const char* A = (const char*)a.A;
    // x: 128 rows x 4 pieces of 16 bytes per K chunk, one per thread
    const int xrow = tid >> 2, xq = tid & 3;
    const bool xok = m0 + xrow < a.M;
    const unsigned char* xp = X + (int64_t)(m0 + xrow) * a.ldx + xq * 16;
    const unsigned char* sp = a.mx_s + mx_perm_row(m0 + xrow) * 4;

    u32x4 rx, ra[NTW];
    unsigned rs = 0;
    auto fetch = [&](int k0) {
        rx = u32x4{0u, 0u, 0u, 0u};
        rs = 127;
        if (xok) {
            rx = *(const u32x4*)(xp + k0);
            rs = sp[(int64_t)(k0 >> 7) * a.mx_rows * 4 + (((k0 & 127) + xq * 16) >> 5)];
        }
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int p = i * LD_THREADS + tid, row = p >> 3, ch = p & 7;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (row < a.N) v = *(const u32x4*)(A + 2 * ((int64_t)row * a.lda + k0 + ch * 8));
            ra[i] = v;
        }
    };
    auto commit = [&]() {
        const float sc = __uint_as_float(rs ? rs << 23 : 0x00400000u);   // 2^(rs - 127)
        u32x4 o[2];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)rx[w], false), up = __builtin_amdgcn_cvt_pk_f32_fp8((int)rx[w], true);
            o[w >> 1][(w & 1) * 2] = pack2bf(lo[0] * sc, lo[1] * sc);
            o[w >> 1][(w & 1) * 2 + 1] = pack2bf(up[0] * sc, up[1] * sc);
        }
        *(u32x4*)(tX + lora_swz(xrow, xq * 2)) = o[0];
        *(u32x4*)(tX + lora_swz(xrow, xq * 2 + 1)) = o[1];
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int p = i * LD_THREADS + tid;
            if ((p >> 3) < a.N) *(u32x4*)(tA + lora_swz(p >> 3, p & 7)) = ra[i];
        }
    };

    f32x16 acc[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    const int nt = a.K / LD_BK;
    fetch(0);
    for (int t = 0; t < nt; ++t) {
        commit();
        __syncthreads();
        if (t + 1 < nt) fetch((t + 1) * LD_BK);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bf16x8 xf = *(const bf16x8*)(tX + lora_swz(wm * 32 + fr, kk * 2 + hi));
#pragma unroll
            for (int i = 0; i < NTW; ++i) {
                if (i < ntw) {
                    const bf16x8 af = *(const bf16x8*)(tA + lora_swz((wn * ntw + i) * 32 + fr, kk * 2 + hi));
                    acc[i] = lora_mfma<bf16_t>(af, xf, acc[i]);   // D[i = column of T][j = row of x]
                }
            }
        }
        __syncthreads();
    }
    const int m = m0 + wm * 32 + fr;
    if (m >= a.M) return;
    bf16_t* out = (bf16_t*)a.out + (int64_t)m * a.ldo;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        if (i < ntw) {
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int n = (wn * ntw + i) * 32 + 8 * rq + 4 * hi;
                u32x2 w;
                w[0] = pack2bf(acc[i][rq * 4 + 0], acc[i][rq * 4 + 1]);
                w[1] = pack2bf(acc[i][rq * 4 + 2], acc[i][rq * 4 + 3]);
                *(u32x2*)(out + n) = w;
            }
        }
    }
}

int launch_lora_down_mx(const LoraDownArgs& a, hipStream_t st) {
    S2V_REQUIRE(a.x && a.A && a.out && a.mx_s && a.M > 0 && a.N > 0 && a.K > 0, "lora_down_mx: bad argument");
    S2V_REQUIRE(a.N % 64 == 0 && a.N <= 128 && a.K % 128 == 0 && a.ldx % 16 == 0 && a.lda % 8 == 0 && a.ldo % 4 == 0,
                "lora_down_mx: N must be 64 or 128, K a multiple of 128, rows 16-byte aligned");
    S2V_REQUIRE(a.mx_rows % 128 == 0 && a.mx_rows >= (a.M + 127) / 128 * 128, "lora_down_mx: the block scales must cover M padded to 128 rows");
    const int grid = (a.M + LD_BM - 1) / LD_BM, lds = LD_LDS(a.N);
    S2V_TRY(ensure_lds_attr((const void*)lora_down_mx_k<2>, LD_LDS(128)));
    hipLaunchKernelGGL((lora_down_mx_k<2>), dim3(grid), dim3(LD_THREADS), lds, st, a);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- attach time --------------------------------------------------------------------------------------------------------------------
// dst[j][k] = rnd(A[j][k]) for j < rank, 0 for rank <= j < rows: the adapter's A [rank][K] (fp32) into its rows of the layer's A stack
template <typename T>
__global__ void lora_pack_a_k(const float* __restrict__ A, int rank, int rows, int K, T* __restrict__ dst, int64_t ldd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * K) return;
    const int j = (int)(i / K), k = (int)(i - (int64_t)j * K);
    ET<T>::st(dst + (int64_t)j * ldd + k, j < rank ? A[(int64_t)j * K + k] : 0.f);
}
// dst[n][j] = rnd(scale * B[n][j]) for j < rank, 0 for rank <= j < cols: s * B [N][rank] (fp32, the product taken in fp32) into the
// weight's tail columns
template <typename T>
__global__ void lora_pack_b_k(const float* __restrict__ B, int rank, int cols, int N, float scale, T* __restrict__ dst, int64_t ldd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * cols) return;
    const int n = (int)(i / cols), j = (int)(i - (int64_t)n * cols);
    ET<T>::st(dst + (int64_t)n * ldd + j, j < rank ? scale * B[(int64_t)n * rank + j] : 0.f);
}

int launch_lora_pack_a(const float* A, int rank, int rows, int K, void* dst, int64_t ldd, int dtype, hipStream_t st) {
    const int64_t n = (int64_t)rows * K;
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(lora_pack_a_k<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, rank, rows, K, (T*)dst, ldd));
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}
int launch_lora_pack_b(const float* B, int rank, int cols, int N, float scale, void* dst, int64_t ldd, int dtype, hipStream_t st) {
    const int64_t n = (int64_t)N * cols;
    S2V_DT_DISPATCH(dtype, hipLaunchKernelGGL(lora_pack_b_k<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, B, rank, cols, N, scale, (T*)dst, ldd));
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}
