// Byte-moving kernels of Ulysses sequence parallelism: the packs and unpacks around the two
// all-to-alls of every block and the compaction of the gathered noise prediction.  No arithmetic: every kernel copies 16-byte pieces of
// rows (or, for the MX block scales of the fp8 engine's O exchange, dwords), so a sharded step moves exactly the bits the single engine computes.
#define S2V_HOST
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;  // 16-byte pieces per lane: 16 KiB in flight per workgroup, loads issued before the stores

// piece u of (segment k, row i): dst[dst_off(k) + dmap(i) * dst_ld + 16 u] = src[src_off(k) + smap(i) * src_ld + 16 u]
__global__ __launch_bounds__(kThreads) void shard_copy_k(const ShardCopyArgs a) {
    const int k = blockIdx.y;
    const int ko = k / a.nseg_inner, ki = k - ko * a.nseg_inner;
    const char* src = a.src + ko * a.src_seg_outer + ki * a.src_seg_inner;
    char* dst = a.dst + ko * a.dst_seg_outer + ki * a.dst_seg_inner;
    const int64_t total = (int64_t)a.rows * a.width16;
    const int64_t base = (int64_t)blockIdx.x * (kThreads * kUnroll) + threadIdx.x;
    u32x4 v[kUnroll];
    int64_t doff[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
        const int64_t e = base + (int64_t)j * kThreads;
        doff[j] = -1;
        if (e < total) {
            const int i = (int)(e / a.width16), u = (int)(e - (int64_t)i * a.width16);
            const int si = a.src_map ? a.src_map[i] : i;
            const int di = a.dst_map ? a.dst_map[i] : i;
            if (si >= 0 && di >= 0) {
                v[j] = *(const u32x4*)(src + (int64_t)si * a.src_ld + 16 * (int64_t)u);
                doff[j] = (int64_t)di * a.dst_ld + 16 * (int64_t)u;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j)
        if (doff[j] >= 0) *(u32x4*)(dst + doff[j]) = v[j];
}

// dword (segment k, row i, K-tile kt) of the MX block scales, kt fastest: the compact side of a pack / unpack is then read or written in order
__global__ __launch_bounds__(kThreads) void shard_scales_k(const ShardScaleArgs a) {
    const int k = blockIdx.y;
    const unsigned* src = a.src + k * a.src_seg;
    unsigned* dst = a.dst + k * a.dst_seg;
    const int64_t total = (int64_t)a.rows * a.nkt;
    const int64_t base = (int64_t)blockIdx.x * (kThreads * kUnroll) + threadIdx.x;
    unsigned v[kUnroll];
    int64_t doff[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
        const int64_t e = base + (int64_t)j * kThreads;
        doff[j] = -1;
        if (e < total) {
            const int i = (int)(e / a.nkt), kt = (int)(e - (int64_t)i * a.nkt);
            const int si = a.src_map ? a.src_map[i] : i;
            const int di = a.dst_map ? a.dst_map[i] : i;
            if (si >= 0 && di >= 0) {
                v[j] = src[kt * a.src_kt + (a.src_perm ? mx_perm_row(si) : (int64_t)si) * a.src_row];
                doff[j] = kt * a.dst_kt + (a.dst_perm ? mx_perm_row(di) : (int64_t)di) * a.dst_row;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j)
        if (doff[j] >= 0) dst[doff[j]] = v[j];
}

}  // namespace

int launch_shard_copy(const ShardCopyArgs& a, hipStream_t st) {
    S2V_REQUIRE(a.rows >= 0 && a.width16 >= 0 && a.nseg >= 1 && a.nseg_inner >= 1 && a.nseg % a.nseg_inner == 0, "launch_shard_copy: bad shape");
    S2V_REQUIRE(((uintptr_t)a.src | (uintptr_t)a.dst | (uintptr_t)a.src_ld | (uintptr_t)a.dst_ld | (uintptr_t)a.src_seg_outer |
                 (uintptr_t)a.src_seg_inner | (uintptr_t)a.dst_seg_outer | (uintptr_t)a.dst_seg_inner) % 16 == 0,
                "launch_shard_copy: addresses and strides must be 16-byte aligned");
    const int64_t total = (int64_t)a.rows * a.width16;
    if (total == 0) return 0;
    const int64_t per = (int64_t)kThreads * kUnroll;
    S2V_REQUIRE((total + per - 1) / per < (1ll << 31) && a.nseg < 65536, "launch_shard_copy: grid too large");
    dim3 grid((unsigned)((total + per - 1) / per), (unsigned)a.nseg);
    hipLaunchKernelGGL(shard_copy_k, grid, dim3(kThreads), 0, st, a);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_shard_scales(const ShardScaleArgs& a, hipStream_t st) {
    S2V_REQUIRE(a.src && a.dst && a.rows >= 0 && a.nkt >= 1 && a.nseg >= 1, "launch_shard_scales: bad shape");
    const int64_t total = (int64_t)a.rows * a.nkt;
    if (total == 0) return 0;
    const int64_t per = (int64_t)kThreads * kUnroll;
    S2V_REQUIRE((total + per - 1) / per < (1ll << 31) && a.nseg < 65536, "launch_shard_scales: grid too large");
    dim3 grid((unsigned)((total + per - 1) / per), (unsigned)a.nseg);
    hipLaunchKernelGGL(shard_scales_k, grid, dim3(kThreads), 0, st, a);
    S2V_CHECK_HIP(hipGetLastError());
    return 0;
}
