// C ABI of the CogVideoX 3-D causal VAE decode (include/s2v_hip.h, s2v_vae_*): weight ingest / re-packing, buffer plan,
// and the launch sequence of AutoencoderKLCogVideoX.decode (autoencoder_kl_cogvideox.py:1231-1282, 1374-1455).
#define S2V_HOST
#include "common.h"
#include "kernels.h"
#include "vae_kernels.h"
#include "../../include/s2v_hip.h"

#include <cmath>
#include <cstdio>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>
#include <algorithm>
#include <cstdlib>

static inline int64_t rup64(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

struct ConvL {
    int cin = 0, cout = 0, kt = 3;      // kt: 3 causal 3x3x3, 1 per-frame 3x3, 0 pointwise 1x1x1
    char* w = nullptr; char* b = nullptr;  // repacked [cout_pad][taps*cin], [cout]
    char* pad = nullptr; int64_t pad_bytes = 0;  // own zero-bordered operand buffer (conv cache in frames 0,1 when kt==3)
    int level = 0;
};
struct SNormL {
    int C = 0;
    char* gn_w = nullptr; char* gn_b = nullptr;
    float *wy = nullptr, *by = nullptr, *wb = nullptr, *bb = nullptr;
};
struct ResnetL { SNormL n1, n2; ConvL c1, c2, sc; bool has_sc = false; int cin = 0, cout = 0; };
struct StageL { std::vector<ResnetL> res; bool has_up = false; ConvL up; int compress_time = 0; };

struct VSlot { int kind; void* dst; int64_t d0, d1, taps; bool loaded; };  // kind 0 vector(model dtype) 1 conv repack 2 snorm W^T fp32 3 fp32 vector

struct s2v_vae {
    s2v_vae_config cfg;
    int dtype = 0, esz = 0, G = 0, Cz = 0;
    bool mfma = false, h16 = false, finalized = false;
    bool encoder = false;  // plan built by s2v_vae_enc_create (reference-image encode) instead of the decoder
    ConvL conv_in, conv_out;
    SNormL norm_out;
    std::vector<StageL> stages;
    std::unordered_map<std::string, VSlot> slots;
    std::vector<void*> allocs;
    // geometry-dependent
    int th = 0, tw = 0;        // allocated tile capacity (latent)
    int cur_h = 0, cur_w = 0;  // layout the zero borders are currently valid for
    int fmax[8] = {0};
    char* dense[3] = {nullptr, nullptr, nullptr};
    int64_t dense_bytes = 0;
    char* zq = nullptr; char* yt = nullptr; char* bt = nullptr;
    double* sums = nullptr; double* gn_part = nullptr;
    std::vector<void*> geo_allocs;
    std::vector<char*> tiles; std::vector<int> tile_h, tile_w;
    int tiles_F = 0;
    // Tiled decode: the tiles are independent until the blends, and at the latent levels a tile's GEMMs are a handful of workgroups
    // (30 x 45 x 2 rows = 11 row tiles on 256 CUs).  NWS workspace sets -- every geometry-dependent buffer above, once per set -- let
    // tiles k, k + 1, ... run concurrently on side streams; the members above always alias the ACTIVE set (ws_activate), so the launch
    // sequences are written once.
    struct WS {
        std::vector<char*> pads;  // in for_each_conv order
        char* dense[3] = {nullptr, nullptr, nullptr};
        char *zq = nullptr, *yt = nullptr, *bt = nullptr;
        double *sums = nullptr, *gn_part = nullptr;
        int cur_h = 0, cur_w = 0;
    };
    std::vector<WS> ws;
    int ws_active = 0, ws_req = 0;  // ws_req: sets asked for when ws was built (memory may have granted fewer)
    int fault_geo_at = 0, fault_geo_seen = 0;  // S2V_VAE_FAULT_GEO_ALLOC (dmalloc)
    int64_t set_bytes = 0;          // bytes of one set at the current capacity
    std::vector<hipStream_t> side;  // one per workspace set beyond the first
    std::vector<hipEvent_t> ev_side;
    hipEvent_t ev_fork = nullptr;
    // every weight lives in ONE arena (replicas receive it by one broadcast, s2v_vae_weight_arena): the plan is built twice,
    // a sizing pass (arena == nullptr) that only adds up the carve-outs, then the real pass that bumps through the arena
    char* arena = nullptr;
    int64_t arena_bytes = 0, arena_off = 0;
    bool sizing = false;
};

static int vfail(const char* m) { return s2v_fail(__FILE__, __LINE__, m, -1); }

template <typename T>
static int wmalloc(s2v_vae* v, T** p, int64_t bytes) {  // weight carve-out (256-byte aligned, zero-initialised with the arena)
    const int64_t sz = rup64(bytes > 0 ? bytes : 16, 256);
    *p = v->sizing ? nullptr : (T*)(v->arena + v->arena_off);
    v->arena_off += sz;
    return 0;
}
template <typename T>
static int dmalloc(s2v_vae* v, T** p, int64_t bytes, bool geo = false) {
    void* q = nullptr;
    // fault injection for tests/test_gpu_vae.py: S2V_VAE_FAULT_GEO_ALLOC=n makes the n-th workspace ("geo") allocation of a
    // prepare_tile_capacity call fail as an out-of-memory hipMalloc would; read per call (a getenv on an allocation path, never on a launch path)
    if (geo && v->fault_geo_at > 0 && ++v->fault_geo_seen == v->fault_geo_at)
        return s2v_fail(__FILE__, __LINE__, "dmalloc: injected allocation failure (S2V_VAE_FAULT_GEO_ALLOC)", -2);
    S2V_CHECK_HIP(hipMalloc(&q, (size_t)(bytes > 0 ? bytes : 16)));
    S2V_CHECK_HIP(hipMemset(q, 0, (size_t)(bytes > 0 ? bytes : 16)));
    (geo ? v->geo_allocs : v->allocs).push_back(q);
    *p = (T*)q;
    return 0;
}

static int make_conv(s2v_vae* v, ConvL& c, const std::string& name, int cin, int cout, int kt, int level) {
    c.cin = cin; c.cout = cout; c.kt = kt; c.level = level;
    const int taps = kt == 3 ? 27 : (kt == 1 ? 9 : 1);
    S2V_TRY(wmalloc(v, &c.w, rup64(cout, 256) * taps * cin * v->esz));
    S2V_TRY(wmalloc(v, &c.b, (int64_t)cout * v->esz));
    v->slots[name + ".weight"] = VSlot{1, c.w, cout, cin, taps, false};
    v->slots[name + ".bias"] = VSlot{0, c.b, cout, 1, 1, false};
    return 0;
}
// decoder: CogVideoXSpatialNorm3D (GroupNorm under ".norm_layer." and the conv_y / conv_b tables over zq); encoder: nn.GroupNorm alone
static int make_norm(s2v_vae* v, SNormL& n, const std::string& name, int C) {
    n.C = C;
    const bool spatial = !v->encoder;
    const int Cz = v->Cz;
    S2V_TRY(wmalloc(v, &n.gn_w, (int64_t)C * v->esz));
    S2V_TRY(wmalloc(v, &n.gn_b, (int64_t)C * v->esz));
    const std::string gn = name + (spatial ? ".norm_layer" : "");
    v->slots[gn + ".weight"] = VSlot{0, n.gn_w, C, 1, 1, false};
    v->slots[gn + ".bias"] = VSlot{0, n.gn_b, C, 1, 1, false};
    if (!spatial) return 0;
    S2V_TRY(wmalloc(v, &n.wy, (int64_t)C * Cz * 4));
    S2V_TRY(wmalloc(v, &n.wb, (int64_t)C * Cz * 4));
    S2V_TRY(wmalloc(v, &n.by, (int64_t)C * 4));
    S2V_TRY(wmalloc(v, &n.bb, (int64_t)C * 4));
    v->slots[name + ".conv_y.conv.weight"] = VSlot{2, n.wy, C, Cz, 1, false};
    v->slots[name + ".conv_b.conv.weight"] = VSlot{2, n.wb, C, Cz, 1, false};
    v->slots[name + ".conv_y.conv.bias"] = VSlot{3, n.by, C, 1, 1, false};
    v->slots[name + ".conv_b.conv.bias"] = VSlot{3, n.bb, C, 1, 1, false};
    return 0;
}
static int make_resnet(s2v_vae* v, ResnetL& r, const std::string& name, int cin, int cout, int level) {
    r.cin = cin; r.cout = cout; r.has_sc = cin != cout;
    S2V_TRY(make_norm(v, r.n1, name + ".norm1", cin));
    S2V_TRY(make_conv(v, r.c1, name + ".conv1.conv", cin, cout, 3, level));
    S2V_TRY(make_norm(v, r.n2, name + ".norm2", cout));
    S2V_TRY(make_conv(v, r.c2, name + ".conv2.conv", cout, cout, 3, level));
    if (r.has_sc) S2V_TRY(make_conv(v, r.sc, name + ".conv_shortcut", cin, cout, 0, level));
    return 0;
}

extern "C" void s2v_vae_destroy(s2v_vae* v) {
    if (!v) return;
    for (auto st_ : v->side) (void)hipStreamDestroy(st_);
    for (auto e : v->ev_side) (void)hipEventDestroy(e);
    if (v->ev_fork) (void)hipEventDestroy(v->ev_fork);
    (void)hipDeviceSynchronize();
    for (void* p : v->allocs) (void)hipFree(p);
    for (void* p : v->geo_allocs) (void)hipFree(p);
    for (char* p : v->tiles) (void)hipFree(p);
    if (v->arena) (void)hipFree(v->arena);
    delete v;
}

static int build_two_pass(s2v_vae* v, int (*build)(s2v_vae*)) {
    v->sizing = true;
    v->arena_off = 0;
    S2V_TRY(build(v));
    v->arena_bytes = v->arena_off;
    S2V_CHECK_HIP(hipMalloc((void**)&v->arena, (size_t)v->arena_bytes));
    S2V_CHECK_HIP(hipMemset(v->arena, 0, (size_t)v->arena_bytes));
    v->sizing = false;
    v->arena_off = 0;
    v->stages.clear();
    v->slots.clear();
    S2V_TRY(build(v));
    return dmalloc(v, &v->sums, sizeof(double) * 2 * v->G);
}

static int build_decoder(s2v_vae* v) {
    const s2v_vae_config* cfg = &v->cfg;
    const int nb = cfg->num_blocks;
    // decoder channel plan = reversed block_out_channels (autoencoder_kl_cogvideox.py:871-915)
    std::vector<int> rc(nb);
    for (int i = 0; i < nb; ++i) rc[i] = cfg->block_out_channels[nb - 1 - i];
    const int tlevel = (int)std::lround(std::log2((double)cfg->temporal_compression_ratio));
    int r = make_conv(v, v->conv_in, "decoder.conv_in.conv", v->Cz, rc[0], 3, 0);
    v->stages.resize(nb + 1);
    char nm[128];
    if (!r) {
        v->stages[0].res.resize(2);
        for (int i = 0; i < 2 && !r; ++i) {
            snprintf(nm, sizeof(nm), "decoder.mid_block.resnets.%d", i);
            r = make_resnet(v, v->stages[0].res[i], nm, rc[0], rc[0], 0);
        }
    }
    int prev = rc[0], level = 0;
    for (int b = 0; b < nb && !r; ++b) {
        StageL& s = v->stages[b + 1];
        s.res.resize(cfg->layers_per_block + 1);
        for (int i = 0; i <= cfg->layers_per_block && !r; ++i) {
            snprintf(nm, sizeof(nm), "decoder.up_blocks.%d.resnets.%d", b, i);
            r = make_resnet(v, s.res[i], nm, i == 0 ? prev : rc[b], rc[b], level);
        }
        prev = rc[b];
        s.has_up = b != nb - 1;
        s.compress_time = b < tlevel;
        if (s.has_up && !r) {
            snprintf(nm, sizeof(nm), "decoder.up_blocks.%d.upsamplers.0.conv", b);
            r = make_conv(v, s.up, nm, rc[b], rc[b], 1, level + 1);
            level++;
        }
    }
    if (!r) r = make_norm(v, v->norm_out, "decoder.norm_out", rc[nb - 1]);
    if (!r) r = make_conv(v, v->conv_out, "decoder.conv_out.conv", rc[nb - 1], cfg->out_channels, 3, level);
    return r;
}

// The encoder's plan (CogVideoXEncoder3D, autoencoder_kl_cogvideox.py:755-814: conv_in, DownBlock3D x4 of plain-GroupNorm resnets +
// CogVideoXDownsample3D, MidBlock3D, norm_out, conv_out): stages[0 .. nb-1] = down blocks (StageL::up is the stride-2 downsampler conv),
// stages[nb] = mid block; ConvL::level l works at (tile height >> l) x (tile width >> l).
static int build_encoder(s2v_vae* v) {
    const s2v_vae_config* cfg = &v->cfg;
    const int nb = cfg->num_blocks;
    const int tlevel = (int)std::lround(std::log2((double)cfg->temporal_compression_ratio));
    int r = make_conv(v, v->conv_in, "encoder.conv_in.conv", cfg->out_channels, cfg->block_out_channels[0], 3, 0);
    v->stages.resize(nb + 1);
    char nm[128];
    int prev = cfg->block_out_channels[0], level = 0;
    for (int b = 0; b < nb && !r; ++b) {
        StageL& s = v->stages[b];
        const int co = cfg->block_out_channels[b];
        s.res.resize(cfg->layers_per_block);
        for (int i = 0; i < cfg->layers_per_block && !r; ++i) {
            snprintf(nm, sizeof(nm), "encoder.down_blocks.%d.resnets.%d", b, i);
            r = make_resnet(v, s.res[i], nm, i == 0 ? prev : co, co, level);
        }
        prev = co;
        s.has_up = b != nb - 1;  // here: has a downsampler
        s.compress_time = b < tlevel;
        if (s.has_up && !r) {
            snprintf(nm, sizeof(nm), "encoder.down_blocks.%d.downsamplers.0.conv", b);
            r = make_conv(v, s.up, nm, co, co, 1, level);  // operand at the level it reads; output one level down
            level++;
        }
    }
    if (!r) {
        v->stages[nb].res.resize(2);
        for (int i = 0; i < 2 && !r; ++i) {
            snprintf(nm, sizeof(nm), "encoder.mid_block.resnets.%d", i);
            r = make_resnet(v, v->stages[nb].res[i], nm, prev, prev, level);
        }
    }
    if (!r) r = make_norm(v, v->norm_out, "encoder.norm_out", prev);
    if (!r) r = make_conv(v, v->conv_out, "encoder.conv_out.conv", prev, 2 * v->Cz, 3, level);
    return r;
}

static int vae_create(const char* fn, const s2v_vae_config* cfg, s2v_vae** out, bool encoder) {
    static thread_local std::string m;
    auto bad = [&](const char* why) { m = std::string(fn) + ": " + why; return m.c_str(); };
    S2V_REQUIRE(cfg && out, bad("null argument"));
    S2V_REQUIRE(cfg->dtype == S2V_DTYPE_F32 || cfg->dtype == S2V_DTYPE_BF16 || cfg->dtype == S2V_DTYPE_F16, bad("unsupported dtype"));
    S2V_REQUIRE(cfg->num_blocks >= 1 && cfg->num_blocks <= 6, bad("1..6 blocks"));
    s2v_vae* v = new s2v_vae();
    v->cfg = *cfg;
    v->dtype = cfg->dtype;
    v->esz = cfg->dtype == S2V_DTYPE_F32 ? 4 : 2;
    v->G = cfg->norm_num_groups;
    v->Cz = cfg->latent_channels;
    v->mfma = cfg->dtype == S2V_DTYPE_BF16 && !cfg->force_simple;
    v->h16 = cfg->dtype == S2V_DTYPE_F16 && !cfg->force_simple;  // fp16: convolutions / shortcuts with cin % 64 == 0 on v_mfma_f32_32x32x16_f16 (gemm_f16)
    v->encoder = encoder;
    const int r = build_two_pass(v, encoder ? build_encoder : build_decoder);
    if (r) { s2v_vae_destroy(v); return r; }
    *out = v;
    return 0;
}
extern "C" int s2v_vae_create(const s2v_vae_config* cfg, s2v_vae** out) { return vae_create("s2v_vae_create", cfg, out, false); }
// The reference-image / video ENCODE handle (src/video_generate.py:26-38): weights load through s2v_vae_load_weight
// under the reference's "encoder.*" names and it is destroyed by s2v_vae_destroy.
extern "C" int s2v_vae_enc_create(const s2v_vae_config* cfg, s2v_vae** out) { return vae_create("s2v_vae_enc_create", cfg, out, true); }

/* One device range holding every weight of the handle (decoder or encoder), for the replica broadcast; a replica that
 * received it calls s2v_vae_mark_weights_loaded instead of s2v_vae_load_weight + s2v_vae_finalize. */
extern "C" int s2v_vae_weight_arena(s2v_vae* v, void** dev_ptr, int64_t* bytes) {
    S2V_REQUIRE(v && dev_ptr && bytes, "s2v_vae_weight_arena: null argument");
    *dev_ptr = v->arena;
    *bytes = v->arena_bytes;
    return 0;
}
extern "C" int s2v_vae_mark_weights_loaded(s2v_vae* v) {
    S2V_REQUIRE(v, "s2v_vae_mark_weights_loaded: null argument");
    for (auto& kv : v->slots) kv.second.loaded = true;
    v->finalized = true;
    return 0;
}

template <typename TS>
__global__ void to_f32_transposed_k(const TS* src, int rows, int cols, float* dst) {  // dst[c][r] = src[r][c]
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int r = i / cols, c = i - r * cols;
    dst[(size_t)c * rows + r] = ET<TS>::ld(src + i);
}

extern "C" int s2v_vae_load_weight(s2v_vae* v, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim,
                                   int32_t src_dtype, s2v_stream stream) {
    S2V_REQUIRE(v && name && dev_ptr && shape, "s2v_vae_load_weight: null argument");
    S2V_REQUIRE(src_dtype == S2V_DTYPE_F32 || src_dtype == S2V_DTYPE_BF16 || src_dtype == S2V_DTYPE_F16, "s2v_vae_load_weight: unsupported dtype");
    auto it = v->slots.find(name);
    if (it == v->slots.end()) {
        std::string m = std::string("s2v_vae_load_weight: unknown tensor name: ") + name;
        return s2v_fail(__FILE__, __LINE__, m.c_str(), -3);
    }
    VSlot& s = it->second;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    if (n != s.d0 * s.d1 * s.taps || shape[0] != s.d0) {
        std::string m = std::string("s2v_vae_load_weight: shape mismatch for ") + name;
        return s2v_fail(__FILE__, __LINE__, m.c_str(), -3);
    }
    hipStream_t st = (hipStream_t)stream;
    if (s.kind == 0) S2V_TRY(launch_convert(dev_ptr, src_dtype, s.dst, v->dtype, n, st));
    else if (s.kind == 3) S2V_TRY(launch_convert(dev_ptr, src_dtype, s.dst, S2V_F32, n, st));
    else if (s.kind == 1) S2V_TRY(launch_conv_w_repack(dev_ptr, src_dtype, (int)s.d0, (int)s.d1, (int)s.taps, s.dst, v->dtype, st));
    else {
        // the reference holds conv_y / conv_b in the model dtype: round first (through a scratch of that dtype unless the source already is
        // of it or the model is fp32), then widen + transpose
        const int tot = (int)n;
        const void* srcp = dev_ptr;
        int sdt = src_dtype;
        void* tmp = nullptr;
        if (v->dtype != S2V_DTYPE_F32 && src_dtype != v->dtype) {
            S2V_CHECK_HIP(hipMalloc(&tmp, 2 * (size_t)n));
            const int r = launch_convert(dev_ptr, src_dtype, tmp, v->dtype, n, st);
            if (r) { (void)hipFree(tmp); return r; }
            srcp = tmp; sdt = v->dtype;
        }
        S2V_DT_DISPATCH(sdt, hipLaunchKernelGGL(to_f32_transposed_k<T>, dim3((tot + 255) / 256), dim3(256), 0, st, (const T*)srcp, (int)s.d0, (int)s.d1, (float*)s.dst))
        if (tmp) { (void)hipStreamSynchronize(st); (void)hipFree(tmp); }
        S2V_CHECK_HIP(hipGetLastError());
    }
    if (s.kind == 3 && v->dtype != S2V_DTYPE_F32 && src_dtype != v->dtype) {
        // bias held in the model dtype by the reference: round through it
        void* tmp = nullptr;
        S2V_CHECK_HIP(hipMalloc(&tmp, 2 * (size_t)n));
        int r = launch_convert(dev_ptr, src_dtype, tmp, v->dtype, n, st);
        if (!r) r = launch_convert(tmp, v->dtype, s.dst, S2V_F32, n, st);
        (void)hipStreamSynchronize(st);
        (void)hipFree(tmp);
        if (r) return r;
    }
    s.loaded = true;
    return 0;
}

extern "C" int s2v_vae_finalize(s2v_vae* v) {
    S2V_REQUIRE(v, "null vae");
    for (auto& kv : v->slots)
        if (!kv.second.loaded) {
            std::string m = std::string("s2v_vae_finalize: tensor was never loaded: ") + kv.first;
            return s2v_fail(__FILE__, __LINE__, m.c_str(), -3);
        }
    v->finalized = true;
    return 0;
}

// ---- geometry ------------------------------------------------------------------------------------------------
static int up_frames(int F, int ct) { return (!ct || F == 1) ? F : ((F & 1) ? 1 + 2 * (F - 1) : 2 * F); }

static void for_each_conv(s2v_vae* v, const std::function<void(ConvL&)>& fn) {
    fn(v->conv_in);
    for (auto& s : v->stages) {
        for (auto& r : s.res) { fn(r.c1); fn(r.c2); }
        if (s.has_up) fn(s.up);
    }
    fn(v->conv_out);
}

// the live members <-> workspace set k
static void ws_save(s2v_vae* v, int k) {
    s2v_vae::WS& w = v->ws[k];
    w.pads.clear();
    for_each_conv(v, [&](ConvL& c) { w.pads.push_back(c.pad); });
    for (int i = 0; i < 3; ++i) w.dense[i] = v->dense[i];
    w.zq = v->zq; w.yt = v->yt; w.bt = v->bt; w.sums = v->sums; w.gn_part = v->gn_part;
    w.cur_h = v->cur_h; w.cur_w = v->cur_w;
}
// set k -> the live members, unconditionally
static void ws_load(s2v_vae* v, int k) {
    const s2v_vae::WS& w = v->ws[k];
    size_t i = 0;
    for_each_conv(v, [&](ConvL& c) { c.pad = w.pads[i++]; });
    for (int j = 0; j < 3; ++j) v->dense[j] = w.dense[j];
    v->zq = w.zq; v->yt = w.yt; v->bt = w.bt; v->sums = w.sums; v->gn_part = w.gn_part;
    v->cur_h = w.cur_h; v->cur_w = w.cur_w;
    v->ws_active = k;
}
static void ws_activate(s2v_vae* v, int k) {
    if (v->ws.empty() || k == v->ws_active) return;
    v->ws[v->ws_active].cur_h = v->cur_h; v->ws[v->ws_active].cur_w = v->cur_w;
    ws_load(v, k);
}

// Conv c's operand at window th x tw (latents for the decoder, pixels for the encoder): the window at c's level (the decoder works up,
// the encoder down) and fl[level] frames (the largest frame batch at that level), plus the two cache frames of a causal convolution
struct Operand {
    int64_t H, W, F, frames;  // F: frames with the cache
    int64_t padded_bytes(const s2v_vae* v, const ConvL& c) const { return F * (H + 2) * (W + 2) * c.cin * v->esz; }
    int64_t dense_bytes(const s2v_vae* v, const ConvL& c) const { return frames * H * W * std::max(c.cin, c.cout) * v->esz; }
};
static Operand operand_extent(const s2v_vae* v, const ConvL& c, int th, int tw, const int* fl) {
    const int64_t H = v->encoder ? th >> c.level : (int64_t)th << c.level, W = v->encoder ? tw >> c.level : (int64_t)tw << c.level;
    return {H, W, fl[c.level] + (c.kt == 3 ? 2 : 0), fl[c.level]};
}
// every conv's operand buffer and the three dense buffers for windows up to th x tw, into the live members
static int alloc_operands(s2v_vae* v, int th, int tw, const int* fl) {
    int rc = 0;
    int64_t dmax = 0;
    for_each_conv(v, [&](ConvL& c) {
        const Operand o = operand_extent(v, c, th, tw, fl);
        c.pad_bytes = o.padded_bytes(v, c) + 1024;
        if (!rc) rc = dmalloc(v, &c.pad, c.pad_bytes, true);
        dmax = std::max(dmax, o.dense_bytes(v, c));
    });
    if (rc) return rc;
    v->dense_bytes = dmax + (int64_t)256 * 1024 * v->esz;  // + one 128-row MFMA tile of slack
    for (int i = 0; i < 3; ++i) S2V_TRY(dmalloc(v, &v->dense[i], v->dense_bytes, true));
    return 0;
}

// one workspace set (every operand / cache / scratch buffer of a decode at window th x tw) into the live members
static int alloc_workspace_set(s2v_vae* v, int th, int tw, int fz_max) {
    S2V_TRY(alloc_operands(v, th, tw, v->fmax));
    S2V_TRY(dmalloc(v, &v->zq, (int64_t)fz_max * th * tw * v->Cz * v->esz + 64, true));
    int cmax = 0;
    for_each_conv(v, [&](ConvL& c) { cmax = c.cin > cmax ? c.cin : cmax; });
    S2V_TRY(dmalloc(v, &v->yt, (int64_t)fz_max * th * tw * cmax * v->esz + 64, true));
    S2V_TRY(dmalloc(v, &v->bt, (int64_t)fz_max * th * tw * cmax * v->esz + 64, true));
    int lv = 0;
    for (size_t s = 1; s < v->stages.size(); ++s) if (v->stages[s].has_up) lv++;
    const int64_t pmax = (int64_t)v->fmax[lv] * ((int64_t)th << lv) * ((int64_t)tw << lv);
    S2V_TRY(dmalloc(v, &v->gn_part, gn_stats_scratch_bytes(pmax, v->G) + 64, true));
    S2V_TRY(dmalloc(v, &v->sums, sizeof(double) * 2 * v->G, true));
    return 0;
}

// Workspace for windows up to th x tw latents, fz_max latent frames per batch, `nws` sets (tiles in flight).
// The capacity fields (th / tw / fmax / ws_req) and v->ws are committed only AFTER the sets exist: a failed allocation leaves the
// context at "no capacity" (the next decode allocates again instead of running on empty sets -- ADVICE r3), a failed set k > 0 is
// freed and the decode proceeds with k sets.  The number of sets is bounded by 70 % of the free memory at this moment (other ranks
// on the device and torch's caching allocator may move that figure: hence the retry-with-fewer path) and by a byte cap (a quarter of the
// device's memory unless S2V_VAE_WORKSPACE_MAX_GB says otherwise).
static int prepare_tile_capacity(s2v_vae* v, int th, int tw, int fz_max, int nws = 1) {
    // Sets sized for a LARGER window than this request leave fewer tiles in flight than the byte cap allows: an untiled decode of 90 x 160 latents
    // (one 57.7 GB set) followed by the tiled decode of the same latents (30 x 45-latent tiles: 5.5 GB per set, six fit) used to keep the one big
    // set and run the twenty tiles one after the other -- 1.9 s instead of 1.4 (bench.py times untiled, then tiled; at 480 x 720
    // three 21.7 GB sets instead of six of 5.5 GB).  A request for several sets that the present capacity cannot serve is rebuilt at the REQUESTED
    // size; the next untiled decode grows it again (a decoder that alternates the two modes re-allocates each time: the pipeline only tiles).
    const bool oversized = !v->ws.empty() && (v->th > th || v->tw > tw) && nws > 1 && (int)v->ws.size() < nws;
    if (!oversized && v->th >= th && v->tw >= tw && v->fmax[0] >= fz_max && v->ws_req >= nws && !v->ws.empty()) return 0;
    S2V_CHECK_HIP(hipDeviceSynchronize());
    for (void* p : v->geo_allocs) (void)hipFree(p);
    v->geo_allocs.clear();
    if (!oversized) {  // growing: never below what an earlier decode needed
        th = th > v->th ? th : v->th;
        tw = tw > v->tw ? tw : v->tw;
        nws = std::max(nws, v->ws_req);
    }
    fz_max = fz_max > v->fmax[0] ? fz_max : v->fmax[0];
    const int nws_req = nws;
    // from here until the commit below the context has NO capacity
    v->th = v->tw = 0; v->ws_req = 0; v->ws.clear(); v->ws_active = 0; v->cur_h = v->cur_w = 0;
    for (int i = 0; i < 8; ++i) v->fmax[i] = 0;
    // frames per level
    int f = fz_max, lvl = 0;
    v->fmax[0] = f;
    for (size_t s = 1; s < v->stages.size(); ++s)
        if (v->stages[s].has_up) { f = up_frames(f, v->stages[s].compress_time); v->fmax[++lvl] = f; }
    {  // as many sets as 70 % of the free memory (and the optional byte cap) hold, never fewer than one
        int64_t set_bytes = 0, dmax = 0;
        for_each_conv(v, [&](ConvL& c) {
            const Operand o = operand_extent(v, c, th, tw, v->fmax);
            set_bytes += o.padded_bytes(v, c);
            dmax = std::max(dmax, o.dense_bytes(v, c));
        });
        set_bytes += 3 * dmax;
        v->set_bytes = set_bytes;
        size_t free_b = 0, total_b = 0;
        double budget = -1.0;
        // default byte cap: a quarter of the device's memory (MI355X: 72 GB = three ~21.7 GB sets at the real widths, 602 ms per 49 x 480 x 720
        // decode against 554 with six sets and 130 GB -- profiles/r03_vae_tiles_in_flight.txt; VERDICT r4: 130 GB of workspaces to save 0.15 s
        // is not a default).  S2V_VAE_WORKSPACE_MAX_GB = n caps at n GB instead, <= 0 lifts the byte cap (70 % of the free memory remains).
        double cap = -1.0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) { budget = 0.7 * (double)free_b; cap = 0.25 * (double)total_b; }
        if (const char* e = getenv("S2V_VAE_WORKSPACE_MAX_GB")) cap = atof(e) * 1e9;
        if (cap > 0 && (budget < 0 || cap < budget)) budget = cap;
        if (budget >= 0 && set_bytes > 0)
            nws = (int)std::max<int64_t>(1, std::min<int64_t>(nws, (int64_t)budget / set_bytes));
    }
    std::vector<s2v_vae::WS> sets;
    int rc = 0;
    v->fault_geo_seen = 0;
    {
        const char* e = getenv("S2V_VAE_FAULT_GEO_ALLOC");
        v->fault_geo_at = e ? atoi(e) : 0;
    }
    for (int k = 0; k < nws; ++k) {
        const size_t mark = v->geo_allocs.size();
        rc = alloc_workspace_set(v, th, tw, fz_max);
        if (rc) {  // give the partial set back; with k sets built the decode runs k tiles in flight
            (void)hipGetLastError();
            for (size_t i = mark; i < v->geo_allocs.size(); ++i) (void)hipFree(v->geo_allocs[i]);
            v->geo_allocs.resize(mark);
            break;
        }
        v->ws.push_back(s2v_vae::WS());
        v->cur_h = v->cur_w = 0;
        ws_save(v, (int)v->ws.size() - 1);
    }
    if (v->ws.empty()) {  // not even one set: stay at "no capacity" and report the allocation failure
        for (int i = 0; i < 8; ++i) v->fmax[i] = 0;
        for_each_conv(v, [&](ConvL& c) { c.pad = nullptr; });
        return rc ? rc : vfail("prepare_tile_capacity: no workspace set could be allocated");
    }
    nws = (int)v->ws.size();
    // The live members hold whatever alloc_workspace_set wrote LAST -- the last set built, or the freed pointers of a set that failed part-way
    // (with one surviving set ws_activate(0) returned early and the next decode wrote through them).  Reload set 0 unconditionally.
    ws_load(v, 0);
    while ((int)v->side.size() < nws - 1) {
        hipStream_t sst = nullptr; hipEvent_t e = nullptr;
        S2V_CHECK_HIP(hipStreamCreateWithFlags(&sst, hipStreamNonBlocking));
        S2V_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        v->side.push_back(sst); v->ev_side.push_back(e);
    }
    if (!v->ev_fork) S2V_CHECK_HIP(hipEventCreateWithFlags(&v->ev_fork, hipEventDisableTiming));
    // commit: the capacity this context now really has (ws_req keeps the REQUEST so that a memory-bounded result is not retried on
    // every decode; a later, larger request allocates again)
    v->th = th; v->tw = tw; v->ws_req = nws_req;
    return 0;
}

// A new window size: the zero ring of every padded operand moves.  Decoder (ring_only): only the ring of the new size is cleared
// (launch_zero_border: interiors are rewritten by their producers before they are read; the buffers were zeroed when they were
// allocated) -- with nine tiles of four sizes dealt to six workspace sets the whole-buffer memsets (20 GB per set) were 35-40 ms of a
// 555 ms tiled decode.  The encoder's one-frame buffers are small and keep the plain memset.
static int set_layout(s2v_vae* v, int h, int w, hipStream_t st, bool ring_only = false) {
    if (v->cur_h == h && v->cur_w == w) return 0;
    int rc = 0;
    for_each_conv(v, [&](ConvL& c) {
        if (rc) return;
        const Operand o = operand_extent(v, c, h, w, v->fmax);
        if (ring_only) rc = launch_zero_border(c.pad, (int)o.F, (int)o.H, (int)o.W, c.cin, v->esz, st);
        else if (hipMemsetAsync(c.pad, 0, (size_t)c.pad_bytes, st) != hipSuccess) rc = -2;
    });
    if (rc) return vfail("clearing the operand borders failed");
    v->cur_h = h; v->cur_w = w;
    return 0;
}

// ---- launch sequences --------------------------------------------------------------------------------------------
#ifdef S2V_DIAG
// tools/vae_conv_rates.py: EVERY GEMM-shaped launch of the decode in launch order -- convolutions AND the 1 x 1 shortcut GEMMs between them --
// so that the log zips one-to-one with the GEMM kernels of a kernel trace (round 4 logged the convolutions only and matched the rest by grid
// size: a shortcut GEMM with a convolution's grid then stood in for it, and rows above the 2.5 PF peak appeared)
static void vae_gemm_log(const GemmArgs& g, int epi, bool mfma, const char* kind) {
    if (const char* lg = getenv("S2V_VAE_CONV_LOG"))
        if (FILE* f = fopen(lg, "a")) { fprintf(f, "%d %d %d %d %d %s\n", g.M, g.N, g.K, epi, (int)mfma, kind); fclose(f); }
}
#endif
// the GEMM kernel of a convolution or a 1 x 1 shortcut: bf16 MFMA when the channel count fills its K tiles, fp16 MFMA where gemm_f16 takes
// the shape, the generic kernel otherwise
static bool gemm_is_bf16_mfma(const s2v_vae* v, const GemmArgs& g) { return v->mfma && (g.conv ? g.cin : g.K) % 64 == 0; }
#ifdef S2V_DIAG
static int g_vae_diag_route = 0;  // s2v_diag_vae_conv_run: which branch of launch_gemm the last GEMM took (1 bf16 MFMA, 2 fp16 MFMA, 3 gemm_f32m, 4 generic)
#define S2V_VAE_ROUTE(r) g_vae_diag_route = (r)
#else
#define S2V_VAE_ROUTE(r) (void)0
#endif
static int launch_gemm(s2v_vae* v, GemmArgs& g, int epi, hipStream_t st) {
    if (gemm_is_bf16_mfma(v, g)) { S2V_VAE_ROUTE(1); return launch_gemm_bf16(g, epi, st); }  // cout = 3 (conv_out) without the direct kernel: one padded 128-column tile
    if (v->h16 && gemm_f16_ok(g, epi)) { S2V_VAE_ROUTE(2); return launch_gemm_f16(g, epi, st); }
    g.valu_only = v->cfg.force_simple;
    S2V_VAE_ROUTE(v->dtype == S2V_F32 && gemm_f32m_ok(g) ? 3 : 4);
    return launch_gemm_simple(g, epi, v->dtype, st);
}
// direct_dst (conv_out only): the [C][Ftot][H][W] tile output -- when the direct small-N kernel qualifies (launch_conv_out_direct) it writes there
// and *did_direct is set; otherwise the implicit GEMM writes `out` and the caller converts the layout
static int run_conv(s2v_vae* v, ConvL& c, int F, int H, int W, bool first, int epi, const void* resid, void* out,
                    hipStream_t st, char* direct_dst = nullptr, int Ftot = 0, int f0 = 0, bool* did_direct = nullptr) {
    const int64_t fb = (int64_t)(H + 2) * (W + 2) * c.cin * v->esz;
    if (c.kt == 3 && first) {
        S2V_CHECK_HIP(hipMemcpyAsync(c.pad, c.pad + 2 * fb, fb, hipMemcpyDeviceToDevice, st));
        S2V_CHECK_HIP(hipMemcpyAsync(c.pad + fb, c.pad + 2 * fb, fb, hipMemcpyDeviceToDevice, st));
    }
    const int taps = c.kt == 3 ? 27 : 9;
    bool direct = false;
    bool want_direct = direct_dst && c.kt == 3 && epi == EPI_BIAS && !v->cfg.force_simple && (v->mfma || v->h16);
#ifdef S2V_DIAG
    if (getenv("S2V_VAE_NO_DIRECT_CONV_OUT")) want_direct = false;  // same-box A/B against the implicit-GEMM conv_out (diagnostics build only)
#endif
    if (want_direct) {
        const int rc = launch_conv_out_direct(c.pad, c.w, taps * c.cin, c.b, F, H, W, c.cin, c.cout, direct_dst, Ftot, f0, v->dtype, st);
        if (rc < 0) return rc;
        direct = rc == 1;
    }
    if (did_direct) *did_direct = direct;
    GemmArgs g{};
    g.A = c.pad; g.W = c.w; g.ldw = taps * c.cin; g.bias = c.b; g.C = out; g.ldc = c.cout;
    g.M = F * H * W; g.N = c.cout; g.K = taps * c.cin;
    g.R = resid; g.ldr = c.cout;
    g.conv = 1; g.cin = c.cin; g.Hp = H + 2; g.Wp = W + 2; g.oH = H; g.oW = W; g.kt = c.kt;
    g.w_rows_padded = (int)rup64(c.cout, 256);
#ifdef S2V_DIAG
    if (const char* e = getenv("S2V_VAE_ADD_EXPERIMENT")) {  // timing experiments on the residual-add epilogue (results are wrong): 1 = no add, 2 = residual from another buffer
        if (epi == EPI_BIAS_ADD && atoi(e) == 1) { epi = EPI_BIAS; g.R = nullptr; }
        if (epi == EPI_BIAS_ADD && atoi(e) == 2) g.R = (const char*)c.pad;  // some other resident buffer of at least M x cout elements
    }
    if (!direct) vae_gemm_log(g, epi, gemm_is_bf16_mfma(v, g), "conv");
#endif
    if (!direct) S2V_TRY(launch_gemm(v, g, epi, st));  // otherwise conv_out ran as the direct kernel
    if (c.kt == 3) {  // conv cache: the last two frames of the operand become frames 0, 1 of the next batch (adjacent on both sides: one copy unless they overlap)
        if (F >= 2) S2V_CHECK_HIP(hipMemcpyAsync(c.pad, c.pad + (int64_t)F * fb, 2 * fb, hipMemcpyDeviceToDevice, st));
        else {
            S2V_CHECK_HIP(hipMemcpyAsync(c.pad, c.pad + (int64_t)F * fb, fb, hipMemcpyDeviceToDevice, st));
            S2V_CHECK_HIP(hipMemcpyAsync(c.pad + fb, c.pad + (int64_t)(F + 1) * fb, fb, hipMemcpyDeviceToDevice, st));
        }
    }
    return 0;
}

// GroupNorm statistics over the frame batch, then normalise + SiLU into the next conv's operand (frames 2.. of out_pad).  The decoder's handle
// has the yt / bt tables of the spatial norm and passes the zq window (Fz, hz, wz); the encoder's has none (the kernel then applies plain
// GroupNorm) and passes 1, 1, 1.
struct ZqWin { int F, h, w; };
static int run_norm(s2v_vae* v, const SNormL& n, const void* x, int F, int H, int W, ZqWin z, void* out_pad, hipStream_t st) {
    S2V_TRY(launch_gn_stats(x, (int64_t)F * H * W, n.C, v->G, v->sums, v->gn_part, v->dtype, st));
    SNormArgs a{};
    a.x = x; a.F = F; a.H = H; a.W = W; a.C = n.C; a.G = v->G; a.sums = v->sums; a.eps = v->cfg.norm_eps;
    a.gn_w = n.gn_w; a.gn_b = n.gn_b; a.wy = n.wy; a.by = n.by; a.wb = n.wb; a.bb = n.bb;
    a.zq = v->zq; a.Fz = z.F; a.hz = z.h; a.wz = z.w; a.Cz = v->Cz; a.out = out_pad; a.f_off = 2; a.silu = 1; a.yt = v->yt; a.bt = v->bt;
    return launch_snorm_apply(a, v->dtype, st);
}

// one resnet on dense[cur] (scratch dense[t1], dense[t2]): norm, conv, norm, the 1 x 1 shortcut GEMM where the channel count changes, conv +
// add; the result is in dense[cur] again (with a shortcut cur and t2 trade places)
static int run_resnet(s2v_vae* v, ResnetL& r, int F, int H, int W, ZqWin z, bool first, int& cur, int t1, int& t2, hipStream_t st) {
    S2V_TRY(run_norm(v, r.n1, v->dense[cur], F, H, W, z, r.c1.pad, st));
    S2V_TRY(run_conv(v, r.c1, F, H, W, first, EPI_BIAS, nullptr, v->dense[t1], st));
    S2V_TRY(run_norm(v, r.n2, v->dense[t1], F, H, W, z, r.c2.pad, st));
    if (!r.has_sc) return run_conv(v, r.c2, F, H, W, first, EPI_BIAS_ADD, v->dense[cur], v->dense[cur], st);
    GemmArgs g{};
    g.A = v->dense[cur]; g.lda = r.cin; g.W = r.sc.w; g.ldw = r.cin; g.bias = r.sc.b;
    g.C = v->dense[t2]; g.ldc = r.cout; g.M = F * H * W; g.N = r.cout; g.K = r.cin;
    g.a_rows_padded = (int)rup64(g.M, 256);  // dense buffers carry a 256-row slack
#ifdef S2V_DIAG
    vae_gemm_log(g, EPI_BIAS, gemm_is_bf16_mfma(v, g), "shortcut");
#endif
    S2V_TRY(launch_gemm(v, g, EPI_BIAS, st));
    S2V_TRY(run_conv(v, r.c2, F, H, W, first, EPI_BIAS_ADD, v->dense[t2], v->dense[t2], st));
    std::swap(cur, t2);
    return 0;
}

// one decoder pass over a frame batch of `Fz` latent frames of an (h x w) latent window; writes its output frames
static int decode_batch(s2v_vae* v, int Fz, int h, int w, bool first, char* dst, int Ftot, int f0, int* frames_out,
                        hipStream_t st) {
    int cur = 0, t1 = 1, t2 = 2;
    int F = Fz, H = h, W = w;
    const ZqWin z{Fz, h, w};
    S2V_TRY(launch_dense_to_padded(v->zq, Fz, h, w, v->Cz, v->conv_in.pad, 2, v->dtype, st));
    S2V_TRY(run_conv(v, v->conv_in, F, H, W, first, EPI_BIAS, nullptr, v->dense[cur], st));
    for (auto& s : v->stages) {
        for (auto& r : s.res) S2V_TRY(run_resnet(v, r, F, H, W, z, first, cur, t1, t2, st));
        if (s.has_up) {
            S2V_TRY(launch_upsample(v->dense[cur], F, H, W, s.up.cin, s.compress_time, s.up.pad, v->dtype, st));
            F = up_frames(F, s.compress_time); H *= 2; W *= 2;
            S2V_TRY(run_conv(v, s.up, F, H, W, first, EPI_BIAS, nullptr, v->dense[t1], st));
            std::swap(cur, t1);
        }
    }
    S2V_TRY(run_norm(v, v->norm_out, v->dense[cur], F, H, W, z, v->conv_out.pad, st));
    bool direct = false;
    S2V_TRY(run_conv(v, v->conv_out, F, H, W, first, EPI_BIAS, nullptr, v->dense[t1], st, dst, Ftot, f0, &direct));
    if (!direct) S2V_TRY(launch_to_ncfhw(v->dense[t1], F, H, W, v->cfg.out_channels, dst, Ftot, f0, v->dtype, st));
    *frames_out = F;
    return 0;
}

// Frame batches of the reference (autoencoder_kl_cogvideox.py:1237-1245 decode, num_latent_frames_batch_size = 2; :1177-1202 _encode,
// num_sample_frames_batch_size = 8): the first batch takes fbs + F % fbs frames, every later batch fbs; fewer than 2 fbs frames are one batch
enum { DEC_FRAME_BATCH = 2, ENC_FRAME_BATCH = 8 };
struct Batch { int s, e; };
static std::vector<Batch> frame_batches(int F, int fbs) {
    const int nb = F / fbs > 1 ? F / fbs : 1, rem = F % fbs;
    std::vector<Batch> b;
    for (int i = 0; i < nb; ++i) b.push_back({fbs * i + (i == 0 ? 0 : rem), std::min(fbs * (i + 1) + rem, F)});
    return b;
}
static int out_frames_of(s2v_vae* v, int F) {
    int tot = 0;
    for (auto b : frame_batches(F, DEC_FRAME_BATCH)) {
        int f = b.e - b.s;
        for (size_t s = 1; s < v->stages.size(); ++s)
            if (v->stages[s].has_up) f = up_frames(f, v->stages[s].compress_time);
        tot += f;
    }
    return tot;
}
static int spatial_scale(s2v_vae* v) { return 1 << (v->cfg.num_blocks - 1); }

// The tiling of the reference's tiled_decode / tiled_encode (autoencoder_kl_cogvideox.py:1102-1114 the tile sizes, :1400-1406 / :1317-1323
// overlap, blend extent and crop limit with their int() truncations, :1437-1450 / :1354-1367 the raster-order blend, crop and concatenation) --
// one rule with input and output swapped.  Tiles are sample_size / 2 pixels = that / 2^(blocks - 1) latents; the decoder cuts latents and
// pastes pixels, the encoder cuts pixels and pastes latents.  Tile origins step by the overlap, a fraction (5/6, 4/5) of the INPUT-side tile;
// blend extent (1/6, 1/5) and crop limit (the rest) are fractions of the OUTPUT-side tile; edge tiles are whatever is left of the input, so a
// blend takes no more rows than either neighbour has.  Pure arithmetic: no handle, no device (tests/test_vae_tile_plan_cpu.py).
struct Tile {
    int y, x, h, w;  // input window
    int oh, ow;      // its output: h * scale decoding, h / scale encoding
    int bv, bh;      // rows blended with the tile above, columns with the tile to the left (0: first row / column)
    int ch, cw;      // crop of the blended output
    int py, px;      // where the crop lands in the whole output
};
struct TilePlan { bool tiled = false; int rows = 1, cols = 1, out_h = 0, out_w = 0; std::vector<Tile> tiles; };  // tiles in raster order
static bool vae_tile_plan(int sample_h, int sample_w, int num_blocks, bool encode, int H, int W, int tiling, TilePlan* p) {  // false: degenerate overlap
    const int sc = 1 << (num_blocks - 1), ts_h = sample_h / 2, ts_w = sample_w / 2;
    const int tl_h = (int)((double)ts_h / sc), tl_w = (int)((double)ts_w / sc);
    const int in_h = encode ? ts_h : tl_h, in_w = encode ? ts_w : tl_w, to_h = encode ? tl_h : ts_h, to_w = encode ? tl_w : ts_w;
    const int ov_h = (int)(in_h * (1.0 - 1.0 / 6.0)), ov_w = (int)(in_w * (1.0 - 1.0 / 5.0));
    const int bl_h = (int)(to_h * (1.0 / 6.0)), bl_w = (int)(to_w * (1.0 / 5.0));
    const int lim_h = to_h - bl_h, lim_w = to_w - bl_w;
    auto out = [&](int n) { return encode ? n / sc : n * sc; };
    *p = TilePlan();
    p->tiled = tiling && (W > in_w || H > in_h);
    if (!p->tiled) {
        p->out_h = out(H); p->out_w = out(W);
        p->tiles.push_back({0, 0, H, W, p->out_h, p->out_w, 0, 0, p->out_h, p->out_w, 0, 0});
        return true;
    }
    if (ov_h <= 0 || ov_w <= 0) return false;
    p->rows = (H + ov_h - 1) / ov_h; p->cols = (W + ov_w - 1) / ov_w;
    for (int i = 0; i < H; i += ov_h) {
        p->out_w = 0;
        for (int j = 0; j < W; j += ov_w) {
            Tile t{i, j, std::min(in_h, H - i), std::min(in_w, W - j)};
            t.oh = out(t.h); t.ow = out(t.w);
            t.bv = i > 0 ? std::min(std::min(p->tiles[p->tiles.size() - p->cols].oh, t.oh), bl_h) : 0;
            t.bh = j > 0 ? std::min(std::min(p->tiles.back().ow, t.ow), bl_w) : 0;
            t.ch = std::min(t.oh, lim_h); t.cw = std::min(t.ow, lim_w);
            t.py = p->out_h; t.px = p->out_w;
            p->out_w += t.cw;
            p->tiles.push_back(t);
        }
        p->out_h += p->tiles.back().ch;
    }
    return true;
}
static bool tile_plan_of(const s2v_vae* v, bool encode, int H, int W, int tiling, TilePlan* p) {
    return vae_tile_plan(v->cfg.sample_height, v->cfg.sample_width, v->cfg.num_blocks, encode, H, W, tiling, p);
}
#ifdef S2V_DIAG
// vae_tile_plan without a handle: head = {tiled, rows, cols, out_h, out_w}; tiles = the twelve fields of Tile, tile after tile, for at most max_tiles
extern "C" __attribute__((visibility("default"))) int s2v_diag_vae_tile_plan(int32_t sample_h, int32_t sample_w, int32_t num_blocks, int32_t encode,
                                                                              int32_t H, int32_t W, int32_t tiling, int32_t* head, int32_t* tiles,
                                                                              int32_t max_tiles) {
    S2V_REQUIRE(head && tiles && sample_h > 0 && sample_w > 0 && num_blocks >= 1 && num_blocks <= 6 && H >= 1 && W >= 1, "s2v_diag_vae_tile_plan: bad argument");
    TilePlan p;
    S2V_REQUIRE(vae_tile_plan(sample_h, sample_w, num_blocks, encode != 0, H, W, tiling, &p), "s2v_diag_vae_tile_plan: degenerate tile overlap");
    S2V_REQUIRE((int64_t)p.tiles.size() <= max_tiles, "s2v_diag_vae_tile_plan: more tiles than the caller has room for");
    const int32_t h5[5] = {p.tiled, p.rows, p.cols, p.out_h, p.out_w};
    std::copy(h5, h5 + 5, head);
    static_assert(sizeof(Tile) == 12 * sizeof(int32_t), "Tile is twelve ints");
    std::copy((const int32_t*)p.tiles.data(), (const int32_t*)(p.tiles.data() + p.tiles.size()), tiles);
    return 0;
}
#endif

extern "C" int s2v_vae_workspace_info(s2v_vae* v, int32_t* sets, int64_t* bytes_per_set) {
    S2V_REQUIRE(v && sets && bytes_per_set, "s2v_vae_workspace_info: null argument");
    *sets = (int32_t)v->ws.size();
    *bytes_per_set = v->set_bytes;
    return 0;
}

extern "C" int s2v_vae_out_shape(s2v_vae* v, int32_t F, int32_t h, int32_t w, int32_t tiling, int32_t* Fo, int32_t* Ho,
                                 int32_t* Wo) {
    S2V_REQUIRE(v && Fo && Ho && Wo && F >= 1 && h >= 1 && w >= 1, "s2v_vae_out_shape: bad argument");
    *Fo = out_frames_of(v, F);
    TilePlan p;
    S2V_REQUIRE(tile_plan_of(v, false, h, w, tiling, &p), "s2v_vae_out_shape: degenerate tile overlap");
    *Ho = p.out_h; *Wo = p.out_w;
    return 0;
}

// per-tile outputs [C][Fo][oh][ow] of a tiled call (re-allocated only when the tiling or the output frame count changes)
static int ensure_tile_buffers(s2v_vae* v, const TilePlan& p, int C, int Fo) {
    const size_t nt = p.tiles.size();
    bool same = v->tiles.size() == nt && v->tiles_F == Fo;
    for (size_t k = 0; same && k < nt; ++k) same = v->tile_h[k] == p.tiles[k].oh && v->tile_w[k] == p.tiles[k].ow;
    if (same) return 0;
    S2V_CHECK_HIP(hipDeviceSynchronize());
    for (char* q : v->tiles) (void)hipFree(q);
    v->tiles.assign(nt, nullptr); v->tile_h.assign(nt, 0); v->tile_w.assign(nt, 0);
    for (size_t k = 0; k < nt; ++k) {
        v->tile_h[k] = p.tiles[k].oh; v->tile_w[k] = p.tiles[k].ow;
        S2V_CHECK_HIP(hipMalloc((void**)&v->tiles[k], (size_t)C * Fo * v->tile_h[k] * v->tile_w[k] * v->esz + 16));
    }
    v->tiles_F = Fo;
    return 0;
}
// raster-order in-place blends (neighbours are read already blended), then crop + paste into the whole output; a tile is CF planes of oh x ow
static int blend_and_paste(s2v_vae* v, const TilePlan& p, int CF, void* out, hipStream_t st) {
    for (size_t k = 0; k < p.tiles.size(); ++k) {
        const Tile& t = p.tiles[k];
        for (int vertical = 1; vertical >= 0; --vertical) {
            const int E = vertical ? t.bv : t.bh;
            if (E <= 0) continue;
            const size_t ka = vertical ? k - p.cols : k - 1;
            S2V_TRY(launch_blend(v->tiles[ka], p.tiles[ka].oh, p.tiles[ka].ow, v->tiles[k], t.oh, t.ow, CF, E, vertical, v->dtype, st));
        }
        S2V_TRY(launch_paste(v->tiles[k], t.oh, t.ow, t.ch, t.cw, out, p.out_h, p.out_w, t.py, t.px, CF, v->dtype, st));
    }
    return 0;
}

static int decode_window(s2v_vae* v, const char* lat, int F, int h, int w, int y0, int x0, int th, int tw, char* dst,
                         int Ftot, int scaled, hipStream_t st) {
    S2V_TRY(set_layout(v, th, tw, st, true));
    const float inv_sf = scaled ? (float)(1.0 / (double)v->cfg.scaling_factor) : 1.0f;
    int f0 = 0;
    bool first = true;
    for (auto b : frame_batches(F, DEC_FRAME_BATCH)) {
        const int Fz = b.e - b.s;
        S2V_TRY(launch_latent_to_zq(lat + (int64_t)b.s * v->Cz * h * w * v->esz, Fz, v->Cz, h, w, inv_sf, v->zq, y0, x0, th,
                                    tw, v->dtype, st));
        int fo = 0;
        S2V_TRY(decode_batch(v, Fz, th, tw, first, dst, Ftot, f0, &fo, st));
        f0 += fo;
        first = false;
    }
    return 0;
}

extern "C" int s2v_vae_decode(s2v_vae* v, const void* latents, int32_t F, int32_t h, int32_t w, int32_t tiling,
                              int32_t scaled, void* out, s2v_stream stream) {
    S2V_REQUIRE(v && latents && out, "s2v_vae_decode: null argument");
    S2V_REQUIRE(!v->encoder, "s2v_vae_decode: this handle holds the encoder");
    S2V_REQUIRE(v->finalized, "s2v_vae_decode: weights not finalized");
    S2V_REQUIRE(F >= 1 && h >= 1 && w >= 1, "s2v_vae_decode: bad geometry");
    hipStream_t st = (hipStream_t)stream;
    const int Ftot = out_frames_of(v, F);
    int fz_max = 0;
    for (auto b : frame_batches(F, DEC_FRAME_BATCH)) fz_max = std::max(fz_max, b.e - b.s);
    TilePlan p;
    S2V_REQUIRE(tile_plan_of(v, false, h, w, tiling, &p), "s2v_vae_decode: degenerate tile overlap");
    if (!p.tiled) {
        S2V_TRY(prepare_tile_capacity(v, h, w, fz_max));
        ws_activate(v, 0);
        return decode_window(v, (const char*)latents, F, h, w, 0, 0, h, w, (char*)out, Ftot, scaled, st);
    }
    const size_t nt = p.tiles.size();
    // tiles in flight: 49 x 480 x 720 at the real widths measured 928 / 684 / 602 / 605 / 554 / 590 ms with 1 / 2 / 3 / 4 / 6 / 9 sets
    // (profiles/r03_vae_tiles_in_flight.txt; round 6: 505-510 ms with six); up to six, as many as the byte cap of prepare_tile_capacity holds (a set
    // sized for a 30 x 45-latent tile is 5.5 GB: all six)
    int nws_cap = 6;
    if (const char* e = getenv("S2V_VAE_TILES_IN_FLIGHT")) nws_cap = std::max(1, atoi(e));
    int nws = (int)std::min<size_t>(nt, (size_t)nws_cap);
    S2V_TRY(prepare_tile_capacity(v, p.tiles[0].h, p.tiles[0].w, fz_max, nws));  // the first tile is the largest
    nws = std::min(nws, (int)v->ws.size());
    const int C = v->cfg.out_channels;
    S2V_TRY(ensure_tile_buffers(v, p, C, Ftot));
    // tile k runs on workspace set k mod nws: set 0 on the caller's stream, the others on side streams forked from it and joined
    // before the blends (tiles of one set serialise on its stream: they share its buffers)
    if (nws > 1) S2V_CHECK_HIP(hipEventRecord(v->ev_fork, st));
    for (int q = 1; q < nws; ++q) S2V_CHECK_HIP(hipStreamWaitEvent(v->side[q - 1], v->ev_fork, 0));
    // raster order, round-robin over the sets (largest-tile-first onto the least loaded set measured the same at 3-4 sets and 18 % worse
    // at 6: what overlaps well is a big tile's chip-filling GEMMs with a small tile's latency-bound ones, which raster order pairs up)
    for (size_t k = 0; k < nt; ++k) {
        const Tile& t = p.tiles[k];
        const int q = (int)(k % nws);
        ws_activate(v, q);
        S2V_TRY(decode_window(v, (const char*)latents, F, h, w, t.y, t.x, t.h, t.w, v->tiles[k], Ftot, scaled, q == 0 ? st : v->side[q - 1]));
    }
    ws_activate(v, 0);
    for (int q = 1; q < nws; ++q) {
        S2V_CHECK_HIP(hipEventRecord(v->ev_side[q - 1], v->side[q - 1]));
        S2V_CHECK_HIP(hipStreamWaitEvent(st, v->ev_side[q - 1], 0));
    }
    return blend_and_paste(v, p, C * Ftot, out, st);
}

extern "C" int s2v_vae_postprocess_u8(const void* video, int32_t C, int32_t F, int32_t H, int32_t W, uint8_t* out, int32_t dtype,
                                      s2v_stream stream) {
    S2V_REQUIRE(video && out, "s2v_vae_postprocess_u8: null argument");
    return launch_postprocess_u8(video, C, F, H, W, out, dtype, (hipStream_t)stream);
}

static int postprocess_masked(const char* fn, const void* video, const void* keep, int32_t keep_dtype, const uint8_t* mask, int32_t C, int32_t F,
                              int32_t H, int32_t W, void* out, int out_u8, int32_t dtype, s2v_stream stream) {
    static thread_local std::string m;
    auto bad = [&](const char* why) { m = std::string(fn) + ": " + why; return m.c_str(); };
    S2V_REQUIRE(video && keep && mask && out, bad("null argument"));
    S2V_REQUIRE(C >= 1 && F >= 1 && H >= 1 && W >= 1, bad("bad shape"));
    for (int dt : {dtype, keep_dtype}) S2V_REQUIRE(dt == S2V_F32 || dt == S2V_BF16 || dt == S2V_F16, bad("unsupported dtype"));
    return launch_postprocess_masked(video, keep, keep_dtype, mask, C, F, H, W, out, out_u8, dtype, (hipStream_t)stream);
}

extern "C" int s2v_vae_postprocess_masked(const void* video, const void* keep, int32_t keep_dtype, const uint8_t* mask, int32_t C, int32_t F,
                                          int32_t H, int32_t W, float* out, int32_t dtype, s2v_stream stream) {
    return postprocess_masked("s2v_vae_postprocess_masked", video, keep, keep_dtype, mask, C, F, H, W, out, 0, dtype, stream);
}

extern "C" int s2v_vae_postprocess_u8_masked(const void* video, const void* keep, int32_t keep_dtype, const uint8_t* mask, int32_t C, int32_t F,
                                             int32_t H, int32_t W, uint8_t* out, int32_t dtype, s2v_stream stream) {
    return postprocess_masked("s2v_vae_postprocess_u8_masked", video, keep, keep_dtype, mask, C, F, H, W, out, 1, dtype, stream);
}

extern "C" int s2v_vae_postprocess(const void* video, int32_t C, int32_t F, int32_t H, int32_t W, float* out, int32_t dtype,
                                   s2v_stream stream) {
    S2V_REQUIRE(video && out, "s2v_vae_postprocess: null argument");
    return launch_postprocess(video, C, F, H, W, out, dtype, (hipStream_t)stream);
}

// =====================================================================================================================
// ENCODE of the reference image or a video (AutoencoderKLCogVideoX._encode / tiled_encode, autoencoder_kl_cogvideox.py:1177-1203, 1300-1372)
// on a handle of s2v_vae_enc_create, untiled or tiled, moments out; the posterior sample is s2v_vae_gaussian_sample.

// CogVideoXDownsample3D with compress_time: frame pairs averaged, the first frame kept alone when the count is odd
static int down_frames(int F, int ct) { return !ct ? F : ((F & 1) ? (F + 1) / 2 : F / 2); }
// frames at every level of one encoder pass over Fb input frames
static void enc_level_frames(s2v_vae* v, int Fb, int* fl) {
    int f = Fb, lvl = 0;
    fl[0] = f;
    for (auto& s : v->stages)
        if (s.has_up) { f = down_frames(f, s.compress_time); fl[++lvl] = f; }
}
static int enc_latent_frames(s2v_vae* v, int F) {
    int tot = 0, fl[8];
    for (auto b : frame_batches(F, ENC_FRAME_BATCH)) {
        enc_level_frames(v, b.e - b.s, fl);
        int lv = 0;
        for (auto& s : v->stages) lv += s.has_up ? 1 : 0;
        tot += fl[lv];
    }
    return tot;
}
static bool enc_frames_ok(int F) { return F == 1 || (F > 1 && (F - 1) % 8 == 0); }

// One workspace set for windows up to TH x TW pixels and Fb frames per batch (the largest batch of the video, not the video).
// Like the decoder's prepare_tile_capacity: the capacity fields are committed only after every buffer exists (a failed allocation leaves
// the handle at "no capacity"), and a video encode on a set sized for a LARGER window rebuilds it at the requested size instead of
// keeping the big one (an untiled 480 x 720 encode of 9 frames holds ~8 GB at the real widths; its 240 x 360 tiles need a quarter).
static int enc_prepare(s2v_vae* v, int TH, int TW, int Fb = 1) {
    const bool oversized = Fb > 1 && v->th > 0 && (v->th > TH || v->tw > TW);
    if (!oversized && v->th >= TH && v->tw >= TW && v->fmax[0] >= Fb) return 0;
    S2V_CHECK_HIP(hipDeviceSynchronize());
    for (void* p : v->geo_allocs) (void)hipFree(p);
    v->geo_allocs.clear();
    if (!oversized) { TH = std::max(TH, v->th); TW = std::max(TW, v->tw); }
    Fb = std::max(Fb, v->fmax[0]);
    v->th = v->tw = 0; v->cur_h = v->cur_w = 0;
    for (int i = 0; i < 8; ++i) v->fmax[i] = 0;
    int fl[8] = {0};
    enc_level_frames(v, Fb, fl);
    S2V_TRY(alloc_operands(v, TH, TW, fl));  // the downsampler's operand holds the pooled frames: at most fl[level]
    S2V_TRY(dmalloc(v, &v->gn_part, gn_stats_scratch_bytes((int64_t)Fb * TH * TW, v->G) + 64, true));
    v->th = TH; v->tw = TW;
    for (int i = 0; i < 8; ++i) v->fmax[i] = fl[i];
    return 0;
}

// CogVideoXDownsample3D's spatial half, per frame: F.pad(x, (0,1,0,1)) then Conv2d(3x3, stride 2): the operand sits at (1,1) of its
// zero-bordered buffer, so reading from (1,1) with stride 2 sees the zero column / row on the right / bottom only
static int run_conv_down(s2v_vae* v, ConvL& c, int F, int H, int W, void* out, hipStream_t st) {
    GemmArgs g{};
    g.A = c.pad + ((int64_t)(W + 2) + 1) * c.cin * v->esz; g.W = c.w; g.ldw = 9 * c.cin; g.bias = c.b; g.C = out; g.ldc = c.cout;
    g.M = F * (H / 2) * (W / 2); g.N = c.cout; g.K = 9 * c.cin;
    g.conv = 1; g.cin = c.cin; g.Hp = H + 2; g.Wp = W + 2; g.oH = H / 2; g.oW = W / 2; g.kt = 1; g.cstride = 2;
    g.w_rows_padded = (int)rup64(c.cout, 256);
    return launch_gemm(v, g, EPI_BIAS, st);
}

// encoder pass over frames [fs, fs + Fb) (one frame batch) of the (th x tw) pixel window at (y0, x0) of video [3][Fv][H][W];
// writes latent frames [f0, f0 + *frames_out) of dst = moments [2Cz][Fl][th/s][tw/s].  first: the batch that starts the conv caches.
static int encode_batch(s2v_vae* v, const void* video, int Fv, int fs, int Fb, int Himg, int Wimg, int y0, int x0, int th, int tw,
                        bool first, char* dst, int Fl, int f0, int* frames_out, hipStream_t st) {
    int cur = 0, t1 = 1, t2 = 2;
    int F = Fb, H = th, W = tw;
    const ZqWin z{1, 1, 1};  // no zq: plain GroupNorm
    S2V_TRY(launch_image_to_padded(video, v->cfg.out_channels, Fb, Fv, fs, Himg, Wimg, y0, x0, th, tw, v->conv_in.pad, 2, v->dtype, st));
    S2V_TRY(run_conv(v, v->conv_in, F, H, W, first, EPI_BIAS, nullptr, v->dense[cur], st));
    for (auto& s : v->stages) {
        for (auto& r : s.res) S2V_TRY(run_resnet(v, r, F, H, W, z, first, cur, t1, t2, st));
        if (s.has_up) {  // downsampler: the temporal average pool (compress_time, more than one frame) is fused into the operand write
            if (s.compress_time && F > 1) {
                S2V_TRY(launch_time_pool_to_padded(v->dense[cur], F, H, W, s.up.cin, s.up.pad, v->dtype, st));
                F = down_frames(F, 1);
            } else {
                S2V_TRY(launch_dense_to_padded(v->dense[cur], F, H, W, s.up.cin, s.up.pad, 0, v->dtype, st));
            }
            S2V_TRY(run_conv_down(v, s.up, F, H, W, v->dense[t1], st));
            std::swap(cur, t1);
            H /= 2; W /= 2;
        }
    }
    S2V_TRY(run_norm(v, v->norm_out, v->dense[cur], F, H, W, z, v->conv_out.pad, st));
    S2V_TRY(run_conv(v, v->conv_out, F, H, W, first, EPI_BIAS, nullptr, v->dense[t1], st));
    *frames_out = F;
    return launch_to_ncfhw(v->dense[t1], F, H, W, 2 * v->Cz, dst, Fl, f0, v->dtype, st);
}

// every frame batch of one window, conv caches threaded from batch to batch (each spatial tile has its own batches and caches)
static int encode_window(s2v_vae* v, const void* video, int Fv, int Himg, int Wimg, int y0, int x0, int th, int tw, char* dst, int Fl,
                         hipStream_t st) {
    S2V_TRY(set_layout(v, th, tw, st));
    int f0 = 0;
    bool first = true;
    for (auto b : frame_batches(Fv, ENC_FRAME_BATCH)) {
        int fo = 0;
        S2V_TRY(encode_batch(v, video, Fv, b.s, b.e - b.s, Himg, Wimg, y0, x0, th, tw, first, dst, Fl, f0, &fo, st));
        f0 += fo;
        first = false;
    }
    return 0;
}

extern "C" int s2v_vae_encode_shape(s2v_vae* v, int32_t H, int32_t W, int32_t tiling, int32_t* ho, int32_t* wo) {
    S2V_REQUIRE(v && v->encoder && ho && wo && H >= 1 && W >= 1, "s2v_vae_encode_shape: bad argument");
    TilePlan p;
    S2V_REQUIRE(tile_plan_of(v, true, H, W, tiling, &p), "s2v_vae_encode_shape: degenerate tile overlap");
    *ho = p.out_h; *wo = p.out_w;
    return 0;
}

static int encode_video(s2v_vae* v, const void* video, int F, int H, int W, int tiling, void* moments, hipStream_t st) {
    const int sc = spatial_scale(v);
    const int Fl = enc_latent_frames(v, F);
    int fb_max = 0;
    for (auto b : frame_batches(F, ENC_FRAME_BATCH)) fb_max = std::max(fb_max, b.e - b.s);
    TilePlan p;
    S2V_REQUIRE(tile_plan_of(v, true, H, W, tiling, &p), "s2v_vae_encode: degenerate tile overlap");
    if (!p.tiled) {
        S2V_REQUIRE(H % sc == 0 && W % sc == 0, "s2v_vae_encode: image sides must be multiples of the spatial compression");
        S2V_TRY(enc_prepare(v, H, W, fb_max));
        return encode_window(v, video, F, H, W, 0, 0, H, W, (char*)moments, Fl, st);
    }
    for (const Tile& t : p.tiles) S2V_REQUIRE(t.h % sc == 0, "s2v_vae_encode: tile height not a multiple of the spatial compression");
    for (const Tile& t : p.tiles) S2V_REQUIRE(t.w % sc == 0, "s2v_vae_encode: tile width not a multiple of the spatial compression");
    S2V_TRY(enc_prepare(v, p.tiles[0].h, p.tiles[0].w, fb_max));  // the first tile is the largest
    const int C = 2 * v->Cz;
    S2V_TRY(ensure_tile_buffers(v, p, C, Fl));
    for (size_t k = 0; k < p.tiles.size(); ++k) {
        const Tile& t = p.tiles[k];
        S2V_TRY(encode_window(v, video, F, H, W, t.y, t.x, t.h, t.w, v->tiles[k], Fl, st));
    }
    return blend_and_paste(v, p, C * Fl, moments, st);  // latent-space blends over every latent frame
}

extern "C" int s2v_vae_encode(s2v_vae* v, const void* image, int32_t H, int32_t W, int32_t tiling, void* moments,
                              s2v_stream stream) {
    S2V_REQUIRE(v && image && moments, "s2v_vae_encode: null argument");
    S2V_REQUIRE(v->encoder, "s2v_vae_encode: this handle holds the decoder (use s2v_vae_enc_create)");
    S2V_REQUIRE(v->finalized, "s2v_vae_encode: weights not finalized");
    return encode_video(v, image, 1, H, W, tiling, moments, (hipStream_t)stream);
}

extern "C" int s2v_vae_encode_video_shape(s2v_vae* v, int32_t F, int32_t H, int32_t W, int32_t tiling, int32_t* Fl, int32_t* h,
                                          int32_t* w) {
    S2V_REQUIRE(v && v->encoder && Fl && h && w, "s2v_vae_encode_video_shape: bad argument");
    S2V_REQUIRE(enc_frames_ok(F), "s2v_vae_encode_video_shape: the frame count must be 1 or 8k + 1");
    S2V_TRY(s2v_vae_encode_shape(v, H, W, tiling, h, w));
    *Fl = enc_latent_frames(v, F);
    return 0;
}

extern "C" int s2v_vae_encode_video(s2v_vae* v, const void* video, int32_t F, int32_t H, int32_t W, int32_t tiling, void* moments,
                                    s2v_stream stream) {
    S2V_REQUIRE(v && video && moments, "s2v_vae_encode_video: null argument");
    S2V_REQUIRE(v->encoder, "s2v_vae_encode_video: this handle holds the decoder (use s2v_vae_enc_create)");
    S2V_REQUIRE(v->finalized, "s2v_vae_encode_video: weights not finalized");
    S2V_REQUIRE(enc_frames_ok(F), "s2v_vae_encode_video: the frame count must be 1 or 8k + 1");
    S2V_REQUIRE(H >= 1 && W >= 1, "s2v_vae_encode_video: bad geometry");
    return encode_video(v, video, F, H, W, tiling, moments, (hipStream_t)stream);
}

extern "C" int s2v_vae_gaussian_sample(const void* moments, const void* noise, int32_t latent_channels, int64_t n_spatial, void* out,
                                       int32_t dtype, s2v_stream stream) {
    S2V_REQUIRE(moments && noise && out && latent_channels > 0 && n_spatial > 0, "s2v_vae_gaussian_sample: bad argument");
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_vae_gaussian_sample: unsupported dtype");
    return launch_gaussian_sample(moments, noise, (int64_t)latent_channels * n_spatial, out, dtype, (hipStream_t)stream);
}

#ifdef S2V_DIAG
// =====================================================================================================================
// ONE convolution layer of a handle, as decode_batch / encode_batch issue it (tests/test_gpu_vae_conv_exact.py, oracle/vae_conv_cases.py):
// the product's capacity call, set_layout's ring clearing, one launch_* producer from a caller-owned source, run_conv / run_conv_down
// with their cache copies and kernel choice, launch_to_ncfhw where conv_out did not run as the direct kernel.  Nothing here builds a
// GemmArgs.  Diagnostics build only.
static ConvL* conv_by_index(s2v_vae* v, int index) {
    ConvL* hit = nullptr;
    int i = 0;
    for_each_conv(v, [&](ConvL& c) { if (i++ == index) hit = &c; });
    return hit;
}
// out = {cin, cout, kt, level, number of convolutions of the handle}
extern "C" __attribute__((visibility("default"))) int s2v_diag_vae_conv_info(s2v_vae* v, int32_t index, int32_t* out) {
    S2V_REQUIRE(v && out, "s2v_diag_vae_conv_info: null argument");
    int n = 0;
    for_each_conv(v, [&](ConvL&) { n++; });
    const ConvL* c = conv_by_index(v, index);
    S2V_REQUIRE(c, "s2v_diag_vae_conv_info: no convolution of that index");
    out[0] = c->cin; out[1] = c->cout; out[2] = c->kt; out[3] = c->level; out[4] = n;
    return 0;
}
// the workspace for level-0 windows up to th x tw and `frames` frames per batch: prepare_tile_capacity (decoder) / enc_prepare (encoder)
extern "C" __attribute__((visibility("default"))) int s2v_diag_vae_conv_prepare(s2v_vae* v, int32_t th, int32_t tw, int32_t frames) {
    S2V_REQUIRE(v && th >= 1 && tw >= 1 && frames >= 1, "s2v_diag_vae_conv_prepare: bad argument");
    if (v->encoder) return enc_prepare(v, th, tw, frames);
    S2V_TRY(prepare_tile_capacity(v, th, tw, frames));
    ws_activate(v, 0);
    return 0;
}
enum { DIAG_PROD_DENSE2 = 0, DIAG_PROD_DENSE0 = 1, DIAG_PROD_UP = 2, DIAG_PROD_UP_CT = 3, DIAG_PROD_POOL = 4, DIAG_PROD_IMAGE = 5 };
/* p: 0 layer (for_each_conv order)   1..3 F, H, W of the SOURCE as the producer takes it (upsample: before the doubling; time pool: before
 *    the pooling; otherwise the convolution's own)   4 first   5 epilogue (EPI_BIAS / EPI_BIAS_ADD with `resid`)   6 producer (DIAG_PROD_*)
 *    7..12 image window: Fall, fs, Himg, Wimg, y0, x0   13 output: 0 dense rows [M][cout], 1 the [cout][Ftot][H][W] tile   14 Ftot   15 f0
 *    16 fill: 0 none, 1 a 16-bit, 2 a 32-bit pattern over the layer's whole operand buffer BEFORE the ring is cleared and the producer runs
 *    17 the pattern   18 stride 2 (run_conv_down)
 * info: 0 the direct kernel ran   1 route of the GEMM (1 bf16 MFMA, 2 fp16 MFMA, 3 gemm_f32m, 4 the generic kernel; 0 none)
 *    2..4 F, H, W of the convolution's operand   5 output rows M */
extern "C" __attribute__((visibility("default"))) int s2v_diag_vae_conv_run(s2v_vae* v, const int32_t* p, const void* src, const void* resid, void* out,
                                                                             int32_t* info, s2v_stream stream) {
    S2V_REQUIRE(v && p && src && out && info, "s2v_diag_vae_conv_run: null argument");
    // run_conv's A/B switches of the diagnostics build would change what runs or what it returns
    S2V_REQUIRE(!getenv("S2V_VAE_NO_DIRECT_CONV_OUT") && !getenv("S2V_VAE_ADD_EXPERIMENT"), "s2v_diag_vae_conv_run: unset S2V_VAE_NO_DIRECT_CONV_OUT and S2V_VAE_ADD_EXPERIMENT");
    ConvL* cp = conv_by_index(v, p[0]);
    S2V_REQUIRE(cp, "s2v_diag_vae_conv_run: no convolution of that index");
    ConvL& c = *cp;
    hipStream_t st = (hipStream_t)stream;
    const int prod = p[6], epi = p[5], stride2 = p[18];
    int F = p[1], H = p[2], W = p[3];
    S2V_REQUIRE(F >= 1 && H >= 1 && W >= 1, "s2v_diag_vae_conv_run: bad geometry");
    S2V_REQUIRE(c.kt == 3 || c.kt == 1, "s2v_diag_vae_conv_run: a 1 x 1 shortcut is no convolution layer");
    S2V_REQUIRE(prod >= DIAG_PROD_DENSE2 && prod <= DIAG_PROD_IMAGE, "s2v_diag_vae_conv_run: unknown producer");
    S2V_REQUIRE((c.kt == 3) == (prod == DIAG_PROD_DENSE2 || prod == DIAG_PROD_IMAGE), "s2v_diag_vae_conv_run: a causal layer's operand starts at frame 2, a per-frame layer's at frame 0");
    S2V_REQUIRE(epi == EPI_BIAS || (epi == EPI_BIAS_ADD && resid), "s2v_diag_vae_conv_run: EPI_BIAS, or EPI_BIAS_ADD with a residual");
    if (prod == DIAG_PROD_UP || prod == DIAG_PROD_UP_CT) { F = up_frames(F, prod == DIAG_PROD_UP_CT); H *= 2; W *= 2; }
    if (prod == DIAG_PROD_POOL) { S2V_REQUIRE(F > 1, "s2v_diag_vae_conv_run: the time pool takes more than one frame"); F = down_frames(F, 1); }
    if (stride2) S2V_REQUIRE(c.kt == 1 && H % 2 == 0 && W % 2 == 0 && epi == EPI_BIAS && p[13] == 0, "s2v_diag_vae_conv_run: stride 2 is a per-frame layer on even sides, bias only, dense rows");
    // the level-0 window whose layout puts H x W at this layer's level, and the capacity of the workspace
    const int th = v->encoder ? H << c.level : H >> c.level, tw = v->encoder ? W << c.level : W >> c.level;
    S2V_REQUIRE(v->th > 0 && c.pad, "s2v_diag_vae_conv_run: no workspace (s2v_diag_vae_conv_prepare)");
    S2V_REQUIRE(th >= 1 && tw >= 1 && th <= v->th && tw <= v->tw, "s2v_diag_vae_conv_run: window beyond the workspace's capacity");
    const Operand o = operand_extent(v, c, th, tw, v->fmax);
    S2V_REQUIRE(o.H == H && o.W == W, "s2v_diag_vae_conv_run: the sides are no window of this layer's level");
    S2V_REQUIRE(F <= o.frames && o.padded_bytes(v, c) + 1024 <= c.pad_bytes, "s2v_diag_vae_conv_run: frames beyond the workspace's capacity");
    if (prod == DIAG_PROD_POOL) S2V_REQUIRE(p[1] <= o.frames, "s2v_diag_vae_conv_run: frames beyond the workspace's capacity");
    if (p[16]) {
        S2V_REQUIRE((p[16] == 1 || p[16] == 2) && c.pad_bytes % 4 == 0, "s2v_diag_vae_conv_run: the fill is a 16- or a 32-bit pattern");
        if (p[16] == 1) S2V_CHECK_HIP(hipMemsetD16Async((hipDeviceptr_t)c.pad, (unsigned short)p[17], (size_t)c.pad_bytes / 2, st));
        else S2V_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)c.pad, p[17], (size_t)c.pad_bytes / 4, st));
        v->cur_h = v->cur_w = 0;  // no ring is valid any more
    }
    S2V_TRY(set_layout(v, th, tw, st, !v->encoder));  // as decode_window / encode_window
    switch (prod) {
        case DIAG_PROD_DENSE2: S2V_TRY(launch_dense_to_padded(src, F, H, W, c.cin, c.pad, 2, v->dtype, st)); break;
        case DIAG_PROD_DENSE0: S2V_TRY(launch_dense_to_padded(src, F, H, W, c.cin, c.pad, 0, v->dtype, st)); break;
        case DIAG_PROD_UP: case DIAG_PROD_UP_CT: S2V_TRY(launch_upsample(src, p[1], p[2], p[3], c.cin, prod == DIAG_PROD_UP_CT, c.pad, v->dtype, st)); break;
        case DIAG_PROD_POOL: S2V_TRY(launch_time_pool_to_padded(src, p[1], H, W, c.cin, c.pad, v->dtype, st)); break;
        default:
            S2V_REQUIRE(p[11] >= 0 && p[12] >= 0 && p[11] + H <= p[9] && p[12] + W <= p[10], "s2v_diag_vae_conv_run: the window leaves the image");
            S2V_TRY(launch_image_to_padded(src, c.cin, F, p[7], p[8], p[9], p[10], p[11], p[12], H, W, c.pad, 2, v->dtype, st));
    }
    bool direct = false;
    g_vae_diag_route = 0;
    const int M = stride2 ? F * (H / 2) * (W / 2) : F * H * W;
    if (stride2) S2V_TRY(run_conv_down(v, c, F, H, W, out, st));
    else if (p[13] == 0) S2V_TRY(run_conv(v, c, F, H, W, p[4] != 0, epi, resid, out, st));
    else {
        S2V_REQUIRE(p[15] >= 0 && p[15] + F <= p[14], "s2v_diag_vae_conv_run: the frames leave the tile");
        S2V_REQUIRE((int64_t)M * c.cout * v->esz + (int64_t)256 * 1024 * v->esz <= v->dense_bytes, "s2v_diag_vae_conv_run: rows beyond the dense buffers");
        S2V_TRY(run_conv(v, c, F, H, W, p[4] != 0, epi, resid, v->dense[1], st, (char*)out, p[14], p[15], &direct));
        if (!direct) S2V_TRY(launch_to_ncfhw(v->dense[1], F, H, W, c.cout, out, p[14], p[15], v->dtype, st));
    }
    info[0] = direct; info[1] = g_vae_diag_route; info[2] = F; info[3] = H; info[4] = W; info[5] = M;
    return 0;
}
#endif
