// C ABI of libs2v_hip.so (see include/s2v_hip.h): context, weight ingest / re-packing, workspace, and the launch
// sequences of the transformer forward, the block / attention seams and the fused denoise step.
#define S2V_HOST
#include "common.h"
#include "kernels.h"
#include "../../include/s2v_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

thread_local std::string g_s2v_err;
int s2v_fail(const char* file, int line, const char* msg, int code) {
    char buf[512];
    snprintf(buf, sizeof(buf), "%s:%d: %s", file, line, msg);
    g_s2v_err = buf;
    return code;
}

static inline int64_t rup(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

struct Slot {
    char* dst = nullptr;   // destination inside the arena
    int64_t rows = 0, cols = 0, ld = 0;
    bool loaded = false;
    // runtime LoRA (lora_runtime_rank > 0): how s2v_lora_attach reaches this weight -- LORA_BRANCH: the adapter branch runs beside the base
    // weight (s * B in the tail columns [tail_col, tail_col + lr) of the weight's rows, A in rows of the layer's A stack at lora_a);
    // LORA_REMERGE: the live slot is rebuilt from the context's base copy with the merge arithmetic of s2v_merge_lora
    int lora = 0;
    char* lora_a = nullptr;
    int64_t tail_col = 0;
    // fp8 weight formats with lora_runtime_fp8: e4m3 rows take no 16-bit tail, so rnd(s * B) goes into an array of its own, rows lr_fp8 apart
    char* lora_bs = nullptr;
};
enum { LORA_NONE = 0, LORA_BRANCH = 1, LORA_REMERGE = 2 };

// the four big linears of a block.  What any site needs to know about one of them -- its shape, how many adapters share it, its state-dict
// names -- is lin_shape()'s; what a layer stores for it is a LinW
enum { LIN_QKV, LIN_OUT, LIN_FF1, LIN_FF2, LIN_NUM };
struct LinShape {
    int64_t N, K;          // output rows, depth
    int parts;             // adapters side by side in the output columns (q | k | v of the fused QKV), N / parts rows each
    const char* stem[3];   // state-dict name of each part, inside "transformer_blocks.<l>."
    int64_t n_pad() const { return rup(N, 256); }                    // weight rows are padded to the 256-column GEMM tile (zero rows)
    int64_t pitch(int64_t lr) const { return K + parts * lr; }       // runtime LoRA: every part gets lr zero tail columns, ld = K + R
    int lora_seg() const { return parts > 1 ? (int)(N / parts) : 0; }  // GemmArgs::lora_seg: output columns per adapter, 0 = one adapter
};
static LinShape lin_shape(int which, int64_t D) {
    switch (which) {
    case LIN_QKV: return {3 * D, D, 3, {"attn1.to_q", "attn1.to_k", "attn1.to_v"}};
    case LIN_OUT: return {D, D, 1, {"attn1.to_out.0"}};
    case LIN_FF1: return {4 * D, D, 1, {"ff.net.0.proj"}};
    default: return {D, 4 * D, 1, {"ff.net.2"}};
    }
}
struct LinW {
    char *w = nullptr, *b = nullptr;   // weight [n_pad][pitch] and bias [N], model dtype
    char* a = nullptr;                 // runtime LoRA: the A stack, model dtype, zero without an adapter: [parts (lr + flr)][K]
    char* bs = nullptr;                // runtime LoRA beside e4m3 weights (s2v_ctx::flr > 0): Bs = rnd(s * B), model dtype, [n_pad][flr], zero without an adapter
    char* q = nullptr;                 // weight_format 1: the e4m3 copy [n_pad][K] + per-output-channel scales (quantised at finalize)
    float* s = nullptr;
};

struct LayerW {
    char *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    char *nq_w, *nq_b, *nk_w, *nk_b;
    LinW lin[LIN_NUM];
};

struct GraphKey {
    void* latents; float* x0; const void* noise;
    int slot;   // -1: the whole step (s2v_denoise_step); 0 / 1: the forward-only graph of s2v_denoise_split_begin writing that half of the CFG pair
    const void *z0 = nullptr, *noise0 = nullptr, *mask = nullptr;   // the blend operands of the masked step (s2v_denoise_step_masked); null: unmasked
    int mode = 0;   // S2V_STEP_*: the step-cache mode the forward was captured in; every mode has an executable of its own (launch_captured)
    uint64_t amask = 0;   // s2v_attn_map_arm: the layers whose attention the mass kernel follows in this step; every mask has an executable of its own
    uint64_t smask = 0;   // s2v_attn_steer_arm: the layers whose attention launch is the steered kernel in this step; an executable per mask as well
    int triple = 0;       // s2v_denoise_step_guided: the step of [u | r | f] triples, whose last kernel is another one than the pair step's
    int windows = 0;      // s2v_denoise_step_windows: every forward and blend of a long latent's windows, then one scheduler step on the whole of it
    int rescale = 0;      // s2v_set_guidance_rescale armed: two more launches and another last kernel, so an armed and an un-armed step never replay each other
    bool same_but_mode(const GraphKey& o) const {
        return latents == o.latents && x0 == o.x0 && noise == o.noise && slot == o.slot && z0 == o.z0 && noise0 == o.noise0 && mask == o.mask && triple == o.triple &&
               windows == o.windows && rescale == o.rescale;
    }
    uint64_t lmask = 0;   // s2v_attn_local_arm: the layers whose attention launch is the local kernel in this step; an executable per mask as well
    int lkind = 0;        // ... and the kind of the table those layers read (0 a window table, 1 a box table): the kernel choice is baked into the executable
    bool operator==(const GraphKey& o) const { return same_but_mode(o) && mode == o.mode && amask == o.amask && smask == o.smask && lmask == o.lmask && lkind == o.lkind; }
    bool armed() const { return amask != 0 || smask != 0 || lmask != 0; }
};

// kernel classes of the per-class timing (ProfScope, s2v_profile_*): 8 = the Ulysses packs / unpacks, 9 = the LoRA down-projections
enum { PK_QKV = 0, PK_ATTN = 1, PK_OUT = 2, PK_FF1 = 3, PK_FF2 = 4, PK_LNMOD = 5, PK_QKNORM = 6, PK_OTHER = 7, PK_SHARD = 8, PK_LORA = 9, PK_NUM = 10 };

struct s2v_ctx {
    s2v_model_config cfg;
    int kind = S2V_CTX_MODEL;    // cfg.reserved[0]: a model, attention weights only, or geometry + workspace only (include/s2v_hip.h)
    int D = 0, L = 0, dtype = 0, esz = 0, temb = 0;
    bool mfma = false;
    int attn_order = 0;          // AttnArgs::order (S2V_ATTN_ORDER at s2v_create of the DIAGNOSTICS build: an experiment knob, 0 in the product)
    int attn_stagger = 0;        // AttnArgs::stagger (S2V_ATTN_STAGGER, same: 0 in the product)
    bool h16 = false;            // fp16 model dtype: linears on v_mfma_f32_32x32x16_f16 (gemm_f16), attention on attn_f32m<f16_t>
    int mc = 6;                  // modulation chunks per norm{1,2}.linear in the stack: 6, or 9 under lora_adaln_scope = 1 (+ the
                                 // reference-image copy of chunks 0-2: cond_shift, cond_scale, cond_gate)
    float* lora_tmp = nullptr;   // fp32 scratch of s2v_merge_lora
    size_t lora_tmp_bytes = 0;
    bool fp8 = false;            // cfg.weight_format == 1 or 2
    bool attn_p16 = false;       // cfg.attn_p_format == 1: P / V^T of the four-wave attention kernels in fp16 (AttnArgs::p16)
    bool fp8_qk = false;         // cfg.weight_format == 2: additionally q / k as MX e4m3 and QK^T on the scaled fp8 MFMA (attn_q4f)
    unsigned char *q8 = nullptr, *k8 = nullptr; unsigned short* q8s = nullptr; unsigned* k8s = nullptr;  // workspace (fp8_qk): AttnArgs::q8 ... k8s
    char* aq = nullptr;          // workspace: e4m3 activations [Mpad][4D] of the GEMM being fed
    float* aq_scale = nullptr;   // workspace: their per-token scales [Mpad]
    unsigned char *hq = nullptr, *hs = nullptr;  // workspace (fp8): GELU(FF1) as MX e4m3 [Mpad][4D] + block scales [Mpad][4D / 32]
    bool finalized = false;
    // runtime LoRA (cfg.reserved[1] = lora_runtime_rank; include/s2v_hip.h).  lr > 0: the four adapted linears of every block are carved with
    // ld = K + R (R = 3 lr for the fused QKV, lr otherwise), Xn / Hb rows have room for T = x . A^T behind column K, and with an adapter
    // attached every adapted GEMM runs with K' = K + R after a down-projection (lora.hip) has written T
    int lora_cap = 0;            // the rank asked for (0: mode off)
    int lr = 0;                  // lora_cap padded to what the GEMM dispatch needs (64, or 128 when D % 128 == 0); 0 with the mode off / fp8
    // fp8 weight formats with S2V_LORA_FP8_BRANCH: the branch runs beside the e4m3 GEMM (GemmArgs::lora_bs).  flr = lora_cap padded to 64 (the
    // down-projection's column tile; the up-projection steps by 16); the A stacks are carved with flr rows per adapter, the Bs arrays
    // (LinW::bs) [N_pad][flr], and the workspace holds T [Mpad][3 flr].  lr stays 0: nothing of the bf16 operand layout changes.
    int flr = 0;
    char* Tl = nullptr;          // workspace (flr): T = rnd(x . A^T) of the adapted GEMM being fed, rows 3 flr apart
    std::unordered_map<std::string, int> lora_names;   // attached: weight name -> rank
    int lora_rank = 0; float lora_scale = 0.f;          // of the last attach / rescale (s2v_lora_state)
    int64_t graph_captures = 0;
    // the attached state as the ARENA carries it (three words at the arena's end: names attached, rank, scale bits), so that a replica
    // whose arena was filled by a broadcast runs the adapter it received (s2v_mark_weights_loaded reads them back)
    char* lora_hdr = nullptr;
    int32_t lora_hdr_host[4] = {0, 0, 0, 0};
    int lora_replica = 0;        // names attached on the context this arena was copied from (0 on the context that attached them itself)
    bool lora_on() const { return !lora_names.empty() || lora_replica > 0; }
    char *base_mod = nullptr, *base_patch = nullptr, *base_text = nullptr;   // base copies of the re-merged weights (inside the arena)
    int64_t base_mod_bytes = 0, base_patch_bytes = 0, base_text_bytes = 0;
    // weights
    int num_cus = 256;
    int sk_tiles = 0; float* sk_ws = nullptr; unsigned* sk_cnt = nullptr;  // split-K workspace of the geometry (0: none)
    unsigned* vt_amax = nullptr;             // AttnArgs::vt_amax: VT_AMAX_WORDS words (attn_p_format 1)
    int* attn_queue = nullptr;               // nine counters of the persistent attention launch (zero between launches)
    char* kv_ws = nullptr;                   // AttnArgs::kv_ws: counters + partial slots of the KV-split q-blocks, carved with the geometry (in ws)
    int64_t kv_ws_bytes = 0;
    unsigned long long* attn_stats = nullptr;  // AttnArgs::stats: 256 x [slow paths, (wave, KV tile) pairs] of the attn_q4 launches (s2v_attn_slow_stats)
    hipStream_t side = nullptr;              // fork/join stream for the row-tail launches of split GEMMs
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    char* arena = nullptr;
    int64_t arena_bytes = 0;
    std::unordered_map<std::string, Slot> slots;
    std::vector<LayerW> layers;
    char *patch_w, *patch_b, *text_w, *text_b, *te1_w, *te1_b, *te2_w, *te2_b;
    char *nf_w, *nf_b, *no_w, *no_b, *po_w, *po_b;
    char *mod_w, *mod_b;
    int64_t mod_rows = 0;
    // geometry + workspace
    int B = 0, T = 0, F = 0, H = 0, W = 0, R = 0, V = 0, Ntok = 0, ntok_pad = 0;
    int64_t M = 0, Mpad = 0;
    char* ws = nullptr;
    int64_t ws_bytes = 0;
    char *X, *Xn, *QKV, *Hb, *VT, *e0, *e1, *patches, *tailn, *proj, *mod, *tmp_te, *emb, *noise_pred;
    float *rope_cos, *rope_sin;
    float* rope_pk = nullptr;                // [positions][cos pair 0..31 | sin pair 0..31] when the tables repeat every value twice
    bool rope_paired = false;                // (get_3d_rotary_pos_embed: repeat_interleave(2)); the fused QKV epilogue needs it
    char* pos_tab;
    bool have_rope = false, have_pos = false, have_cond = false;
    // one reference per video (s2v_set_conditioning_refs): sample j reads the tokens of reference j mod n_ref at e1_cur + (j mod n_ref) * e1_stride.
    // n_ref = 1 is the workspace's e1; more references sit in e1x, allocated by that set-up call and freed with the workspace
    int n_ref = 1;
    // what the conditioning holds: the CFG pairs [negative x b | positive x b] of s2v_set_conditioning(_refs), or the triples [u x b | r x b | f x b]
    // of s2v_set_conditioning_triples.  B = 6 is three pairs or two triples by shape alone, so every step entry asks this
    bool cond_triples = false;
    char *e1_cur = nullptr, *e1x = nullptr;
    int64_t e1_stride = 0, e1x_bytes = 0;
    float* t_dev = nullptr;
    SchedCoef* coef_dev = nullptr;
    SchedBlend* blend_dev = nullptr;   // the masked step's blend record per video, uploaded beside the coefficient sets
    // masked video-to-video (s2v_set_blend): the call's clean latents, start noise and latent masks (levels) of blend_b videos; held, not copied
    const void *blend_z0 = nullptr, *blend_noise0 = nullptr;
    const unsigned char* blend_mask = nullptr;
    int blend_b = 0;
    // pinned staging ring for per-step scalars: a timestep per sample, a coefficient set and (masked step) a blend record per video
    struct Stage { float t[S2V_MAX_BATCH]; SchedCoef c[S2V_MAX_BATCH / 2]; SchedBlend bl[S2V_MAX_BATCH / 2]; };
    Stage* ring = nullptr;
    int ring_pos = 0;
    // graph
    hipStream_t cap_stream = nullptr;
    // one executable per step-cache mode (GraphKey::mode); the held ones differ in nothing but the mode
    hipGraphExec_t gexec[3] = {nullptr, nullptr, nullptr};
    GraphKey gkey[3] = {{nullptr, nullptr, nullptr, -1}, {nullptr, nullptr, nullptr, -1}, {nullptr, nullptr, nullptr, -1}};
    // ... and one per (mode, layer mask) of an armed step (s2v_attn_map_arm), which is another launch sequence: never replayed for an un-armed step
    std::vector<std::pair<GraphKey, hipGraphExec_t>> gexec_armed;
    bool any_graph() const { return gexec[0] || gexec[1] || gexec[2] || !gexec_armed.empty(); }
    // attention map (include/s2v_hip.h): raw sums of the mass kernel over the armed layer launches, [am_n][B][H][V] fp32, beside the workspace
    bool am_on = false;
    int am_n = 0;                // 1 + text spans: range 0 is the reference stream [T, T + R)
    int am_k0[AM_MAX_RANGES] = {}, am_k1[AM_MAX_RANGES] = {};
    int am_spans[2 * (AM_MAX_RANGES - 1)] = {};   // the text spans as given: the ranges are re-derived when the geometry changes
    float* am_acc = nullptr;
    int64_t am_bytes = 0, am_count = 0;
    uint64_t am_arm = 0;         // the layers of the NEXT forward; am_run: of the forward that is running (run_block reads it)
    uint64_t am_run = 0;
    // attention steering (include/s2v_hip.h): the record the steered kernels read, in device memory of its own; the ranges as given, re-checked
    // and uploaded again when the geometry changes (the query range is the geometry's video rows)
    bool st_on = false;
    AttnSteerRec* st_tab = nullptr;
    int st_n = 0;
    int st_k0[ATTN_STEER_MAX_RANGES] = {}, st_k1[ATTN_STEER_MAX_RANGES] = {};
    float st_w[ATTN_STEER_MAX_RANGES] = {};
    unsigned st_mask[ATTN_STEER_MAX_RANGES] = {};
    uint64_t st_arm = 0;         // the layers of the NEXT forward; st_run: of the forward that is running (run_block reads it)
    uint64_t st_run = 0;
    // steering maps: a context holds ONE record, scalar (st_kind 0, st_tab) or maps (st_kind 1, st_map: kernels.h AttnSteerMapRec with room for
    // st_map_cap planes of st_map_V cells at st_map_Ntok tokens); the ranges, plane indices and weights as given, for a geometry change
    int st_kind = 0;
    AttnSteerMapRec* st_map = nullptr;
    int st_map_cap = 0, st_map_V = 0, st_map_Ntok = 0, st_map_np = 0, st_map_n = 0;
    int st_map_k0[ATTN_STEER_MAX_RANGES] = {}, st_map_k1[ATTN_STEER_MAX_RANGES] = {};
    signed char st_map_plane[ATTN_STEER_MAX_RANGES][ATTN_STEER_MAP_BATCH] = {};
    std::vector<float> st_map_w;
    int64_t st_bytes() const {
        return (st_tab ? (int64_t)sizeof(AttnSteerRec) : 0) + (st_map ? (int64_t)attn_steer_map_words(st_map_Ntok, st_map_V, st_map_cap) * 4 : 0);
    }
    // local attention in time (include/s2v_hip.h): the record the local kernels read (kernels.h "local attention"), in device memory of its own, sized
    // for the geometry's Ntok; la_Ntok: the Ntok it was made for
    bool la_on = false;
    int* la_tab = nullptr;
    int la_Ntok = 0;
    uint64_t la_arm = 0;         // the layers of the NEXT forward; la_run: of the forward that is running (run_block reads it)
    uint64_t la_run = 0;
    // a context holds ONE table, of either kind: la_kind 0 the window table (la_tab), 1 the box table of local attention in space and time (la_box,
    // allocated by the first s2v_attn_local_set_box and kept until the feature goes off, so that a captured step keeps its pointer)
    int la_kind = 0;
    int* la_box = nullptr;
    int64_t la_bytes() const {
        return (la_tab ? (int64_t)(attn_local_ints(la_Ntok) * sizeof(int)) : 0) + (la_box ? (int64_t)(attn_box_ints(la_Ntok) * sizeof(int)) : 0);
    }
    // step cache (include/s2v_hip.h): sc_delta holds IN between the two extra launches of a CAPTURE forward and the residual after it
    int sc_on = 0;               // s2v_step_cache_enable: 0 off, 1 the cache, 2 the cache + sc_in (IN of every forward, for the read-out)
    int sc_arm = 0;              // S2V_STEP_*: the mode of the next forward
    bool sc_valid = false;       // sc_delta is the residual of this geometry / conditioning / weights
    char *sc_delta = nullptr, *sc_in = nullptr;   // dense [B][V][D], model dtype; allocated beside the workspace, not carved from it
    int64_t sc_bytes = 0;        // of both buffers
    // temporal windows (s2v_set_windows; include/s2v_hip.h): a long latent of win_L frames stepped as win_W windows of the geometry's F frames,
    // win_s frames apart, win_pf windows per forward (B = 2 win_pf).  One allocation beside the workspace: the fp32 plane [win_L][C H W], then
    // the weights [F] and their per-frame sums [win_L]
    int win_L = 0, win_s = 0, win_pf = 0, win_W = 0;
    float *win_acc = nullptr, *win_w = nullptr, *win_wsum = nullptr;
    int64_t win_bytes = 0;
    // guidance rescale (s2v_set_guidance_rescale; include/s2v_hip.h).  Armed <=> gr_buf: one allocation beside the workspace for the gr_b videos of the
    // geometry -- the chunk partials [gr_b][chunks][4] fp64, then the sums [4][4] fp64, the factors [4] and phi [4] fp32.  The log (rows of factors,
    // then the device-side count) is an allocation of its own that outlives a disarm: a shrinking batch arms again and goes on logging
    char* gr_buf = nullptr;
    double *gr_partials = nullptr, *gr_sums = nullptr;
    float *gr_factors = nullptr, *gr_phi = nullptr, *gr_log = nullptr;
    unsigned* gr_log_count = nullptr;
    int gr_b = 0;
    int64_t gr_bytes = 0, gr_log_bytes = 0;
    int split_kind = -1;         // scheduler kind of the s2v_denoise_split_begin that has not met its s2v_denoise_split_end yet (-1: none pending)
    // optional per-kernel-class timing with HIP events on the launch stream (bench.py's live roofline figure)
    // + shader-clock stamps (s_memtime / s_memrealtime pairs written by a one-lane kernel right before and right after every profiled launch)
    long long* clk_buf = nullptr;                    // device: CLK_SLOTS x [memtime0, realtime0, memtime1, realtime1]
    long long* clk_cur = nullptr;                    // the slot of the launch a ProfScope is open around (null outside the profile pass)
    std::vector<std::pair<int, int>> clk_rec;         // (class, slot) of every stamped launch since the last s2v_profile_read_clocks
    bool prof_on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[PK_NUM];
    size_t prof_used[PK_NUM] = {};
    // Ulysses shard (s2v_set_shard): sp ranks share one video's step.  With a shard T, R, V, Ntok, M and Mpad above are this rank's rows of
    // every sample -- the mini-sequence [T_r | R_r | V_r] -- and gT, gR, gV, gN the whole streams (equal to T, R, V, Ntok without a shard).
    bool shard = false;
    int sp = 1, sr = 0;
    int gT = 0, gR = 0, gV = 0, gN = 0;
    int t0 = 0, r0 = 0, v0 = 0;                // this rank's first row of each stream
    int Vmax = 0;                              // ceil(gV / sp): rows per sample of every rank's share of the noise all-gather
    char *QKVh = nullptr, *Oh = nullptr;       // head-sharded full-N buffers: q|k|v of head group sr [B*gN][3D/p], attention output [B*gN][D/p]
    char *sbuf = nullptr, *rbuf = nullptr;     // send / recv of the two per-block all-to-alls
    char *nsend = nullptr, *nrecv = nullptr;   // send [B][Vmax][Cout] / recv [sp][B][Vmax][Cout] of the noise all-gather
    char* proj_full = nullptr;                 // the gathered projection [B][gV][Cout]
    int *rmap = nullptr, *nmap = nullptr;      // recv row of the QKV exchange -> global row; recv row of the noise gather -> row of proj_full (-1: pad)
    // fp8 engine (attn_mx_out): the O exchange carries the attention output as MX e4m3 -- Oh holds the bytes [B*gN][D/p], Os the block scales
    // [D/(128p)][Os_rows] (K-tile major, mx_perm_row); omap[i] / omap[Mg + i] = where send row i's bytes (in 16-byte units) / its scale dwords
    // (in dwords) sit in sbuf
    bool o_mx = false;
    unsigned char* Os = nullptr;
    int64_t Os_rows = 0;
    int* omap = nullptr;
    std::vector<int64_t> xcnt[3][4];           // per exchange kind: send counts, send displacements, recv counts, recv displacements (bytes)
    int sh_layer = 0, sh_pending = 0;          // the staged step: layer in flight, exchange the caller owes (S2V_SHARD_*)
};

static const int CLK_SLOTS = 8192;
// shader clock of the profiled launches: ProfScope hands the launch a slot of clk_buf (s2v_ctx::clk_cur -> GemmArgs::clk / AttnArgs::clk); one
// designated workgroup of the kernel stamps s_memtime / s_memrealtime at its entry and exit (common.h clk_stamp).  Kernels without stamps (or
// launches whose designated workgroup left early) leave the slot zero and are skipped.
#define S2V_FP8_QK_AUTO_TOKENS 40000

struct ProfScope {
    s2v_ctx* c; int k; hipStream_t st; bool on;
    ProfScope(s2v_ctx* c_, int k_, hipStream_t st_) : c(c_), k(k_), st(st_) {
        on = c->prof_on && st != c->cap_stream;
        if (!on) return;
        if (c->prof_used[k] == c->prof_ev[k].size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            c->prof_ev[k].push_back({a, b});
        }
        if (c->clk_buf && (int)c->clk_rec.size() < CLK_SLOTS) {
            slot = (int)c->clk_rec.size();
            c->clk_rec.push_back({k, slot});
            c->clk_cur = c->clk_buf + 4 * slot;
        }
        (void)hipEventRecord(c->prof_ev[k][c->prof_used[k]].first, st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(c->prof_ev[k][c->prof_used[k]].second, st);
        c->clk_cur = nullptr;
        c->prof_used[k]++;
    }
    int slot = -1;
};

static const int RING = 256;

// ------------------------------------------------------------------------------------------------------
extern "C" const char* s2v_last_error(void) { return g_s2v_err.c_str(); }
extern "C" const char* s2v_version(void) { return "s2v_hip 0.1 (gfx950)"; }

static Slot* add_slot(s2v_ctx* c, const std::string& name, char* dst, int64_t rows, int64_t cols, int64_t ld) {
    Slot s;
    s.dst = dst; s.rows = rows; s.cols = cols; s.ld = ld;
    c->slots[name] = s;
    return &c->slots[name];
}

// the keys of the first nlin linears of layer l, and with the QKV the per-head LayerNorm(64) of q and k.  A linear of several parts (the fused
// QKV) is one weight [rup(N, 256)][K + R] whose parts own N / parts rows each
static void add_linear_slots(s2v_ctx* c, int l, const LayerW& w, int nlin) {
    const int64_t E = c->esz, lr = c->lr;
    const int64_t fl = c->flr, la = lr + fl;  // fp8 branch: part p's rnd(s * B_p) sits in its own rows of the Bs array
    char nm[160];
#define NM(fmt, ...) (snprintf(nm, sizeof(nm), "transformer_blocks.%d." fmt, l, ##__VA_ARGS__), std::string(nm))
    for (int i = 0; i < nlin; ++i) {
        const LinShape s = lin_shape(i, c->D);
        const LinW& x = w.lin[i];
        const int64_t n = s.N / s.parts, ld = s.pitch(lr);
        for (int p = 0; p < s.parts; ++p) {
            Slot* sl = add_slot(c, NM("%s.weight", s.stem[p]), x.w + p * n * ld * E, n, s.K, ld);
            add_slot(c, NM("%s.bias", s.stem[p]), x.b + p * n * E, 1, n, n);
            if (!la) continue;
            // block-diagonal tail: part p keeps s * B_p in the tail columns [p lr, (p + 1) lr) of its own rows, zeros elsewhere
            sl->lora = LORA_BRANCH; sl->lora_a = x.a + p * la * s.K * E; sl->tail_col = s.K + p * lr;
            if (fl) sl->lora_bs = x.bs + p * n * fl * E;
        }
    }
    add_slot(c, NM("attn1.norm_q.weight"), w.nq_w, 1, 64, 64);
    add_slot(c, NM("attn1.norm_q.bias"), w.nq_b, 1, 64, 64);
    add_slot(c, NM("attn1.norm_k.weight"), w.nk_w, 1, 64, 64);
    add_slot(c, NM("attn1.norm_k.bias"), w.nk_b, 1, 64, 64);
#undef NM
}

// lora_runtime_rank (cfg.reserved[1], 0 .. 128: s2v_create) -> the padded rank the layout is carved for
static void lora_setup(s2v_ctx* c) {
    c->lora_cap = c->cfg.reserved[1] & S2V_LORA_RANK_MASK;
    // the fp8 weight formats keep no 16-bit operand for a branch to extend: without S2V_LORA_FP8_BRANCH nothing is carved and s2v_lora_attach
    // refuses; with it the branch gets operands of its own beside the e4m3 GEMM (s2v_ctx::flr)
    const bool fp8 = c->cfg.weight_format != 0;
    c->lr = (c->lora_cap > 0 && !fp8) ? (int)rup(c->lora_cap, c->D % 128 == 0 ? 128 : 64) : 0;
    c->flr = (c->lora_cap > 0 && fp8 && (c->cfg.reserved[1] & S2V_LORA_FP8_BRANCH)) ? (int)rup(c->lora_cap, 64) : 0;
}

// The arena's layout is one sequence of carve calls, run twice: with no arena yet (A null) a pass only adds up the sizes, with the arena it hands out
// the same pieces.  Every piece starts on a multiple of 256 bytes; a piece of no bytes is null
struct Carver {
    char* A; int64_t E; int64_t off = 0;
    char* bytes(int64_t n) { const int64_t o = off; off += rup(n, 256); return A && n ? A + o : nullptr; }
    char* operator()(int64_t elems) { return bytes(elems * E); }   // elements of the model dtype
};

// the first nlin linears of one layer: each weight followed directly by its bias, the two q/k LayerNorm pairs between bqkv and wo, then the A
// stacks and (fp8 branch) the Bs arrays.  lr: the weights get lr zero tail columns per part; flr: no tail columns, A stacks of flr rows per adapter
// and the Bs arrays instead
static void carve_linears(const s2v_ctx* c, Carver& cv, LayerW& w, int nlin) {
    const int64_t la = c->lr + c->flr;
    for (int i = 0; i < nlin; ++i) {
        const LinShape s = lin_shape(i, c->D);
        w.lin[i].w = cv(s.n_pad() * s.pitch(c->lr)); w.lin[i].b = cv(s.N);
        if (i == LIN_QKV) { w.nq_w = cv(64); w.nq_b = cv(64); w.nk_w = cv(64); w.nk_b = cv(64); }
    }
    for (int i = 0; i < nlin; ++i) { const LinShape s = lin_shape(i, c->D); w.lin[i].a = cv(s.parts * la * s.K); }
    for (int i = 0; i < nlin; ++i) w.lin[i].bs = cv(lin_shape(i, c->D).n_pad() * c->flr);
}

// S2V_CTX_ATTN_WEIGHTS: an arena of num_layers x the attn1 weights, carved exactly as a model carves them (zero pad rows included), so that a
// workspace context runs them through the same GEMM tiles; no stream, event, scratch or workspace of its own
static int create_attn_weights(s2v_ctx* c) {
    c->layers.assign(c->L, LayerW{});
    auto layout = [&]() {
        Carver cv{c->arena, c->esz};
        for (LayerW& w : c->layers) carve_linears(c, cv, w, LIN_OUT + 1);
        c->lora_hdr = cv(c->lr ? 128 : 0);
        return cv.off;
    };
    c->arena_bytes = layout();
    S2V_CHECK_HIP(hipMalloc((void**)&c->arena, c->arena_bytes));
    S2V_CHECK_HIP(hipMemset(c->arena, 0, c->arena_bytes));
    layout();
    for (int l = 0; l < c->L; ++l) add_linear_slots(c, l, c->layers[l], LIN_OUT + 1);
    return 0;
}

// the host-side scratch every context that runs launches needs: step scalars, the pinned staging ring, the capture stream
static bool create_tail(s2v_ctx* c) {
    hipMalloc((void**)&c->t_dev, S2V_MAX_BATCH * sizeof(float));
    hipMalloc((void**)&c->coef_dev, sizeof(SchedCoef) * (S2V_MAX_BATCH / 2));
    hipMalloc((void**)&c->blend_dev, sizeof(SchedBlend) * (S2V_MAX_BATCH / 2));
    hipHostMalloc((void**)&c->ring, sizeof(s2v_ctx::Stage) * RING);
    hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking);
    return c->t_dev && c->coef_dev && c->blend_dev && c->ring && c->cap_stream;
}

extern "C" int s2v_create(const s2v_model_config* cfg, s2v_ctx** out) {
    S2V_REQUIRE(cfg && out, "s2v_create: null argument");
    const int kind = cfg->reserved[0];
    S2V_REQUIRE(kind == S2V_CTX_MODEL || kind == S2V_CTX_ATTN_WEIGHTS || kind == S2V_CTX_ATTN_WORKSPACE,
                "s2v_create: reserved[0] must be S2V_CTX_MODEL, S2V_CTX_ATTN_WEIGHTS or S2V_CTX_ATTN_WORKSPACE");
    S2V_REQUIRE(kind == S2V_CTX_MODEL || cfg->weight_format == 0, "s2v_create: attention-only contexts hold the model dtype (weight_format 0)");
    S2V_REQUIRE(cfg->dtype == S2V_DTYPE_F32 || cfg->dtype == S2V_DTYPE_BF16 || cfg->dtype == S2V_DTYPE_F16, "s2v_create: unsupported dtype");
    S2V_REQUIRE(cfg->patch_size == 2, "s2v_create: patch_size must be 2");
    S2V_REQUIRE(cfg->num_layers > 0 && cfg->num_heads > 0, "s2v_create: bad model size");
    S2V_REQUIRE(cfg->in_channels * 4 <= 4096 && cfg->out_channels > 0, "s2v_create: bad channel count");
    // everything that depends on the configuration alone is refused here, before anything is allocated
    S2V_REQUIRE(cfg->reserved[1] >= 0 && (cfg->reserved[1] & ~(S2V_LORA_RANK_MASK | S2V_LORA_FP8_BRANCH)) == 0 && (cfg->reserved[1] & S2V_LORA_RANK_MASK) <= 128,
                "s2v_create: lora_runtime_rank (reserved[1]) must be 0 .. 128, optionally with the flag S2V_LORA_FP8_BRANCH");
    const int Dc = cfg->num_heads * 64;
    const bool mfma = cfg->dtype == S2V_DTYPE_BF16 && !cfg->force_simple;
    if (kind == S2V_CTX_ATTN_WEIGHTS) {
        S2V_REQUIRE(Dc <= 4096 && Dc % 8 == 0, "s2v_create: bad inner dim");
    } else {
        S2V_REQUIRE(Dc <= 4096, "s2v_create: D > 4096 unsupported");
        S2V_REQUIRE(cfg->time_embed_dim % 8 == 0 && Dc % 8 == 0, "bad dims");
        S2V_REQUIRE(cfg->lora_adaln_scope == 0 || cfg->lora_adaln_scope == 1, "s2v_create: lora_adaln_scope must be 0 or 1");
        S2V_REQUIRE(cfg->attn_p_format == 0 || cfg->attn_p_format == 1, "s2v_create: attn_p_format must be 0 (bf16) or 1 (fp16)");
        S2V_REQUIRE(cfg->weight_format >= 0 && cfg->weight_format <= 3, "s2v_create: weight_format must be 0, 1, 2 or 3");
        S2V_REQUIRE(cfg->weight_format == 0 || (mfma && Dc % 128 == 0),
                    "s2v_create: weight_format 1 / 2 (fp8) needs the bf16 MFMA path and inner_dim % 128 == 0");
    }
    s2v_ctx* c = new s2v_ctx();
    c->cfg = *cfg;
    c->D = Dc;
    c->L = cfg->num_layers;
    c->dtype = cfg->dtype;
    c->esz = cfg->dtype == S2V_DTYPE_F32 ? 4 : 2;
    c->temb = cfg->time_embed_dim;
    c->kind = kind;
    lora_setup(c);
    {
        int dev = 0, ncu = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
            c->num_cus = ncu;
    }
    if (kind == S2V_CTX_ATTN_WEIGHTS) {
        const int r = create_attn_weights(c);
        if (r) { s2v_destroy(c); return r; }
        *out = c;
        return 0;
    }
    // the one exit of a failed allocation below
    auto fail = [&](const char* msg) { s2v_destroy(c); return s2v_fail(__FILE__, __LINE__, msg, -2); };
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess)
        return fail("s2v_create: stream / event creation failed");
    c->mfma = mfma;
    c->h16 = (cfg->dtype == S2V_DTYPE_F16) && !cfg->force_simple;
#ifdef S2V_DIAG  // experiment knobs of the diagnostics build only; clamped: slot * stagger * 64 cycles of s_sleep per launch
    if (const char* e = getenv("S2V_ATTN_STAGGER")) c->attn_stagger = std::min(std::max(atoi(e), 0), 64);
    if (const char* e = getenv("S2V_ATTN_ORDER")) c->attn_order = atoi(e) ? 1 : 0;
#endif
    if (hipMalloc((void**)&c->attn_stats, 4096) != hipSuccess || hipMemset(c->attn_stats, 0, 4096) != hipSuccess)
        return fail("s2v_create: attention census allocation failed");
    if (hipMalloc((void**)&c->vt_amax, sizeof(unsigned) * VT_AMAX_WORDS) != hipSuccess || hipMemset(c->vt_amax, 0, sizeof(unsigned) * VT_AMAX_WORDS) != hipSuccess)
        return fail("s2v_create: V^T magnitude words allocation failed");
    if (hipMalloc((void**)&c->attn_queue, 64) != hipSuccess || hipMemset(c->attn_queue, 0, 64) != hipSuccess)
        return fail("s2v_create: attention queue allocation failed");

    const int64_t D = c->D, E = c->esz, L = c->L, TE = c->temb;
    const int64_t Kp = cfg->in_channels * 4, Cout = cfg->out_channels * 4, TX = cfg->text_embed_dim;
    const int64_t Dp = rup(D, 256);  // weight rows are padded to the 256-column GEMM tile (zero rows)
    const int64_t la = c->lr + c->flr;
    c->mc = cfg->lora_adaln_scope ? 9 : 6;
    const int64_t MC = c->mc;
    c->mod_rows = 2 * L * MC * D + 2 * D;
    c->base_mod_bytes = la ? c->mod_rows * TE * E : 0; c->base_patch_bytes = la ? Dp * Kp * E : 0; c->base_text_bytes = la ? Dp * TX * E : 0;
    c->fp8 = cfg->weight_format >= 1 && cfg->weight_format <= 3;
    c->fp8_qk = cfg->weight_format == 2;
    c->attn_p16 = cfg->attn_p_format == 1;
    if (kind == S2V_CTX_ATTN_WORKSPACE) {  // no arena: the weights come from another context (s2v_attn_forward_with)
        if (!create_tail(c)) return fail("s2v_create: allocation failed");
        *out = c;
        return 0;
    }
    c->layers.assign(L, LayerW{});
    // two passes: size, then carve
    auto layout = [&]() {
        Carver cv{c->arena, E};
        for (LayerW& w : c->layers) {
            w.ln1_w = cv(D); w.ln1_b = cv(D); w.ln2_w = cv(D); w.ln2_b = cv(D);
            carve_linears(c, cv, w, LIN_NUM);
        }
        c->patch_w = cv(Dp * Kp); c->patch_b = cv(D);
        c->text_w = cv(Dp * TX); c->text_b = cv(D);
        c->te1_w = cv(TE * D); c->te1_b = cv(TE); c->te2_w = cv(TE * TE); c->te2_b = cv(TE);
        c->nf_w = cv(D); c->nf_b = cv(D); c->no_w = cv(D); c->no_b = cv(D);
        c->po_w = cv(rup(Cout, 256) * D); c->po_b = cv(Cout);
        c->mod_w = cv(c->mod_rows * TE); c->mod_b = cv(c->mod_rows);
        // runtime LoRA: base copies of the weights an attach re-merges (every norm{1,2}.linear of the modulation stack, patch_embed.proj,
        // patch_embed.text_proj), filled by s2v_finalize_weights
        c->base_mod = cv(c->base_mod_bytes / E); c->base_patch = cv(c->base_patch_bytes / E); c->base_text = cv(c->base_text_bytes / E);
        c->lora_hdr = cv(la ? 128 : 0);
        // fp8 copies live in the same arena (one broadcast replicates everything a replica needs)
        for (LayerW& w : c->layers) {
            if (!c->fp8) break;
            for (int i = 0; i < LIN_NUM; ++i) { const LinShape s = lin_shape(i, D); w.lin[i].q = cv.bytes(s.n_pad() * s.K); }
            for (int i = 0; i < LIN_NUM; ++i) w.lin[i].s = (float*)cv.bytes(lin_shape(i, D).n_pad() * 4);
        }
        return cv.off;
    };
    c->arena_bytes = layout();
    hipError_t e = hipMalloc((void**)&c->arena, c->arena_bytes);
    if (e == hipSuccess) e = hipMemset(c->arena, 0, c->arena_bytes);
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    layout();
    char nm[160];
    for (int l = 0; l < L; ++l) {
        const LayerW& w = c->layers[l];
#define NM(fmt) (snprintf(nm, sizeof(nm), "transformer_blocks.%d." fmt, l), std::string(nm))
        add_slot(c, NM("norm1.norm.weight"), w.ln1_w, 1, D, D);
        add_slot(c, NM("norm1.norm.bias"), w.ln1_b, 1, D, D);
        add_slot(c, NM("norm2.norm.weight"), w.ln2_w, 1, D, D);
        add_slot(c, NM("norm2.norm.bias"), w.ln2_b, 1, D, D);
        add_linear_slots(c, l, w, LIN_NUM);
        add_slot(c, NM("norm1.linear.weight"), c->mod_w + (int64_t)(2 * l) * MC * D * TE * E, 6 * D, TE, TE)->lora = la ? LORA_REMERGE : LORA_NONE;
        add_slot(c, NM("norm1.linear.bias"), c->mod_b + (int64_t)(2 * l) * MC * D * E, 1, 6 * D, 6 * D);
        add_slot(c, NM("norm2.linear.weight"), c->mod_w + (int64_t)(2 * l + 1) * MC * D * TE * E, 6 * D, TE, TE)->lora = la ? LORA_REMERGE : LORA_NONE;
        add_slot(c, NM("norm2.linear.bias"), c->mod_b + (int64_t)(2 * l + 1) * MC * D * E, 1, 6 * D, 6 * D);
#undef NM
    }
    add_slot(c, "patch_embed.proj.weight", c->patch_w, D, Kp, Kp)->lora = la ? LORA_REMERGE : LORA_NONE;
    add_slot(c, "patch_embed.proj.bias", c->patch_b, 1, D, D);
    add_slot(c, "patch_embed.text_proj.weight", c->text_w, D, TX, TX)->lora = la ? LORA_REMERGE : LORA_NONE;
    add_slot(c, "patch_embed.text_proj.bias", c->text_b, 1, D, D);
    add_slot(c, "time_embedding.linear_1.weight", c->te1_w, TE, D, D);
    add_slot(c, "time_embedding.linear_1.bias", c->te1_b, 1, TE, TE);
    add_slot(c, "time_embedding.linear_2.weight", c->te2_w, TE, TE, TE);
    add_slot(c, "time_embedding.linear_2.bias", c->te2_b, 1, TE, TE);
    add_slot(c, "norm_final.weight", c->nf_w, 1, D, D);
    add_slot(c, "norm_final.bias", c->nf_b, 1, D, D);
    add_slot(c, "norm_out.norm.weight", c->no_w, 1, D, D);
    add_slot(c, "norm_out.norm.bias", c->no_b, 1, D, D);
    add_slot(c, "norm_out.linear.weight", c->mod_w + (int64_t)2 * L * MC * D * TE * E, 2 * D, TE, TE);
    add_slot(c, "norm_out.linear.bias", c->mod_b + (int64_t)2 * L * MC * D * E, 1, 2 * D, 2 * D);
    add_slot(c, "proj_out.weight", c->po_w, Cout, D, D);
    add_slot(c, "proj_out.bias", c->po_b, 1, Cout, Cout);
    if (!create_tail(c)) return fail("s2v_create: allocation failed");
    *out = c;
    return 0;
}

extern "C" void s2v_destroy(s2v_ctx* c) {
    if (!c) return;
    for (hipGraphExec_t g : c->gexec) if (g) hipGraphExecDestroy(g);
    for (auto& kg : c->gexec_armed) hipGraphExecDestroy(kg.second);
    if (c->am_acc) hipFree(c->am_acc);
    if (c->sc_delta) hipFree(c->sc_delta);
    if (c->sc_in) hipFree(c->sc_in);
    if (c->cap_stream) hipStreamDestroy(c->cap_stream);
    if (c->side) hipStreamDestroy(c->side);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    if (c->ring) hipHostFree(c->ring);
    if (c->coef_dev) hipFree(c->coef_dev);
    if (c->blend_dev) hipFree(c->blend_dev);
    if (c->t_dev) hipFree(c->t_dev);
    if (c->ws) hipFree(c->ws);
    if (c->e1x) hipFree(c->e1x);
    if (c->win_acc) hipFree(c->win_acc);
    if (c->gr_buf) hipFree(c->gr_buf);
    if (c->gr_log) hipFree(c->gr_log);
    if (c->st_tab) hipFree(c->st_tab);
    if (c->la_tab) hipFree(c->la_tab);
    if (c->la_box) hipFree(c->la_box);
    if (c->attn_queue) hipFree(c->attn_queue);
    if (c->vt_amax) hipFree(c->vt_amax);
    if (c->attn_stats) hipFree(c->attn_stats);
    if (c->clk_buf) hipFree(c->clk_buf);
    if (c->arena) hipFree(c->arena);
    if (c->lora_tmp) hipFree(c->lora_tmp);
    delete c;
}

// the captured step bakes in what it was captured under: whoever changes that drops the graph, and the next graph step captures again
static void drop_graph(s2v_ctx* c) {
    for (hipGraphExec_t& g : c->gexec) if (g) { hipGraphExecDestroy(g); g = nullptr; }
    for (auto& kg : c->gexec_armed) hipGraphExecDestroy(kg.second);
    c->gexec_armed.clear();
}

// attention map: the buffer follows the geometry as the step cache's does (the caller has synchronised the device and dropped the graphs)
static void am_free(s2v_ctx* c) {
    if (c->am_acc) hipFree(c->am_acc);
    c->am_acc = nullptr; c->am_bytes = 0; c->am_count = 0; c->am_arm = 0; c->am_on = false;
}
static int am_alloc(s2v_ctx* c) {
    const int n = c->am_n;
    am_free(c);
    c->am_k0[0] = c->T; c->am_k1[0] = c->T + c->R;
    for (int r = 1; r < n; ++r) {
        c->am_k0[r] = c->am_spans[2 * (r - 1)]; c->am_k1[r] = c->am_spans[2 * (r - 1) + 1];
        S2V_REQUIRE(c->am_k0[r] >= 0 && c->am_k0[r] <= c->am_k1[r] && c->am_k1[r] <= c->T,
                    "s2v_attn_map_enable: a text span must be a token range inside [0, T) of the current geometry");
    }
    const int64_t bytes = (int64_t)n * c->B * c->cfg.num_heads * c->V * 4;
    S2V_CHECK_HIP(hipMalloc((void**)&c->am_acc, bytes));
    S2V_CHECK_HIP(hipMemset(c->am_acc, 0, bytes));
    c->am_bytes = bytes; c->am_on = true; c->am_n = n;
    return 0;
}

// attention steering: off frees the table (the caller has synchronised the device and dropped the graphs)
static void st_free(s2v_ctx* c) {
    if (c->st_tab) hipFree(c->st_tab);
    if (c->st_map) hipFree(c->st_map);
    c->st_tab = nullptr; c->st_on = false; c->st_n = 0; c->st_arm = 0;
    c->st_map = nullptr; c->st_kind = 0; c->st_map_cap = c->st_map_V = c->st_map_Ntok = c->st_map_np = c->st_map_n = 0; c->st_map_w.clear();
}
// steering maps: the record of the held ranges, plane indices and weights at the current geometry, checked before anything is touched, then copied
// to the table.  The table is kept where it holds the record (same Ntok and V, no more planes than its room): a captured step keeps its pointer;
// otherwise it is allocated anew and *moved says so (the caller has synchronised, and drops the captured steps)
static int st_map_upload(s2v_ctx* c, const char* who, int n, const int* k0, const int* k1, const signed char* plane, int n_planes, const float* planes, bool* moved) {
    std::vector<int> r;
    const bool fits = c->st_map && c->st_map_Ntok == c->Ntok && c->st_map_V == c->V && n_planes <= c->st_map_cap;
    const int cap = fits ? c->st_map_cap : n_planes;
    S2V_TRY(attn_steer_map_make(who, n, k0, k1, plane, n_planes, planes, c->T + c->R, c->Ntok, c->Ntok, c->B, cap, &r));
    *moved = !fits;
    if (!fits) {
        if (c->st_map) hipFree(c->st_map);
        c->st_map = nullptr;
        S2V_CHECK_HIP(hipMalloc((void**)&c->st_map, r.size() * 4));
        c->st_map_cap = cap; c->st_map_V = c->V; c->st_map_Ntok = c->Ntok;
    }
    S2V_CHECK_HIP(hipMemcpy(c->st_map, r.data(), r.size() * 4, hipMemcpyHostToDevice));
    return 0;
}
// the record of the held ranges at the current geometry -- every sample's Ntok keys, the video rows as queries -- checked and copied to the table
static int st_upload(s2v_ctx* c, const char* who) {
    AttnSteerRec r{};
    S2V_TRY(attn_steer_make(who, c->st_n, c->st_k0, c->st_k1, c->st_w, c->st_mask, c->T + c->R, c->Ntok, c->Ntok, &r));
    S2V_CHECK_HIP(hipMemcpy(c->st_tab, &r, sizeof(r), hipMemcpyHostToDevice));
    return 0;
}
// what steering cannot run on, by name (enable, arm and the forward ask)
static int st_check(s2v_ctx* c, const char* fn) {
    static thread_local std::string m;
    auto fail = [&](const char* why) { m = std::string(fn) + ": " + why; return s2v_fail(__FILE__, __LINE__, m.c_str(), -1); };
    if (c->kind != S2V_CTX_MODEL) return fail("attention-only contexts (S2V_CTX_ATTN_*) run no forward; the s2v_attn_forward* seams run no steered attention");
    if (c->shard) return fail("a shard context (s2v_set_shard) has no attention steering: its attention sees a head group of all ranks' rows; steering runs on one GPU");
    if (c->dtype == S2V_DTYPE_F16) return fail("an fp16 engine has no steered attention kernel (bf16 runs attn_pp<STEER>, fp32 the generic form)");
    if (c->cfg.weight_format != 0) return fail("fp8 weight formats have no steered attention: their attention writes the MX output, the steered kernel writes bf16 only");
    if (c->attn_p16) return fail("attn_p_format 1 keeps V^T in fp16; the steered kernel reads bf16 V^T (s2v_set_attn_p_format 0)");
    if (!c->ws) return fail("call s2v_set_geometry first (the ranges are checked against the current geometry)");
    if (c->B > 32) return fail("the sample masks hold 32 samples");
    if (c->cond_triples) return fail("the context is conditioned as subject-guidance triples (s2v_set_conditioning_triples): steering assumes CFG pairs");
    if (c->win_acc) return fail("temporal windows are set (s2v_set_windows): steering runs one forward per step");
    return 0;
}

// local attention: off frees the table (the caller has synchronised the device and dropped the graphs)
static void la_free(s2v_ctx* c) {
    if (c->la_tab) hipFree(c->la_tab);
    if (c->la_box) hipFree(c->la_box);
    c->la_tab = nullptr; c->la_box = nullptr; c->la_kind = 0; c->la_on = false; c->la_Ntok = 0; c->la_arm = 0;
}
// the record of (P, lo, hi) at the current geometry, checked by attn_local_make before the table is touched, then copied to it
static int la_upload(s2v_ctx* c, const char* who, int P, const int* lo, const int* hi) {
    std::vector<int> r;
    S2V_TRY(attn_local_make(who, P, c->Ntok, lo, hi, &r));
    S2V_CHECK_HIP(hipDeviceSynchronize());   // a step on any stream may still read the table; a captured step is kept: the table is data
    S2V_CHECK_HIP(hipMemcpy(c->la_tab, r.data(), r.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}
// the table every row of which sees every key: what enable leaves in place
static int la_upload_dense(s2v_ctx* c, const char* who) {
    std::vector<int> lo((size_t)c->Ntok, 1), hi((size_t)c->Ntok, c->Ntok);
    return la_upload(c, who, 1, lo.data(), hi.data());
}
// what local attention cannot run on, by name (enable, arm and the forward ask)
static int la_check(s2v_ctx* c, const char* fn) {
    static thread_local std::string m;
    auto fail = [&](const char* why) { m = std::string(fn) + ": " + why; return s2v_fail(__FILE__, __LINE__, m.c_str(), -1); };
    if (c->kind != S2V_CTX_MODEL) return fail("attention-only contexts (S2V_CTX_ATTN_*) run no forward; the s2v_attn_forward* seams run no local attention");
    if (c->shard) return fail("a shard context (s2v_set_shard) has no local attention: its attention sees a head group of all ranks' rows; local attention runs on one GPU");
    if (c->dtype == S2V_DTYPE_F16) return fail("an fp16 engine has no local attention kernel (bf16 runs attn_pp<LOCAL>, fp32 the generic form)");
    if (c->cfg.weight_format != 0) return fail("fp8 weight formats have no local attention: their attention writes the MX output, the local kernel writes bf16 only");
    if (c->attn_p16) return fail("attn_p_format 1 keeps V^T in fp16; the local kernel reads bf16 V^T (s2v_set_attn_p_format 0)");
    if (!c->ws) return fail("call s2v_set_geometry first (the row table is checked against the current geometry)");
    if (c->cond_triples) return fail("the context is conditioned as subject-guidance triples (s2v_set_conditioning_triples): local attention assumes CFG pairs");
    if (c->win_acc) return fail("temporal windows are set (s2v_set_windows): local attention runs one forward per step");
    return 0;
}

// step cache: whatever makes the stored residual belong to another computation clears its validity, and with it a pending arm (the next
// forward then runs FULL: time, never correctness)
static void sc_invalidate(s2v_ctx* c) { c->sc_valid = false; c->sc_arm = S2V_STEP_FULL; }
static void sc_free(s2v_ctx* c) {
    if (c->sc_delta) hipFree(c->sc_delta);
    if (c->sc_in) hipFree(c->sc_in);
    c->sc_delta = c->sc_in = nullptr; c->sc_bytes = 0; c->sc_on = 0;
    sc_invalidate(c);
}
// the buffers of level `on` for the current geometry (the caller has synchronised the device and dropped the graphs)
static int sc_alloc(s2v_ctx* c, int on) {
    sc_free(c);
    if (!on) return 0;
    const int64_t bytes = (int64_t)c->B * c->V * c->D * c->esz;
    S2V_CHECK_HIP(hipMalloc((void**)&c->sc_delta, bytes));
    if (on == 2 && hipMalloc((void**)&c->sc_in, bytes) != hipSuccess) { sc_free(c); return s2v_fail(__FILE__, __LINE__, "s2v_step_cache_enable: out of device memory", -2); }
    c->sc_bytes = on == 2 ? 2 * bytes : bytes; c->sc_on = on;
    return 0;
}

// temporal windows: the plane belongs to one geometry (the caller has synchronised the device and dropped the graphs)
static void win_free(s2v_ctx* c) {
    if (c->win_acc) hipFree(c->win_acc);
    c->win_acc = c->win_w = c->win_wsum = nullptr;
    c->win_bytes = 0; c->win_L = c->win_s = c->win_pf = c->win_W = 0;
}

// guidance rescale: the partials belong to one geometry (the caller has synchronised the device and dropped the graphs); the log stays
static void gr_free(s2v_ctx* c) {
    if (c->gr_buf) hipFree(c->gr_buf);
    c->gr_buf = nullptr; c->gr_partials = c->gr_sums = nullptr; c->gr_factors = c->gr_phi = nullptr;
    c->gr_b = 0; c->gr_bytes = 0;
}
static void gr_free_log(s2v_ctx* c) {
    if (c->gr_log) hipFree(c->gr_log);
    c->gr_log = nullptr; c->gr_log_count = nullptr; c->gr_log_bytes = 0;
}

// the references beyond the first (s2v_set_conditioning_refs) go with the workspace they were projected for
static void drop_refs(s2v_ctx* c) {
    if (c->e1x) hipFree(c->e1x);
    c->e1x = nullptr; c->e1x_bytes = 0; c->n_ref = 1; c->e1_cur = nullptr;
}

// "transformer_blocks.<l>.norm{1,2}.linear.{weight,bias}"
static bool is_adaln_linear(const char* name) {
    const std::string n = name;
    return n.rfind("transformer_blocks.", 0) == 0 && (n.find(".norm1.linear.") != std::string::npos || n.find(".norm2.linear.") != std::string::npos);
}

extern "C" int s2v_load_weight(s2v_ctx* c, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim,
                               int32_t src_dtype, s2v_stream stream) {
    S2V_REQUIRE(c && name && dev_ptr && shape, "s2v_load_weight: null argument");
    S2V_REQUIRE(!c->finalized, "s2v_load_weight: weights already finalized");
    sc_invalidate(c);
    S2V_REQUIRE(src_dtype == S2V_DTYPE_F32 || src_dtype == S2V_DTYPE_BF16 || src_dtype == S2V_DTYPE_F16, "s2v_load_weight: unsupported source dtype");
    auto it = c->slots.find(name);
    if (it == c->slots.end()) {
        std::string m = std::string("s2v_load_weight: unknown tensor name: ") + name;
        return s2v_fail(__FILE__, __LINE__, m.c_str(), -3);
    }
    Slot& s = it->second;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    if (n != s.rows * s.cols || (ndim >= 2 && shape[0] != s.rows)) {
        std::string m = std::string("s2v_load_weight: shape mismatch for ") + name;
        return s2v_fail(__FILE__, __LINE__, m.c_str(), -3);
    }
    S2V_TRY(launch_convert2d(dev_ptr, src_dtype, s.cols, s.dst, c->dtype, s.ld, s.rows, s.cols, (hipStream_t)stream));
    s.loaded = true;
    if (c->mc == 9 && is_adaln_linear(name)) {
        // lora_adaln_scope 1: the reference-image copy of chunks 0-2 (rows [0, 3D) of the weight, entries [0, 3D) of the bias)
        // sits right behind the six chunks; it starts as the base values and is what s2v_merge_lora then adds to
        const int64_t D3 = 3 * (int64_t)c->D;
        const bool bias = s.rows == 1;
        const int64_t bytes6 = (bias ? 6 * (int64_t)c->D : 6 * (int64_t)c->D * s.ld) * c->esz, bytes3 = bytes6 / 2;
        (void)D3;
        S2V_CHECK_HIP(hipMemcpyAsync(s.dst + bytes6, s.dst, (size_t)bytes3, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return 0;
}

// W[name] += scale * B.A in fp32, rounded once to the model dtype: the arithmetic of s2v_merge_lora (load time) and of the weights a
// runtime attach re-merges from their base copy
static int merge_into(s2v_ctx* c, const char* name, Slot& s, const float* A, const float* B, int32_t rank, float scale, hipStream_t st) {
    // lora_adaln_scope 1: on norm{1,2}.linear the LoRA reaches only the reference-image copy of chunks 0-2 (rows [0, 3D) of B)
    const bool scoped = c->mc == 9 && is_adaln_linear(name);
    char* dst = scoped ? s.dst + 6 * (int64_t)c->D * s.ld * c->esz : s.dst;
    const int64_t rows = scoped ? 3 * (int64_t)c->D : s.rows;
    // one fp32 scratch for all merges of a load (grown to the largest slot, freed by s2v_finalize_weights / s2v_destroy): no
    // allocation or synchronisation per key.  A runtime-mode context allocates it again at its first attach after finalize and keeps it
    // until s2v_destroy (the largest re-merged slot in fp32: 50 MB at 5B, not counted by s2v_device_bytes)
    const size_t need = sizeof(float) * (size_t)rows * (size_t)s.cols;
    if (need > c->lora_tmp_bytes) {
        if (c->lora_tmp) { S2V_CHECK_HIP(hipStreamSynchronize(st)); (void)hipFree(c->lora_tmp); c->lora_tmp = nullptr; c->lora_tmp_bytes = 0; }
        S2V_CHECK_HIP(hipMalloc((void**)&c->lora_tmp, need));
        c->lora_tmp_bytes = need;
    }
    float* tmp = c->lora_tmp;
    int r = launch_convert2d(dst, c->dtype, s.ld, tmp, S2V_F32, s.cols, rows, s.cols, st);
    // tmp[out][in] += scale * sum_k B[out][k] * A[k][in]
    if (!r) r = launch_gemm_strided_f32(B, rank, 1, A, 1, s.cols, tmp, s.cols, (int)rows, (int)s.cols, rank, scale, st);
    if (!r) r = launch_convert2d(tmp, S2V_F32, s.cols, dst, c->dtype, s.ld, rows, s.cols, st);
    return r;  // stream-ordered: the caller keeps A and B alive until the stream has passed (as for s2v_load_weight)
}

extern "C" int s2v_merge_lora(s2v_ctx* c, const char* name, const float* A, const float* B, int32_t rank, float scale,
                              s2v_stream stream) {
    S2V_REQUIRE(c && name && A && B && rank > 0, "s2v_merge_lora: bad argument");
    S2V_REQUIRE(!c->finalized, "s2v_merge_lora: weights already finalized");
    sc_invalidate(c);
    auto it = c->slots.find(name);
    S2V_REQUIRE(it != c->slots.end(), "s2v_merge_lora: unknown tensor name");
    Slot& s = it->second;
    S2V_REQUIRE(s.loaded && s.rows > 1, "s2v_merge_lora: base weight must be a loaded matrix");
    return merge_into(c, name, s, A, B, rank, scale, (hipStream_t)stream);
}

extern "C" int s2v_finalize_weights(s2v_ctx* c, s2v_stream stream) {
    S2V_REQUIRE(c, "s2v_finalize_weights: null context");
    S2V_REQUIRE(c->kind != S2V_CTX_ATTN_WORKSPACE, "s2v_finalize_weights: a workspace context (S2V_CTX_ATTN_WORKSPACE) holds no weights");
    sc_invalidate(c);
    for (auto& kv : c->slots) {
        if (!kv.second.loaded) {
            std::string m = std::string("s2v_finalize_weights: tensor was never loaded: ") + kv.first;
            return s2v_fail(__FILE__, __LINE__, m.c_str(), -3);
        }
    }
    if (c->fp8) {
        // per-output-channel e4m3 quantisation of the (LoRA-merged) bf16 weights; the zero pad rows get scale 1, bytes 0
        hipStream_t st = (hipStream_t)stream;
        for (auto& w : c->layers)
            for (int i = 0; i < LIN_NUM; ++i) {
                const LinShape s = lin_shape(i, c->D);
                S2V_TRY(launch_quant_rows_fp8(w.lin[i].w, s.pitch(c->lr), s.n_pad(), (int)s.K, w.lin[i].q, w.lin[i].s, st));
            }
        S2V_CHECK_HIP(hipStreamSynchronize(st));
    }
    if (c->lora_tmp) {
        S2V_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
        (void)hipFree(c->lora_tmp);
        c->lora_tmp = nullptr;
        c->lora_tmp_bytes = 0;
    }
    if ((c->lr || c->flr) && c->kind == S2V_CTX_MODEL) {
        // runtime LoRA: what the re-merged weights hold now is their base (a LoRA merged before this call stays part of it)
        hipStream_t st = (hipStream_t)stream;
        S2V_CHECK_HIP(hipMemcpyAsync(c->base_mod, c->mod_w, (size_t)c->base_mod_bytes, hipMemcpyDeviceToDevice, st));
        S2V_CHECK_HIP(hipMemcpyAsync(c->base_patch, c->patch_w, (size_t)c->base_patch_bytes, hipMemcpyDeviceToDevice, st));
        S2V_CHECK_HIP(hipMemcpyAsync(c->base_text, c->text_w, (size_t)c->base_text_bytes, hipMemcpyDeviceToDevice, st));
    }
    c->finalized = true;
    return 0;
}

extern "C" int s2v_weight_slot(s2v_ctx* c, const char* name, int64_t* offset_bytes, int64_t* rows, int64_t* cols, int64_t* ld) {
    S2V_REQUIRE(c && name && offset_bytes && rows && cols && ld, "s2v_weight_slot: null argument");
    auto it = c->slots.find(name);
    if (it == c->slots.end()) {
        std::string m = std::string("s2v_weight_slot: unknown tensor name: ") + name;
        return s2v_fail(__FILE__, __LINE__, m.c_str(), -3);
    }
    const Slot& s = it->second;
    *offset_bytes = (int64_t)(s.dst - c->arena);
    *rows = s.rows; *cols = s.cols; *ld = s.ld;
    return 0;
}

extern "C" int s2v_weight_arena(s2v_ctx* c, void** dev_ptr, int64_t* bytes) {
    S2V_REQUIRE(c && dev_ptr && bytes, "s2v_weight_arena: null argument");
    *dev_ptr = c->arena;
    *bytes = c->arena_bytes;
    return 0;
}
// a replica that received the arena by broadcast marks itself loaded
extern "C" int s2v_mark_weights_loaded(s2v_ctx* c) {
    S2V_REQUIRE(c, "null context");
    S2V_REQUIRE(c->kind != S2V_CTX_ATTN_WORKSPACE, "s2v_mark_weights_loaded: a workspace context (S2V_CTX_ATTN_WORKSPACE) holds no weights");
    for (auto& kv : c->slots) kv.second.loaded = true;
    c->finalized = true;
    sc_invalidate(c);
    if (c->lora_hdr) {  // the arena may carry an attached adapter: run it
        S2V_CHECK_HIP(hipDeviceSynchronize());
        S2V_CHECK_HIP(hipMemcpy(c->lora_hdr_host, c->lora_hdr, sizeof(c->lora_hdr_host), hipMemcpyDeviceToHost));
        c->lora_names.clear();
        c->lora_replica = c->lora_hdr_host[0] > 0 ? c->lora_hdr_host[0] : 0;
        c->lora_rank = c->lora_replica ? c->lora_hdr_host[1] : 0;
        memcpy(&c->lora_scale, &c->lora_hdr_host[2], sizeof(float));
        if (!c->lora_replica) c->lora_scale = 0.f;
        drop_graph(c);
        c->have_cond = false;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// rank r's share of a stream of n rows: [r*n/p, (r+1)*n/p)
static inline void shard_range(int n, int p, int r, int* begin, int* len) {
    const int b = (int)((int64_t)r * n / p), e = (int)((int64_t)(r + 1) * n / p);
    *begin = b; *len = e - b;
}

extern "C" int s2v_set_shard(s2v_ctx* c, int32_t world, int32_t rank) {
    S2V_REQUIRE(c, "null context");
    S2V_REQUIRE(c->kind == S2V_CTX_MODEL, "s2v_set_shard: attention-only contexts (S2V_CTX_ATTN_*) are not sharded");
    S2V_REQUIRE(world >= 1 && rank >= 0 && rank < world, "s2v_set_shard: need world >= 1 and 0 <= rank < world");
    S2V_REQUIRE(c->lora_cap == 0, "s2v_set_shard: a shard context does not support the runtime adapter mode (lora_runtime_rank > 0)");
    S2V_REQUIRE(c->cfg.num_heads % world == 0, "s2v_set_shard: the world size must divide num_heads (attention runs num_heads / world heads per rank)");
    // fp8: the attention output reaches the out-projection as MX e4m3 whose scales are dwords of four 32-column blocks = one 128-column K-tile =
    // two heads; with an even head count per rank every dword of that image belongs to exactly one rank's head group
    S2V_REQUIRE(c->cfg.weight_format == 0 || (c->D / world) % 128 == 0,
                "s2v_set_shard: fp8 weight formats need an even number of heads per rank, (inner_dim / world) % 128 == 0 (the MX block-scale dwords of "
                "the attention output hold two heads each)");
    S2V_REQUIRE(c->cfg.out_channels * 4 * c->esz % 16 == 0, "s2v_set_shard: the projected rows must be a multiple of 16 bytes (out_channels * 4 * element size)");
    sc_invalidate(c);
    if (c->shard && c->sp == world && c->sr == rank) return 0;
    S2V_CHECK_HIP(hipDeviceSynchronize());
    drop_graph(c);
    sc_free(c);   // a shard context has no step cache
    am_free(c);   // ... and no attention map
    st_free(c);   // ... and no attention steering
    la_free(c);   // ... and no local attention
    win_free(c);  // ... and no temporal windows
    gr_free(c);   // ... and no guidance rescale
    if (c->ws) { hipFree(c->ws); c->ws = nullptr; }  // the workspace is carved for the shard: s2v_set_geometry comes next
    drop_refs(c);
    c->B = 0;
    c->shard = true; c->sp = world; c->sr = rank;
    c->sh_pending = 0;
    return 0;
}

static bool attn_mx_out(const s2v_ctx* c);

extern "C" int s2v_set_geometry(s2v_ctx* c, int32_t B, int32_t T, int32_t F, int32_t H, int32_t W) {
    S2V_REQUIRE(c, "null context");
    S2V_REQUIRE(c->kind != S2V_CTX_ATTN_WEIGHTS, "s2v_set_geometry: an attention-weights context (S2V_CTX_ATTN_WEIGHTS) never carves a workspace");
    S2V_REQUIRE(B >= 1 && B <= S2V_MAX_BATCH, "s2v_set_geometry: batch must be 1..8 (S2V_MAX_BATCH: the CFG pairs of at most four videos per call)");
    S2V_REQUIRE(T >= 0 && F >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "s2v_set_geometry: bad geometry");
    sc_invalidate(c);
    if (c->win_acc) {   // temporal windows belong to the call that set them: every s2v_set_geometry, the same geometry again included, clears them
        S2V_CHECK_HIP(hipDeviceSynchronize());
        drop_graph(c);
        win_free(c);
    }
    if (c->gr_buf) {    // ... and so do the guidance-rescale values: the partials are sized for the geometry they were set on (the log stays)
        S2V_CHECK_HIP(hipDeviceSynchronize());
        drop_graph(c);
        gr_free(c);
    }
    if (c->ws && B == c->B && T == c->gT && F == c->F && H == c->H && W == c->W) return 0;
    if (c->shard) S2V_REQUIRE(F * (H / 2) * (W / 2) >= c->sp, "s2v_set_geometry: every rank of a shard needs at least one video row");
    S2V_CHECK_HIP(hipDeviceSynchronize());
    drop_graph(c);
    if (c->ws) { hipFree(c->ws); c->ws = nullptr; }
    drop_refs(c);
    c->B = B; c->T = T; c->F = F; c->H = H; c->W = W;
    c->R = (H / 2) * (W / 2);
    c->V = F * c->R;
    c->Ntok = T + c->R + c->V;
    c->gT = c->T; c->gR = c->R; c->gV = c->V; c->gN = c->Ntok;
    c->t0 = c->r0 = c->v0 = 0;
    if (c->shard) {  // every stream split separately: rank r keeps [T_r | R_r | V_r] of each sample
        shard_range(c->gT, c->sp, c->sr, &c->t0, &c->T);
        shard_range(c->gR, c->sp, c->sr, &c->r0, &c->R);
        shard_range(c->gV, c->sp, c->sr, &c->v0, &c->V);
        c->Ntok = c->T + c->R + c->V;
    }
    c->Vmax = (c->gV + c->sp - 1) / c->sp;
    c->sh_pending = 0;
    // weight_format 3 ("fp8-auto"): fp8 linears always, fp8 QK^T from S2V_FP8_QK_AUTO_TOKENS tokens on -- there the attention is > 80 % of the
    // step and the whole-run drift of fp8-qk is the fp8 engine's (profiles/r05_whole_run_c5_10steps.txt: 8.69e-3 against 8.67e-3).  The count is the
    // sequence the attention sees (gN): a shard decides as the single engine does
    c->fp8_qk = c->cfg.weight_format == 2 || (c->cfg.weight_format == 3 && c->gN >= S2V_FP8_QK_AUTO_TOKENS);
    c->ntok_pad = (int)rup(c->gN, 64);
    c->M = (int64_t)B * c->Ntok;
    c->Mpad = rup(c->M, 256) + 256;
    c->have_rope = c->have_pos = c->have_cond = false;
    c->cond_triples = false;
    c->split_kind = -1;
    const int64_t D = c->D, E = c->esz;
    const int64_t Cin4 = c->cfg.in_channels * 4, Cout4 = c->cfg.out_channels * 4;
    const int64_t BVp = rup((int64_t)B * c->V, 256) + 256;
    const int64_t BVg = rup((int64_t)B * c->gV, 256) + 256;  // patchify runs on the whole latent (== BVp without a shard)
    int64_t off = 0;
    auto carve = [&](int64_t bytes) { int64_t o = off; off += rup(bytes, 256); return o; };
    // runtime LoRA: the rows of Xn and Hb have room for T = x . A^T behind column K (3 lr / lr columns)
    const int64_t oX = carve(c->Mpad * D * E), oXn = carve(c->Mpad * (D + 3 * c->lr) * E), oQKV = carve(c->Mpad * 3 * D * E);
    const int64_t oH = carve(c->Mpad * (4 * D + c->lr) * E);
    const int64_t oTl = carve(c->Mpad * 3 * c->flr * E);  // fp8 branch: T has a buffer of its own (it cannot ride behind column K of an e4m3 / MX image)
    const int64_t oVT = carve((int64_t)B * (c->cfg.num_heads / c->sp) * 64 * c->ntok_pad * 2);
    const int64_t oe0 = carve(rup((int64_t)B * T + 128, 128) * D * E), oe1 = carve(rup(c->gR + 128, 128) * D * E);
    const int64_t opat = carve(BVg * Cin4 * E), otail = carve(BVp * D * E), oproj = carve(BVp * Cout4 * E);
    const int64_t omod = carve((int64_t)B * c->mod_rows * E);
    const int64_t ote = carve(((int64_t)B * D + (int64_t)B * c->temb) * E), oemb = carve((int64_t)B * c->temb * E);
    // room for the CFG pair even when the geometry holds ONE sample of it (CFG-parallel, s2v_denoise_split_*: the peer's half arrives here)
    const int64_t onp = carve((int64_t)std::max(B, 2) * F * c->cfg.out_channels * H * W * E);
    const int64_t ocos = carve((int64_t)(c->R + c->V) * 64 * 4), osin = carve((int64_t)(c->R + c->V) * 64 * 4);
    const int64_t opk = carve((int64_t)(c->R + c->V) * 64 * 4);
    const int64_t opos = carve((int64_t)c->V * D * E);
    const int64_t oaq = carve(c->fp8 ? c->Mpad * 4 * D : 0), oaqs = carve(c->fp8 ? c->Mpad * 4 : 0);
    // fp8: the FF1 epilogue leaves GELU(h) as MX e4m3 (bytes + one E8M0 scale per 32 columns), the FF2 reads it in place
    const int64_t ohq = carve(c->fp8 ? c->Mpad * 4 * D : 0), ohs = carve(c->fp8 ? c->Mpad * 4 * D / 32 : 0);
    // fp8_qk: MX e4m3 images of q and k for attn_q4f (AttnArgs::q8 ... k8s); a shard's attention runs its H/p heads over all gN tokens
    const int64_t BH = (int64_t)B * (c->cfg.num_heads / c->sp);
    const int64_t oq8 = carve(c->fp8_qk ? BH * c->gN * 64 : 0), oq8s = carve(c->fp8_qk ? BH * c->gN * 2 : 0);
    const int64_t ok8 = carve(c->fp8_qk ? BH * c->ntok_pad * 64 : 0), ok8s = carve(c->fp8_qk ? BH * c->ntok_pad * 4 : 0);
    // split-K partial tiles + arrival counters (linear(): only geometries whose FF2 has at most half as many 256 x 256 tiles as CUs).  A shard
    // never splits K: split-K changes the reduction order, and a rank's row count must not pick a different one than the single engine's
    c->sk_tiles = (!c->shard && c->mfma && ((c->M + 255) / 256) * ((D + 255) / 256) * 2 <= c->num_cus) ? c->num_cus : 0;
    const int64_t osk = carve((int64_t)c->sk_tiles * 262144), oskc = carve((int64_t)c->sk_tiles * 4);
    // KV split of the four-wave attention launch (kernels.h attn_plan): counters + the partial slots of every head's split q-blocks, at the
    // sequence the attention sees (gN) and the heads of this rank.  Every splitting format has the same plan; the fp8-QK^T formats do not split
    c->kv_ws_bytes = ((c->mfma || c->h16) && !c->fp8_qk) ? attn_kv_ws_bytes(attn_plan((int)c->gN, ATTN_FMT_Q4), BH) : 0;
    const int64_t okv = carve(c->kv_ws_bytes);
    // shard: the head-sharded full-N buffers, the exchange buffers and the row maps
    const int64_t P = c->sp, Dp = D / P, Mg = (int64_t)B * c->gN, Mgpad = rup(Mg, 256) + 256;
    // the O exchange: n rows of a head group are bf16 [n][D/p], or (fp8 engine) MX e4m3 [n][D/p] followed by the rows' scale dwords [n][D/(128p)],
    // padded to 16 bytes so that every peer's chunk starts 16-byte aligned
    c->o_mx = c->shard && attn_mx_out(c);
    const bool omx = c->o_mx;
    auto o_bytes = [&](int64_t n) { return omx ? n * Dp + rup(n * Dp / 32, 16) : n * Dp * E; };
    const int64_t oQh = carve(c->shard ? Mgpad * 3 * Dp * E : 0), oOh = carve(c->shard ? Mgpad * Dp * E : 0);
    const int64_t osb = carve(c->shard ? std::max(c->M * 3 * D * E, o_bytes(Mg) + 16 * P) : 0);
    const int64_t orb = carve(c->shard ? std::max(Mg * 3 * Dp * E, P * o_bytes(c->M)) : 0);
    const int64_t oOs = carve(omx ? Dp / 128 * Mgpad * 4 : 0), oomap = carve(omx ? 2 * Mg * 4 : 0);
    const int64_t ons = carve(c->shard ? (int64_t)B * c->Vmax * Cout4 * E : 0), onr = carve(c->shard ? P * B * c->Vmax * Cout4 * E : 0);
    const int64_t opf = carve(c->shard ? (int64_t)B * c->gV * Cout4 * E : 0);
    const int64_t ormap = carve(c->shard ? Mg * 4 : 0), onmap = carve(c->shard ? P * B * c->Vmax * 4 : 0);
    c->ws_bytes = off;
    S2V_CHECK_HIP(hipMalloc((void**)&c->ws, c->ws_bytes));
    S2V_CHECK_HIP(hipMemset(c->ws, 0, c->ws_bytes));
    char* w = c->ws;
    c->X = w + oX; c->Xn = w + oXn; c->QKV = w + oQKV; c->Hb = w + oH; c->VT = w + oVT; c->e0 = w + oe0; c->e1 = w + oe1;
    c->e1_cur = c->e1; c->e1_stride = rup(c->gR + 128, 128) * D * E;
    c->patches = w + opat; c->tailn = w + otail; c->proj = w + oproj; c->mod = w + omod; c->tmp_te = w + ote;
    c->emb = w + oemb; c->noise_pred = w + onp; c->rope_cos = (float*)(w + ocos); c->rope_sin = (float*)(w + osin);
    c->pos_tab = w + opos; c->rope_pk = (float*)(w + opk); c->rope_paired = false;
    c->aq = w + oaq; c->aq_scale = (float*)(w + oaqs);
    c->Tl = c->flr ? w + oTl : nullptr;
    c->hq = (unsigned char*)(w + ohq); c->hs = (unsigned char*)(w + ohs);
    c->q8 = (unsigned char*)(w + oq8); c->q8s = (unsigned short*)(w + oq8s); c->k8 = (unsigned char*)(w + ok8); c->k8s = (unsigned*)(w + ok8s);
    c->sk_ws = (float*)(w + osk); c->sk_cnt = (unsigned*)(w + oskc);
    c->kv_ws = c->kv_ws_bytes ? w + okv : nullptr;
    if (c->shard) {
        c->QKVh = w + oQh; c->Oh = w + oOh; c->sbuf = w + osb; c->rbuf = w + orb; c->nsend = w + ons; c->nrecv = w + onr; c->proj_full = w + opf;
        c->rmap = (int*)(w + ormap); c->nmap = (int*)(w + onmap);
        c->Os = omx ? (unsigned char*)(w + oOs) : nullptr; c->Os_rows = Mgpad; c->omap = omx ? (int*)(w + oomap) : nullptr;
        // rank g's rows of sample b, in g's local order [T_g | R_g | V_g], concatenated over g = the recv order of the QKV exchange (and the
        // send order of the O exchange); each maps to its row b * gN + (stream offset) in the global [text | ref | video] sequence
        std::vector<int> rmap, nmap;
        rmap.reserve(Mg);
        nmap.assign((size_t)P * B * c->Vmax, -1);
        std::vector<int64_t> ntok(P);
        for (int g = 0; g < P; ++g) {
            int ts, tl, rs, rl, vs, vl;
            shard_range(c->gT, (int)P, g, &ts, &tl); shard_range(c->gR, (int)P, g, &rs, &rl); shard_range(c->gV, (int)P, g, &vs, &vl);
            ntok[g] = tl + rl + vl;
            for (int b = 0; b < B; ++b) {
                const int base = b * c->gN;
                for (int i = 0; i < tl; ++i) rmap.push_back(base + ts + i);
                for (int i = 0; i < rl; ++i) rmap.push_back(base + c->gT + rs + i);
                for (int i = 0; i < vl; ++i) rmap.push_back(base + c->gT + c->gR + vs + i);
                for (int i = 0; i < vl; ++i) nmap[((size_t)g * B + b) * c->Vmax + i] = b * c->gV + vs + i;
            }
        }
        S2V_CHECK_HIP(hipMemcpy(c->rmap, rmap.data(), rmap.size() * 4, hipMemcpyHostToDevice));
        S2V_CHECK_HIP(hipMemcpy(c->nmap, nmap.data(), nmap.size() * 4, hipMemcpyHostToDevice));
        for (auto& k : c->xcnt) for (auto& v : k) v.assign(P, 0);
        int64_t rq = 0, so = 0;
        std::vector<int> omap(omx ? 2 * Mg : 0);
        for (int g = 0, i = 0; g < P; ++g) {
            // QKV: to g my rows' head group g; from g its rows' head group sr
            c->xcnt[0][0][g] = c->M * 3 * Dp * E; c->xcnt[0][1][g] = g * c->M * 3 * Dp * E;
            c->xcnt[0][2][g] = B * ntok[g] * 3 * Dp * E; c->xcnt[0][3][g] = rq; rq += c->xcnt[0][2][g];
            // O: to g its rows of head group sr; from g my rows of head group g
            const int64_t n = B * ntok[g];
            if (omx)  // the chunk to g: the bytes of its n rows (send order = rmap's), then their scale dwords
                for (int64_t j = 0; j < n; ++j, ++i) { omap[i] = (int)((so + j * Dp) / 16); omap[Mg + i] = (int)((so + n * Dp) / 4 + j * (Dp / 128)); }
            c->xcnt[1][0][g] = o_bytes(n); c->xcnt[1][1][g] = so; so += c->xcnt[1][0][g];
            c->xcnt[1][2][g] = o_bytes(c->M); c->xcnt[1][3][g] = g * o_bytes(c->M);
            // noise: the same [B][Vmax] rows to everyone
            c->xcnt[2][0][g] = (int64_t)B * c->Vmax * Cout4 * E; c->xcnt[2][1][g] = 0;
            c->xcnt[2][2][g] = c->xcnt[2][0][g]; c->xcnt[2][3][g] = g * c->xcnt[2][0][g];
        }
        if (omx) S2V_CHECK_HIP(hipMemcpy(c->omap, omap.data(), omap.size() * 4, hipMemcpyHostToDevice));
    }
    if (c->sc_on) S2V_TRY(sc_alloc(c, c->sc_on));   // the step cache follows the geometry
    if (c->am_on) S2V_TRY(am_alloc(c));             // ... and so does the attention map: re-sized, zeroed, the count at 0
    if (c->st_on) {                                 // ... and the steer record; a range that no longer fits refuses and leaves steering off
        c->st_arm = 0;
        int r = st_upload(c, "s2v_set_geometry (attention steering)");
        if (r == 0 && c->st_kind == 1) {            // ... the maps are one weight per video cell: another V refuses by name, the same V re-makes the record
            if (c->st_map_V != c->V) {
                static thread_local char msg[200];
                snprintf(msg, sizeof(msg), "s2v_set_geometry (steering maps): the held planes have %d cells, the new geometry has V = %d video rows; steering is off",
                         c->st_map_V, c->V);
                st_free(c);
                S2V_REQUIRE(false, msg);
            }
            bool moved = false;
            r = st_map_upload(c, "s2v_set_geometry (steering maps)", c->st_map_n, c->st_map_k0, c->st_map_k1, &c->st_map_plane[0][0], c->st_map_np,
                              c->st_map_w.data(), &moved);
        }
        if (r != 0) { st_free(c); return r; }
    }
    if (c->la_on && c->la_Ntok != c->Ntok) {        // ... the local-attention table is one row per token: another Ntok switches the feature off
        la_free(c);
    }
    return 0;
}

extern "C" int s2v_fp8_qk_active(s2v_ctx* c, int32_t* active) {
    S2V_REQUIRE(c && active, "s2v_fp8_qk_active: null argument");
    *active = c->fp8_qk ? 1 : 0;
    return 0;
}

extern "C" int s2v_set_rope(s2v_ctx* c, const float* cos_dev, const float* sin_dev, s2v_stream stream) {
    S2V_REQUIRE(c && c->ws, "s2v_set_rope: call s2v_set_geometry first");
    sc_invalidate(c);
    // the captured step bakes in have_rope and the fused-epilogue decision (rope_paired): a change of either drops the graph
    if (!cos_dev || !sin_dev) {
        if (c->have_rope) drop_graph(c);
        c->have_rope = false;
        return 0;
    }
    const bool had_rope = c->have_rope, was_paired = c->rope_paired;
    const size_t bytes = (size_t)(c->R + c->V) * 64 * 4;
    if (c->shard) {  // the full [ref | video] tables in, this rank's R_r + V_r rows kept
        const size_t row = 64 * 4, rb = (size_t)c->R * row, vb = (size_t)c->V * row;
        const size_t ro = (size_t)c->r0 * row, vo = ((size_t)c->gR + c->v0) * row;
        S2V_CHECK_HIP(hipMemcpyAsync(c->rope_cos, (const char*)cos_dev + ro, rb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        S2V_CHECK_HIP(hipMemcpyAsync(c->rope_sin, (const char*)sin_dev + ro, rb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        S2V_CHECK_HIP(hipMemcpyAsync((char*)c->rope_cos + rb, (const char*)cos_dev + vo, vb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        S2V_CHECK_HIP(hipMemcpyAsync((char*)c->rope_sin + rb, (const char*)sin_dev + vo, vb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    } else {
        S2V_CHECK_HIP(hipMemcpyAsync(c->rope_cos, cos_dev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        S2V_CHECK_HIP(hipMemcpyAsync(c->rope_sin, sin_dev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    c->have_rope = true;
    // The reference builds its tables with repeat_interleave(2) (embeddings.py:get_3d_rotary_pos_embed): cos[2k] == cos[2k+1].  When
    // that holds (checked, once per geometry, on the host) a packed copy [position][32 cos | 32 sin] halves what the fused QKV
    // epilogue has to fetch per row; tables without that structure take the stand-alone qk_norm_rope_k pass instead.
    const size_t n = (size_t)(c->R + c->V) * 64;
    std::vector<float> hc(n), hs(n), pk(n);
    S2V_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    S2V_CHECK_HIP(hipMemcpy(hc.data(), c->rope_cos, bytes, hipMemcpyDeviceToHost));
    S2V_CHECK_HIP(hipMemcpy(hs.data(), c->rope_sin, bytes, hipMemcpyDeviceToHost));
    bool paired = true;
    for (size_t i = 0; i < n && paired; i += 2) paired = hc[i] == hc[i + 1] && hs[i] == hs[i + 1];
    c->rope_paired = paired;
    if (!had_rope || was_paired != paired) drop_graph(c);
    if (paired) {
        for (size_t p = 0; p < n / 64; ++p)
            for (int k = 0; k < 32; ++k) {
                pk[p * 64 + k] = hc[p * 64 + 2 * k];
                pk[p * 64 + 32 + k] = hs[p * 64 + 2 * k];
            }
        S2V_CHECK_HIP(hipMemcpy(c->rope_pk, pk.data(), bytes, hipMemcpyHostToDevice));
    }
    return 0;
}

extern "C" int s2v_set_pos_embed(s2v_ctx* c, const void* table_dev, s2v_stream stream) {
    S2V_REQUIRE(c && c->ws, "s2v_set_pos_embed: call s2v_set_geometry first");
    sc_invalidate(c);
    if (!table_dev) { c->have_pos = false; return 0; }
    // shard: the full [V][D] table in, this rank's V_r rows kept
    S2V_CHECK_HIP(hipMemcpyAsync(c->pos_tab, (const char*)table_dev + (size_t)c->v0 * c->D * c->esz, (size_t)c->V * c->D * c->esz,
                                 hipMemcpyDeviceToDevice, (hipStream_t)stream));
    c->have_pos = true;
    return 0;
}

static int linear(s2v_ctx* c, const GemmArgs& g0, int epi, hipStream_t st) {
    GemmArgs g = g0;
    g.clk = c->clk_cur;
    // every GEMM operand of the transformer lives in a workspace buffer with >= 256 rows of slack behind it
    g.a_rows_padded = (int)(rup(g.M, 256));
    g.w_rows_padded = (int)(rup(g.N, 256));  // every weight of the arena is carved with its rows padded to 256
    if ((c->mfma || c->h16) && g.K % 64 == 0 && g.lda % 8 == 0 && g.ldw % 8 == 0) {
        g.f16 = c->h16 ? 1 : 0;  // the fp16 model dtype takes the same dispatch on the kernels' fp16 instantiations (launch_gemm_bf16)
        const GemmPlan p = gemm_plan(g, epi, c->num_cus, c->sk_tiles);  // split K, tile, row tail: gemm.hip
        g.tile = p.tile;
        if (p.splitk > 1) { g.splitk = p.splitk; g.sk_ws = c->sk_ws; g.sk_cnt = c->sk_cnt; }
        if (p.tail != GEMM_NONE) {
            GemmArgs gm = g, gt = g;
            gt.clk = nullptr;  // the row tail runs beside the main launch on the side stream: one stamp per profiled launch
            gm.M = p.m_main;
            gt.m_begin = p.m_main;
            // fork: the tail runs on the side stream beside the main launch (event fork/join, valid under stream capture)
            S2V_CHECK_HIP(hipEventRecord(c->ev_fork, st));
            S2V_CHECK_HIP(hipStreamWaitEvent(c->side, c->ev_fork, 0));
            S2V_TRY(launch_gemm_bf16(gt, epi, c->side));
            S2V_CHECK_HIP(hipEventRecord(c->ev_join, c->side));
            S2V_TRY(launch_gemm_bf16(gm, epi, st));
            S2V_CHECK_HIP(hipStreamWaitEvent(st, c->ev_join, 0));
            return 0;
        }
        return launch_gemm_bf16(g, epi, st);
    }
    g.valu_only = c->cfg.force_simple;  // fp32: the matrix-pipe kernel (gemm_f32m, same bits) unless the cross-check path is asked for
    return launch_gemm_simple(g, epi, c->dtype, st);
}

// weight_format 1: quantise the activation rows (per token, dynamic) and run the fp8 GEMM against the e4m3 weight copy
// prequant: the producer (ln_modulate_k) already left the e4m3 image and the row scales of A in c->aq / c->aq_scale
// g0.mx_a_s set: A is already an MX image (g0.A bytes, block scales g0.mx_a_s) left by the producing GEMM's epilogue
static int linear_fp8(s2v_ctx* c, const GemmArgs& g0, int epi, const char* wq, const float* wscale, hipStream_t st, bool prequant = false) {
    GemmArgs g = g0;
    g.clk = c->clk_cur;
    g.a_scale = nullptr;
    if (!g.mx_a_s) {
        if (!prequant) S2V_TRY(launch_quant_rows_fp8(g.A, g.lda, g.M, g.K, c->aq, c->aq_scale, st));
        g.A = c->aq; g.a_scale = c->aq_scale;
    }
    g.lda = g.K; g.W = wq; g.ldw = g.K; g.w_scale = wscale;
    g.a_rows_padded = (int)rup(g.M, 256);
    g.w_rows_padded = (int)rup(g.N, 256);
    return launch_gemm_fp8(g, epi, st);
}

extern "C" int s2v_set_conditioning_refs(s2v_ctx* c, const void* text_dev, const void* ref_latents_dev, int32_t n_ref, s2v_stream stream) {
    S2V_REQUIRE(c && c->ws && c->finalized, "s2v_set_conditioning_refs: geometry and weights must be set first");
    S2V_REQUIRE(text_dev && ref_latents_dev, "s2v_set_conditioning_refs: null input");
    sc_invalidate(c);
    const int B = c->B;
    S2V_REQUIRE(n_ref == 1 || n_ref == B || (B % 2 == 0 && n_ref == B / 2),
                "s2v_set_conditioning_refs: n_ref must be 1 (one reference for every sample), B / 2 (one per video of [negative x b | positive x b]) "
                "or B (one per sample): sample j takes reference j mod n_ref");
    hipStream_t st = (hipStream_t)stream;
    const int D = c->D;
    const int64_t E = c->esz;
    // where the reference tokens live: the workspace's e1 for one reference, a buffer of n_ref of them otherwise.  The captured step reads
    // the address and the mapping: a change of either drops it
    char* e1 = c->e1;
    if (n_ref > 1) {
        const int64_t need = n_ref * c->e1_stride;
        if (c->e1x_bytes < need) {
            S2V_CHECK_HIP(hipDeviceSynchronize());
            if (c->e1x) hipFree(c->e1x);
            c->e1x = nullptr; c->e1x_bytes = 0;
            if (c->e1_cur != c->e1) { c->e1_cur = c->e1; c->n_ref = 1; c->have_cond = false; drop_graph(c); }
            S2V_CHECK_HIP(hipMalloc((void**)&c->e1x, need));
            S2V_CHECK_HIP(hipMemset(c->e1x, 0, need));
            c->e1x_bytes = need;
        }
        e1 = c->e1x;
    }
    if (e1 != c->e1_cur || n_ref != c->n_ref || c->cond_triples) drop_graph(c);
    c->e1_cur = e1; c->n_ref = n_ref; c->cond_triples = false;
    c->have_cond = false;
    // text_proj (cogvideox_transformer_3d.py:494).  The MFMA kernel stages 128-row tiles, so the operand is first
    // copied into the (padded, zero-initialised) Hb scratch.
    const int TX = c->cfg.text_embed_dim;
    if (c->T > 0) {
        GemmArgs g{};
        g.A = c->Hb; g.lda = TX; g.W = c->text_w; g.ldw = TX; g.bias = c->text_b;
        g.C = c->e0; g.ldc = D; g.N = D; g.K = TX;
        if (B > 2 && B % 2 == 0 && !c->shard) {
            // several videos: the [negative | positive] pair of each video is projected by a launch of a one-video call's shape (M = 2 T
            // rows: tile and row tail do not depend on how many videos share the call), into X as scratch, then moved to its two places of
            // e0.  Split K is the one thing the shape does not settle: gemm_plan splits only where the GEOMETRY carved a split-K workspace
            // (sk_tiles, from B * Ntok), so at a size where the one-video geometry has one and the batched one has none (configs[0]) this
            // K = text_embed_dim projection sums in another order than it does alone; everywhere else the bits are the one-video call's
            const int b = B / 2;
            const int64_t tb = (int64_t)c->T * TX * E, eb = (int64_t)c->T * D * E;
            g.C = c->X; g.M = 2 * c->T;
            for (int v = 0; v < b; ++v) {
                for (int h = 0; h < 2; ++h)
                    S2V_TRY(launch_convert2d((const char*)text_dev + (int64_t)(v + h * b) * tb, c->dtype, TX, c->Hb + h * tb, c->dtype, TX, c->T, TX, st));
                S2V_TRY(linear(c, g, EPI_BIAS, st));
                for (int h = 0; h < 2; ++h)
                    S2V_TRY(launch_copy_rows(c->X + h * eb, D, nullptr, 0, c->e0 + (int64_t)(v + h * b) * eb, D, c->T, D, c->dtype, st));
            }
        } else {
            if (c->shard) {  // the full [B][gT] embeddings in, this rank's T_r rows of each sample kept
                for (int b = 0; b < B; ++b)
                    S2V_TRY(launch_convert2d((const char*)text_dev + ((int64_t)b * c->gT + c->t0) * TX * c->esz, c->dtype, TX,
                                             c->Hb + (int64_t)b * c->T * TX * c->esz, c->dtype, TX, c->T, TX, st));
            } else {
                S2V_TRY(launch_convert2d(text_dev, c->dtype, TX, c->Hb, c->dtype, TX, (int64_t)B * c->T, TX, st));
            }
            g.M = B * c->T;
            S2V_TRY(linear(c, g, EPI_BIAS, st));
        }
    }
    // reference image latents -> patch tokens (cogvideox_transformer_3d.py:496-501), one launch per reference: what a one-video call runs
    const int K = c->cfg.in_channels * 4;
    const int64_t ref_elems = (int64_t)c->cfg.in_channels * c->H * c->W;
    for (int r = 0; r < n_ref; ++r) {
        S2V_TRY(launch_patchify((const char*)ref_latents_dev + r * ref_elems * E, 0, 1, 1, c->cfg.in_channels, c->H, c->W, c->patches, c->dtype, st));
        GemmArgs g{};
        g.A = c->patches + (int64_t)c->r0 * K * c->esz; g.lda = K; g.W = c->patch_w; g.ldw = K; g.bias = c->patch_b;  // shard: this rank's R_r patches
        g.C = e1 + r * c->e1_stride; g.ldc = D; g.M = c->R; g.N = D; g.K = K;
        if (c->R > 0) S2V_TRY(linear(c, g, EPI_BIAS, st));
    }
    c->have_cond = true;
    return 0;
}

extern "C" int s2v_set_conditioning(s2v_ctx* c, const void* text_dev, const void* ref_latent_dev, s2v_stream stream) {
    return s2v_set_conditioning_refs(c, text_dev, ref_latent_dev, 1, stream);
}

// Subject guidance: the conditioning of b triples on a geometry of B = 3b samples [u x b | r x b | f x b] (include/s2v_hip.h).  The launches are
// the pair set-up's: video v's [negative | positive] text pair through one M = 2T projection into X as scratch, its negative rows then moved to
// samples u_v and r_v and its positive rows to f_v; every reference through the per-reference patch embedding.  The reference table is the e1x
// buffer with one entry per SAMPLE, [null x b | ref x b | ref x b], so the forward's `j mod n_ref` (n_ref = B) stays the mapping: the f entry
// is a copy of the r entry's rows, not a second embedding
extern "C" int s2v_set_conditioning_triples(s2v_ctx* c, const void* text_dev, const void* ref_latents_dev, const void* null_ref_latents_dev,
                                            int32_t n_null, s2v_stream stream) {
    S2V_REQUIRE(c && c->ws && c->finalized, "s2v_set_conditioning_triples: geometry and weights must be set first");
    S2V_REQUIRE(text_dev && ref_latents_dev && null_ref_latents_dev, "s2v_set_conditioning_triples: null input");
    S2V_REQUIRE(!c->shard, "s2v_set_conditioning_triples: a shard context (s2v_set_shard) has no triple step: subject guidance runs on one GPU");
    const int B = c->B, b = B / 3;
    S2V_REQUIRE(B % 3 == 0 && b <= 2, "s2v_set_conditioning_triples: a geometry of B = 3b samples [u x b | r x b | f x b] with b = 1 or 2 videos is required");
    S2V_REQUIRE(n_null == 1 || n_null == b, "s2v_set_conditioning_triples: n_null must be 1 (one null reference for every video) or b (one per video)");
    sc_invalidate(c);
    hipStream_t st = (hipStream_t)stream;
    const int D = c->D;
    const int64_t E = c->esz;
    const int64_t need = (int64_t)B * c->e1_stride;
    if (c->e1x_bytes < need) {
        S2V_CHECK_HIP(hipDeviceSynchronize());
        if (c->e1x) hipFree(c->e1x);
        c->e1x = nullptr; c->e1x_bytes = 0;
        if (c->e1_cur != c->e1) { c->e1_cur = c->e1; c->n_ref = 1; c->have_cond = false; drop_graph(c); }
        S2V_CHECK_HIP(hipMalloc((void**)&c->e1x, need));
        S2V_CHECK_HIP(hipMemset(c->e1x, 0, need));
        c->e1x_bytes = need;
    }
    if (c->e1x != c->e1_cur || B != c->n_ref || !c->cond_triples) drop_graph(c);
    c->e1_cur = c->e1x; c->n_ref = B; c->cond_triples = true;
    c->have_cond = false;
    const int TX = c->cfg.text_embed_dim;
    if (c->T > 0) {
        GemmArgs g{};
        g.A = c->Hb; g.lda = TX; g.W = c->text_w; g.ldw = TX; g.bias = c->text_b;
        g.C = c->X; g.ldc = D; g.M = 2 * c->T; g.N = D; g.K = TX;
        const int64_t tb = (int64_t)c->T * TX * E, eb = (int64_t)c->T * D * E;
        for (int v = 0; v < b; ++v) {
            for (int h = 0; h < 2; ++h)
                S2V_TRY(launch_convert2d((const char*)text_dev + (int64_t)(v + h * b) * tb, c->dtype, TX, c->Hb + h * tb, c->dtype, TX, c->T, TX, st));
            S2V_TRY(linear(c, g, EPI_BIAS, st));
            for (int s3 = 0; s3 < 3; ++s3)   // u and r: the negative rows; f: the positive rows
                S2V_TRY(launch_copy_rows(c->X + (s3 == 2 ? eb : 0), D, nullptr, 0, c->e0 + (int64_t)(v + s3 * b) * eb, D, c->T, D, c->dtype, st));
        }
    }
    const int K = c->cfg.in_channels * 4;
    const int64_t ref_elems = (int64_t)c->cfg.in_channels * c->H * c->W;
    for (int r = 0; r < 2 * b; ++r) {   // entries [0, b): the null references; [b, 2b): the references
        const char* src = r < b ? (const char*)null_ref_latents_dev + (n_null == 1 ? 0 : r) * ref_elems * E : (const char*)ref_latents_dev + (r - b) * ref_elems * E;
        S2V_TRY(launch_patchify(src, 0, 1, 1, c->cfg.in_channels, c->H, c->W, c->patches, c->dtype, st));
        GemmArgs g{};
        g.A = c->patches; g.lda = K; g.W = c->patch_w; g.ldw = K; g.bias = c->patch_b;
        g.C = c->e1x + r * c->e1_stride; g.ldc = D; g.M = c->R; g.N = D; g.K = K;
        if (c->R > 0) S2V_TRY(linear(c, g, EPI_BIAS, st));
    }
    for (int v = 0; v < b && c->R > 0; ++v)
        S2V_TRY(launch_copy_rows(c->e1x + (b + v) * c->e1_stride, D, nullptr, 0, c->e1x + (2 * b + v) * c->e1_stride, D, c->R, D, c->dtype, st));
    c->have_cond = true;
    return 0;
}

// ---- one transformer block on the packed residual buffer X ------------------------------------------------
#ifdef S2V_DIAG
static int g_fp8_mx = 1;
extern "C" __attribute__((visibility("default"))) int s2v_set_fp8_mx(int on) { g_fp8_mx = on; return 0; }
static int g_fused_q8 = 1;
extern "C" __attribute__((visibility("default"))) int s2v_set_fused_q8(int on) { g_fused_q8 = on; return 0; }
static int g_fused_qk = 1;
extern "C" __attribute__((visibility("default"))) int s2v_set_fused_qk(int on) { g_fused_qk = on; return 0; }
// the fused QKV projection (EPI_BIAS_QKNORM) as an operator of the diagnostics build: A [M (rows allocated up to a multiple of 256)][K],
// W [3 D][K], C [M][3 D], LayerNorm(64) parameters of q and k, paired rotary table [positions][32 cos | 32 sin] fp32 -- what the block
// forward launches, so that the kernels that implement it (gemm_g4t's trickle, gemm_g4's / the eight-wave kernels' C++ epilogue) can be
// compared bit for bit on real shapes (tests/test_gpu_gemm_schedules.py) and timed (tools/qkv_trickle_bench.py)
extern "C" __attribute__((visibility("default"))) int s2v_diag_qkv_qknorm(const void* A, const void* W, const void* bias, const void* nq_w, const void* nq_b,
                                                                           const void* nk_w, const void* nk_b, const float* cs, void* C, int32_t M, int32_t D,
                                                                           int32_t K, int32_t tok_per_batch, int32_t text_len, float eps, s2v_stream stream) {
    S2V_REQUIRE(A && W && bias && C && nq_w && nq_b && nk_w && nk_b, "s2v_diag_qkv_qknorm: null argument");
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.bias = bias; g.C = C; g.ldc = 3 * D; g.M = M; g.N = 3 * D; g.K = K;
    g.a_rows_padded = (int)rup(M, 256); g.w_rows_padded = (int)rup(3 * D, 256);
    g.tok_per_batch = tok_per_batch; g.text_len = text_len;
    g.qk_w[0] = nq_w; g.qk_b[0] = nq_b; g.qk_w[1] = nk_w; g.qk_b[1] = nk_b; g.qk_cs = cs; g.qk_D = D; g.qk_eps = eps;
    return launch_gemm_bf16(g, EPI_BIAS_QKNORM, (hipStream_t)stream);
}
#else
static const int g_fused_qk = 1;
#endif
// mx_out (fp8 engine, MFMA path): the attention kernel leaves its output as MX e4m3 in c->aq / c->hs for the out-projection instead of bf16 in Xn
static bool attn_mx_out(const s2v_ctx* c) {
    bool mx = c->fp8 && c->mfma && c->D % 128 == 0;
#ifdef S2V_DIAG
    mx = mx && g_fp8_mx;
#endif
    return mx;
}
// runtime LoRA: T = rnd(x . A^T) into the columns [K, K + N) of the rows of x (lora.hip); the GEMM that follows runs with K' = K + N
static int lora_down(s2v_ctx* c, char* x, int ldx, const char* A, int N, int K, hipStream_t st) {
    LoraDownArgs a{};
    a.x = x; a.ldx = ldx; a.A = A; a.lda = K; a.out = x + (int64_t)K * c->esz; a.ldo = ldx; a.M = (int)c->M; a.N = N; a.K = K;
    ProfScope ps(c, PK_LORA, st);
    return launch_lora_down(a, c->dtype, (c->mfma || c->h16) && K % 64 == 0, st);
}

// runtime LoRA beside e4m3 weights (s2v_ctx::flr): T = rnd(x^ . A^T) into the context's T buffer, x^ = the operand the base GEMM sees at the
// best precision in which it exists -- bf16 rows (mx_s null: Xn, or Hb without the MX form), or an MX image dequantised exactly (lora.hip)
static int lora_down_fp8(s2v_ctx* c, const void* x, int ldx, const unsigned char* mx_s, const char* A, int N, int K, hipStream_t st) {
    LoraDownArgs a{};
    a.x = x; a.ldx = ldx; a.A = A; a.lda = K; a.out = c->Tl; a.ldo = 3 * c->flr; a.M = (int)c->M; a.N = N; a.K = K;
    ProfScope ps(c, PK_LORA, st);
    if (!mx_s) return launch_lora_down(a, c->dtype, true, st);
    a.mx_s = mx_s; a.mx_rows = (int)c->Mpad;
    return launch_lora_down_mx(a, st);
}
// ... and the GEMM's side of it: the branch operands of GemmArgs (seg: output columns per adapter, 0 = one adapter)
static void lora_branch_fp8(const s2v_ctx* c, GemmArgs& g, const char* bs, int seg) {
    g.lora_t = c->Tl; g.lora_ldt = 3 * c->flr; g.lora_bs = bs; g.lora_r = c->flr; g.lora_seg = seg;
}

// where the operand of an adapted linear lives: the 16-bit rows with their pitch and, if its producer left one, the MX image (bytes [rows][K],
// block scales) the fp8 GEMM reads in place of them
struct LinIn {
    char* x; int ldx;
    const void* mx_q = nullptr; const unsigned char* mx_s = nullptr;
};
static const int PK_UNTIMED = -1;

// One of the four big linears of a layer, on the context's rows: lora: the weights carry an attached adapter (their context's lora_names is not
// empty), so the down-projection for the mode in force runs first -- beside e4m3 weights from the best-precision operand into the T buffer, the
// GEMM taking the branch operands; otherwise in place behind column K of the 16-bit rows, the GEMM running with K' = K + R.  g carries the
// destination and the epilogue's own fields; pk: the class the GEMM is timed as (PK_UNTIMED: not at all); prequant: linear_fp8
static int adapted_linear(s2v_ctx* c, const LayerW& w, int which, const LinIn& in, bool lora, GemmArgs g, int epi, bool prequant, int pk, hipStream_t st) {
    const LinShape s = lin_shape(which, c->D);
    const LinW& x = w.lin[which];
    const int K = (int)s.K, Kx = (int)s.pitch(c->lr);
    if (lora && c->flr > 0) {
        if (in.mx_s) S2V_TRY(lora_down_fp8(c, in.mx_q, K, in.mx_s, x.a, s.parts * c->flr, K, st));
        else S2V_TRY(lora_down_fp8(c, in.x, in.ldx, nullptr, x.a, s.parts * c->flr, K, st));
        lora_branch_fp8(c, g, x.bs, s.lora_seg());
    } else if (lora) {
        S2V_TRY(lora_down(c, in.x, in.ldx, x.a, s.parts * c->lr, K, st));
    }
    g.A = in.x; g.lda = in.ldx; g.W = x.w; g.ldw = Kx; g.bias = x.b; g.M = (int)c->M; g.N = (int)s.N; g.K = lora ? Kx : K;
    if (in.mx_s) { g.A = in.mx_q; g.mx_a_s = in.mx_s; g.mx_rows = (int)c->Mpad; }
    auto gemm = [&]() { return c->fp8 ? linear_fp8(c, g, epi, x.q, x.s, st, prequant) : linear(c, g, epi, st); };
    if (pk == PK_UNTIMED) return gemm();
    ProfScope ps(c, pk, st);
    return gemm();
}

// ---- attention: one QKV projection and one core for the single engine (run_attention) and the Ulysses shard (shard_front, shard_attention) ----
// May the per-head LayerNorm + rotary embedding of q and k ride in the QKV projection's epilogue (EPI_BIAS_QKNORM), on the rounded projection
// as the stand-alone kernel does?  The matrix-core kernels only, and rotary tables in the paired form (s2v_set_rope).  g_fused_qk is the A/B
// switch of the diagnostics build: 0 stand-alone kernel, 3 epilogue even for fp8 QK^T (run_attention)
static bool qk_epilogue_ok(const s2v_ctx* c) {
    return (c->mfma || c->h16) && c->D % 64 == 0 && (!c->have_rope || c->rope_paired) && g_fused_qk != 0;
}

static void set_qk_epilogue(const s2v_ctx* c, const LayerW& w, GemmArgs& g) {
    g.tok_per_batch = c->Ntok; g.text_len = c->T;
    g.qk_w[0] = w.nq_w; g.qk_b[0] = w.nq_b; g.qk_w[1] = w.nk_w; g.qk_b[1] = w.nk_b;
    g.qk_cs = c->have_rope ? c->rope_pk : nullptr;
    g.qk_D = c->D; g.qk_eps = 1e-6f;
}

// q/k LayerNorm + rotary embedding on the context's rows of QKV, without V^T: who wants it adds vt / vt_f16 / vt_amax
static QkNormRopeArgs qk_norm_args(const s2v_ctx* c, const LayerW& w) {
    QkNormRopeArgs q{};
    q.qkv = c->QKV; q.ld_qkv = 3 * c->D; q.B = c->B; q.H = c->cfg.num_heads; q.Ntok = c->Ntok; q.text_len = c->T; q.ntok_pad = c->ntok_pad;
    q.nq_w = w.nq_w; q.nq_b = w.nq_b; q.nk_w = w.nk_w; q.nk_b = w.nk_b; q.eps = 1e-6f;
    q.cos = c->have_rope ? c->rope_cos : nullptr; q.sin = c->have_rope ? c->rope_sin : nullptr;
    return q;
}

// Xn (row pitch pX) -> QKV on the context's rows.  lora: the weights carry an attached adapter (their context's lora_names is not empty) and the
// GEMM runs with K = pX behind the down-projection; qk_epi: EPI_BIAS_QKNORM; prequant: linear_fp8
static int qkv_proj(s2v_ctx* c, const LayerW& w, int pX, bool lora, bool qk_epi, bool prequant, hipStream_t st) {
    GemmArgs g{};
    g.C = c->QKV; g.ldc = 3 * c->D;
    if (qk_epi) set_qk_epilogue(c, w, g);
    // the branch beside the e4m3 GEMM: Xn holds the bf16 rows also under prequant (block_norm)
    return adapted_linear(c, w, LIN_QKV, {c->Xn, pX}, lora, g, qk_epi ? EPI_BIAS_QKNORM : EPI_BIAS, prequant, PK_QKV, st);
}

// what the callers of attn_core differ in: the q | k | v rows, heads and tokens per sample (the kernel and its formats are chosen on Ntok), the
// output rows and, fp8 engine (attn_mx_out), where the output goes as MX e4m3 instead: bytes, block scales, rows of the scale image
struct AttnOperands {
    const void* qkv; int ld_qkv, H, Ntok;
    void* out; int ld_out;
    unsigned char *mx_q, *mx_s; int64_t mx_rows;
};
// where q and k get their LayerNorm + rotary embedding: before the core (the projection's epilogue; a shard: at the latest before its exchange);
// by the core in the stand-alone pass over c->QKV, which writes V^T as well; by the core inside the MX quantisation of fp8 QK^T
enum { QK_DONE = 0, QK_STANDALONE = 1, QK_IN_QUANT = 2 };

// (q/k-norm,) V^T, (fp8 QK^T: q and k as MX e4m3,) attention.  w: the layer's norm weights, for QK_STANDALONE / QK_IN_QUANT
// steer: the record of a steered layer (s2v_attn_steer_arm) -- the attention launch is then attn_pp<STEER> (bf16) or the steered generic kernel (fp32)
// local: the record of a local layer (s2v_attn_local_arm) -- the attention launch is then attn_pp<LOCAL> (bf16) or the local generic kernel (fp32)
// smap: the map record of a steered layer while the context holds maps (s2v_attn_steer_set_maps) -- attn_pp<MAP> or the mapped generic kernel
static int attn_core(s2v_ctx* c, const AttnOperands& o, int qk, const LayerW* w, hipStream_t st, const AttnSteerRec* steer = nullptr,
                     const int* local = nullptr, bool box = false, const AttnSteerMapRec* smap = nullptr) {
    const bool mx = attn_mx_out(c), matrix = c->mfma || c->h16;
    // fp16 P / V^T is the four-wave kernels' (attn_q4h / attn_q4fh); short sequences run attn_pp on bf16 V^T
    const bool p16 = c->attn_p16 && c->mfma && (c->fp8_qk || attn_runs_q4(o.Ntok, mx));
    S2V_REQUIRE(!p16 || (int64_t)c->B * o.H <= VT_AMAX_WORDS, "attention: B * heads too large for the fp16 V^T");
    if (qk == QK_STANDALONE) {
        QkNormRopeArgs q = qk_norm_args(c, *w);
        q.vt = matrix ? c->VT : nullptr; q.vt_f16 = p16 ? 1 : 0; q.vt_amax = c->vt_amax;  // fp16 dtype: the pass moves fp16 bits
        ProfScope ps(c, PK_QKNORM, st);
        S2V_TRY(launch_qk_norm_rope(q, c->dtype, st));
    } else if (matrix) {
        ProfScope ps(c, PK_QKNORM, st);
        S2V_TRY(launch_v_transpose(o.qkv, o.ld_qkv, c->B, o.H, o.Ntok, c->VT, c->ntok_pad, st, p16 ? c->vt_amax : nullptr));
    }
    AttnArgs a{};
    a.qkv = o.qkv; a.ld_qkv = o.ld_qkv; a.vt = c->VT; a.ntok_pad = c->ntok_pad; a.out = o.out; a.ld_out = o.ld_out;
    a.B = c->B; a.H = o.H; a.Ntok = o.Ntok; a.scale = 0.125f;
    a.queue = c->attn_queue; a.num_cus = c->num_cus;  // launches of one context are ordered on its stream: one queue suffices
    a.p16 = p16 ? 1 : 0; a.vt_amax = c->vt_amax;
    // the split workspace of the geometry where this call fits it (every caller at the geometry's own token count and heads does); a call of
    // another shape through the AttnProcessor seam takes the process-wide one (attention_q4.hip), with the operator entries' restriction
    if (c->kv_ws && attn_kv_ws_bytes(attn_plan(o.Ntok, ATTN_FMT_Q4), (int64_t)c->B * o.H) <= c->kv_ws_bytes) { a.kv_ws = c->kv_ws; a.kv_ws_bytes = c->kv_ws_bytes; }
    a.stats = c->attn_stats;
    a.valu_only = c->cfg.force_simple;
    a.stagger = c->attn_stagger;
    a.order = c->attn_order;
    if (mx) { a.mx_q = o.mx_q; a.mx_s = o.mx_s; a.mx_rows = (int)o.mx_rows; }
    if (c->fp8_qk) {  // q (times scale * log2 e) and k as MX e4m3, QK^T on the scaled fp8 MFMA (the pass is timed with the V^T pass)
        const float prescale = a.scale * 1.4426950408889634f;
        a.q8 = c->q8; a.q8s = c->q8s; a.k8 = c->k8; a.k8s = c->k8s;
        ProfScope ps(c, PK_QKNORM, st);
        if (qk == QK_IN_QUANT) S2V_TRY(launch_qk_norm_quant_mx(qk_norm_args(c, *w), prescale, c->q8, c->q8s, c->k8, c->k8s, st));
        else S2V_TRY(launch_qk_quant_mx(o.qkv, o.ld_qkv, c->B, o.H, o.Ntok, c->ntok_pad, prescale, c->q8, c->q8s, c->k8, c->k8s, st));
    }
    ProfScope ps(c, PK_ATTN, st);
    a.clk = c->clk_cur;
    if (steer) {
        S2V_REQUIRE(!mx && !p16 && !c->fp8_qk && !c->h16, "attention: a steered layer on an engine the steered kernels do not serve");
        return c->mfma ? launch_attn_bf16_steer(a, steer, st) : launch_attn_simple_steer(a, steer, c->dtype, st);
    }
    if (smap) {
        S2V_REQUIRE(!mx && !p16 && !c->fp8_qk && !c->h16, "attention: a mapped layer on an engine the steered kernels do not serve");
        S2V_REQUIRE(o.Ntok == c->st_map_Ntok, "attention: the steering maps were made for another Ntok");
        return c->mfma ? launch_attn_bf16_steer_map(a, smap, st) : launch_attn_simple_steer_map(a, smap, c->dtype, st);
    }
    if (local) {
        S2V_REQUIRE(!mx && !p16 && !c->fp8_qk && !c->h16, "attention: a local layer on an engine the local kernels do not serve");
        S2V_REQUIRE(o.Ntok == c->la_Ntok, "attention: the local-attention table was made for another Ntok");
        if (box) return c->mfma ? launch_attn_bf16_box(a, local, st) : launch_attn_simple_box(a, local, c->dtype, st);   // box: `local` is the box record
        return c->mfma ? launch_attn_bf16_local(a, local, st) : launch_attn_simple_local(a, local, c->dtype, st);
    }
    if (c->fp8_qk) return launch_attn_q4f(a, true, st);
    if (c->mfma) return launch_attn_bf16(a, st);
    if (c->h16) return launch_attn_f16(a, st);   // fp16 dtype: q, k, V^T, P in fp16 on v_mfma_f32_32x32x16_f16
    return launch_attn_simple(a, c->dtype, st);
}

// Xn -> QKV -> (qk-norm, rope, V^T) -> attention -> Xn (reused as the attention output buffer; fp8 engine: MX e4m3 in aq / hs)
// w: the layer's weights -- c's own, or another context's of the same dtype / heads / weight_format (s2v_attn_forward_with)
// mass: an armed layer of the attention map -- the mass kernel follows the attention launch on the same stream.  c->QKV then holds q and k normed
// and rotated (QK_DONE: by the projection's epilogue; QK_STANDALONE: by the core's own pass) and nothing has written it since: V^T, the attention
// kernels and the MX output of the fp8 engine only read it.  QK_IN_QUANT (fp8 QK^T) leaves q and k un-normed in c->QKV: s2v_attn_map_arm refuses it
static int am_launch(s2v_ctx* c, hipStream_t st) {
    S2V_REQUIRE(c->am_on && c->am_acc && !c->fp8_qk, "attention map: an armed layer without s2v_attn_map_enable, or under fp8 QK^T");
    AttnMassArgs a{};
    a.qkv = c->QKV; a.ld_qkv = 3 * c->D; a.B = c->B; a.H = c->cfg.num_heads; a.Ntok = c->Ntok;
    a.q0 = c->T + c->R; a.nq = c->V; a.n = c->am_n;
    for (int r = 0; r < c->am_n; ++r) { a.k0[r] = c->am_k0[r]; a.k1[r] = c->am_k1[r]; }
    a.out = c->am_acc; a.accumulate = 1;
    return launch_attn_mass(a, c->dtype, (c->mfma || c->h16) ? 0 : 1, st);
}

static int run_attention(s2v_ctx* c, const LayerW& w, hipStream_t st, bool prequant = false, bool lora = false, bool mass = false, bool steer = false,
                         bool local = false) {
    const int D = c->D, pX = D + 3 * c->lr;
    // fp8 QK^T (weight_format 2 / 3 beyond its token threshold): q and k reach the attention kernel only as MX e4m3 images, so their LayerNorm + rotary
    // embedding ride in the pass that makes the images (qk_norm_quant_mx_k: the same bytes moved, the same bits produced) and the projection keeps the plain
    // bias epilogue -- its exposed q/k-norm epilogue is 20-25 % of an fp8 tile, whose K loop is half as long as the bf16 one
    const bool epi_ok = qk_epilogue_ok(c), norm_in_quant = epi_ok && c->fp8_qk && g_fused_qk != 3;
    S2V_TRY(qkv_proj(c, w, pX, lora, epi_ok && !norm_in_quant, prequant, st));
    const AttnOperands o{c->QKV, 3 * D, c->cfg.num_heads, c->Ntok, c->Xn, pX, (unsigned char*)c->aq, c->hs, c->Mpad};
    S2V_REQUIRE(!steer || c->st_tab, "attention: a steered layer without s2v_attn_steer_enable");
    S2V_REQUIRE(!local || c->la_tab, "attention: a local layer without s2v_attn_local_enable");
    const bool box = local && c->la_kind == 1;
    S2V_REQUIRE(!box || c->la_box, "attention: a box layer without s2v_attn_local_set_box");
    const bool maps = steer && c->st_kind == 1;
    S2V_REQUIRE(!maps || c->st_map, "attention: a mapped layer without s2v_attn_steer_set_maps");
    S2V_TRY(attn_core(c, o, norm_in_quant ? QK_IN_QUANT : epi_ok ? QK_DONE : QK_STANDALONE, &w, st, steer && !maps ? c->st_tab : nullptr,
                      !local ? nullptr : box ? c->la_box : c->la_tab, box, maps ? c->st_map : nullptr));
    return mass ? am_launch(c, st) : 0;
}

// the pieces of a block on the packed residual buffer X (rows: the context's M), in the order run_block launches them
static int block_norm(s2v_ctx* c, int l, int half, const char* mod_base /* [B][mod_stride] rows of this layer's norm1 */, int64_t mod_stride,
                      hipStream_t st, bool* prequant_out) {
    const LayerW& w = c->layers[l];
    const int D = c->D;
    const int64_t E = c->esz;
    const char* mb = mod_base + (int64_t)half * c->mc * D * E;
    LnModArgs n{};
    n.x = c->X; n.ldx = D; n.y = c->Xn; n.ldy = D + 3 * c->lr;
    n.w = half ? w.ln2_w : w.ln1_w; n.b = half ? w.ln2_b : w.ln1_b; n.eps = c->cfg.norm_eps;
    n.shift_vid = mb; n.scale_vid = mb + D * E; n.shift_txt = mb + 3 * D * E; n.scale_txt = mb + 4 * D * E;
    n.mod_stride = (int)mod_stride; n.B = c->B; n.Ntok = c->Ntok; n.text_len = c->T; n.D = D;
    if (c->mc == 9) { n.shift_ref = mb + 6 * D * E; n.scale_ref = mb + 7 * D * E; n.ref_len = c->R; }
    // fp8 linears: the LayerNorm output feeds exactly one projection (QKV / FF1), so it is quantised where it is produced
    bool prequant = c->fp8;
#ifdef S2V_DIAG
    prequant = prequant && g_fused_q8;
#endif
    if (prequant) { n.q8 = c->aq; n.q8_scale = c->aq_scale; n.q8_keep_y = (c->flr > 0 && c->lora_on()) ? 1 : 0; }
    *prequant_out = prequant;
    ProfScope ps(c, PK_LNMOD, st);
    return launch_ln_modulate(n, c->dtype, st);
}

// the gate + residual epilogue of the out-projection (half 0) / FF2 (half 1)
static GemmArgs block_gate(const s2v_ctx* c, int half, const char* mod_base, int64_t mod_stride) {
    const int D = c->D;
    const int64_t E = c->esz;
    const char* mb = mod_base + (int64_t)half * c->mc * D * E;
    GemmArgs g{};
    g.X = c->X; g.ldx = D; g.gate_vid = mb + 2 * D * E; g.gate_txt = mb + 5 * D * E; g.gate_stride = (int)mod_stride;
    g.tok_per_batch = c->Ntok; g.text_len = c->T; g.M = (int)c->M; g.N = D;
    if (c->mc == 9) { g.gate_ref = mb + 8 * D * E; g.ref_len = c->R; }
    return g;
}

// the out-projection of what run_attention / the shard's O exchange left: Xn, or (attn_mx_out) the MX image in aq / hs, against the layer's LIN_OUT behind
// the adapter's down-projection.  g carries the destination and the epilogue's own fields; timed: the GEMM counts as PK_OUT (the block, not the
// AttnProcessor seam)
static int out_proj(s2v_ctx* c, const LayerW& w, bool lora, GemmArgs g, int epi, bool timed, hipStream_t st) {
    LinIn in{c->Xn, c->D + 3 * c->lr};
    if (attn_mx_out(c)) { in.mx_q = c->aq; in.mx_s = c->hs; }
    return adapted_linear(c, w, LIN_OUT, in, lora, g, epi, false, timed ? PK_OUT : PK_UNTIMED, st);
}

static int block_ff(s2v_ctx* c, int l, GemmArgs g, bool prequant, hipStream_t st) {
    const LayerW& w = c->layers[l];
    const int D = c->D, pX = D + 3 * c->lr, pH = 4 * D + c->lr;
    const bool lora = c->lora_on();
    GemmArgs f{};
    f.C = c->Hb; f.ldc = pH;
    bool mx = c->fp8 && (4 * D) % 128 == 0;
#ifdef S2V_DIAG
    mx = mx && g_fp8_mx;
#endif
    if (mx) { f.mx_out_q = c->hq; f.mx_out_s = c->hs; f.mx_rows = (int)c->Mpad; }
    S2V_TRY(adapted_linear(c, w, LIN_FF1, {c->Xn, pX}, lora, f, EPI_BIAS_GELU, prequant, PK_FF1, st));
    LinIn h{c->Hb, pH};  // FF2: the operand is the FF1 epilogue's MX image (or, without the MX form, the bf16 rows in Hb)
    if (mx) { h.mx_q = c->hq; h.mx_s = c->hs; }
    return adapted_linear(c, w, LIN_FF2, h, lora, g, EPI_BIAS_GATE_RES, false, PK_FF2, st);
}

static int run_block(s2v_ctx* c, int l, const char* mod_base /* [B][mod_stride] rows of this layer's norm1 */,
                     int64_t mod_stride, hipStream_t st) {
    for (int half = 0; half < 2; ++half) {
        bool prequant = false;
        S2V_TRY(block_norm(c, l, half, mod_base, mod_stride, st, &prequant));
        const GemmArgs g = block_gate(c, half, mod_base, mod_stride);
        if (half == 0) {
            S2V_TRY(run_attention(c, c->layers[l], st, prequant, c->lora_on(), (c->am_run >> l) & 1, (c->st_run >> l) & 1, (c->la_run >> l) & 1));
            S2V_TRY(out_proj(c, c->layers[l], c->lora_on(), g, EPI_BIAS_GATE_RES, true, st));
        } else {
            S2V_TRY(block_ff(c, l, g, prequant, st));
        }
    }
    return 0;
}

// time embedding, every modulation of the step, and the residual streams [text | ref | video] of each sample in X (a shard: this rank's rows
// [T_r | R_r | V_r]; the latent is patchified whole and the rank's V_r patch rows embedded)
// latents: sample b reads the latent at (b mod n_lat) * lat_bstride elements (n_lat = 0: at b * lat_bstride)
// video_only (the step cache's REUSE forward): of the modulations only the norm_out rows -- the last 2 D rows of the stack, left compact as
// [B][2 D] at the start of c->mod -- and of the streams only the video rows; the text and reference rows of X are not written
static int embed_streams(s2v_ctx* c, const void* latents, int64_t lat_bstride, int n_lat, const float* t_dev, hipStream_t st, bool video_only = false) {
    const int D = c->D, B = c->B;
    const int64_t E = c->esz;
    // 1. timestep embedding + every AdaLN modulation of the step in one batched GEMV (temb is block-invariant)
    S2V_TRY(launch_time_embed(t_dev, B, D, c->te1_w, c->te1_b, c->te2_w, c->te2_b, c->temb, c->tmp_te, c->emb, c->dtype, st));
    {
        ProfScope ps(c, PK_OTHER, st);  // the step's modulation GEMV: every norm1 / norm2 / norm_out linear in one launch
        const int64_t r0 = c->mod_rows - 2 * D;   // norm_out's rows
        if (video_only) S2V_TRY(launch_mod_gemv(c->emb, B, c->temb, c->mod_w + r0 * c->temb * E, c->mod_b + r0 * E, 2 * D, c->mod, c->dtype, st));
        else S2V_TRY(launch_mod_gemv(c->emb, B, c->temb, c->mod_w, c->mod_b, c->mod_rows, c->mod, c->dtype, st));
    }
    // 2. residual streams: [text | ref | video] per sample
    const int K = c->cfg.in_channels * 4;
    S2V_TRY(launch_patchify(latents, lat_bstride, B, c->F, c->cfg.in_channels, c->H, c->W, c->patches, c->dtype, st, n_lat));
    for (int b = 0; b < B; ++b) {
        char* xb = c->X + (int64_t)b * c->Ntok * D * E;
        if (!video_only) {
            S2V_TRY(launch_copy_rows(c->e0 + (int64_t)b * c->T * D * E, D, nullptr, 0, xb, D, c->T, D, c->dtype, st));
            S2V_TRY(launch_copy_rows(c->e1_cur + (b % c->n_ref) * c->e1_stride, D, nullptr, 0, xb + (int64_t)c->T * D * E, D, c->R, D, c->dtype, st));
        }
        char* xv = xb + (int64_t)(c->T + c->R) * D * E;
        GemmArgs g{};
        g.A = c->patches + ((int64_t)b * c->gV + c->v0) * K * E; g.lda = K; g.W = c->patch_w; g.ldw = K; g.bias = c->patch_b;
        g.C = xv; g.ldc = D; g.M = c->V; g.N = D; g.K = K;
        S2V_TRY(linear(c, g, EPI_BIAS, st));
        if (!c->cfg.use_rope) S2V_TRY(launch_copy_rows(xv, D, c->pos_tab, D, xv, D, c->V, D, c->dtype, st));
    }
    return 0;
}

// final norms + projection on the video rows of X -> c->proj [B * V][Cout]
// compact_mod: norm_out's modulation sits as [B][2 D] at the start of c->mod (embed_streams with video_only), not at its place in the stack
static int tail_proj(s2v_ctx* c, hipStream_t st, bool compact_mod = false) {
    const int D = c->D, B = c->B;
    const int64_t E = c->esz;
    const char* mo = compact_mod ? c->mod : c->mod + (int64_t)2 * c->L * c->mc * D * E;
    TailNormArgs t{};
    t.x = c->X; t.ldx = D; t.y = c->tailn; t.ldy = D; t.w1 = c->nf_w; t.b1 = c->nf_b; t.w2 = c->no_w; t.b2 = c->no_b;
    t.eps = c->cfg.norm_eps; t.shift = mo; t.scale = mo + D * E; t.mod_stride = compact_mod ? 2 * D : (int)c->mod_rows;
    t.B = B; t.Ntok = c->Ntok; t.row0 = c->T + c->R; t.V = c->V; t.D = D;
    S2V_TRY(launch_tail_norm(t, c->dtype, st));
    const int Co = c->cfg.out_channels * 4;
    GemmArgs g{};
    g.A = c->tailn; g.lda = D; g.W = c->po_w; g.ldw = D; g.bias = c->po_b; g.C = c->proj; g.ldc = Co;
    g.M = B * c->V; g.N = Co; g.K = D;
    return linear(c, g, EPI_BIAS, st);
}

// the step cache's launch on the video rows of X (rows [T + R, T + R + V) of every sample) against a dense buffer
static int sc_launch(s2v_ctx* c, int op, char* cache, char* keep2, hipStream_t st) {
    return launch_step_cache(op, c->X + (int64_t)(c->T + c->R) * c->D * c->esz, (int64_t)c->Ntok * c->D, cache, keep2, c->B, (int64_t)c->V * c->D, c->dtype, st);
}
// the mode armed for the forward that is about to run (s2v_step_cache_arm): taken once per entry call, outside any capture
static int sc_take_arm(s2v_ctx* c) {
    const int m = c->sc_on ? c->sc_arm : S2V_STEP_FULL;
    c->sc_arm = S2V_STEP_FULL;
    if (m == S2V_STEP_CAPTURE) c->sc_valid = false;   // valid again once the forward is on the stream (sc_done)
    return m;
}
static int sc_done(s2v_ctx* c, int mode, int r) {
    if (r == 0 && mode == S2V_STEP_CAPTURE) c->sc_valid = true;
    return r;
}
// the layer mask armed for the forward that is about to run (s2v_attn_map_arm): one-shot, taken once per entry call, outside any capture
static uint64_t am_take_arm(s2v_ctx* c) {
    const uint64_t m = c->am_on ? c->am_arm : 0;
    c->am_arm = 0;
    return m;
}
// the host count: one per armed layer launch of a forward that is on the stream (a replayed graph runs them without running this code's body)
// the steer layer mask armed for the forward that is about to run (s2v_attn_steer_arm): one-shot as well
static uint64_t st_take_arm(s2v_ctx* c) {
    const uint64_t m = c->st_on ? c->st_arm : 0;
    c->st_arm = 0;
    return m;
}
// the local layer mask armed for the forward that is about to run (s2v_attn_local_arm): one-shot as well
static uint64_t la_take_arm(s2v_ctx* c) {
    const uint64_t m = c->la_on ? c->la_arm : 0;
    c->la_arm = 0;
    return m;
}
static int am_done(s2v_ctx* c, uint64_t am, int r) {
    if (r == 0) c->am_count += __builtin_popcountll(am);
    return r;
}

// mode: S2V_STEP_* (include/s2v_hip.h); FULL is the forward as it is without a step cache
// am: the layers whose attention the mass kernel follows (s2v_attn_map_arm; 0: the launches of a forward without the feature)
static int forward_impl(s2v_ctx* c, const void* latents, int64_t lat_bstride, int n_lat, const float* t_dev, void* out,
                        hipStream_t st, int mode = S2V_STEP_FULL, uint64_t am = 0, uint64_t sm = 0, uint64_t lm = 0) {
    S2V_REQUIRE(c->ws && c->finalized && c->have_cond, "transformer_forward: geometry, weights and conditioning required");
    S2V_REQUIRE(!c->cfg.use_rope || c->have_rope, "transformer_forward: RoPE tables missing (s2v_set_rope)");
    S2V_REQUIRE(c->cfg.use_rope || c->have_pos, "transformer_forward: sincos table missing (s2v_set_pos_embed)");
    S2V_REQUIRE(!c->shard, "transformer_forward: a shard context (s2v_set_shard) runs the staged step only (s2v_shard_step_* / s2v_denoise_step_ulysses)");
    const int D = c->D;
    const int64_t E = c->esz;
    const bool reuse = mode == S2V_STEP_REUSE;
    S2V_REQUIRE(mode == S2V_STEP_FULL || (c->sc_on && c->sc_delta), "transformer_forward: a step-cache mode without s2v_step_cache_enable");
    S2V_REQUIRE(!reuse || c->sc_valid, "transformer_forward: S2V_STEP_REUSE without a captured residual");
    S2V_REQUIRE(!am || !reuse, "transformer_forward: an attention map is armed (s2v_attn_map_arm) together with S2V_STEP_REUSE: the block stack does not run");
    S2V_REQUIRE(!am || (c->am_on && !c->fp8_qk), "transformer_forward: an attention map is armed without s2v_attn_map_enable, or while fp8 QK^T is active");
    if (lm) {   // lm: the layers whose attention launch is the local kernel (s2v_attn_local_arm; 0: the launches of a forward without the feature)
        S2V_REQUIRE(!reuse, "transformer_forward: local attention is armed (s2v_attn_local_arm) together with S2V_STEP_REUSE: the block stack does not run");
        S2V_REQUIRE(!am, "transformer_forward: local attention is armed (s2v_attn_local_arm) together with an attention map (s2v_attn_map_arm): the map reads "
                         "the un-windowed softmax");
        S2V_REQUIRE(!sm, "transformer_forward: local attention is armed (s2v_attn_local_arm) together with attention steering (s2v_attn_steer_arm)");
        S2V_REQUIRE(c->la_on && c->la_tab && c->la_Ntok == c->Ntok, "transformer_forward: local attention is armed without s2v_attn_local_enable");
        S2V_TRY(la_check(c, "transformer_forward (local attention armed)"));
    }
    if (sm) {   // sm: the layers whose attention launch is the steered kernel (s2v_attn_steer_arm; 0: the launches of a forward without the feature)
        S2V_REQUIRE(!reuse, "transformer_forward: attention steering is armed (s2v_attn_steer_arm) together with S2V_STEP_REUSE: the block stack does not run");
        S2V_REQUIRE(!am, "transformer_forward: attention steering is armed (s2v_attn_steer_arm) together with an attention map (s2v_attn_map_arm): the map reads "
                         "the un-steered softmax");
        S2V_REQUIRE(c->st_on && c->st_tab, "transformer_forward: attention steering is armed without s2v_attn_steer_enable");
        S2V_TRY(st_check(c, "transformer_forward (attention steering armed)"));
    }
    S2V_TRY(embed_streams(c, latents, lat_bstride, n_lat, t_dev, st, reuse));
    if (mode == S2V_STEP_CAPTURE) S2V_TRY(sc_launch(c, SC_KEEP, c->sc_delta, c->sc_in, st));   // IN
    else if (c->sc_in) S2V_TRY(sc_launch(c, SC_KEEP, c->sc_in, nullptr, st));                  // enable 2: IN of every forward, for the read-out
    if (reuse) {
        S2V_TRY(sc_launch(c, SC_ADD, c->sc_delta, nullptr, st));                               // X_video = rnd(IN' + delta)
    } else {
        // 3. blocks
        c->am_run = am; c->st_run = sm; c->la_run = lm;
        for (int l = 0; l < c->L; ++l) {
            const int r = run_block(c, l, c->mod + (int64_t)(2 * l) * c->mc * D * E, c->mod_rows, st);
            if (r != 0) { c->am_run = 0; c->st_run = 0; c->la_run = 0; return r; }
        }
        c->am_run = 0; c->st_run = 0; c->la_run = 0;
        if (mode == S2V_STEP_CAPTURE) S2V_TRY(sc_launch(c, SC_SUB, c->sc_delta, nullptr, st)); // delta = rnd(OUT - IN)
    }
    // 4. tail
    S2V_TRY(tail_proj(c, st, reuse));
    const int Co = c->cfg.out_channels * 4;
    S2V_TRY(launch_unpatchify(c->proj, Co, c->V, out, c->B, c->F, c->cfg.out_channels, c->H, c->W, c->dtype, st));
    return 0;
}

extern "C" int s2v_transformer_forward(s2v_ctx* c, const void* latents, int64_t lat_bstride, const float* timesteps_dev,
                                       void* out, s2v_stream stream) {
    S2V_REQUIRE(c && latents && timesteps_dev && out, "s2v_transformer_forward: null argument");
    const int mode = sc_take_arm(c);
    const uint64_t am = am_take_arm(c), sm = st_take_arm(c), lm = la_take_arm(c);
    return am_done(c, am, sc_done(c, mode, forward_impl(c, latents, lat_bstride, 0, timesteps_dev, out, (hipStream_t)stream, mode, am, sm, lm)));
}

extern "C" int s2v_transformer_forward_videos(s2v_ctx* c, const void* latents, int32_t n_lat, const float* timesteps_dev, void* out,
                                              s2v_stream stream) {
    S2V_REQUIRE(c && latents && timesteps_dev && out, "s2v_transformer_forward_videos: null argument");
    const int mode = sc_take_arm(c);
    const uint64_t am = am_take_arm(c), sm = st_take_arm(c), lm = la_take_arm(c);
    S2V_REQUIRE(c->ws && n_lat >= 1 && c->B % n_lat == 0, "s2v_transformer_forward_videos: n_lat must divide the geometry's batch (sample j embeds latent j mod n_lat)");
    return am_done(c, am, sc_done(c, mode, forward_impl(c, latents, (int64_t)c->F * c->cfg.in_channels * c->H * c->W, n_lat, timesteps_dev, out, (hipStream_t)stream, mode, am, sm, lm)));
}

// the residual streams of every sample between the caller's dense tensors (s0: n0 rows, s1: n1 rows, video: V rows per sample; n0 + n1 = T + R)
// and a packed buffer [B][n0 | n1 | V] of row pitch `pitch` elements -- into it, or out of it.  A stream without rows is skipped
static int copy_streams(s2v_ctx* c, bool to_packed, char* packed, int pitch, char* s0, int n0, char* s1, int n1, char* video, hipStream_t st) {
    const int D = c->D;
    const int64_t E = c->esz;
    char* const src[3] = {s0, s1, video};
    const int n[3] = {n0, n1, c->V};
    for (int b = 0; b < c->B; ++b) {
        char* pk = packed + (int64_t)b * c->Ntok * pitch * E;
        for (int i = 0; i < 3; pk += (int64_t)n[i] * pitch * E, ++i) {
            if (!n[i]) continue;
            char* t = src[i] + (int64_t)b * n[i] * D * E;
            if (to_packed) S2V_TRY(launch_copy_rows(t, D, nullptr, 0, pk, pitch, n[i], D, c->dtype, st));
            else S2V_TRY(launch_copy_rows(pk, pitch, nullptr, 0, t, D, n[i], D, c->dtype, st));
        }
    }
    return 0;
}

extern "C" int s2v_block_forward(s2v_ctx* c, int32_t layer, const void* hidden, const void* enc0, const void* enc1,
                                 const void* temb, void* out_hidden, void* out_enc0, void* out_enc1, s2v_stream stream) {
    S2V_REQUIRE(c && c->ws && c->finalized, "s2v_block_forward: geometry and weights required");
    S2V_REQUIRE(!c->shard, "s2v_block_forward: a shard context (s2v_set_shard) runs the staged step only");
    S2V_REQUIRE(st_take_arm(c) == 0, "s2v_block_forward: attention steering is armed (s2v_attn_steer_arm): the block and AttnProcessor seams run no steered attention");
    S2V_REQUIRE(la_take_arm(c) == 0, "s2v_block_forward: local attention is armed (s2v_attn_local_arm): the block and AttnProcessor seams run no local attention");
    S2V_REQUIRE(layer >= 0 && layer < c->L, "s2v_block_forward: bad layer");
    S2V_REQUIRE(hidden && enc1 && temb && out_hidden && out_enc1, "s2v_block_forward: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int D = c->D, B = c->B;
    const int64_t E = c->esz;
    // this layer's two modulation linears are contiguous in the stack: rows [(2l)*6D, (2l+2)*6D)
    const int64_t r0 = (int64_t)(2 * layer) * c->mc * D;
    char* modl = c->mod;  // [B][12D]
    S2V_TRY(launch_mod_gemv(temb, B, c->temb, c->mod_w + r0 * c->temb * E, c->mod_b + r0 * E, 2 * c->mc * D, modl, c->dtype, st));
    S2V_TRY(copy_streams(c, true, c->X, D, (char*)enc0, c->T, (char*)enc1, c->R, (char*)hidden, st));
    S2V_TRY(run_block(c, layer, modl, 2 * c->mc * D, st));
    return copy_streams(c, false, c->X, D, (char*)out_enc0, c->T, (char*)out_enc1, c->R, (char*)out_hidden, st);
}

// the AttnProcessor seam on c's geometry and workspace with the weights w (c's own layer, or another context's); encoder = [text | ref] of each sample
static int attn_forward_impl(s2v_ctx* c, const LayerW& w, bool lora, const void* hidden, const void* encoder, void* out_hidden, void* out_encoder,
                             hipStream_t st) {
    const int D = c->D, TR = c->T + c->R;
    S2V_TRY(copy_streams(c, true, c->Xn, D + 3 * c->lr, nullptr, 0, (char*)encoder, TR, (char*)hidden, st));
    S2V_TRY(run_attention(c, w, st, false, lora));
    GemmArgs g{};
    g.C = c->Hb; g.ldc = D;
    S2V_TRY(out_proj(c, w, lora, g, EPI_BIAS, false, st));  // the same operands run_block feeds its out-projection
    return copy_streams(c, false, c->Hb, D, nullptr, 0, (char*)out_encoder, TR, (char*)out_hidden, st);
}

extern "C" int s2v_attn_forward(s2v_ctx* c, int32_t layer, const void* hidden, const void* encoder, void* out_hidden,
                                void* out_encoder, s2v_stream stream) {
    S2V_REQUIRE(c && c->ws && c->finalized, "s2v_attn_forward: geometry and weights required");
    S2V_REQUIRE(!c->shard, "s2v_attn_forward: a shard context (s2v_set_shard) runs the staged step only");
    S2V_REQUIRE(st_take_arm(c) == 0, "s2v_attn_forward: attention steering is armed (s2v_attn_steer_arm): the AttnProcessor seams run no steered attention");
    S2V_REQUIRE(la_take_arm(c) == 0, "s2v_attn_forward: local attention is armed (s2v_attn_local_arm): the AttnProcessor seams run no local attention");
    S2V_REQUIRE(layer >= 0 && layer < c->L, "s2v_attn_forward: bad layer");
    S2V_REQUIRE(hidden && encoder && out_hidden && out_encoder, "s2v_attn_forward: null argument");
    return attn_forward_impl(c, c->layers[layer], c->lora_on(), hidden, encoder, out_hidden, out_encoder, (hipStream_t)stream);
}

extern "C" int s2v_attn_forward_with(s2v_ctx* c, const s2v_ctx* wc, int32_t layer, const void* hidden, const void* encoder, void* out_hidden,
                                     void* out_encoder, s2v_stream stream) {
    S2V_REQUIRE(c && wc, "s2v_attn_forward_with: null context");
    S2V_REQUIRE(c->ws, "s2v_attn_forward_with: the workspace context has no geometry (s2v_set_geometry)");
    S2V_REQUIRE(!c->shard && !wc->shard, "s2v_attn_forward_with: a shard context (s2v_set_shard) runs the staged step only");
    S2V_REQUIRE(st_take_arm(c) == 0, "s2v_attn_forward_with: attention steering is armed (s2v_attn_steer_arm): the AttnProcessor seams run no steered attention");
    S2V_REQUIRE(la_take_arm(c) == 0, "s2v_attn_forward_with: local attention is armed (s2v_attn_local_arm): the AttnProcessor seams run no local attention");
    S2V_REQUIRE(wc->finalized && wc->kind != S2V_CTX_ATTN_WORKSPACE, "s2v_attn_forward_with: the weights are not loaded (s2v_finalize_weights)");
    S2V_REQUIRE(wc->dtype == c->dtype, "s2v_attn_forward_with: the weights context has another dtype");
    S2V_REQUIRE(wc->cfg.num_heads == c->cfg.num_heads && wc->D == c->D, "s2v_attn_forward_with: the weights context has another num_heads / inner dim");
    S2V_REQUIRE(wc->cfg.weight_format == c->cfg.weight_format, "s2v_attn_forward_with: the weights context has another weight_format");
    S2V_REQUIRE(wc->lora_cap == c->lora_cap, "s2v_attn_forward_with: the weights context has another lora_runtime_rank (the workspace owns the activation "
                                             "pitch, the weights context the tails and the A stacks: create both with the same value)");
    S2V_REQUIRE(layer >= 0 && layer < (int)wc->layers.size(), "s2v_attn_forward_with: bad layer");
    S2V_REQUIRE(hidden && encoder && out_hidden && out_encoder, "s2v_attn_forward_with: null argument");
    return attn_forward_impl(c, wc->layers[layer], wc->lora_on(), hidden, encoder, out_hidden, out_encoder, (hipStream_t)stream);
}

// ---- runtime LoRA: attach / rescale / detach after s2v_finalize_weights (include/s2v_hip.h) ---------------------------------------------
static int lora_checks(s2v_ctx* c, const char* fn) {
    static thread_local std::string m;
    auto fail = [&](const char* why) { m = std::string(fn) + ": " + why; return s2v_fail(__FILE__, __LINE__, m.c_str(), -1); };
    if (c->lora_cap == 0) return fail("the runtime adapter mode is off (lora_runtime_rank = 0: this context merges LoRA at load time, s2v_merge_lora)");
    if (c->cfg.weight_format != 0 && c->flr == 0)
        return fail("fp8 weight formats run a runtime adapter branch only when the context was created for it (lora_runtime_fp8 / S2V_LORA_FP8_BRANCH in "
                    "reserved[1]); without the flag weight_format must be 0, the model dtype");
    if (c->shard) return fail("a shard context (s2v_set_shard) does not support runtime adapters");
    if (c->kind == S2V_CTX_ATTN_WORKSPACE) return fail("a workspace context (S2V_CTX_ATTN_WORKSPACE) holds no weights");
    if (!c->finalized) return fail("the weights are not finalized (before s2v_finalize_weights use s2v_merge_lora)");
    return 0;
}

// the base copy of a re-merged slot: same offset inside the copy of its region
static char* lora_base_of(s2v_ctx* c, const char* live) {
    if (live >= c->mod_w && live < c->mod_w + c->base_mod_bytes) return c->base_mod + (live - c->mod_w);
    if (live >= c->patch_w && live < c->patch_w + c->base_patch_bytes) return c->base_patch + (live - c->patch_w);
    if (live >= c->text_w && live < c->text_w + c->base_text_bytes) return c->base_text + (live - c->text_w);
    return nullptr;
}

// the values of one adapter: branch weights get A into the stack (with_a) and rnd(scale * B) into the tail; re-merged weights are rebuilt
// from their base copy with s2v_merge_lora's arithmetic
static int lora_write(s2v_ctx* c, const char* name, Slot& s, const float* A, const float* B, int rank, float scale, bool with_a, hipStream_t st) {
    const int64_t E = c->esz;
    if (s.lora == LORA_BRANCH) {
        if (with_a) S2V_TRY(launch_lora_pack_a(A, rank, c->lr + c->flr, (int)s.cols, s.lora_a, s.cols, c->dtype, st));
        if (s.lora_bs) return launch_lora_pack_b(B, rank, c->flr, (int)s.rows, scale, s.lora_bs, c->flr, c->dtype, st);  // beside e4m3 weights
        return launch_lora_pack_b(B, rank, c->lr, (int)s.rows, scale, s.dst + s.tail_col * E, s.ld, c->dtype, st);
    }
    char* base = lora_base_of(c, s.dst);
    S2V_REQUIRE(base, "s2v_lora_attach: no base copy for this weight");
    const int64_t bytes = s.rows * s.ld * E;
    S2V_CHECK_HIP(hipMemcpyAsync(s.dst, base, (size_t)bytes, hipMemcpyDeviceToDevice, st));
    // lora_adaln_scope 1: the reference-image copy of chunks 0-2 sits right behind the six chunks and starts as their base values
    if (c->mc == 9 && is_adaln_linear(name)) S2V_CHECK_HIP(hipMemcpyAsync(s.dst + bytes, base, (size_t)(bytes / 2), hipMemcpyDeviceToDevice, st));
    // patch_embed.proj / text_proj made the hoisted conditioning: it has to be set again (a captured step reads the buffers it rewrites)
    if (!is_adaln_linear(name)) c->have_cond = false;
    return merge_into(c, name, s, A, B, rank, scale, st);
}

static int lora_find(s2v_ctx* c, const char* fn, const char* name, int rank, Slot** out) {
    static thread_local std::string m;
    auto it = c->slots.find(name);
    if (it == c->slots.end() || it->second.lora == LORA_NONE) {
        m = std::string(fn) + (it == c->slots.end() ? ": unknown tensor name: " : ": not a LoRA target of this context: ") + name;
        return s2v_fail(__FILE__, __LINE__, m.c_str(), -3);
    }
    if (rank > c->lora_cap) {
        m = std::string(fn) + ": rank " + std::to_string(rank) + " is over the capacity lora_runtime_rank = " + std::to_string(c->lora_cap) + " of this context (" + name + ")";
        return s2v_fail(__FILE__, __LINE__, m.c_str(), -1);
    }
    *out = &it->second;
    return 0;
}

// the attached state into the arena (stream-ordered behind the values it describes)
static int lora_write_hdr(s2v_ctx* c, hipStream_t st) {
    c->lora_hdr_host[0] = (int32_t)(c->lora_names.size() + (size_t)c->lora_replica);
    c->lora_hdr_host[1] = c->lora_rank;
    memcpy(&c->lora_hdr_host[2], &c->lora_scale, sizeof(float));
    S2V_CHECK_HIP(hipMemcpyAsync(c->lora_hdr, c->lora_hdr_host, sizeof(c->lora_hdr_host), hipMemcpyHostToDevice, st));
    return 0;
}

static void lora_drop_graph(s2v_ctx* c) {
    if (c->any_graph()) (void)hipDeviceSynchronize();  // the graph may still be replaying
    drop_graph(c);
}

extern "C" int s2v_lora_attach(s2v_ctx* c, const char* name, const float* A, const float* B, int32_t rank, float scale, s2v_stream stream) {
    S2V_REQUIRE(c && name && A && B && rank > 0, "s2v_lora_attach: bad argument");
    S2V_TRY(lora_checks(c, "s2v_lora_attach"));
    sc_invalidate(c);
    Slot* s = nullptr;
    S2V_TRY(lora_find(c, "s2v_lora_attach", name, rank, &s));
    S2V_TRY(lora_write(c, name, *s, A, B, rank, scale, true, (hipStream_t)stream));
    lora_drop_graph(c);   // with the first adapter the adapted GEMMs change to K' = K + R: the captured step is re-captured at its next use
    if (c->lora_replica) { c->lora_replica = 0; }   // a replica that attaches itself owns its state from here on
    c->lora_names[name] = rank;
    c->lora_rank = rank; c->lora_scale = scale;
    return lora_write_hdr(c, (hipStream_t)stream);
}

extern "C" int s2v_lora_set_scale(s2v_ctx* c, const char* name, const float* A, const float* B, int32_t rank, float scale, s2v_stream stream) {
    S2V_REQUIRE(c && name && A && B && rank > 0, "s2v_lora_set_scale: bad argument");
    S2V_TRY(lora_checks(c, "s2v_lora_set_scale"));
    sc_invalidate(c);
    Slot* s = nullptr;
    S2V_TRY(lora_find(c, "s2v_lora_set_scale", name, rank, &s));
    auto it = c->lora_names.find(name);
    S2V_REQUIRE(it != c->lora_names.end() && it->second == rank, "s2v_lora_set_scale: no adapter of this rank was attached under this name on this context (s2v_lora_attach)");
    // values only: the same launches read the same addresses, a captured step stays valid
    S2V_TRY(lora_write(c, name, *s, A, B, rank, scale, false, (hipStream_t)stream));
    c->lora_scale = scale;
    return lora_write_hdr(c, (hipStream_t)stream);
}

extern "C" int s2v_lora_detach(s2v_ctx* c, s2v_stream stream) {
    S2V_REQUIRE(c, "s2v_lora_detach: null context");
    S2V_TRY(lora_checks(c, "s2v_lora_detach"));
    sc_invalidate(c);
    hipStream_t st = (hipStream_t)stream;
    if (!c->lora_on()) return 0;
    const int64_t E = c->esz, lr = c->lr, fl = c->flr;
    const bool model = c->kind == S2V_CTX_MODEL;
    // zero what an attach wrote beside the base weights -- fp8 branch: the Bs arrays, otherwise the tail columns -- and the A stacks: a later
    // attach of fewer names must not meet these values.  An attention-weights context holds the first two linears only
    for (auto& w : c->layers)
        for (int i = 0; i < (model ? LIN_NUM : LIN_OUT + 1); ++i) {
            const LinShape s = lin_shape(i, c->D);
            const LinW& x = w.lin[i];
            if (fl) S2V_CHECK_HIP(hipMemsetAsync(x.bs, 0, (size_t)(s.n_pad() * fl * E), st));
            else S2V_CHECK_HIP(hipMemset2DAsync(x.w + s.K * E, (size_t)(s.pitch(lr) * E), 0, (size_t)(s.parts * lr * E), (size_t)s.n_pad(), st));
            S2V_CHECK_HIP(hipMemsetAsync(x.a, 0, (size_t)(s.parts * (lr + fl) * s.K * E), st));
        }
    if (model) {
        // the modulation stack interleaves, under lora_adaln_scope 1, the reference-image copies with the six chunks: rebuild slot by slot
        for (auto& kv : c->slots) {
            Slot& s = kv.second;
            if (s.lora != LORA_REMERGE) continue;
            char* base = lora_base_of(c, s.dst);
            const int64_t bytes = s.rows * s.ld * E;
            S2V_CHECK_HIP(hipMemcpyAsync(s.dst, base, (size_t)bytes, hipMemcpyDeviceToDevice, st));
            if (c->mc == 9 && is_adaln_linear(kv.first.c_str())) S2V_CHECK_HIP(hipMemcpyAsync(s.dst + bytes, base, (size_t)(bytes / 2), hipMemcpyDeviceToDevice, st));
        }
    }
    if (model) c->have_cond = false;   // patch_embed.proj / text_proj are the base again: s2v_set_conditioning comes next
    lora_drop_graph(c);
    c->lora_names.clear();
    c->lora_replica = 0;
    c->lora_rank = 0; c->lora_scale = 0.f;
    return lora_write_hdr(c, st);
}

extern "C" int s2v_lora_state(s2v_ctx* c, int32_t* attached, int32_t* rank, float* scale, int64_t* graph_captures) {
    S2V_REQUIRE(c && attached && rank && scale && graph_captures, "s2v_lora_state: null argument");
    *attached = (int32_t)c->lora_names.size() + c->lora_replica;
    *rank = c->lora_rank; *scale = c->lora_scale; *graph_captures = c->graph_captures;
    return 0;
}

extern "C" int s2v_device_bytes(s2v_ctx* c, int64_t* arena, int64_t* workspace) {
    S2V_REQUIRE(c && arena && workspace, "s2v_device_bytes: null argument");
    *arena = c->arena ? c->arena_bytes : 0;
    *workspace = c->ws ? c->ws_bytes + c->e1x_bytes + c->sc_bytes + c->am_bytes + c->win_bytes + c->st_bytes() + c->la_bytes() + c->gr_bytes + (c->gr_buf ? c->gr_log_bytes : 0) : 0;
    return 0;
}

// ------------------------------------------------------------------------------------------------------
static void fill_coef(SchedCoef& d, const s2v_sched_coef& s) {
    d.kind = s.kind; d.guidance = s.guidance; d.c_x0_x = s.c_x0_x; d.c_x0_v = s.c_x0_v; d.a_t = s.a_t; d.b_t = s.b_t;
    d.m1 = s.m1; d.m2 = s.m2; d.m3 = s.m3; d.m4 = s.m4; d.mn = s.mn; d.guidance_subject = s.guidance_subject;
}

static SchedBlend fill_blend(const s2v_blend& s) { return SchedBlend{s.sqrt_alpha, s.sqrt_one_minus_alpha, s.last != 0, s.keep_max}; }

extern "C" int s2v_add_noise(const void* sample, const void* noise, int64_t n, float sqrt_alpha, float sqrt_one_minus_alpha, void* out,
                             int32_t dtype, s2v_stream stream) {
    S2V_REQUIRE(sample && noise && out && n > 0, "s2v_add_noise: bad argument");
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_add_noise: unsupported dtype");
    return launch_add_noise(sample, noise, n, sqrt_alpha, sqrt_one_minus_alpha, out, dtype, (hipStream_t)stream);
}

// s2v_sched_step (factors == null) and s2v_sched_step_rescale (its RESCALE form): one body, the entry's own wording for what differs
static int sched_step_entry(const s2v_sched_coef* coef_host, const void* noise_pred, int32_t flags, const void* latents_in, void* latents_out,
                            float* x0_hist, const void* noise, int64_t n, int32_t dtype, const float* factors, s2v_stream stream) {
    S2V_REQUIRE(coef_host && noise_pred && latents_in && latents_out, "s2v_sched_step: null argument");
    S2V_REQUIRE(coef_host->kind == 0 || noise, "s2v_sched_step: DPM step needs a noise tensor");
    S2V_REQUIRE(coef_host->kind != 2 || x0_hist, "s2v_sched_step: DPM multistep needs x0_hist");
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_sched_step: unsupported dtype");
    S2V_REQUIRE((flags & 9) != 9, "s2v_sched_step: flags bit0 (the CFG pair [2, n]) and bit3 (the subject-guidance triple [3, n]) exclude each other");
    SchedArgs a{};
    a.noise_pred = noise_pred; a.latents_in = latents_in; a.latents_out = latents_out; a.x0_hist = x0_hist;
    a.noise = noise; a.n = n; a.nvid = 1; a.n_vid = n; a.cfg = (flags & 8) ? SCHED_CFG_TRIPLE : flags & 1; a.np_f32 = (flags >> 1) & 1; a.out_f32 = (flags >> 2) & 1;
    a.coef = nullptr;
    fill_coef(a.cval, *coef_host);
    return launch_sched_step(a, dtype, (hipStream_t)stream, factors);
}
extern "C" int s2v_sched_step(s2v_ctx* c, const s2v_sched_coef* coef_host, const void* noise_pred, int32_t flags,
                              const void* latents_in, void* latents_out, float* x0_hist, const void* noise, int64_t n,
                              int32_t dtype, s2v_stream stream) {
    (void)c;
    S2V_REQUIRE(!(flags & S2V_SCHED_RESCALE), "s2v_sched_step: flags bit4 (the RESCALE form of the guidance rescale) needs the device factor, which rides in s2v_sched_step_rescale");
    return sched_step_entry(coef_host, noise_pred, flags, latents_in, latents_out, x0_hist, noise, n, dtype, nullptr, stream);
}
extern "C" int s2v_sched_step_rescale(s2v_ctx* c, const s2v_sched_coef* coef_host, const void* noise_pred, int32_t flags, const void* latents_in,
                                      void* latents_out, float* x0_hist, const void* noise, int64_t n, int32_t dtype, const float* factors,
                                      s2v_stream stream) {
    (void)c;
    S2V_REQUIRE((flags & S2V_SCHED_RESCALE) && factors, "s2v_sched_step_rescale: flags bit4 (S2V_SCHED_RESCALE) and a device pointer to the video's factor are required");
    return sched_step_entry(coef_host, noise_pred, flags, latents_in, latents_out, x0_hist, noise, n, dtype, factors, stream);
}

static int sched_step_masked_entry(const s2v_sched_coef* coef_host, const s2v_blend* blend_host, const void* noise_pred, int32_t flags,
                                   const void* latents_in, void* latents_out, float* x0_hist, const void* noise, const void* z0,
                                   const void* noise0, const uint8_t* latent_mask, int32_t F, int32_t C, int32_t H, int32_t W, int32_t dtype,
                                   const float* factors, s2v_stream stream) {
    S2V_REQUIRE(coef_host && blend_host && noise_pred && latents_in && latents_out && z0 && noise0 && latent_mask, "s2v_sched_step_masked: null argument");
    S2V_REQUIRE(F >= 1 && C >= 1 && H >= 1 && W >= 1, "s2v_sched_step_masked: the latent is [F, C, H, W]");
    S2V_REQUIRE(coef_host->kind == 0 || noise, "s2v_sched_step_masked: DPM step needs a noise tensor");
    S2V_REQUIRE(coef_host->kind != 2 || x0_hist, "s2v_sched_step_masked: DPM multistep needs x0_hist");
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_sched_step_masked: unsupported dtype");
    S2V_REQUIRE(!(flags & 4), "s2v_sched_step_masked: the blend runs on the latents rounded to `dtype` (flags bit2, fp32 output, is refused)");
    S2V_REQUIRE(blend_host->keep_max >= 0 && blend_host->keep_max <= 255, "s2v_sched_step_masked: keep_max must be a level 0..255");
    S2V_REQUIRE((flags & 9) != 9, "s2v_sched_step_masked: flags bit0 (the CFG pair [2, n]) and bit3 (the subject-guidance triple [3, n]) exclude each other");
    SchedMaskArgs a{};
    a.noise_pred = noise_pred; a.latents_in = latents_in; a.latents_out = latents_out; a.x0_hist = x0_hist;
    a.noise = noise; a.n = (int64_t)F * C * H * W; a.nvid = 1; a.n_vid = a.n; a.cfg = (flags & 8) ? SCHED_CFG_TRIPLE : flags & 1; a.np_f32 = (flags >> 1) & 1;
    a.coef = nullptr;
    fill_coef(a.cval, *coef_host);
    a.z0 = z0; a.noise0 = noise0; a.mask = latent_mask; a.chw = C * H * W; a.hw = H * W; a.mask_vid = F * H * W;
    a.blend = nullptr; a.bval = fill_blend(*blend_host);
    return launch_sched_step_masked(a, dtype, (hipStream_t)stream, factors);
}
extern "C" int s2v_sched_step_masked(s2v_ctx* c, const s2v_sched_coef* coef_host, const s2v_blend* blend_host, const void* noise_pred, int32_t flags,
                                     const void* latents_in, void* latents_out, float* x0_hist, const void* noise, const void* z0,
                                     const void* noise0, const uint8_t* latent_mask, int32_t F, int32_t C, int32_t H, int32_t W, int32_t dtype,
                                     s2v_stream stream) {
    (void)c;
    S2V_REQUIRE(!(flags & S2V_SCHED_RESCALE), "s2v_sched_step_masked: flags bit4 (the RESCALE form of the guidance rescale) needs the device factor, which rides in s2v_sched_step_masked_rescale");
    return sched_step_masked_entry(coef_host, blend_host, noise_pred, flags, latents_in, latents_out, x0_hist, noise, z0, noise0, latent_mask, F, C, H, W, dtype,
                                   nullptr, stream);
}
extern "C" int s2v_sched_step_masked_rescale(s2v_ctx* c, const s2v_sched_coef* coef_host, const s2v_blend* blend_host, const void* noise_pred,
                                             int32_t flags, const void* latents_in, void* latents_out, float* x0_hist, const void* noise,
                                             const void* z0, const void* noise0, const uint8_t* latent_mask, int32_t F, int32_t C, int32_t H,
                                             int32_t W, int32_t dtype, const float* factors, s2v_stream stream) {
    (void)c;
    S2V_REQUIRE((flags & S2V_SCHED_RESCALE) && factors, "s2v_sched_step_masked_rescale: flags bit4 (S2V_SCHED_RESCALE) and a device pointer to the video's factor are required");
    return sched_step_masked_entry(coef_host, blend_host, noise_pred, flags, latents_in, latents_out, x0_hist, noise, z0, noise0, latent_mask, F, C, H, W, dtype,
                                   factors, stream);
}

extern "C" int s2v_mask_to_latent(const void* mask, int32_t mask_dtype, int32_t F, int32_t H, int32_t W, uint8_t* latent_mask, uint8_t* pixel_mask,
                                  s2v_stream stream) {
    S2V_REQUIRE(mask && latent_mask, "s2v_mask_to_latent: null argument");
    return launch_mask_to_latent(mask, mask_dtype, F, H, W, latent_mask, pixel_mask, (hipStream_t)stream);
}

extern "C" int s2v_map_to_latent(const void* map, int32_t map_dtype, int32_t F, int32_t H, int32_t W, uint8_t* latent_level, uint8_t* pixel_mask,
                                 s2v_stream stream) {
    S2V_REQUIRE(map && latent_level, "s2v_map_to_latent: null argument");
    return launch_map_to_latent(map, map_dtype, F, H, W, latent_level, pixel_mask, (hipStream_t)stream);
}

// the step's scalars to the device through the next slot of the pinned ring (the uploads are asynchronous: a slot must outlive its copies, RING
// steps ahead of the device are allowed): b videos, sample j of the S2V_MAX_BATCH slots at timesteps[j mod b], video k's coefficient set coefs[k]
// (the sets past b repeat the last one).  Whatever b is, the timesteps go up in one copy and the coefficient sets in one
// The masked step's blend records (blends != null: b of them) ride in the same slot and go up in a third copy
static int stage_step(s2v_ctx* c, const float* timesteps, const s2v_sched_coef* coefs, int b, hipStream_t st, const s2v_blend* blends = nullptr) {
    s2v_ctx::Stage& sg = c->ring[c->ring_pos];
    c->ring_pos = (c->ring_pos + 1) % RING;
    for (int i = 0; i < S2V_MAX_BATCH; ++i) sg.t[i] = timesteps[i % b];
    for (int k = 0; k < S2V_MAX_BATCH / 2; ++k) fill_coef(sg.c[k], coefs[k < b ? k : b - 1]);
    S2V_CHECK_HIP(hipMemcpyAsync(c->t_dev, sg.t, sizeof(float) * S2V_MAX_BATCH, hipMemcpyHostToDevice, st));
    S2V_CHECK_HIP(hipMemcpyAsync(c->coef_dev, sg.c, sizeof(SchedCoef) * (S2V_MAX_BATCH / 2), hipMemcpyHostToDevice, st));
    if (blends) {
        for (int k = 0; k < S2V_MAX_BATCH / 2; ++k) sg.bl[k] = fill_blend(blends[k < b ? k : b - 1]);
        S2V_CHECK_HIP(hipMemcpyAsync(c->blend_dev, sg.bl, sizeof(SchedBlend) * (S2V_MAX_BATCH / 2), hipMemcpyHostToDevice, st));
    }
    return 0;
}
static int stage_step(s2v_ctx* c, float timestep, const s2v_sched_coef* coef_host, hipStream_t st) {
    return stage_step(c, &timestep, coef_host, 1, st);
}

// the graph cache: replay the captured `body` on st; a first use or another key captures body(cap_stream) anew.  A body that fails ends the
// capture and returns its code with no graph held
// One executable per step-cache mode (key.mode): a plan that alternates between modes captures each kind once.  A key that differs from a
// held one in anything but the mode drops every executable, as the single one was dropped before modes existed
template <class Body>
static int launch_captured(s2v_ctx* c, const GraphKey& key, hipStream_t st, Body body) {
    bool other = false;
    for (int m = 0; m < 3; ++m) other = other || (c->gexec[m] && !c->gkey[m].same_but_mode(key));
    for (auto& kg : c->gexec_armed) other = other || !kg.first.same_but_mode(key);
    if (other) drop_graph(c);
    hipGraphExec_t fresh = nullptr;
    hipGraphExec_t* slot = key.armed() ? &fresh : &c->gexec[key.mode];   // an armed step: its own executable per (mode, layer masks)
    if (key.armed())
        for (auto& kg : c->gexec_armed) if (kg.first == key) slot = &kg.second;
    hipGraphExec_t& gexec = *slot;
    if (!gexec) {
        hipGraph_t graph = nullptr;
        S2V_CHECK_HIP(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
        const int r = body(c->cap_stream);
        hipError_t e = hipStreamEndCapture(c->cap_stream, &graph);
        if (r != 0) { if (graph) hipGraphDestroy(graph); return r; }
        S2V_CHECK_HIP(e);
        e = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        if (e != hipSuccess) gexec = nullptr;
        S2V_CHECK_HIP(e);
        c->graph_captures++;
        if (key.armed()) c->gexec_armed.emplace_back(key, gexec);
        else c->gkey[key.mode] = key;
    }
    S2V_CHECK_HIP(hipGraphLaunch(gexec, st));
    return 0;
}

// (CFG +) scheduler step on the context's noise_pred with the coefficients stage_step uploaded, latents updated in place.  nvid videos:
// latents / x0_hist / noise [nvid][F,C,H,W] and noise_pred [negative x nvid | positive x nvid], so the conditional half starts n elements in;
// video k is stepped with the k-th uploaded coefficient set
static int sched_on_pair(s2v_ctx* c, void* latents, float* x0_hist, const void* noise, int cfg_flag, hipStream_t st, int nvid = 1, const float* factor = nullptr) {
    SchedArgs a{};
    a.noise_pred = c->noise_pred; a.latents_in = latents; a.latents_out = latents; a.x0_hist = x0_hist; a.noise = noise;
    a.nvid = nvid; a.n_vid = (int64_t)c->F * c->cfg.out_channels * c->H * c->W;
    a.n = nvid * a.n_vid; a.cfg = cfg_flag; a.coef = c->coef_dev;
    return launch_sched_step(a, c->dtype, st, factor);
}

// ---- guidance rescale (include/s2v_hip.h) ---------------------------------------------------------------------------------------------------
static int64_t video_elems(const s2v_ctx* c) { return (int64_t)c->F * c->cfg.out_channels * c->H * c->W; }

extern "C" int s2v_set_guidance_rescale(s2v_ctx* c, const float* phi, int32_t b) {
    S2V_REQUIRE(c, "s2v_set_guidance_rescale: null context");
    if (!phi && b == 0) {   // clear: nothing held, s2v_device_bytes as without the feature
        if (c->gr_buf || c->gr_log) { S2V_CHECK_HIP(hipDeviceSynchronize()); drop_graph(c); gr_free(c); gr_free_log(c); }
        return 0;
    }
    S2V_REQUIRE(phi && b >= 1 && b <= S2V_MAX_BATCH / 2, "s2v_set_guidance_rescale: phi values of 1 <= b <= 4 videos, or NULL with b = 0 to clear");
    for (int k = 0; k < b; ++k)   // written so that NaN fails it
        S2V_REQUIRE(phi[k] >= 0.f && phi[k] <= 1.f, "s2v_set_guidance_rescale: every phi must lie in [0, 1] (NaN is refused as well)");
    S2V_REQUIRE(c->kind == S2V_CTX_MODEL, "s2v_set_guidance_rescale: attention-only contexts (S2V_CTX_ATTN_*) run no step");
    S2V_REQUIRE(!c->shard, "s2v_set_guidance_rescale: a shard context (s2v_set_shard) has no rescaled step: the statistic spans the whole video, which no rank of a "
                           "Ulysses group holds before the noise all-gather; guidance rescale runs on one GPU");
    S2V_REQUIRE(c->ws, "s2v_set_guidance_rescale: call s2v_set_geometry first (the values belong to the geometry's videos)");
    S2V_REQUIRE(c->B != 1, "s2v_set_guidance_rescale: a geometry with B = 1 runs no CFG (it is one sample of a CFG-parallel pair, and the split entries have no "
                           "rescaled form): guidance rescale runs the CFG pairs or triples of b videos on one GPU");
    S2V_REQUIRE(!c->win_acc, "s2v_set_guidance_rescale: temporal windows are set (s2v_set_windows): s2v_denoise_step_windows combines the windows before its one "
                             "scheduler step, and a statistic per window is another feature");
    S2V_REQUIRE((c->B % 2 == 0 && b == c->B / 2) || (c->B % 3 == 0 && b == c->B / 3),
                "s2v_set_guidance_rescale: b must be the videos of the geometry (B / 2 for CFG pairs, B / 3 for subject-guidance triples)");
    S2V_REQUIRE(c->cfg.in_channels == c->cfg.out_channels, "s2v_set_guidance_rescale: in/out channels must match");
    bool any = false;
    for (int k = 0; k < b; ++k) any = any || phi[k] != 0.f;
    if (!any) {   // all zero arms nothing: the entries run the launches they ran (the log stays for a batch that arms again)
        if (c->gr_buf) { S2V_CHECK_HIP(hipDeviceSynchronize()); drop_graph(c); gr_free(c); }
        return 0;
    }
    S2V_CHECK_HIP(hipDeviceSynchronize());   // a step in flight may still read the values about to be replaced
    if (!c->gr_buf || c->gr_b != b) {
        drop_graph(c);
        gr_free(c);
        const int64_t part = rup((int64_t)b * cfg_stats_chunks(video_elems(c)) * 4 * 8, 256);
        const int64_t bytes = part + (S2V_MAX_BATCH / 2) * (4 * 8 + 4 + 4);
        S2V_CHECK_HIP(hipMalloc((void**)&c->gr_buf, bytes));
        c->gr_partials = (double*)c->gr_buf; c->gr_sums = (double*)(c->gr_buf + part);
        c->gr_factors = (float*)(c->gr_sums + (S2V_MAX_BATCH / 2) * 4); c->gr_phi = c->gr_factors + S2V_MAX_BATCH / 2;
        S2V_CHECK_HIP(hipMemset(c->gr_buf + part, 0, bytes - part));
        c->gr_bytes = bytes; c->gr_b = b;
    }
    if (!c->gr_log) {
        const int64_t bytes = (int64_t)CFG_LOG_STEPS * CFG_LOG_COLS * 4 + 4;
        S2V_CHECK_HIP(hipMalloc((void**)&c->gr_log, bytes));
        S2V_CHECK_HIP(hipMemset(c->gr_log, 0, bytes));
        c->gr_log_count = (unsigned*)(c->gr_log + CFG_LOG_STEPS * CFG_LOG_COLS); c->gr_log_bytes = bytes;
    }
    S2V_CHECK_HIP(hipMemcpy(c->gr_phi, phi, sizeof(float) * b, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int s2v_guidance_rescale_read(s2v_ctx* c, double* sums, float* factors, float* log, int32_t* log_count) {
    S2V_REQUIRE(c, "s2v_guidance_rescale_read: null context");
    S2V_REQUIRE((!sums && !factors) || c->gr_buf, "s2v_guidance_rescale_read: sums and factors are those of an armed context (s2v_set_guidance_rescale with a non-zero phi)");
    S2V_CHECK_HIP(hipDeviceSynchronize());
    if (sums) S2V_CHECK_HIP(hipMemcpy(sums, c->gr_sums, sizeof(double) * 4 * c->gr_b, hipMemcpyDeviceToHost));
    if (factors) S2V_CHECK_HIP(hipMemcpy(factors, c->gr_factors, sizeof(float) * c->gr_b, hipMemcpyDeviceToHost));
    unsigned count = 0;
    if (c->gr_log) S2V_CHECK_HIP(hipMemcpy(&count, c->gr_log_count, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (log && count) S2V_CHECK_HIP(hipMemcpy(log, c->gr_log, sizeof(float) * CFG_LOG_COLS * (count < CFG_LOG_STEPS ? count : CFG_LOG_STEPS), hipMemcpyDeviceToHost));
    if (log_count) *log_count = (int32_t)count;
    return 0;
}

// an armed step's two launches behind the forward: the statistics of the context's noise_pred on the b videos and their factors (logged)
static int rescale_stats(s2v_ctx* c, int cfg, int b, hipStream_t st) {
    CfgStatsArgs s{};
    s.noise_pred = c->noise_pred; s.nvid = b; s.n_vid = video_elems(c); s.n = b * s.n_vid; s.cfg = cfg; s.coef = c->coef_dev; s.partials = c->gr_partials;
    S2V_TRY(launch_cfg_stats(s, c->dtype, st));
    CfgFinalArgs f{};
    f.partials = c->gr_partials; f.chunks = cfg_stats_chunks(s.n_vid); f.nvid = b; f.n_vid = s.n_vid; f.phi = c->gr_phi; f.sums = c->gr_sums;
    f.factors = c->gr_factors; f.log = c->gr_log; f.log_count = c->gr_log_count;
    return launch_cfg_finalize(f, st);
}

extern "C" int s2v_op_cfg_stats(const void* noise_pred, int32_t flags, int32_t nvid, int64_t n_vid, const float* guidance, const float* guidance_subject,
                                const float* phi, double* sums, float* factors, int32_t dtype, s2v_stream stream) {
    S2V_REQUIRE(noise_pred && guidance && phi && sums && factors, "s2v_op_cfg_stats: null argument");
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_op_cfg_stats: unsupported dtype");
    S2V_REQUIRE(((flags & 1) != 0) != ((flags & 8) != 0), "s2v_op_cfg_stats: flags bit0 (the CFG pair) or bit3 (the subject-guidance triple), exactly one of them");
    S2V_REQUIRE(!(flags & 8) || guidance_subject, "s2v_op_cfg_stats: the triple needs guidance_subject");
    S2V_REQUIRE(nvid >= 1 && nvid <= S2V_MAX_BATCH / 2 && n_vid >= 1, "s2v_op_cfg_stats: 1 <= nvid <= 4 videos of n_vid >= 1 elements");
    for (int k = 0; k < nvid; ++k) S2V_REQUIRE(phi[k] >= 0.f && phi[k] <= 1.f, "s2v_op_cfg_stats: every phi must lie in [0, 1] (NaN is refused as well)");
    hipStream_t st = (hipStream_t)stream;
    const int chunks = cfg_stats_chunks(n_vid);
    const int64_t part = rup((int64_t)nvid * chunks * 4 * 8, 256), coef_off = part + nvid * (4 * 8 + 4 + 4);
    char* buf = nullptr;
    S2V_CHECK_HIP(hipMalloc((void**)&buf, rup(coef_off, 16) + sizeof(SchedCoef) * nvid));
    double* sums_dev = (double*)(buf + part);
    float *factors_dev = (float*)(sums_dev + 4 * nvid), *phi_dev = factors_dev + nvid;
    SchedCoef* coef_dev = (SchedCoef*)(buf + rup(coef_off, 16));
    SchedCoef coefs[S2V_MAX_BATCH / 2] = {};
    for (int k = 0; k < nvid; ++k) { coefs[k].guidance = guidance[k]; coefs[k].guidance_subject = guidance_subject ? guidance_subject[k] : 0.f; }
    int r = 0;
    auto hip = [&](hipError_t e) { if (e != hipSuccess && r == 0) r = s2v_fail(__FILE__, __LINE__, hipGetErrorString(e), -2); return e == hipSuccess; };
    if (hip(hipMemcpy(coef_dev, coefs, sizeof(SchedCoef) * nvid, hipMemcpyHostToDevice)) && hip(hipMemcpy(phi_dev, phi, sizeof(float) * nvid, hipMemcpyHostToDevice))) {
        CfgStatsArgs s{};
        s.noise_pred = noise_pred; s.nvid = nvid; s.n_vid = n_vid; s.n = nvid * n_vid; s.cfg = (flags & 8) ? SCHED_CFG_TRIPLE : 1; s.coef = coef_dev;
        s.np_f32 = (flags >> 1) & 1; s.partials = (double*)buf;
        CfgFinalArgs f{};
        f.partials = s.partials; f.chunks = chunks; f.nvid = nvid; f.n_vid = n_vid; f.phi = phi_dev; f.sums = sums_dev; f.factors = factors_dev;
        r = launch_cfg_stats(s, dtype, st);
        if (r == 0) r = launch_cfg_finalize(f, st);
        if (r == 0 && hip(hipStreamSynchronize(st)) && hip(hipMemcpy(sums, sums_dev, sizeof(double) * 4 * nvid, hipMemcpyDeviceToHost)))
            hip(hipMemcpy(factors, factors_dev, sizeof(float) * nvid, hipMemcpyDeviceToHost));
    }
    hipFree(buf);
    return r;
}

static int step_launches(s2v_ctx* c, void* latents, float* x0_hist, const void* noise, hipStream_t st, int mode, uint64_t am, uint64_t sm, uint64_t lm) {
    // b videos: sample j of [negative x b | positive x b] embeds video j mod b straight from `latents` (one video: the stride of 0 it always had)
    const int b = c->B >= 2 ? c->B / 2 : 1;
    S2V_TRY(forward_impl(c, latents, b > 1 ? (int64_t)c->F * c->cfg.in_channels * c->H * c->W : 0, b > 1 ? b : 0, c->t_dev, c->noise_pred, st, mode, am, sm, lm));
    if (c->gr_buf) S2V_TRY(rescale_stats(c, 1, b, st));   // armed only on B >= 2 (s2v_set_guidance_rescale)
    return sched_on_pair(c, latents, x0_hist, noise, c->B >= 2 ? 1 : 0, st, b, c->gr_buf ? c->gr_factors : nullptr);
}

// the whole step of b = B/2 videos (b = 1 for B = 1 or 2) at timesteps[b] and coefs[b]; s2v_denoise_step's wording serves both entries
static int denoise_step_impl(s2v_ctx* c, void* latents, const float* timesteps, const s2v_sched_coef* coefs, float* x0_hist, const void* noise,
                             int32_t use_graph, hipStream_t st) {
    const int mode = sc_take_arm(c);
    const uint64_t am = am_take_arm(c), sm = st_take_arm(c), lm = la_take_arm(c);
    S2V_REQUIRE(c->ws && (c->B == 1 || c->B % 2 == 0), "s2v_denoise_step: geometry with B = 1 or an even B = 2b (the CFG pairs of b videos) required");
    S2V_REQUIRE(!c->cond_triples, "s2v_denoise_step: the context is conditioned as subject-guidance triples [u x b | r x b | f x b] (s2v_set_conditioning_triples): "
                                  "its step is s2v_denoise_step_guided");
    S2V_REQUIRE(!c->win_acc, "s2v_denoise_step: temporal windows are set (s2v_set_windows): the geometry is one forward's windows of a long latent, and "
                             "its step is s2v_denoise_step_windows");
    S2V_REQUIRE(c->cfg.in_channels == c->cfg.out_channels, "s2v_denoise_step: in/out channels must match");
    const int b = c->B >= 2 ? c->B / 2 : 1;
    for (int k = 0; k < b; ++k) S2V_REQUIRE(coefs[k].kind == 0 || (noise && x0_hist), "s2v_denoise_step: DPM needs noise and x0_hist");
    S2V_REQUIRE(!c->shard, use_graph ? "s2v_denoise_step: hipGraph capture is not supported for a shard context (s2v_set_shard): its step is staged around "
                                       "the exchanges and runs eagerly (s2v_shard_step_* / s2v_denoise_step_ulysses)"
                                     : "s2v_denoise_step: a shard context (s2v_set_shard) runs the staged step (s2v_shard_step_* / s2v_denoise_step_ulysses)");
    S2V_REQUIRE(!c->gr_buf || c->gr_b == b, "s2v_denoise_step: s2v_set_guidance_rescale set the values of another number of videos than this geometry's b = B/2");
    S2V_TRY(stage_step(c, timesteps, coefs, b, st));
    if (!use_graph) return am_done(c, am, sc_done(c, mode, step_launches(c, latents, x0_hist, noise, st, mode, am, sm, lm)));
    GraphKey key{latents, x0_hist, noise, -1};
    key.mode = mode; key.amask = am; key.smask = sm; key.lmask = lm; key.lkind = lm ? c->la_kind : 0; key.rescale = c->gr_buf ? 1 : 0;
    return am_done(c, am, sc_done(c, mode, launch_captured(c, key, st, [&](hipStream_t s) { return step_launches(c, latents, x0_hist, noise, s, mode, am, sm, lm); })));
}

extern "C" int s2v_denoise_step(s2v_ctx* c, void* latents, float timestep, const s2v_sched_coef* coef_host,
                                float* x0_hist, const void* noise, int32_t use_graph, s2v_stream stream) {
    S2V_REQUIRE(c && latents && coef_host, "s2v_denoise_step: null argument");
    float t[S2V_MAX_BATCH / 2];
    s2v_sched_coef k[S2V_MAX_BATCH / 2];
    for (int i = 0; i < S2V_MAX_BATCH / 2; ++i) { t[i] = timestep; k[i] = *coef_host; }   // the scalar repeated for every video
    return denoise_step_impl(c, latents, t, k, x0_hist, noise, use_graph, (hipStream_t)stream);
}

extern "C" int s2v_denoise_step_videos(s2v_ctx* c, void* latents, const float* timesteps, const s2v_sched_coef* coefs, float* x0_hist,
                                       const void* noise, int32_t use_graph, s2v_stream stream) {
    S2V_REQUIRE(c && latents && timesteps && coefs, "s2v_denoise_step_videos: null argument");
    return denoise_step_impl(c, latents, timesteps, coefs, x0_hist, noise, use_graph, (hipStream_t)stream);
}

// ---- masked video-to-video: the step with the blend in its last kernel ----------------------------------------------------------------
extern "C" int s2v_set_blend(s2v_ctx* c, const void* z0, const void* noise0, const uint8_t* latent_mask, int32_t b) {
    S2V_REQUIRE(c, "s2v_set_blend: null context");
    const bool clear = !z0 && !noise0 && !latent_mask && b == 0;
    S2V_REQUIRE(clear || (z0 && noise0 && latent_mask && b >= 1 && b <= S2V_MAX_BATCH / 2),
                "s2v_set_blend: z0, noise0 and the latent mask of 1 <= b <= 4 videos, or all null with b = 0 to clear");
    c->blend_z0 = z0; c->blend_noise0 = noise0; c->blend_mask = latent_mask; c->blend_b = b;
    drop_graph(c);   // the captured step bakes the operands in (they are part of its key)
    return 0;
}

static int masked_step_launches(s2v_ctx* c, void* latents, float* x0_hist, const void* noise, hipStream_t st, int mode, uint64_t am, uint64_t sm, uint64_t lm) {
    const int b = c->B / 2;
    S2V_TRY(forward_impl(c, latents, b > 1 ? (int64_t)c->F * c->cfg.in_channels * c->H * c->W : 0, b > 1 ? b : 0, c->t_dev, c->noise_pred, st, mode, am, sm, lm));
    SchedMaskArgs a{};
    a.noise_pred = c->noise_pred; a.latents_in = latents; a.latents_out = latents; a.x0_hist = x0_hist; a.noise = noise;
    a.nvid = b; a.n_vid = (int64_t)c->F * c->cfg.out_channels * c->H * c->W;
    a.n = b * a.n_vid; a.cfg = 1; a.coef = c->coef_dev;
    a.z0 = c->blend_z0; a.noise0 = c->blend_noise0; a.mask = c->blend_mask;
    a.chw = c->cfg.out_channels * c->H * c->W; a.hw = c->H * c->W; a.mask_vid = c->F * a.hw; a.blend = c->blend_dev;
    if (c->gr_buf) S2V_TRY(rescale_stats(c, 1, b, st));   // over the whole video, kept cells included
    return launch_sched_step_masked(a, c->dtype, st, c->gr_buf ? c->gr_factors : nullptr);
}

extern "C" int s2v_denoise_step_masked(s2v_ctx* c, void* latents, const float* timesteps, const s2v_sched_coef* coefs, const s2v_blend* blends,
                                       float* x0_hist, const void* noise, int32_t use_graph, s2v_stream stream) {
    S2V_REQUIRE(c && latents && timesteps && coefs && blends, "s2v_denoise_step_masked: null argument");
    const int mode = sc_take_arm(c);
    const uint64_t am = am_take_arm(c), sm = st_take_arm(c), lm = la_take_arm(c);
    S2V_REQUIRE(!c->shard, "s2v_denoise_step_masked: a shard context (s2v_set_shard) has no masked step: masked video-to-video runs on one GPU");
    S2V_REQUIRE(c->ws && c->B != 1, "s2v_denoise_step_masked: a geometry with B = 1 is one sample of a CFG-parallel pair, and the split entries "
                                    "(s2v_denoise_split_begin / _end, s2v_denoise_step_cfg_parallel) have no masked form: masked video-to-video runs the "
                                    "CFG pairs of b videos, B = 2b, on one GPU");
    S2V_REQUIRE(c->B % 2 == 0, "s2v_denoise_step_masked: an even B = 2b (the CFG pairs of b videos) is required");
    S2V_REQUIRE(!c->cond_triples, "s2v_denoise_step_masked: the context is conditioned as subject-guidance triples [u x b | r x b | f x b] "
                                  "(s2v_set_conditioning_triples): its masked step is s2v_denoise_step_guided with blends");
    S2V_REQUIRE(!c->win_acc, "s2v_denoise_step_masked: temporal windows are set (s2v_set_windows): the windowed step (s2v_denoise_step_windows) has no "
                             "masked form");
    S2V_REQUIRE(c->cfg.in_channels == c->cfg.out_channels, "s2v_denoise_step_masked: in/out channels must match");
    const int b = c->B / 2;
    S2V_REQUIRE(c->blend_z0 && c->blend_b == b, "s2v_denoise_step_masked: s2v_set_blend has not set the blend operands of this geometry's b = B/2 videos");
    for (int k = 0; k < b; ++k) S2V_REQUIRE(coefs[k].kind == 0 || (noise && x0_hist), "s2v_denoise_step_masked: DPM needs noise and x0_hist");
    for (int k = 0; k < b; ++k) S2V_REQUIRE(blends[k].keep_max >= 0 && blends[k].keep_max <= 255, "s2v_denoise_step_masked: keep_max must be a level 0..255");
    S2V_REQUIRE(!c->gr_buf || c->gr_b == b, "s2v_denoise_step_masked: s2v_set_guidance_rescale set the values of another number of videos than this geometry's b = B/2");
    hipStream_t st = (hipStream_t)stream;
    S2V_TRY(stage_step(c, timesteps, coefs, b, st, blends));
    if (!use_graph) return am_done(c, am, sc_done(c, mode, masked_step_launches(c, latents, x0_hist, noise, st, mode, am, sm, lm)));
    GraphKey key{latents, x0_hist, noise, -1};
    key.z0 = c->blend_z0; key.noise0 = c->blend_noise0; key.mask = c->blend_mask; key.mode = mode; key.amask = am; key.smask = sm; key.lmask = lm; key.lkind = lm ? c->la_kind : 0;
    key.rescale = c->gr_buf ? 1 : 0;
    return am_done(c, am, sc_done(c, mode, launch_captured(c, key, st, [&](hipStream_t s) { return masked_step_launches(c, latents, x0_hist, noise, s, mode, am, sm, lm); })));
}

// ---- subject guidance: the step of b triples [u x b | r x b | f x b] -----------------------------------------------------------------------------
// forward on B = 3b samples sharing each video's latent (sample j embeds video j mod b), then the triple combine and the scheduler step in the
// last kernel -- with `masked` the blend of s2v_set_blend behind it
static int guided_step_launches(s2v_ctx* c, void* latents, float* x0_hist, const void* noise, hipStream_t st, bool masked) {
    const int b = c->B / 3;
    S2V_TRY(forward_impl(c, latents, b > 1 ? (int64_t)c->F * c->cfg.in_channels * c->H * c->W : 0, b > 1 ? b : 0, c->t_dev, c->noise_pred, st, S2V_STEP_FULL, 0));
    SchedMaskArgs a{};
    a.noise_pred = c->noise_pred; a.latents_in = latents; a.latents_out = latents; a.x0_hist = x0_hist; a.noise = noise;
    a.nvid = b; a.n_vid = (int64_t)c->F * c->cfg.out_channels * c->H * c->W;
    a.n = b * a.n_vid; a.cfg = SCHED_CFG_TRIPLE; a.coef = c->coef_dev;
    const float* factor = c->gr_buf ? c->gr_factors : nullptr;
    if (factor) S2V_TRY(rescale_stats(c, SCHED_CFG_TRIPLE, b, st));   // f is the triple's f plane
    if (!masked) return launch_sched_step(a, c->dtype, st, factor);
    a.z0 = c->blend_z0; a.noise0 = c->blend_noise0; a.mask = c->blend_mask;
    a.chw = c->cfg.out_channels * c->H * c->W; a.hw = c->H * c->W; a.mask_vid = c->F * a.hw; a.blend = c->blend_dev;
    return launch_sched_step_masked(a, c->dtype, st, factor);
}

extern "C" int s2v_denoise_step_guided(s2v_ctx* c, void* latents, const float* timesteps, const s2v_sched_coef* coefs, const s2v_blend* blends,
                                       float* x0_hist, const void* noise, int32_t use_graph, s2v_stream stream) {
    S2V_REQUIRE(c && latents && timesteps && coefs, "s2v_denoise_step_guided: null argument");
    // the arms are one-shot and taken by every step entry, refused or not
    const int mode = sc_take_arm(c);
    const uint64_t am = am_take_arm(c), sm = st_take_arm(c), lm = la_take_arm(c);
    S2V_REQUIRE(sm == 0, "s2v_denoise_step_guided: attention steering is armed (s2v_attn_steer_arm), and steering assumes CFG pairs");
    S2V_REQUIRE(lm == 0, "s2v_denoise_step_guided: local attention is armed (s2v_attn_local_arm), and local attention assumes CFG pairs");
    S2V_REQUIRE(!c->shard, "s2v_denoise_step_guided: a shard context (s2v_set_shard) has no triple step: subject guidance runs on one GPU");
    // a pending split lives on a B = 1 geometry, so it is named before the geometry is
    S2V_REQUIRE(c->split_kind < 0, "s2v_denoise_step_guided: a CFG-parallel split is pending (s2v_denoise_split_begin): the split entries run CFG pairs, "
                                   "subject guidance runs on one GPU");
    S2V_REQUIRE(c->ws && c->B % 3 == 0 && c->B / 3 <= 2, "s2v_denoise_step_guided: a geometry of B = 3b samples [u x b | r x b | f x b] with b = 1 or 2 videos is required");
    S2V_REQUIRE(c->have_cond && c->cond_triples, "s2v_denoise_step_guided: the conditioning was not set by s2v_set_conditioning_triples (the context holds "
                                                 "CFG pairs, or no conditioning)");
    S2V_REQUIRE(!c->win_acc, "s2v_denoise_step_guided: temporal windows are set (s2v_set_windows): the windowed step (s2v_denoise_step_windows) runs "
                             "CFG pairs");
    S2V_REQUIRE(mode == S2V_STEP_FULL, "s2v_denoise_step_guided: a step-cache mode (s2v_step_cache_arm: CAPTURE / REUSE) is armed, and the step cache assumes CFG pairs");
    S2V_REQUIRE(am == 0, "s2v_denoise_step_guided: an attention map is armed (s2v_attn_map_arm), and the attention map assumes CFG pairs");
    S2V_REQUIRE(c->cfg.in_channels == c->cfg.out_channels, "s2v_denoise_step_guided: in/out channels must match");
    const int b = c->B / 3;
    for (int k = 0; k < b; ++k) S2V_REQUIRE(coefs[k].kind == 0 || (noise && x0_hist), "s2v_denoise_step_guided: DPM needs noise and x0_hist");
    if (blends) {
        S2V_REQUIRE(c->blend_z0 && c->blend_b == b, "s2v_denoise_step_guided: s2v_set_blend has not set the blend operands of this geometry's b = B/3 videos");
        for (int k = 0; k < b; ++k) S2V_REQUIRE(blends[k].keep_max >= 0 && blends[k].keep_max <= 255, "s2v_denoise_step_guided: keep_max must be a level 0..255");
    }
    S2V_REQUIRE(!c->gr_buf || c->gr_b == b, "s2v_denoise_step_guided: s2v_set_guidance_rescale set the values of another number of videos than this geometry's b = B/3");
    hipStream_t st = (hipStream_t)stream;
    const bool masked = blends != nullptr;
    S2V_TRY(stage_step(c, timesteps, coefs, b, st, blends));
    if (!use_graph) return guided_step_launches(c, latents, x0_hist, noise, st, masked);
    GraphKey key{latents, x0_hist, noise, -1};
    key.triple = 1; key.rescale = c->gr_buf ? 1 : 0;
    if (masked) { key.z0 = c->blend_z0; key.noise0 = c->blend_noise0; key.mask = c->blend_mask; }
    return launch_captured(c, key, st, [&](hipStream_t s) { return guided_step_launches(c, latents, x0_hist, noise, s, masked); });
}

// ---- temporal windows: a long latent stepped as overlapping windows of the geometry's F frames (include/s2v_hip.h) ---------------------------
extern "C" int s2v_set_windows(s2v_ctx* c, int32_t L, int32_t stride, int32_t per_forward, const float* weights) {
    S2V_REQUIRE(c, "s2v_set_windows: null context");
    if (L == 0) {
        if (c->win_acc) { S2V_CHECK_HIP(hipDeviceSynchronize()); drop_graph(c); win_free(c); }
        return 0;
    }
    S2V_REQUIRE(c->kind == S2V_CTX_MODEL, "s2v_set_windows: attention-only contexts (S2V_CTX_ATTN_*) run no step");
    S2V_REQUIRE(!c->shard, "s2v_set_windows: a shard context (s2v_set_shard) has no windowed step: temporal windows run on one GPU");
    S2V_REQUIRE(!c->gr_buf, "s2v_set_windows: guidance rescale is armed (s2v_set_guidance_rescale): the windowed step has no rescaled form");
    S2V_REQUIRE(c->ws, "s2v_set_windows: call s2v_set_geometry first (B = 2 per_forward samples of F = the window's frames)");
    S2V_REQUIRE(c->B != 1, "s2v_set_windows: a geometry with B = 1 is one sample of a CFG-parallel pair: the windowed step runs the CFG pairs of "
                           "per_forward windows, B = 2 per_forward, on one GPU");
    S2V_REQUIRE(!c->cond_triples, "s2v_set_windows: the context is conditioned as subject-guidance triples (s2v_set_conditioning_triples): the "
                                  "windowed step runs CFG pairs");
    S2V_REQUIRE(c->sc_arm == S2V_STEP_FULL, "s2v_set_windows: a step-cache mode is armed (s2v_step_cache_arm): the step cache holds one forward's "
                                            "residual, a windowed step runs several");
    S2V_REQUIRE(c->am_arm == 0, "s2v_set_windows: an attention map is armed (s2v_attn_map_arm): the attention map follows one forward per step, a "
                                "windowed step runs several");
    S2V_REQUIRE(per_forward >= 1 && 2 * per_forward <= S2V_MAX_BATCH && c->B == 2 * per_forward,
                "s2v_set_windows: the geometry must hold B = 2 per_forward samples, [negative x per_forward | positive x per_forward], 1 <= per_forward <= 4");
    const int F = c->F;
    S2V_REQUIRE(weights && stride >= 1 && stride <= F && L >= F && (L - F) % stride == 0,
                "s2v_set_windows: windows of the geometry's F frames, 1 <= stride <= F apart, must tile the L frames exactly: L >= F and (L - F) % stride == 0");
    const int W = (L - F) / stride + 1;
    S2V_REQUIRE(W % per_forward == 0, "s2v_set_windows: per_forward must divide the number of windows W = (L - F) / stride + 1");
    S2V_REQUIRE(c->cfg.in_channels == c->cfg.out_channels, "s2v_set_windows: in/out channels must match");
    const int64_t chw = (int64_t)c->cfg.out_channels * c->H * c->W;
    S2V_REQUIRE(L * chw < ((int64_t)1 << 31), "s2v_set_windows: a long latent of fewer than 2^31 elements");
    S2V_CHECK_HIP(hipDeviceSynchronize());
    drop_graph(c);
    win_free(c);
    // the sum of the weights over the windows that cover a frame, accumulated in window order as the plane is
    std::vector<float> host((size_t)F + L, 0.f);
    for (int j = 0; j < F; ++j) host[j] = weights[j];
    for (int k = 0; k < W; ++k)
        for (int j = 0; j < F; ++j) host[F + k * stride + j] += weights[j];
    const int64_t plane = rup(L * chw * 4, 256);
    S2V_CHECK_HIP(hipMalloc((void**)&c->win_acc, plane + (int64_t)host.size() * 4));
    c->win_w = (float*)((char*)c->win_acc + plane); c->win_wsum = c->win_w + F;
    c->win_bytes = plane + (int64_t)host.size() * 4;
    S2V_CHECK_HIP(hipMemcpy(c->win_w, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    c->win_L = L; c->win_s = stride; c->win_pf = per_forward; c->win_W = W;
    return 0;
}

static WindowBlendArgs window_blend_args(const void* noise_pred, float* acc, const float* w, const float* wsum, int L, int F, int s, int k0, int wb, int chw) {
    WindowBlendArgs a{};
    a.noise_pred = noise_pred; a.acc = acc; a.w = w; a.wsum = wsum; a.L = L; a.F = F; a.s = s; a.W = s >= 1 ? (L - F) / s + 1 : 0;
    a.k0 = k0; a.wb = wb; a.chw = chw;
    return a;
}

// W / per_forward rounds of [forward on the batch's windows, blend into the plane], then the scheduler step on the long latent from the plane
static int windows_step_launches(s2v_ctx* c, void* latents, float* x0_hist, const void* noise, hipStream_t st) {
    const int pf = c->win_pf;
    const int64_t chw = (int64_t)c->cfg.out_channels * c->H * c->W, hop = (int64_t)c->win_s * chw;
    for (int k0 = 0; k0 < c->win_W; k0 += pf) {
        // sample j of [negative x pf | positive x pf] embeds window k0 + j mod pf straight from the long latent (one window: the pair's stride of 0)
        S2V_TRY(forward_impl(c, (const char*)latents + k0 * hop * c->esz, pf > 1 ? hop : 0, pf > 1 ? pf : 0, c->t_dev, c->noise_pred, st));
        WindowBlendArgs w = window_blend_args(c->noise_pred, c->win_acc, c->win_w, c->win_wsum, c->win_L, c->F, c->win_s, k0, pf, (int)chw);
        w.coef = c->coef_dev;
        S2V_TRY(launch_window_blend(w, c->dtype, st));
    }
    SchedArgs a{};
    a.noise_pred = c->win_acc; a.latents_in = latents; a.latents_out = latents; a.x0_hist = x0_hist; a.noise = noise;
    a.nvid = 1; a.n_vid = a.n = c->win_L * chw; a.cfg = 0; a.np_f32 = 1; a.coef = c->coef_dev;
    return launch_sched_step(a, c->dtype, st);
}

extern "C" int s2v_denoise_step_windows(s2v_ctx* c, void* latents, float timestep, const s2v_sched_coef* coef_host, float* x0_hist, const void* noise,
                                        int32_t use_graph, s2v_stream stream) {
    S2V_REQUIRE(c && latents && coef_host, "s2v_denoise_step_windows: null argument");
    // the arms are one-shot and taken by every step entry, refused or not
    const int mode = sc_take_arm(c);
    const uint64_t am = am_take_arm(c);
    S2V_REQUIRE(st_take_arm(c) == 0, "s2v_denoise_step_windows: attention steering is armed (s2v_attn_steer_arm): steering runs one forward per step, a windowed "
                                     "step runs several");
    S2V_REQUIRE(la_take_arm(c) == 0, "s2v_denoise_step_windows: local attention is armed (s2v_attn_local_arm): local attention runs one forward per step, a "
                                     "windowed step runs several");
    S2V_REQUIRE(!c->gr_buf, "s2v_denoise_step_windows: guidance rescale is armed (s2v_set_guidance_rescale): the windows are combined before the one scheduler "
                            "step, and a statistic per window is another feature");
    S2V_REQUIRE(c->win_acc, "s2v_denoise_step_windows: no temporal windows are set (s2v_set_windows): a plain geometry steps with s2v_denoise_step");
    S2V_REQUIRE(c->have_cond && !c->cond_triples, "s2v_denoise_step_windows: the conditioning must hold the CFG pairs [negative x per_forward | positive x per_forward] "
                                                  "(s2v_set_conditioning)");
    S2V_REQUIRE(mode == S2V_STEP_FULL, "s2v_denoise_step_windows: a step-cache mode (s2v_step_cache_arm: CAPTURE / REUSE) is armed: the step cache holds one "
                                       "forward's residual, a windowed step runs several");
    S2V_REQUIRE(am == 0, "s2v_denoise_step_windows: an attention map is armed (s2v_attn_map_arm): the attention map follows one forward per step, a "
                         "windowed step runs several");
    S2V_REQUIRE(coef_host->kind == 0 || (noise && x0_hist), "s2v_denoise_step_windows: DPM needs noise and x0_hist");
    hipStream_t st = (hipStream_t)stream;
    S2V_TRY(stage_step(c, timestep, coef_host, st));
    if (!use_graph) return windows_step_launches(c, latents, x0_hist, noise, st);
    GraphKey key{latents, x0_hist, noise, -1};
    key.windows = 1;
    return launch_captured(c, key, st, [&](hipStream_t s) { return windows_step_launches(c, latents, x0_hist, noise, s); });
}

extern "C" int s2v_op_window_blend(const void* noise_pred, float* acc, const float* weights, const float* wsum, float guidance, int32_t L, int32_t F,
                                   int32_t stride, int32_t k0, int32_t wb, int32_t chw, int32_t dtype, s2v_stream stream) {
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_op_window_blend: unsupported dtype");
    WindowBlendArgs a = window_blend_args(noise_pred, acc, weights, wsum, L, F, stride, k0, wb, chw);
    a.gval = guidance;
    return launch_window_blend(a, dtype, (hipStream_t)stream);
}

// ---- CFG-parallel (round 6): ONE video on TWO GPUs ---------------------------------------------------------------------------------
// The CFG pair of custom_cogvideox_pipe.py:255-279 is two independent forwards that meet only in `noise_pred_uncond + g * (noise_pred_text -
// noise_pred_uncond)` (:266-279).  Each rank of a pair holds a B = 1 geometry with ITS half of the prompt embeddings (slot 0 = negative /
// unconditional, slot 1 = positive: the order of :196) and the un-duplicated reference tokens (cogvideox_transformer_3d.py:503-504 duplicates them
// only to fill the pair).  begin: the rank's forward into half `slot` of the context-owned pair buffer (a forward-only hipGraph);  the caller
// exchanges the halves (s2v_rccl_allgather in place, or any transport -- the collective stays OUTSIDE the captured graph);  end: fp32 CFG +
// scheduler step + round on the pair, run REDUNDANTLY by both ranks (:266-296): both hold bit-identical latents without a second collective.
int s2v_rccl_pair_check(s2v_rccl_comm* comm, int slot);  // rccl.hip (not exported)
static int64_t pair_half_bytes(const s2v_ctx* c) { return (int64_t)c->F * c->cfg.out_channels * c->H * c->W * c->esz; }

extern "C" int s2v_denoise_split_begin(s2v_ctx* c, const void* latents, float timestep, const s2v_sched_coef* coef_host, int32_t slot,
                                       int32_t use_graph, s2v_stream stream) {
    // a begin is pending only once its forward is on the stream: whatever fails below, s2v_denoise_split_end finds none
    if (c) c->split_kind = -1;
    S2V_REQUIRE(c && latents && coef_host, "s2v_denoise_split_begin: null argument");
    S2V_REQUIRE(sc_take_arm(c) == S2V_STEP_FULL, "s2v_denoise_split_begin: a step-cache mode (s2v_step_cache_arm: CAPTURE / REUSE) is armed, and CFG-parallel "
                                                 "has its own forward per rank: the step cache runs on one GPU (s2v_denoise_step)");
    S2V_REQUIRE(am_take_arm(c) == 0, "s2v_denoise_split_begin: an attention map is armed (s2v_attn_map_arm), and a CFG-parallel split holds one sample of the pair "
                                     "per rank: the attention map runs on one GPU (s2v_denoise_step)");
    S2V_REQUIRE(st_take_arm(c) == 0, "s2v_denoise_split_begin: attention steering is armed (s2v_attn_steer_arm), and a CFG-parallel split holds one sample of the "
                                     "pair per rank: steering runs on one GPU (s2v_denoise_step)");
    S2V_REQUIRE(la_take_arm(c) == 0, "s2v_denoise_split_begin: local attention is armed (s2v_attn_local_arm), and a CFG-parallel split holds one sample of the "
                                     "pair per rank: local attention runs on one GPU (s2v_denoise_step)");
    S2V_REQUIRE(!c->gr_buf, "s2v_denoise_split_begin: guidance rescale is armed (s2v_set_guidance_rescale), and the CFG-parallel split entries have no rescaled "
                            "form: guidance rescale runs on one GPU (s2v_denoise_step)");
    S2V_REQUIRE(c->ws && c->B == 1, "s2v_denoise_split_begin: a geometry with B = 1 (one sample of the CFG pair per rank) is required; a batched call (several videos) runs on one GPU (s2v_denoise_step)");
    S2V_REQUIRE(!c->shard, "s2v_denoise_split_begin: CFG-parallel on a shard context is not supported");
    S2V_REQUIRE(slot == 0 || slot == 1, "s2v_denoise_split_begin: slot must be 0 (unconditional) or 1 (conditional)");
    S2V_REQUIRE(c->cfg.in_channels == c->cfg.out_channels, "s2v_denoise_split_begin: in/out channels must match");
    hipStream_t st = (hipStream_t)stream;
    S2V_TRY(stage_step(c, timestep, coef_host, st));
    char* out = c->noise_pred + (int64_t)slot * pair_half_bytes(c);
    auto forward = [&](hipStream_t s) { return forward_impl(c, latents, 0, 0, c->t_dev, out, s); };
    S2V_TRY(use_graph ? launch_captured(c, GraphKey{(void*)latents, nullptr, nullptr, slot}, st, forward) : forward(st));
    c->split_kind = coef_host->kind;
    return 0;
}

extern "C" int s2v_cfg_pair(s2v_ctx* c, void** dev_ptr, int64_t* bytes_per_half) {
    S2V_REQUIRE(c && c->ws && dev_ptr && bytes_per_half, "s2v_cfg_pair: no workspace");
    *dev_ptr = c->noise_pred;
    *bytes_per_half = pair_half_bytes(c);
    return 0;
}

extern "C" int s2v_denoise_split_end(s2v_ctx* c, void* latents, float* x0_hist, const void* noise, s2v_stream stream) {
    S2V_REQUIRE(c && latents, "s2v_denoise_split_end: null argument");
    S2V_REQUIRE(c->ws && c->B == 1, "s2v_denoise_split_end: a geometry with B = 1 is required (s2v_denoise_split_begin ran before); a batched call (several videos) runs on one GPU (s2v_denoise_step)");
    // the step's coefficients live on the device since s2v_denoise_split_begin: one end per begin, and a DPM step brings its noise and x0 history
    S2V_REQUIRE(c->split_kind >= 0, "s2v_denoise_split_end: no s2v_denoise_split_begin is pending (its coefficients are the step's)");
    S2V_REQUIRE(c->split_kind == 0 || (noise && x0_hist), "s2v_denoise_split_end: DPM needs noise and x0_hist");
    c->split_kind = -1;
    return sched_on_pair(c, latents, x0_hist, noise, 1, (hipStream_t)stream);  // the coefficients s2v_denoise_split_begin uploaded
}

extern "C" int s2v_denoise_step_cfg_parallel(s2v_ctx* c, s2v_rccl_comm* comm, int32_t slot, void* latents, float timestep,
                                             const s2v_sched_coef* coef_host, float* x0_hist, const void* noise, int32_t use_graph,
                                             s2v_stream stream) {
    S2V_REQUIRE(c && comm && latents && coef_host, "s2v_denoise_step_cfg_parallel: null argument");
    S2V_REQUIRE(coef_host->kind == 0 || (noise && x0_hist), "s2v_denoise_step_cfg_parallel: DPM needs noise and x0_hist");
    S2V_TRY(s2v_rccl_pair_check(comm, slot));  // a two-rank communicator whose rank IS the slot: the in-place all-gather puts rank r's bytes into half r
    S2V_TRY(s2v_denoise_split_begin(c, latents, timestep, coef_host, slot, use_graph, stream));
    const int64_t half = pair_half_bytes(c);
    S2V_TRY(s2v_rccl_allgather(comm, c->noise_pred + (int64_t)slot * half, c->noise_pred, half, stream));  // in place: rank r owns half r
    return s2v_denoise_split_end(c, latents, x0_hist, noise, stream);
}

// ---- Ulysses sequence parallelism: ONE video's step on p GPUs -------------------------------------------------------------------------------
// Every row-wise kernel runs on the rank's mini-sequence [T_r | R_r | V_r] of each sample; the attention runs on heads [r*H/p, (r+1)*H/p) of all
// gN tokens, in global token order.  Two all-to-alls per block (QKV rows -> heads, attention output heads -> rows) and one all-gather of the
// projected video rows per step; the caller moves the bytes (s2v_shard_buffers) or s2v_denoise_step_ulysses does it over RCCL.
int s2v_rccl_shard_check(s2v_rccl_comm* comm, int world, int rank);  // rccl.hip (not exported)

// LN1 of layer l, the QKV projection with q/k LayerNorm + RoPE on the rank's rows, pack: chunk g of sbuf = [M][q_g | k_g | v_g].  fp8 engine: the
// projection is the single engine's fp8 GEMM on the LN1 pre-quantisation; with fp8 QK^T too the q/k LayerNorm + RoPE stay in the epilogue here (the
// single engine folds them into its quantisation pass, qk_norm_quant_mx_k: the same bits) and q / k are quantised after the exchange
static int shard_front(s2v_ctx* c, int l, hipStream_t st) {
    const LayerW& w = c->layers[l];
    const int D = c->D;
    const int64_t E = c->esz, Dp = D / c->sp;
    const char* mb = c->mod + (int64_t)(2 * l) * c->mc * D * E;
    bool prequant = false;
    S2V_TRY(block_norm(c, l, 0, mb, c->mod_rows, st, &prequant));
    const bool fused = qk_epilogue_ok(c);
    S2V_TRY(qkv_proj(c, w, D, false, fused, prequant, st));
    if (!fused) {  // vt stays null: V^T is made after the exchange, on the head-sharded buffer
        ProfScope ps(c, PK_QKNORM, st);
        S2V_TRY(launch_qk_norm_rope(qk_norm_args(c, w), c->dtype, st));
    }
    ShardCopyArgs a{};
    a.src = c->QKV; a.dst = c->sbuf; a.rows = (int)c->M; a.width16 = (int)(Dp * E / 16);
    a.src_ld = 3 * D * E; a.dst_ld = 3 * Dp * E;
    a.nseg = 3 * c->sp; a.nseg_inner = 3;
    a.src_seg_outer = Dp * E; a.src_seg_inner = D * E; a.dst_seg_outer = c->M * 3 * Dp * E; a.dst_seg_inner = Dp * E;
    ProfScope ps(c, PK_SHARD, st);
    return launch_shard_copy(a, st);
}

// unpack the QKV exchange into global token order, V^T, attention on the rank's heads, pack: chunk q of sbuf = rank q's rows of the output.  The
// kernel and formats are run_attention's, chosen on the whole sequence gN; fp8 engine: the output leaves the kernel as MX e4m3 (Oh bytes, Os
// scales) and is packed as such -- per peer its rows' bytes, then their scale dwords
static int shard_attention(s2v_ctx* c, hipStream_t st) {
    const int64_t E = c->esz, Dp = c->D / c->sp, Mg = (int64_t)c->B * c->gN;
    const int H = c->cfg.num_heads / c->sp;
    const bool mx = c->o_mx;
    S2V_REQUIRE(mx == attn_mx_out(c), "shard_attention: the attention output format changed after s2v_set_geometry (set the geometry again)");
    {
        ShardCopyArgs a{};
        a.src = c->rbuf; a.dst = c->QKVh; a.rows = (int)Mg; a.width16 = (int)(3 * Dp * E / 16);
        a.src_ld = a.dst_ld = 3 * Dp * E; a.dst_map = c->rmap; a.nseg = 1; a.nseg_inner = 1;
        ProfScope ps(c, PK_SHARD, st);
        S2V_TRY(launch_shard_copy(a, st));
    }
    const AttnOperands q{c->QKVh, (int)(3 * Dp), H, c->gN, c->Oh, (int)Dp, (unsigned char*)c->Oh, c->Os, c->Os_rows};
    S2V_TRY(attn_core(c, q, QK_DONE, nullptr, st));  // fp8 QK^T: q / k of the rank's heads are quantised here, after the exchange
    ShardCopyArgs o{};
    o.src = c->Oh; o.dst = c->sbuf; o.rows = (int)Mg; o.width16 = (int)(Dp * E / 16);
    o.src_ld = o.dst_ld = Dp * E; o.src_map = c->rmap; o.nseg = 1; o.nseg_inner = 1;
    if (mx) { o.width16 = (int)(Dp / 16); o.src_ld = Dp; o.dst_ld = 16; o.dst_map = c->omap; }  // omap: the byte offset / 16 of each send row
    ProfScope ps(c, PK_SHARD, st);
    S2V_TRY(launch_shard_copy(o, st));
    if (!mx) return 0;
    ShardScaleArgs s{};  // scale dwords (kt, global row rmap[i]) of Os -> sbuf dword omap[Mg + i] + kt
    s.src = (const unsigned*)c->Os; s.dst = (unsigned*)c->sbuf; s.rows = (int)Mg; s.nkt = (int)(Dp / 128); s.nseg = 1;
    s.src_map = c->rmap; s.dst_map = c->omap + Mg;
    s.src_row = 1; s.src_kt = c->Os_rows; s.src_perm = 1;
    s.dst_row = 1; s.dst_kt = 1;
    return launch_shard_scales(s, st);
}

// unpack the O exchange (head group g -> columns g*D/p of Xn), out-projection, LN2, FF; then the next layer's front or the tail
// fp8 engine: the MX image goes where run_attention's kernel leaves it for the out-projection -- bytes to aq [M][D] at columns g*D/p, scale dwords to
// hs at K-tiles g*D/(128p) ..., rows mx_perm_row(local row) of mx_rows = Mpad
static int shard_back(s2v_ctx* c, int l, hipStream_t st, int* pending) {
    const int D = c->D;
    const int64_t E = c->esz, Dp = D / c->sp;
    if (c->o_mx) {
        const int64_t nkt = Dp / 128, chunk = c->M * Dp + rup(c->M * nkt * 4, 16);  // one peer's chunk: [M][D/p] bytes, [M][nkt] scale dwords, pad
        ShardCopyArgs a{};
        a.src = c->rbuf; a.dst = c->aq; a.rows = (int)c->M; a.width16 = (int)(Dp / 16);
        a.src_ld = Dp; a.dst_ld = D; a.nseg = c->sp; a.nseg_inner = 1;
        a.src_seg_outer = chunk; a.dst_seg_outer = Dp;
        ShardScaleArgs s{};
        s.src = (const unsigned*)(c->rbuf + c->M * Dp); s.dst = (unsigned*)c->hs; s.rows = (int)c->M; s.nkt = (int)nkt; s.nseg = c->sp;
        s.src_row = nkt; s.src_kt = 1; s.src_seg = chunk / 4;
        s.dst_row = 1; s.dst_kt = c->Mpad; s.dst_seg = nkt * c->Mpad; s.dst_perm = 1;
        ProfScope ps(c, PK_SHARD, st);
        S2V_TRY(launch_shard_copy(a, st));
        S2V_TRY(launch_shard_scales(s, st));
    } else {
        ShardCopyArgs a{};
        a.src = c->rbuf; a.dst = c->Xn; a.rows = (int)c->M; a.width16 = (int)(Dp * E / 16);
        a.src_ld = Dp * E; a.dst_ld = D * E; a.nseg = c->sp; a.nseg_inner = 1;
        a.src_seg_outer = c->M * Dp * E; a.dst_seg_outer = Dp * E;
        ProfScope ps(c, PK_SHARD, st);
        S2V_TRY(launch_shard_copy(a, st));
    }
    const char* mb = c->mod + (int64_t)(2 * l) * c->mc * D * E;
    S2V_TRY(out_proj(c, c->layers[l], c->lora_on(), block_gate(c, 0, mb, c->mod_rows), EPI_BIAS_GATE_RES, true, st));
    bool prequant = false;
    S2V_TRY(block_norm(c, l, 1, mb, c->mod_rows, st, &prequant));
    S2V_TRY(block_ff(c, l, block_gate(c, 1, mb, c->mod_rows), prequant, st));
    if (l + 1 < c->L) {
        S2V_TRY(shard_front(c, l + 1, st));
        *pending = S2V_SHARD_QKV_EXCHANGE;
        return 0;
    }
    S2V_TRY(tail_proj(c, st));
    const int64_t Co = c->cfg.out_channels * 4;
    ShardCopyArgs a{};
    a.src = c->proj; a.dst = c->nsend; a.rows = c->V; a.width16 = (int)(Co * E / 16);
    a.src_ld = a.dst_ld = Co * E; a.nseg = c->B; a.nseg_inner = 1;
    a.src_seg_outer = (int64_t)c->V * Co * E; a.dst_seg_outer = (int64_t)c->Vmax * Co * E;
    ProfScope ps(c, PK_SHARD, st);
    S2V_TRY(launch_shard_copy(a, st));
    *pending = S2V_SHARD_NOISE_GATHER;
    return 0;
}

extern "C" int s2v_shard_layout(s2v_ctx* c, int32_t* out) {
    S2V_REQUIRE(c && out, "s2v_shard_layout: null argument");
    S2V_REQUIRE(c->shard && c->ws, "s2v_shard_layout: call s2v_set_shard, then s2v_set_geometry");
    for (int g = 0; g < c->sp; ++g) {
        int b, n;
        shard_range(c->gT, c->sp, g, &b, &n); out[3 * g] = n;
        shard_range(c->gR, c->sp, g, &b, &n); out[3 * g + 1] = n;
        shard_range(c->gV, c->sp, g, &b, &n); out[3 * g + 2] = n;
    }
    return 0;
}

extern "C" int s2v_shard_buffers(s2v_ctx* c, int32_t kind, void** send, void** recv, int64_t* send_counts, int64_t* send_displs,
                                 int64_t* recv_counts, int64_t* recv_displs) {
    S2V_REQUIRE(c && send && recv && send_counts && send_displs && recv_counts && recv_displs, "s2v_shard_buffers: null argument");
    S2V_REQUIRE(c->shard && c->ws, "s2v_shard_buffers: call s2v_set_shard, then s2v_set_geometry");
    S2V_REQUIRE(kind == S2V_SHARD_QKV_EXCHANGE || kind == S2V_SHARD_O_EXCHANGE || kind == S2V_SHARD_NOISE_GATHER, "s2v_shard_buffers: unknown exchange kind");
    const int k = kind - 1;
    *send = kind == S2V_SHARD_NOISE_GATHER ? c->nsend : c->sbuf;
    *recv = kind == S2V_SHARD_NOISE_GATHER ? c->nrecv : c->rbuf;
    for (int g = 0; g < c->sp; ++g) {
        send_counts[g] = c->xcnt[k][0][g]; send_displs[g] = c->xcnt[k][1][g];
        recv_counts[g] = c->xcnt[k][2][g]; recv_displs[g] = c->xcnt[k][3][g];
    }
    return 0;
}

extern "C" int s2v_shard_step_begin(s2v_ctx* c, const void* latents, float timestep, const s2v_sched_coef* coef_host, int32_t* pending,
                                    s2v_stream stream) {
    S2V_REQUIRE(c && latents && coef_host && pending, "s2v_shard_step_begin: null argument");
    S2V_REQUIRE(c->shard, "s2v_shard_step_begin: not a shard context (s2v_set_shard)");
    S2V_REQUIRE(c->ws && (c->B == 1 || c->B == 2), "s2v_shard_step_begin: geometry with B = 1 or 2 (CFG pair) required; a batched call (several videos) runs on one GPU (s2v_denoise_step)");
    S2V_REQUIRE(c->finalized && c->have_cond, "s2v_shard_step_begin: weights and conditioning required");
    S2V_REQUIRE(!c->cfg.use_rope || c->have_rope, "s2v_shard_step_begin: RoPE tables missing (s2v_set_rope)");
    S2V_REQUIRE(c->cfg.use_rope || c->have_pos, "s2v_shard_step_begin: sincos table missing (s2v_set_pos_embed)");
    S2V_REQUIRE(c->cfg.in_channels == c->cfg.out_channels, "s2v_shard_step_begin: in/out channels must match");
    hipStream_t st = (hipStream_t)stream;
    S2V_TRY(stage_step(c, timestep, coef_host, st));
    c->sh_pending = 0;
    S2V_TRY(embed_streams(c, latents, 0, 0, c->t_dev, st));
    S2V_TRY(shard_front(c, 0, st));
    c->split_kind = coef_host->kind;
    c->sh_layer = 0;
    *pending = c->sh_pending = S2V_SHARD_QKV_EXCHANGE;
    return 0;
}

extern "C" int s2v_shard_step_resume(s2v_ctx* c, int32_t* pending, s2v_stream stream) {
    S2V_REQUIRE(c && pending, "s2v_shard_step_resume: null argument");
    S2V_REQUIRE(c->shard && (c->sh_pending == S2V_SHARD_QKV_EXCHANGE || c->sh_pending == S2V_SHARD_O_EXCHANGE),
                "s2v_shard_step_resume: no exchange is pending (s2v_shard_step_begin first; after S2V_SHARD_NOISE_GATHER comes s2v_shard_step_end)");
    hipStream_t st = (hipStream_t)stream;
    int next = 0;
    if (c->sh_pending == S2V_SHARD_QKV_EXCHANGE) {
        c->sh_pending = 0;  // a failure leaves no step pending
        S2V_TRY(shard_attention(c, st));
        next = S2V_SHARD_O_EXCHANGE;
    } else {
        c->sh_pending = 0;
        S2V_TRY(shard_back(c, c->sh_layer, st, &next));
        if (next == S2V_SHARD_QKV_EXCHANGE) c->sh_layer++;
    }
    *pending = c->sh_pending = next;
    return 0;
}

extern "C" int s2v_shard_step_end(s2v_ctx* c, void* latents, float* x0_hist, const void* noise, s2v_stream stream) {
    S2V_REQUIRE(c && latents, "s2v_shard_step_end: null argument");
    S2V_REQUIRE(c->shard && c->sh_pending == S2V_SHARD_NOISE_GATHER, "s2v_shard_step_end: the noise gather is not pending");
    S2V_REQUIRE(c->split_kind == 0 || (noise && x0_hist), "s2v_shard_step_end: DPM needs noise and x0_hist");
    c->sh_pending = 0;
    c->split_kind = -1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t E = c->esz, Co = c->cfg.out_channels * 4;
    {
        ShardCopyArgs a{};
        a.src = c->nrecv; a.dst = c->proj_full; a.rows = c->sp * c->B * c->Vmax; a.width16 = (int)(Co * E / 16);
        a.src_ld = a.dst_ld = Co * E; a.dst_map = c->nmap; a.nseg = 1; a.nseg_inner = 1;
        ProfScope ps(c, PK_SHARD, st);
        S2V_TRY(launch_shard_copy(a, st));
    }
    S2V_TRY(launch_unpatchify(c->proj_full, (int)Co, c->gV, c->noise_pred, c->B, c->F, c->cfg.out_channels, c->H, c->W, c->dtype, st));
    return sched_on_pair(c, latents, x0_hist, noise, c->B == 2 ? 1 : 0, st);
}

extern "C" int s2v_denoise_step_ulysses(s2v_ctx* c, s2v_rccl_comm* comm, void* latents, float timestep, const s2v_sched_coef* coef_host,
                                        float* x0_hist, const void* noise, s2v_stream stream) {
    S2V_REQUIRE(c && comm && latents && coef_host, "s2v_denoise_step_ulysses: null argument");
    S2V_REQUIRE(c->shard, "s2v_denoise_step_ulysses: not a shard context (s2v_set_shard)");
    S2V_REQUIRE(coef_host->kind == 0 || (noise && x0_hist), "s2v_denoise_step_ulysses: DPM needs noise and x0_hist");
    S2V_TRY(s2v_rccl_shard_check(comm, c->sp, c->sr));
    int pending = 0;
    std::vector<int64_t> sc(c->sp), sd(c->sp), rc(c->sp), rd(c->sp);
    S2V_TRY(s2v_shard_step_begin(c, latents, timestep, coef_host, &pending, stream));
    for (;;) {
        void *sb = nullptr, *rb = nullptr;
        S2V_TRY(s2v_shard_buffers(c, pending, &sb, &rb, sc.data(), sd.data(), rc.data(), rd.data()));
        S2V_TRY(s2v_rccl_alltoallv(comm, sb, sc.data(), sd.data(), rb, rc.data(), rd.data(), stream));
        if (pending == S2V_SHARD_NOISE_GATHER) break;
        S2V_TRY(s2v_shard_step_resume(c, &pending, stream));
    }
    return s2v_shard_step_end(c, latents, x0_hist, noise, stream);
}

// Per-kernel-class timing (HIP events recorded on the launch stream around every launch of the class).
// classes: 0 qkv GEMM, 1 attention, 2 out-proj GEMM, 3 FF1 GEMM, 4 FF2 GEMM, 5 LN-modulate, 6 qk-norm/rope/V^T
extern "C" int s2v_profile_enable(s2v_ctx* c, int32_t on) {
    S2V_REQUIRE(c, "null context");
    c->prof_on = on != 0;
    for (int k = 0; k < PK_NUM; ++k) c->prof_used[k] = 0;
    c->clk_rec.clear();
    if (on && !c->clk_buf) S2V_CHECK_HIP(hipMalloc((void**)&c->clk_buf, sizeof(long long) * 4 * CLK_SLOTS));
    if (on) S2V_CHECK_HIP(hipMemset(c->clk_buf, 0, sizeof(long long) * 4 * CLK_SLOTS));
    return 0;
}
// Average shader clock (MHz) under the launches of every class since s2v_profile_enable(1): sum of s_memtime spans / sum of s_memrealtime spans
// (100 MHz ticks) of the stamp pairs around them; 0 for a class without stamped launches.  Synchronises; clears the records.
extern "C" int s2v_profile_read_clocks(s2v_ctx* c, float* mhz_by_class, int32_t nclass) {
    S2V_REQUIRE(c && mhz_by_class, "s2v_profile_read_clocks: null argument");
    S2V_CHECK_HIP(hipDeviceSynchronize());
    std::vector<long long> h((size_t)4 * c->clk_rec.size());
    if (!h.empty()) S2V_CHECK_HIP(hipMemcpy(h.data(), c->clk_buf, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
    double cyc[PK_NUM] = {0}, ticks[PK_NUM] = {0};
    for (auto& r : c->clk_rec) {
        const long long* s = h.data() + 4 * r.second;
        if (s[2] > s[0] && s[3] > s[1]) { cyc[r.first] += (double)(s[2] - s[0]); ticks[r.first] += (double)(s[3] - s[1]); }
    }
    for (int k = 0; k < nclass && k < PK_NUM; ++k) mhz_by_class[k] = ticks[k] > 0 ? (float)(cyc[k] / ticks[k] * 100.0) : 0.f;
    c->clk_rec.clear();
    // the slots are handed out again from 0: a later pass that did not go through s2v_profile_enable(1) must not read these stamps
    if (c->clk_buf) S2V_CHECK_HIP(hipMemset(c->clk_buf, 0, sizeof(long long) * 4 * CLK_SLOTS));
    return 0;
}
// Synchronises, then returns total milliseconds and launch counts per class since the last read; resets.
extern "C" int s2v_profile_read(s2v_ctx* c, float* ms_by_class, int32_t* launches_by_class, int32_t nclass) {
    S2V_REQUIRE(c && ms_by_class && launches_by_class, "s2v_profile_read: null argument");
    S2V_CHECK_HIP(hipDeviceSynchronize());
    for (int k = 0; k < nclass && k < PK_NUM; ++k) {
        float tot = 0.f;
        for (size_t i = 0; i < c->prof_used[k]; ++i) {
            float ms = 0.f;
            S2V_CHECK_HIP(hipEventElapsedTime(&ms, c->prof_ev[k][i].first, c->prof_ev[k][i].second));
            tot += ms;
        }
        ms_by_class[k] = tot;
        launches_by_class[k] = (int32_t)c->prof_used[k];
        c->prof_used[k] = 0;
    }
    return 0;
}

extern "C" int s2v_last_noise_pred(s2v_ctx* c, void** dev_ptr) {
    S2V_REQUIRE(c && c->ws && dev_ptr, "s2v_last_noise_pred: no workspace");
    *dev_ptr = c->noise_pred;
    return 0;
}

// ---- attention map (include/s2v_hip.h) ---------------------------------------------------------------------------------------------------
extern "C" int s2v_attn_map_enable(s2v_ctx* c, int32_t on, const int32_t* text_spans_host, int32_t n_spans) {
    S2V_REQUIRE(c, "s2v_attn_map_enable: null context");
    if (!on) {
        if (c->am_on) { S2V_CHECK_HIP(hipDeviceSynchronize()); drop_graph(c); }
        am_free(c);
        return 0;
    }
    S2V_REQUIRE(c->kind == S2V_CTX_MODEL, "s2v_attn_map_enable: attention-only contexts (S2V_CTX_ATTN_*) run no forward");
    S2V_REQUIRE(!c->shard, "s2v_attn_map_enable: a shard context (s2v_set_shard) has no attention map: its attention sees a head group of all ranks' rows; the map runs on one GPU");
    S2V_REQUIRE(c->ws, "s2v_attn_map_enable: call s2v_set_geometry first (the sums are [1 + spans][B][H][V] of the current geometry)");
    S2V_REQUIRE(n_spans >= 0 && n_spans <= AM_MAX_RANGES - 1 && (n_spans == 0 || text_spans_host), "s2v_attn_map_enable: 0..3 text spans (2 ints each) are accepted");
    for (int i = 0; i < n_spans; ++i)
        S2V_REQUIRE(text_spans_host[2 * i] >= 0 && text_spans_host[2 * i] <= text_spans_host[2 * i + 1] && text_spans_host[2 * i + 1] <= c->T,
                    "s2v_attn_map_enable: a text span must be a token range inside [0, T) of the current geometry");
    S2V_CHECK_HIP(hipDeviceSynchronize());
    drop_graph(c);
    for (int i = 0; i < 2 * n_spans; ++i) c->am_spans[i] = text_spans_host[i];
    c->am_n = 1 + n_spans;
    return am_alloc(c);
}

extern "C" int s2v_attn_map_arm(s2v_ctx* c, uint64_t layer_mask) {
    S2V_REQUIRE(c, "s2v_attn_map_arm: null context");
    if (layer_mask) {
        S2V_REQUIRE(!c->shard, "s2v_attn_map_arm: a shard context (s2v_set_shard) has no attention map: the map runs on one GPU");
        S2V_REQUIRE(c->am_on && c->am_acc, "s2v_attn_map_arm: the attention map is not enabled (s2v_attn_map_enable)");
        S2V_REQUIRE(!c->fp8_qk, "s2v_attn_map_arm: fp8 QK^T is active at this geometry (q and k exist normed only as MX e4m3 images): the attention map "
                                "runs with 16-bit attention (the plain \"fp8\" weight format included)");
        S2V_REQUIRE(c->L >= 64 || (layer_mask >> c->L) == 0, "s2v_attn_map_arm: a layer bit at or beyond num_layers is set");
        S2V_REQUIRE(c->st_arm == 0, "s2v_attn_map_arm: attention steering is armed for the next forward (s2v_attn_steer_arm): the map reads the un-steered softmax");
        S2V_REQUIRE(c->la_arm == 0, "s2v_attn_map_arm: local attention is armed for the next forward (s2v_attn_local_arm): the map reads the un-windowed softmax");
        S2V_REQUIRE(c->sc_arm != S2V_STEP_REUSE, "s2v_attn_map_arm: S2V_STEP_REUSE is armed for the next forward (s2v_step_cache_arm): the block stack does not run, "
                                                 "there is no attention to follow");
    }
    c->am_arm = layer_mask;
    return 0;
}

// ---- attention steering (include/s2v_hip.h) -----------------------------------------------------------------------------------------------
extern "C" int s2v_attn_steer_enable(s2v_ctx* c, int32_t on) {
    S2V_REQUIRE(c, "s2v_attn_steer_enable: null context");
    if (!on) {
        if (c->st_on) { S2V_CHECK_HIP(hipDeviceSynchronize()); drop_graph(c); }
        st_free(c);
        return 0;
    }
    S2V_TRY(st_check(c, "s2v_attn_steer_enable"));
    if (c->st_on) return 0;
    S2V_CHECK_HIP(hipDeviceSynchronize());
    drop_graph(c);
    S2V_CHECK_HIP(hipMalloc((void**)&c->st_tab, sizeof(AttnSteerRec)));
    c->st_on = true; c->st_n = 0; c->st_arm = 0;
    const int r = st_upload(c, "s2v_attn_steer_enable");   // n = 0: a record that steers nothing
    if (r != 0) st_free(c);
    return r;
}

extern "C" int s2v_attn_steer_set(s2v_ctx* c, int32_t n, const s2v_attn_steer_range* ranges_host) {
    S2V_REQUIRE(c, "s2v_attn_steer_set: null context");
    S2V_REQUIRE(c->st_on && c->st_tab, "s2v_attn_steer_set: attention steering is not enabled (s2v_attn_steer_enable)");
    S2V_REQUIRE(n >= 0 && n <= ATTN_STEER_MAX_RANGES && (n == 0 || ranges_host), "s2v_attn_steer_set: 0..4 key ranges are accepted");
    int k0[ATTN_STEER_MAX_RANGES], k1[ATTN_STEER_MAX_RANGES]; float w[ATTN_STEER_MAX_RANGES]; unsigned m[ATTN_STEER_MAX_RANGES];
    for (int i = 0; i < n; ++i) { k0[i] = ranges_host[i].k0; k1[i] = ranges_host[i].k1; w[i] = ranges_host[i].w; m[i] = ranges_host[i].sample_mask; }
    AttnSteerRec r{};
    S2V_TRY(attn_steer_make("s2v_attn_steer_set", n, k0, k1, w, m, c->T + c->R, c->Ntok, c->Ntok, &r));   // checked before anything is replaced
    S2V_CHECK_HIP(hipDeviceSynchronize());   // a step on any stream may still read the table; a captured step is kept: the table is data
    if (c->st_kind == 1) {                   // ... unless the context held maps: one record, of one kind -- the captured steps launch the map kernels
        drop_graph(c);
        if (c->st_map) hipFree(c->st_map);
        c->st_map = nullptr; c->st_kind = 0; c->st_map_cap = c->st_map_V = c->st_map_Ntok = c->st_map_np = c->st_map_n = 0; c->st_map_w.clear();
    }
    c->st_n = n;
    for (int i = 0; i < n; ++i) { c->st_k0[i] = k0[i]; c->st_k1[i] = k1[i]; c->st_w[i] = w[i]; c->st_mask[i] = m[i]; }
    S2V_CHECK_HIP(hipMemcpy(c->st_tab, &r, sizeof(r), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int s2v_attn_steer_set_maps(s2v_ctx* c, int32_t n, const s2v_attn_steer_map_range* ranges_host, int32_t n_planes, const float* planes_host) {
    S2V_REQUIRE(c, "s2v_attn_steer_set_maps: null context");
    S2V_REQUIRE(c->st_on && c->st_tab, "s2v_attn_steer_set_maps: attention steering is not enabled (s2v_attn_steer_enable)");
    S2V_REQUIRE(n >= 0 && n <= ATTN_STEER_MAX_RANGES && (n == 0 || ranges_host), "s2v_attn_steer_set_maps: 0..4 key ranges are accepted");
    int k0[ATTN_STEER_MAX_RANGES] = {}, k1[ATTN_STEER_MAX_RANGES] = {};
    signed char pl[ATTN_STEER_MAX_RANGES][ATTN_STEER_MAP_BATCH];
    for (int i = 0; i < ATTN_STEER_MAX_RANGES; ++i)
        for (int b = 0; b < ATTN_STEER_MAP_BATCH; ++b) pl[i][b] = i < n ? ranges_host[i].plane[b] : -1;
    for (int i = 0; i < n; ++i) { k0[i] = ranges_host[i].k0; k1[i] = ranges_host[i].k1; }
    S2V_CHECK_HIP(hipDeviceSynchronize());   // a step on any stream may still read the table
    bool moved = false;                      // st_map_upload makes and checks the whole record before it touches the table
    const bool was_scalar = c->st_kind == 0;
    S2V_TRY(st_map_upload(c, "s2v_attn_steer_set_maps", n, k0, k1, &pl[0][0], n_planes, planes_host, &moved));
    if (moved || was_scalar) drop_graph(c);  // another table or another kind of record: the captured steps go; else they replay with the new maps
    c->st_kind = 1; c->st_map_n = n; c->st_map_np = n_planes;
    c->st_n = 0;   // the scalar record beside it is forgotten: a geometry change re-checks the maps' ranges only
    for (int i = 0; i < ATTN_STEER_MAX_RANGES; ++i) {
        c->st_map_k0[i] = k0[i]; c->st_map_k1[i] = k1[i];
        for (int b = 0; b < ATTN_STEER_MAP_BATCH; ++b) c->st_map_plane[i][b] = pl[i][b];
    }
    c->st_map_w.assign(planes_host, planes_host + (size_t)n_planes * c->V);
    return 0;
}

extern "C" int s2v_attn_steer_arm(s2v_ctx* c, uint64_t layer_mask) {
    S2V_REQUIRE(c, "s2v_attn_steer_arm: null context");
    if (layer_mask) {
        S2V_REQUIRE(c->st_on && c->st_tab, "s2v_attn_steer_arm: attention steering is not enabled (s2v_attn_steer_enable)");
        S2V_TRY(st_check(c, "s2v_attn_steer_arm"));
        S2V_REQUIRE(c->L >= 64 || (layer_mask >> c->L) == 0, "s2v_attn_steer_arm: a layer bit at or beyond num_layers is set");
        S2V_REQUIRE(c->am_arm == 0, "s2v_attn_steer_arm: an attention map is armed for the next forward (s2v_attn_map_arm): the map reads the un-steered softmax");
        S2V_REQUIRE(c->la_arm == 0, "s2v_attn_steer_arm: local attention is armed for the next forward (s2v_attn_local_arm): a layer runs one attention kernel");
        S2V_REQUIRE(c->sc_arm != S2V_STEP_REUSE, "s2v_attn_steer_arm: S2V_STEP_REUSE is armed for the next forward (s2v_step_cache_arm): the block stack does not run, "
                                                 "there is no attention to steer");
    }
    c->st_arm = layer_mask;
    return 0;
}

extern "C" int s2v_op_attention_steer(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok, int32_t dtype, int32_t impl,
                                      const s2v_attn_steer_record* record_host, s2v_stream stream) {
    S2V_REQUIRE(qkv && out && record_host, "s2v_op_attention_steer: null argument");
    S2V_REQUIRE(B >= 1 && B <= 32 && H >= 1 && Ntok >= 1, "s2v_op_attention_steer: 1 <= B <= 32 (the sample masks hold 32 samples), H >= 1, Ntok >= 1");
    S2V_REQUIRE(impl == 0 || impl == 1, "s2v_op_attention_steer: impl 0 (MFMA, bf16) or 1 (generic)");
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_op_attention_steer: unsupported dtype");
    S2V_REQUIRE(impl == 1 || (dtype == S2V_DTYPE_BF16 && vt_scratch), "s2v_op_attention_steer: impl 0 is bf16 and needs vt_scratch");
    AttnSteerRec r{};
    S2V_TRY(attn_steer_make("s2v_op_attention_steer", record_host->n, record_host->k0, record_host->k1, record_host->w, record_host->sample_mask,
                            record_host->q0, record_host->q1, Ntok, &r));
    // operator level: one table per process, on the device of the first call (as the fp16 V^T words of s2v_op_attention impl 3 / 4): such calls stay on
    // that device and on one stream.  The upload is ordered on the stream, so earlier launches have read the record they were given
    static AttnSteerRec* op_tab = nullptr;
    static AttnSteerRec* op_stage = nullptr;   // pinned ring: the asynchronous copy reads it after the call returns
    static int op_pos = 0;
    static bool op_bound = false;              // the one stream these calls are ordered on: a second stream would race the upload against a kernel
    static hipStream_t op_stream = nullptr;
    S2V_REQUIRE(!op_bound || op_stream == (hipStream_t)stream, "s2v_op_attention_steer: another stream than the first call's: the process-wide record table is "
                                                               "ordered on one stream (contexts hold their own table: s2v_attn_steer_set)");
    op_bound = true; op_stream = (hipStream_t)stream;
    if (!op_tab) S2V_CHECK_HIP(hipMalloc((void**)&op_tab, sizeof(AttnSteerRec)));
    if (!op_stage) S2V_CHECK_HIP(hipHostMalloc((void**)&op_stage, sizeof(AttnSteerRec) * 64));
    hipStream_t st = (hipStream_t)stream;
    if (op_pos == 64) { S2V_CHECK_HIP(hipStreamSynchronize(st)); op_pos = 0; }
    op_stage[op_pos] = r;
    S2V_CHECK_HIP(hipMemcpyAsync(op_tab, &op_stage[op_pos++], sizeof(r), hipMemcpyHostToDevice, st));
    const int D = H * 64;
    AttnArgs a{};
    a.qkv = qkv; a.ld_qkv = 3 * D; a.out = out; a.ld_out = D; a.B = B; a.H = H; a.Ntok = Ntok; a.scale = 0.125f;
    a.ntok_pad = (int)rup(Ntok, 64);
    if (impl == 0) {
        a.vt = vt_scratch;
        S2V_TRY(launch_v_transpose(qkv, 3 * D, B, H, Ntok, vt_scratch, a.ntok_pad, st, nullptr));
        return launch_attn_bf16_steer(a, op_tab, st);
    }
    a.valu_only = 1;
    return launch_attn_simple_steer(a, op_tab, dtype, st);
}

extern "C" int s2v_op_attention_steer_map(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok, int32_t dtype, int32_t impl,
                                          const s2v_attn_steer_map_record* record_host, const float* planes_host, s2v_stream stream) {
    S2V_REQUIRE(qkv && out && record_host, "s2v_op_attention_steer_map: null argument");
    S2V_REQUIRE(B >= 1 && B <= ATTN_STEER_MAP_BATCH && H >= 1 && Ntok >= 1, "s2v_op_attention_steer_map: 1 <= B <= 8 (a plane index per range and sample), H >= 1, Ntok >= 1");
    S2V_REQUIRE(impl == 0 || impl == 1 || impl == 2, "s2v_op_attention_steer_map: impl 0 (MFMA, bf16), 1 (generic) or 2 (MFMA, bf16, the persistent launch)");
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_op_attention_steer_map: unsupported dtype");
    S2V_REQUIRE(impl == 1 || (dtype == S2V_DTYPE_BF16 && vt_scratch), "s2v_op_attention_steer_map: impl 0 is bf16 and needs vt_scratch (and so is impl 2)");
    // operator level: one table per process, grown as needed, as s2v_op_attention_steer keeps its record: one device, one stream.  The record is of
    // any size, so a call with a NEW record synchronises the stream before the table is replaced and before its host copy goes; a call that repeats
    // the last call's record, planes, B and Ntok byte for byte launches on the table as it stands (a benchmark times the launch, not the host's logs)
    static int* op_tab = nullptr;
    static size_t op_words = 0;
    static bool op_bound = false;
    static hipStream_t op_stream = nullptr;
    static s2v_attn_steer_map_record op_rec{};
    static std::vector<float> op_planes;
    static int op_B = 0, op_Ntok = 0;
    const bool shape_ok = record_host->n_planes >= 1 && record_host->n_planes <= ATTN_STEER_MAP_MAX_PLANES && record_host->q0 >= 0 && record_host->q0 < record_host->q1 &&
                          record_host->q1 <= Ntok && planes_host;
    const size_t n_w = shape_ok ? (size_t)record_host->n_planes * (record_host->q1 - record_host->q0) : 0;
    const bool same = shape_ok && op_tab && op_bound && op_stream == (hipStream_t)stream && op_B == B && op_Ntok == Ntok &&
                      memcmp(&op_rec, record_host, sizeof(op_rec)) == 0 && op_planes.size() == n_w && memcmp(op_planes.data(), planes_host, n_w * 4) == 0;
    std::vector<int> r;
    if (!same)
        S2V_TRY(attn_steer_map_make("s2v_op_attention_steer_map", record_host->n, record_host->k0, record_host->k1, &record_host->plane[0][0],
                                    record_host->n_planes, planes_host, record_host->q0, record_host->q1, Ntok, B, record_host->n_planes, &r));
    S2V_REQUIRE(!op_bound || op_stream == (hipStream_t)stream, "s2v_op_attention_steer_map: another stream than the first call's: the process-wide record table is "
                                                               "ordered on one stream (contexts hold their own table: s2v_attn_steer_set_maps)");
    op_bound = true; op_stream = (hipStream_t)stream;
    hipStream_t st = (hipStream_t)stream;
    if (!same) {
        S2V_CHECK_HIP(hipStreamSynchronize(st));
        op_planes.clear();   // nothing is held while the table is in between
        if (r.size() > op_words) {
            if (op_tab) S2V_CHECK_HIP(hipFree(op_tab));
            op_tab = nullptr; op_words = 0;
            S2V_CHECK_HIP(hipMalloc((void**)&op_tab, r.size() * 4));
            op_words = r.size();
        }
        S2V_CHECK_HIP(hipMemcpyAsync(op_tab, r.data(), r.size() * 4, hipMemcpyHostToDevice, st));
        S2V_CHECK_HIP(hipStreamSynchronize(st));
        op_rec = *record_host; op_B = B; op_Ntok = Ntok;
        op_planes.assign(planes_host, planes_host + n_w);
    }
    const int D = H * 64;
    AttnArgs a{};
    a.qkv = qkv; a.ld_qkv = 3 * D; a.out = out; a.ld_out = D; a.B = B; a.H = H; a.Ntok = Ntok; a.scale = 0.125f;
    a.ntok_pad = (int)rup(Ntok, 64);
    if (impl == 0 || impl == 2) {
        a.vt = vt_scratch;
        if (impl == 2) {   // the persistent twin on a queue of the process (nine counters, zero between launches: the last workgroup zeroes them)
            static int* op_queue = nullptr;
            static int op_cus = 0;
            if (!op_queue) {
                int dev = 0;
                hipDeviceProp_t prop;
                S2V_CHECK_HIP(hipGetDevice(&dev));
                S2V_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
                S2V_CHECK_HIP(hipMalloc((void**)&op_queue, 9 * sizeof(int)));
                S2V_CHECK_HIP(hipMemset(op_queue, 0, 9 * sizeof(int)));
                S2V_CHECK_HIP(hipDeviceSynchronize());
                op_cus = prop.multiProcessorCount;
            }
            S2V_REQUIRE(op_cus >= 8, "s2v_op_attention_steer_map: impl 2 needs a device of at least 8 compute units");
            a.queue = op_queue; a.num_cus = op_cus;
        }
        S2V_TRY(launch_v_transpose(qkv, 3 * D, B, H, Ntok, vt_scratch, a.ntok_pad, st, nullptr));
        return launch_attn_bf16_steer_map(a, (const AttnSteerMapRec*)op_tab, st, impl == 2);
    }
    a.valu_only = 1;
    return launch_attn_simple_steer_map(a, (const AttnSteerMapRec*)op_tab, dtype, st);
}

// ---- local attention in time (include/s2v_hip.h) --------------------------------------------------------------------------------------------
extern "C" int s2v_attn_local_enable(s2v_ctx* c, int32_t on) {
    S2V_REQUIRE(c, "s2v_attn_local_enable: null context");
    if (!on) {
        if (c->la_on) { S2V_CHECK_HIP(hipDeviceSynchronize()); drop_graph(c); }
        la_free(c);
        return 0;
    }
    S2V_TRY(la_check(c, "s2v_attn_local_enable"));
    if (c->la_on) return 0;
    S2V_CHECK_HIP(hipDeviceSynchronize());
    drop_graph(c);
    S2V_CHECK_HIP(hipMalloc((void**)&c->la_tab, attn_local_ints(c->Ntok) * sizeof(int)));
    c->la_on = true; c->la_Ntok = c->Ntok; c->la_arm = 0;
    const int r = la_upload_dense(c, "s2v_attn_local_enable");   // a table that windows nothing
    if (r != 0) la_free(c);
    return r;
}

extern "C" int s2v_attn_local_set(s2v_ctx* c, int32_t P, const int32_t* rows_lo, const int32_t* rows_hi) {
    S2V_REQUIRE(c, "s2v_attn_local_set: null context");
    S2V_REQUIRE(c->la_on && c->la_tab && c->la_Ntok == c->Ntok, "s2v_attn_local_set: local attention is not enabled (s2v_attn_local_enable)");
    S2V_REQUIRE(rows_lo && rows_hi, "s2v_attn_local_set: null row table");
    S2V_TRY(la_upload(c, "s2v_attn_local_set", P, rows_lo, rows_hi));   // checked before anything is replaced; a captured step is kept: the table is data
    if (c->la_kind != 0) { drop_graph(c); c->la_kind = 0; }   // ... unless the table it replaces was a box table: the captured steps launch the box kernel
    return 0;
}

// the box table of local attention in space and time: checked by attn_box_make before anything is replaced, then uploaded to a table of its own.  It
// replaces a window table (the captured steps launch the window kernel: dropped); a box table after a box table keeps them -- the table is data
extern "C" int s2v_attn_local_set_box(s2v_ctx* c, int32_t P, int32_t S, const int32_t* rows_lo, const int32_t* rows_hi, const int32_t* offs_lo,
                                      const int32_t* offs_hi) {
    S2V_REQUIRE(c, "s2v_attn_local_set_box: null context");
    S2V_TRY(la_check(c, "s2v_attn_local_set_box"));
    S2V_REQUIRE(c->la_on && c->la_tab && c->la_Ntok == c->Ntok, "s2v_attn_local_set_box: local attention is not enabled (s2v_attn_local_enable)");
    S2V_REQUIRE(rows_lo && rows_hi && offs_lo && offs_hi, "s2v_attn_local_set_box: null row table");
    std::vector<int> r;
    S2V_TRY(attn_box_make("s2v_attn_local_set_box", P, S, c->Ntok, rows_lo, rows_hi, offs_lo, offs_hi, &r));
    S2V_CHECK_HIP(hipDeviceSynchronize());   // a step on any stream may still read the table
    if (!c->la_box) S2V_CHECK_HIP(hipMalloc((void**)&c->la_box, attn_box_ints(c->Ntok) * sizeof(int)));
    S2V_CHECK_HIP(hipMemcpy(c->la_box, r.data(), r.size() * sizeof(int), hipMemcpyHostToDevice));
    if (c->la_kind != 1) { drop_graph(c); c->la_kind = 1; }
    return 0;
}

extern "C" int s2v_attn_local_arm(s2v_ctx* c, uint64_t layer_mask) {
    S2V_REQUIRE(c, "s2v_attn_local_arm: null context");
    if (layer_mask) {
        S2V_REQUIRE(c->la_on && c->la_tab, "s2v_attn_local_arm: local attention is not enabled (s2v_attn_local_enable)");
        S2V_TRY(la_check(c, "s2v_attn_local_arm"));
        S2V_REQUIRE(c->L >= 64 || (layer_mask >> c->L) == 0, "s2v_attn_local_arm: a layer bit at or beyond num_layers is set");
        S2V_REQUIRE(c->am_arm == 0, "s2v_attn_local_arm: an attention map is armed for the next forward (s2v_attn_map_arm): the map reads the un-windowed softmax");
        S2V_REQUIRE(c->st_arm == 0, "s2v_attn_local_arm: attention steering is armed for the next forward (s2v_attn_steer_arm): a layer runs one attention kernel");
        S2V_REQUIRE(c->sc_arm != S2V_STEP_REUSE, "s2v_attn_local_arm: S2V_STEP_REUSE is armed for the next forward (s2v_step_cache_arm): the block stack does not run, "
                                                 "there is no attention to window");
    }
    c->la_arm = layer_mask;
    return 0;
}

extern "C" int s2v_op_attention_local(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok, int32_t dtype, int32_t impl,
                                      int32_t P, const int32_t* rows_lo, const int32_t* rows_hi, s2v_stream stream) {
    S2V_REQUIRE(qkv && out, "s2v_op_attention_local: null argument");
    S2V_REQUIRE(B >= 1 && H >= 1 && Ntok >= 1, "s2v_op_attention_local: B >= 1, H >= 1, Ntok >= 1");
    S2V_REQUIRE(impl == 0 || impl == 1, "s2v_op_attention_local: impl 0 (MFMA, bf16) or 1 (generic)");
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_op_attention_local: unsupported dtype");
    S2V_REQUIRE(impl == 1 || (dtype == S2V_DTYPE_BF16 && vt_scratch), "s2v_op_attention_local: impl 0 is bf16 and needs vt_scratch");
    std::vector<int> r;
    S2V_TRY(attn_local_make("s2v_op_attention_local", P, Ntok, rows_lo, rows_hi, &r));
    // operator level: one table per process, on the device of the first call, grown when a longer sequence comes.  The entry synchronises the stream
    // before it replaces the table and uploads it with a blocking copy: a test and benchmark entry, not thread-safe; contexts hold their own table
    static int* op_tab = nullptr;
    static size_t op_ints = 0;
    hipStream_t st = (hipStream_t)stream;
    S2V_CHECK_HIP(hipStreamSynchronize(st));
    if (r.size() > op_ints) {
        if (op_tab) { S2V_CHECK_HIP(hipFree(op_tab)); op_tab = nullptr; op_ints = 0; }
        S2V_CHECK_HIP(hipMalloc((void**)&op_tab, r.size() * sizeof(int)));
        op_ints = r.size();
    }
    S2V_CHECK_HIP(hipMemcpy(op_tab, r.data(), r.size() * sizeof(int), hipMemcpyHostToDevice));
    const int D = H * 64;
    AttnArgs a{};
    a.qkv = qkv; a.ld_qkv = 3 * D; a.out = out; a.ld_out = D; a.B = B; a.H = H; a.Ntok = Ntok; a.scale = 0.125f;
    a.ntok_pad = (int)rup(Ntok, 64);
    if (impl == 0) {
        // the nine counters of the persistent form (zero between launches), so that this entry runs what a context runs at the same size
        static int* op_queue = nullptr;
        static int op_ncu = 0;
        if (!op_queue) {
            int dev = 0;
            S2V_CHECK_HIP(hipGetDevice(&dev));
            S2V_CHECK_HIP(hipDeviceGetAttribute(&op_ncu, hipDeviceAttributeMultiprocessorCount, dev));
            S2V_CHECK_HIP(hipMalloc((void**)&op_queue, 64));
            S2V_CHECK_HIP(hipMemset(op_queue, 0, 64));
        }
        a.vt = vt_scratch; a.queue = op_queue; a.num_cus = op_ncu;
        S2V_TRY(launch_v_transpose(qkv, 3 * D, B, H, Ntok, vt_scratch, a.ntok_pad, st, nullptr));
        return launch_attn_bf16_local(a, op_tab, st);
    }
    a.valu_only = 1;
    return launch_attn_simple_local(a, op_tab, dtype, st);
}

// the box kernel on its own: s2v_op_attention_local with the box table (a table and counters of its own)
extern "C" int s2v_op_attention_box(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok, int32_t dtype, int32_t impl,
                                      int32_t P, int32_t S, const int32_t* rows_lo, const int32_t* rows_hi, const int32_t* offs_lo, const int32_t* offs_hi,
                                    s2v_stream stream) {
    S2V_REQUIRE(qkv && out, "s2v_op_attention_box: null argument");
    S2V_REQUIRE(B >= 1 && H >= 1 && Ntok >= 1, "s2v_op_attention_box: B >= 1, H >= 1, Ntok >= 1");
    S2V_REQUIRE(impl == 0 || impl == 1, "s2v_op_attention_box: impl 0 (MFMA, bf16) or 1 (generic)");
    S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_op_attention_box: unsupported dtype");
    S2V_REQUIRE(impl == 1 || (dtype == S2V_DTYPE_BF16 && vt_scratch), "s2v_op_attention_box: impl 0 is bf16 and needs vt_scratch");
    // operator level: one table per process, on the device of the first call, grown when a longer sequence comes.  The entry synchronises the stream
    // before it replaces the table and uploads it with a blocking copy: a test and benchmark entry, not thread-safe; contexts hold their own table.
    // The record is built and uploaded once per table: a call with the table of the call before it (compared word for word) launches on the
    // record that is there, as a context's steps do between two s2v_attn_local_set_box
    static int* op_tab = nullptr;
    static size_t op_ints = 0;
    static std::vector<int> op_key;   // P, S, Ntok and the four row arrays of the record in op_tab
    hipStream_t st = (hipStream_t)stream;
    const bool arrays = rows_lo && rows_hi && offs_lo && offs_hi;
    bool same = arrays && op_tab && op_key.size() == 3 + 4 * (size_t)Ntok && op_key[0] == P && op_key[1] == S && op_key[2] == Ntok;
    for (int k = 0; same && k < 4; ++k)
        same = memcmp(op_key.data() + 3 + (size_t)k * Ntok, k == 0 ? rows_lo : k == 1 ? rows_hi : k == 2 ? offs_lo : offs_hi, (size_t)Ntok * sizeof(int)) == 0;
    if (!same) {
        std::vector<int> r;
        S2V_TRY(attn_box_make("s2v_op_attention_box", P, S, Ntok, rows_lo, rows_hi, offs_lo, offs_hi, &r));   // refused before the device is touched
        S2V_CHECK_HIP(hipStreamSynchronize(st));
        op_key.clear();   // nothing is remembered while the table is being replaced
        if (r.size() > op_ints) {
            if (op_tab) { S2V_CHECK_HIP(hipFree(op_tab)); op_tab = nullptr; op_ints = 0; }
            S2V_CHECK_HIP(hipMalloc((void**)&op_tab, r.size() * sizeof(int)));
            op_ints = r.size();
        }
        S2V_CHECK_HIP(hipMemcpy(op_tab, r.data(), r.size() * sizeof(int), hipMemcpyHostToDevice));
        op_key.reserve(3 + 4 * (size_t)Ntok);
        op_key.push_back(P); op_key.push_back(S); op_key.push_back(Ntok);
        for (const int32_t* p : {rows_lo, rows_hi, offs_lo, offs_hi}) op_key.insert(op_key.end(), p, p + Ntok);
    } else {
        S2V_CHECK_HIP(hipStreamSynchronize(st));
    }
    const int D = H * 64;
    AttnArgs a{};
    a.qkv = qkv; a.ld_qkv = 3 * D; a.out = out; a.ld_out = D; a.B = B; a.H = H; a.Ntok = Ntok; a.scale = 0.125f;
    a.ntok_pad = (int)rup(Ntok, 64);
    if (impl == 0) {
        // the nine counters of the persistent form (zero between launches), so that this entry runs what a context runs at the same size
        static int* op_queue = nullptr;
        static int op_ncu = 0;
        if (!op_queue) {
            int dev = 0;
            S2V_CHECK_HIP(hipGetDevice(&dev));
            S2V_CHECK_HIP(hipDeviceGetAttribute(&op_ncu, hipDeviceAttributeMultiprocessorCount, dev));
            S2V_CHECK_HIP(hipMalloc((void**)&op_queue, 64));
            S2V_CHECK_HIP(hipMemset(op_queue, 0, 64));
        }
        a.vt = vt_scratch; a.queue = op_queue; a.num_cus = op_ncu;
        S2V_TRY(launch_v_transpose(qkv, 3 * D, B, H, Ntok, vt_scratch, a.ntok_pad, st, nullptr));
        return launch_attn_bf16_box(a, op_tab, st);
    }
    a.valu_only = 1;
    return launch_attn_simple_box(a, op_tab, dtype, st);
}

extern "C" int s2v_attn_map_reset(s2v_ctx* c) {
    S2V_REQUIRE(c && c->am_on && c->am_acc, "s2v_attn_map_reset: the attention map is not enabled (s2v_attn_map_enable)");
    S2V_CHECK_HIP(hipDeviceSynchronize());   // launches of any stream may still add to the sums
    S2V_CHECK_HIP(hipMemset(c->am_acc, 0, c->am_bytes));
    c->am_count = 0;
    return 0;
}

extern "C" int s2v_attn_map_read(s2v_ctx* c, int32_t per_head, void* out_dev, int64_t* count, s2v_stream stream) {
    S2V_REQUIRE(c && count, "s2v_attn_map_read: null argument");
    S2V_REQUIRE(c->am_on && c->am_acc, "s2v_attn_map_read: the attention map is not enabled (s2v_attn_map_enable)");
    S2V_REQUIRE(out_dev, "s2v_attn_map_read: null argument");
    *count = c->am_count;
    hipStream_t st = (hipStream_t)stream;
    if (per_head) {
        S2V_CHECK_HIP(hipMemcpyAsync(out_dev, c->am_acc, (size_t)c->am_bytes, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    S2V_REQUIRE(c->am_count >= 1, "s2v_attn_map_read: the head mean needs at least one armed layer launch (the count is 0)");
    return launch_attn_mass_mean(c->am_acc, c->am_n, c->B, c->cfg.num_heads, c->V, c->am_count, (float*)out_dev, st);
}

extern "C" int s2v_op_attn_mass(const void* qkv, int32_t B, int32_t H, int32_t Ntok, int32_t q0, int32_t nq, const int32_t* ranges_host, int32_t n,
                                float* out, int32_t accumulate, int32_t dtype, int32_t impl, s2v_stream stream) {
    S2V_REQUIRE(qkv && ranges_host && out, "s2v_op_attn_mass: null argument");
    S2V_REQUIRE(n >= 1 && n <= AM_MAX_RANGES, "s2v_op_attn_mass: the number of key ranges must be 1..4");
    S2V_REQUIRE(B >= 1 && H >= 1 && Ntok >= 1, "s2v_op_attn_mass: bad shape");
    for (int r = 0; r < n; ++r)
        S2V_REQUIRE(ranges_host[2 * r] >= 0 && ranges_host[2 * r] <= ranges_host[2 * r + 1] && ranges_host[2 * r + 1] <= Ntok,
                    "s2v_op_attn_mass: a key range must lie inside [0, Ntok] with k0 <= k1");
    S2V_REQUIRE(q0 >= 0 && nq >= 1 && (int64_t)q0 + nq <= Ntok, "s2v_op_attn_mass: the query rows [q0, q0 + nq) must lie inside the sample (q0 + nq <= Ntok)");
    S2V_REQUIRE(impl == 0 || impl == 1, "s2v_op_attn_mass: impl is 0 (matrix pipe) or 1 (generic)");
    S2V_REQUIRE(impl != 0 || dtype != S2V_DTYPE_F32, "s2v_op_attn_mass: impl 0 (matrix pipe) runs bf16 / fp16 storage; fp32 runs impl 1");
    AttnMassArgs a{};
    a.qkv = qkv; a.ld_qkv = 3 * H * 64; a.B = B; a.H = H; a.Ntok = Ntok; a.q0 = q0; a.nq = nq; a.n = n;
    for (int r = 0; r < n; ++r) { a.k0[r] = ranges_host[2 * r]; a.k1[r] = ranges_host[2 * r + 1]; }
    a.out = out; a.accumulate = accumulate ? 1 : 0;
    return launch_attn_mass(a, dtype, impl, (hipStream_t)stream);
}

extern "C" int s2v_op_attn_mass_mean(const float* acc, int32_t n, int32_t B, int32_t H, int32_t nq, int64_t count, float* out, s2v_stream stream) {
    return launch_attn_mass_mean(acc, n, B, H, nq, count, out, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------
// ---- step cache (include/s2v_hip.h) -------------------------------------------------------------------------------------------------
extern "C" int s2v_step_cache_enable(s2v_ctx* c, int32_t on) {
    S2V_REQUIRE(c, "s2v_step_cache_enable: null context");
    S2V_REQUIRE(on >= 0 && on <= 2, "s2v_step_cache_enable: 0 (off), 1 (the cache) or 2 (the cache and the IN buffer of the read-out)");
    S2V_REQUIRE(!on || c->kind == S2V_CTX_MODEL, "s2v_step_cache_enable: attention-only contexts (S2V_CTX_ATTN_*) run no forward");
    S2V_REQUIRE(!on || !c->shard, "s2v_step_cache_enable: a shard context (s2v_set_shard) has no step cache: it runs on one GPU");
    S2V_REQUIRE(!on || c->ws, "s2v_step_cache_enable: call s2v_set_geometry first (the cache is [B][V][D] of the current geometry)");
    if (on == c->sc_on) { sc_invalidate(c); return 0; }
    S2V_CHECK_HIP(hipDeviceSynchronize());
    drop_graph(c);   // a captured step bakes in the buffers and (enable 2) the IN copy
    return sc_alloc(c, on);
}

extern "C" int s2v_step_cache_arm(s2v_ctx* c, int32_t mode) {
    S2V_REQUIRE(c, "s2v_step_cache_arm: null context");
    S2V_REQUIRE(mode == S2V_STEP_FULL || mode == S2V_STEP_CAPTURE || mode == S2V_STEP_REUSE, "s2v_step_cache_arm: S2V_STEP_FULL, S2V_STEP_CAPTURE or S2V_STEP_REUSE");
    if (mode != S2V_STEP_FULL) {
        S2V_REQUIRE(!c->shard, "s2v_step_cache_arm: a shard context (s2v_set_shard) runs the staged step, which has no cached form: the step cache runs on one GPU");
        S2V_REQUIRE(c->sc_on && c->sc_delta, "s2v_step_cache_arm: the step cache is not enabled (s2v_step_cache_enable)");
        S2V_REQUIRE(mode != S2V_STEP_REUSE || c->sc_valid, "s2v_step_cache_arm: no captured residual for this geometry / conditioning / weights");
        S2V_REQUIRE(mode != S2V_STEP_REUSE || !c->st_arm, "s2v_step_cache_arm: S2V_STEP_REUSE while attention steering is armed for the next forward (s2v_attn_steer_arm): "
                                                          "the block stack does not run, there is no attention to steer");
        S2V_REQUIRE(mode != S2V_STEP_REUSE || !c->la_arm, "s2v_step_cache_arm: S2V_STEP_REUSE while local attention is armed for the next forward (s2v_attn_local_arm): "
                                                          "the block stack does not run, there is no attention to window");
        S2V_REQUIRE(mode != S2V_STEP_REUSE || !c->am_arm, "s2v_step_cache_arm: S2V_STEP_REUSE while an attention map is armed for the next forward (s2v_attn_map_arm): "
                                                          "the block stack does not run, there is no attention to follow");
    }
    c->sc_arm = mode;
    return 0;
}

extern "C" int s2v_step_cache_state(s2v_ctx* c, int32_t* enabled, int32_t* valid, int64_t* bytes) {
    S2V_REQUIRE(c && enabled && valid && bytes, "s2v_step_cache_state: null argument");
    *enabled = c->sc_on; *valid = c->sc_valid ? 1 : 0; *bytes = c->sc_bytes;
    return 0;
}

extern "C" int s2v_step_cache_read(s2v_ctx* c, int32_t which, void* out_dev, s2v_stream stream) {
    S2V_REQUIRE(c && out_dev, "s2v_step_cache_read: null argument");
    S2V_REQUIRE(which >= 0 && which <= 2, "s2v_step_cache_read: which is 0 (IN), 1 (OUT) or 2 (the residual)");
    S2V_REQUIRE(c->ws && !c->shard, "s2v_step_cache_read: a geometry on an unsharded context is required");
    S2V_REQUIRE(which != 0 || c->sc_in, "s2v_step_cache_read: IN is kept only under s2v_step_cache_enable(ctx, 2)");
    S2V_REQUIRE(which != 2 || (c->sc_delta && c->sc_valid), "s2v_step_cache_read: no captured residual for this geometry / conditioning / weights");
    hipStream_t st = (hipStream_t)stream;
    if (which == 1) return sc_launch(c, SC_KEEP, (char*)out_dev, nullptr, st);
    S2V_CHECK_HIP(hipMemcpyAsync(out_dev, which == 0 ? c->sc_in : c->sc_delta, (size_t)c->B * c->V * c->D * c->esz, hipMemcpyDeviceToDevice, st));
    return 0;
}

extern "C" int s2v_op_step_cache(int32_t op, void* x, int64_t x_bstride, void* cache, int32_t B, int64_t n, int32_t dtype, s2v_stream stream) {
    S2V_REQUIRE(x && cache && B >= 1 && n >= 1 && x_bstride >= n, "s2v_op_step_cache: null argument, or samples that overlap (x_bstride < n)");
    S2V_REQUIRE(dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_F16, "s2v_op_step_cache: dtype must be f32, bf16 or f16");
    return launch_step_cache(op, x, x_bstride, cache, nullptr, B, n, dtype, (hipStream_t)stream);
}

extern "C" int s2v_time_embedding(s2v_ctx* c, const float* timesteps_host, int32_t n, void* out_dev, s2v_stream stream) {
    S2V_REQUIRE(c && timesteps_host && out_dev && n >= 1, "s2v_time_embedding: null argument");
    S2V_REQUIRE(c->kind == S2V_CTX_MODEL && c->finalized, "s2v_time_embedding: a model context with finalized weights is required");
    hipStream_t st = (hipStream_t)stream;
    // scratch of its own (no geometry needed): the timesteps, then launch_time_embed's [chunk][D] sinusoid and [chunk][temb] hidden
    const int64_t E = c->esz, tmp_bytes = (int64_t)S2V_MAX_BATCH * (c->D + c->temb) * E;
    char* buf = nullptr;
    S2V_CHECK_HIP(hipMalloc((void**)&buf, 256 + tmp_bytes));
    int r = 0;
    for (int i0 = 0; i0 < n && !r; i0 += S2V_MAX_BATCH) {
        const int nb = std::min<int>(S2V_MAX_BATCH, n - i0);
        hipError_t e = hipStreamSynchronize(st);   // the previous chunk has read the scratch
        if (e == hipSuccess) e = hipMemcpy(buf, timesteps_host + i0, sizeof(float) * nb, hipMemcpyHostToDevice);
        if (e != hipSuccess) { r = s2v_fail(__FILE__, __LINE__, hipGetErrorString(e), -2); break; }
        r = launch_time_embed((const float*)buf, nb, c->D, c->te1_w, c->te1_b, c->te2_w, c->te2_b, c->temb, buf + 256, (char*)out_dev + (int64_t)i0 * c->temb * E,
                              c->dtype, st);
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(buf);
    return r;
}

extern "C" int s2v_op_linear(const void* A, const void* W, const void* bias, void* C, int32_t M, int32_t N, int32_t K,
                             int32_t epilogue, int32_t dtype, int32_t impl, s2v_stream stream) {
    S2V_REQUIRE(A && W && C, "s2v_op_linear: null argument");
    S2V_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_BIAS_GELU, "s2v_op_linear: epilogue must be 0 or 1");
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.bias = bias; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K;
    if (impl == 0) {
        S2V_REQUIRE(dtype == S2V_DTYPE_BF16, "s2v_op_linear: the MFMA kernel is bf16 only");
        S2V_REQUIRE(M % 128 == 0 && N % 128 == 0, "s2v_op_linear: impl 0 needs M and N padded to 128 by the caller");
        g.a_rows_padded = M;  // the 256-row ring kernel is used when M is a multiple of 256
        return launch_gemm_bf16(g, epilogue, (hipStream_t)stream);
    }
    if (impl == 2) {  // the engine's split-K form of a few-tile GEMM (linear()), with a workspace of its own: synchronous
        S2V_REQUIRE(dtype == S2V_DTYPE_BF16 && M % 256 == 0 && N % 256 == 0, "s2v_op_linear: impl 2 is bf16 with M and N multiples of 256");
        const int64_t tiles = (int64_t)(M / 256) * (N / 256);
        const int S = gemm_choose_splitk(tiles, K, device_cus());
        S2V_REQUIRE(S > 1, "s2v_op_linear: impl 2: this shape does not split (tiles * 2 <= CUs, K / S a multiple of 128 and >= 1024)");
        char* ws = nullptr;
        const size_t pb = (size_t)S * tiles * 262144;
        S2V_CHECK_HIP(hipMalloc((void**)&ws, pb + tiles * 4));
        g.a_rows_padded = M; g.w_rows_padded = N;
        g.splitk = S; g.sk_ws = (float*)ws; g.sk_cnt = (unsigned*)(ws + pb);
        int rc = hipMemsetAsync(ws + pb, 0, tiles * 4, (hipStream_t)stream) == hipSuccess ? 0 : -2;
        if (rc == 0) rc = launch_gemm_bf16(g, epilogue, (hipStream_t)stream);
        if (rc == 0) rc = launch_gemm_bf16(g, epilogue, (hipStream_t)stream);  // twice: the counters must be back at zero
        hipStreamSynchronize((hipStream_t)stream);
        hipFree(ws);
        return rc;
    }
    if (impl == 4) {  // fp16 operands on v_mfma_f32_32x32x16_f16 (what the fp16 engine runs); M, N padded to 128 by the caller
        S2V_REQUIRE(dtype == S2V_DTYPE_F16, "s2v_op_linear: impl 4 is fp16 only");
        S2V_REQUIRE(M % 128 == 0 && N % 128 == 0, "s2v_op_linear: impl 4 needs M and N padded to 128 by the caller");
        g.a_rows_padded = M; g.w_rows_padded = N;
        return launch_gemm_f16(g, epilogue, (hipStream_t)stream);
    }
    if (impl == 3 || (impl >= 30 && impl <= 33)) {  // fp32 operands on the fp32 matrix pipe (what the fp32 engine runs; bit-identical to impl 1)
        S2V_REQUIRE(dtype == S2V_DTYPE_F32, "s2v_op_linear: impl 3 / 30 .. 33 are fp32 only");
        if (impl >= 30) g.tile = impl;  // 30 .. 33: force the 128 x 128 / 128 x 64 / 64 x 128 / 64 x 64 tile (3: the launcher's own choice)
        return launch_gemm_f32m(g, epilogue, (hipStream_t)stream);
    }
    g.valu_only = 1;
    return launch_gemm_simple(g, epilogue, dtype, (hipStream_t)stream);
}

// The plan-and-launch of linear() for the operator entries: gemm_plan at this device's CU count (split K where the caller brought a workspace
// of sk_tiles partial tiles, GemmArgs::tile, the row tail), main and tail launch on the same stream
static int launch_planned(const GemmArgs& g0, int epi, int64_t sk_tiles, float* sk_ws, unsigned* sk_cnt, hipStream_t st) {
    GemmArgs g = g0;
    const GemmPlan p = gemm_plan(g, epi, device_cus(), sk_tiles);
    g.tile = p.tile;
    if (p.splitk > 1) { g.splitk = p.splitk; g.sk_ws = sk_ws; g.sk_cnt = sk_cnt; }
    if (p.tail != GEMM_NONE) {
        GemmArgs gm = g, gt = g;
        gm.M = p.m_main; gt.m_begin = p.m_main;
        S2V_TRY(launch_gemm_bf16(gm, epi, st));
        return launch_gemm_bf16(gt, epi, st);
    }
    return launch_gemm_bf16(g, epi, st);
}

// One linear as a context's linear() runs it, on the caller's operands (include/s2v_hip.h).  With a split-K workspace the launch runs twice
// where the epilogue allows it (as s2v_op_linear impl 2: the second launch starts from the counters the first one left), and the counters are
// read back: anything but zero is an error
extern "C" int s2v_op_linear_planned(const void* A, int32_t lda, const void* W, int32_t ldw, const void* bias, void* C, int32_t ldc, int32_t M, int32_t N,
                                     int32_t K, int32_t epilogue, int32_t dtype, const void* gate_txt, const void* gate_ref, const void* gate_vid,
                                     int32_t gate_stride, int32_t tok_per_batch, int32_t text_len, int32_t ref_len, const void* R, int32_t ldr,
                                     int32_t tile, int64_t sk_tiles, s2v_stream stream) {
    S2V_REQUIRE(A && W && C && M > 0 && N > 0 && K > 0, "s2v_op_linear_planned: bad argument");
    S2V_REQUIRE(dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_op_linear_planned: bf16 or fp16 (the dtypes whose linears run on the matrix cores)");
    S2V_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_BIAS_GELU || epilogue == EPI_BIAS_GATE_RES || epilogue == EPI_BIAS_ADD,
                "s2v_op_linear_planned: epilogue must be 0 (bias), 1 (GELU), 2 (gate + residual) or 3 (residual add)");
    S2V_REQUIRE(K % 64 == 0 && lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K && ldc >= N,
                "s2v_op_linear_planned: K a multiple of 64, lda and ldw multiples of 8 and >= K, ldc >= N (what linear() sends to the matrix cores)");
    S2V_REQUIRE(tile >= 0 && tile <= 2, "s2v_op_linear_planned: tile must be 0 (the plan's), 1 (256 x 128) or 2 (128 x 128)");
    S2V_REQUIRE(epilogue != EPI_BIAS_GATE_RES || (gate_txt && gate_vid && tok_per_batch > 0 && text_len >= 0 && ref_len >= 0),
                "s2v_op_linear_planned: epilogue 2 needs the text and video gates and tok_per_batch > 0 (C is the residual, updated in place)");
    S2V_REQUIRE(epilogue != EPI_BIAS_ADD || (R && ldr >= N), "s2v_op_linear_planned: epilogue 3 needs R with ldr >= N");
    S2V_REQUIRE(sk_tiles >= 0 && sk_tiles <= 1024 && (sk_tiles == 0 || dtype == S2V_DTYPE_BF16),
                "s2v_op_linear_planned: a split-K workspace holds at most 1024 partial tiles and is bf16 only");
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.a_rows_padded = (int)rup(M, 256); g.w_rows_padded = (int)rup(N, 256); g.f16 = dtype == S2V_DTYPE_F16 ? 1 : 0;
    g.tile = tile;
    g.tok_per_batch = tok_per_batch > 0 ? tok_per_batch : M; g.text_len = text_len; g.ref_len = ref_len;
    if (epilogue == EPI_BIAS_GATE_RES) { g.X = C; g.ldx = ldc; g.gate_txt = gate_txt; g.gate_ref = gate_ref; g.gate_vid = gate_vid; g.gate_stride = gate_stride; }
    if (epilogue == EPI_BIAS_ADD) { g.R = R; g.ldr = ldr; }
    if (sk_tiles == 0) return launch_planned(g, epilogue, 0, nullptr, nullptr, st);
    char* ws = nullptr;
    const size_t pb = (size_t)sk_tiles * 262144, cb = (size_t)sk_tiles * 4;
    S2V_CHECK_HIP(hipMalloc((void**)&ws, pb + cb));
    std::vector<unsigned> cnt((size_t)sk_tiles, 0u);
    auto run = [&]() -> int {
        S2V_CHECK_HIP(hipMemsetAsync(ws + pb, 0, cb, st));
        S2V_TRY(launch_planned(g, epilogue, sk_tiles, (float*)ws, (unsigned*)(ws + pb), st));
        if (epilogue != EPI_BIAS_GATE_RES) S2V_TRY(launch_planned(g, epilogue, sk_tiles, (float*)ws, (unsigned*)(ws + pb), st));  // (in place: once)
        S2V_CHECK_HIP(hipMemcpyAsync(cnt.data(), ws + pb, cb, hipMemcpyDeviceToHost, st));
        return 0;
    };
    const int rc = run();
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    if (rc != 0) return rc;
    for (unsigned v : cnt) S2V_REQUIRE(v == 0, "s2v_op_linear_planned: a split-K arrival counter did not return to zero");
    return 0;
}

// One adapted linear as the runtime adapter mode runs it (s2v_lora_attach), on operands of its own: x and W are copied into scratch rows with room
// for the K extension, A goes into a stack and rnd(scale * B) into W's tail (the attach-time kernels), the down-projection writes T behind x, and
// the GEMM the engine's linear() would launch for this shape runs with K' = K + R.  Allocates its scratch; synchronous.
extern "C" int s2v_op_linear_lora(const void* x, const void* W, const void* bias, const float* A, const float* B, int32_t rank, float scale, void* C,
                                  int32_t M, int32_t N, int32_t K, int32_t epilogue, const void* aux0, const void* aux1, int32_t dtype, s2v_stream stream) {
    S2V_REQUIRE(x && W && A && B && C && rank > 0 && M > 0 && N > 0, "s2v_op_linear_lora: bad argument");
    S2V_REQUIRE(dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F16, "s2v_op_linear_lora: bf16 or fp16 (the dtypes whose linears run on the matrix cores)");
    S2V_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_BIAS_GELU || epilogue == EPI_BIAS_GATE_RES || epilogue == EPI_BIAS_QKNORM,
                "s2v_op_linear_lora: epilogue must be 0 (bias), 1 (GELU), 2 (gate + residual) or 4 (q/k-norm)");
    S2V_REQUIRE(K % 64 == 0 && N % 8 == 0 && rank <= 128, "s2v_op_linear_lora: K a multiple of 64, N of 8, rank <= 128");
    S2V_REQUIRE(epilogue != EPI_BIAS_GATE_RES || aux0, "s2v_op_linear_lora: epilogue 2 needs the gate vector [N] in aux0 (C is the residual, updated in place)");
    S2V_REQUIRE(epilogue != EPI_BIAS_QKNORM || (aux0 && aux1 && N % 192 == 0), "s2v_op_linear_lora: epilogue 4 needs N = 3 * qk_D, LayerNorm weights [2][64] in aux0 and biases [2][64] in aux1");
    hipStream_t st = (hipStream_t)stream;
    const int64_t E = 2, R = rup(rank, K % 128 == 0 ? 128 : 64), Kx = K + R, Mp = rup(M, 256) + 256, Np = rup(N, 256);
    const int64_t bx = rup(Mp * Kx * E, 256), bw = rup(Np * Kx * E, 256), ba = rup(R * K * E, 256);
    char* ws = nullptr;
    S2V_CHECK_HIP(hipMalloc((void**)&ws, (size_t)(bx + bw + ba)));
    char *xe = ws, *we = ws + bx, *as = we + bw;
    auto run = [&]() -> int {
        S2V_CHECK_HIP(hipMemsetAsync(ws, 0, (size_t)(bx + bw + ba), st));
        S2V_TRY(launch_convert2d(x, dtype, K, xe, dtype, Kx, M, K, st));
        S2V_TRY(launch_convert2d(W, dtype, K, we, dtype, Kx, N, K, st));
        S2V_TRY(launch_lora_pack_a(A, rank, (int)R, K, as, K, dtype, st));
        S2V_TRY(launch_lora_pack_b(B, rank, (int)R, N, scale, we + (int64_t)K * E, Kx, dtype, st));
        LoraDownArgs d{};
        d.x = xe; d.ldx = (int)Kx; d.A = as; d.lda = K; d.out = xe + (int64_t)K * E; d.ldo = (int)Kx; d.M = M; d.N = (int)R; d.K = K;
        S2V_TRY(launch_lora_down(d, dtype, true, st));
        GemmArgs g{};
        g.A = xe; g.lda = (int)Kx; g.W = we; g.ldw = (int)Kx; g.bias = bias; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = (int)Kx;
        g.a_rows_padded = (int)rup(M, 256); g.w_rows_padded = (int)Np; g.f16 = dtype == S2V_DTYPE_F16 ? 1 : 0;
        g.tok_per_batch = M; g.text_len = 0;
        if (epilogue == EPI_BIAS_GATE_RES) { g.X = C; g.ldx = N; g.gate_vid = aux0; g.gate_txt = aux0; g.gate_stride = 0; }
        if (epilogue == EPI_BIAS_QKNORM) {
            g.qk_w[0] = aux0; g.qk_w[1] = (const char*)aux0 + 64 * E; g.qk_b[0] = aux1; g.qk_b[1] = (const char*)aux1 + 64 * E;
            g.qk_cs = nullptr; g.qk_D = N / 3; g.qk_eps = 1e-6f;
        }
        return launch_planned(g, epilogue, 0, nullptr, nullptr, st);
    };
    const int rc = run();
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    return rc;
}

// An fp8 linear on scratch, with or without an adapter, as the s2v_op_*fp8* entry points run it: x [M][K] and W [N][K] (bf16, rows K apart) are
// quantised per row to e4m3 into xq / wq with their scales in xs / ws, and the product runs on the fp8 matrix cores.  mx_s set: x is not
// quantised -- xq already holds the operand as an MX image with these block scales.  mx_out_q set: the epilogue leaves its output as an MX image
// as well.  A set: the adapter branch beside it, as the fp8 engines run it with S2V_LORA_FP8_BRANCH -- A into a stack, rnd(scale * B) into a Bs
// array (the attach-time kernels), T = rnd(x^ . A^T) from the best-precision operand (the bf16 rows of x, or the MX image dequantised exactly:
// the down-projection kernels), and T . Bs^T added to the dequantised accumulator before bias / GELU (GemmArgs::lora_bs)
struct Fp8Op {
    const void *x, *W, *bias; void* C; int M, N, K;
    char *xq, *wq; float *xs, *ws;
    const unsigned char* mx_s; unsigned char *mx_out_q, *mx_out_s;
    const float *A, *B; int rank; float scale;
    char *a_st, *bs, *t;   // A stack [R][K], Bs [N][R], T [M][R], bf16, R = rank rounded up to 64
};
static Fp8Op fp8_op(const void* x, const void* W, const void* bias, void* C, int M, int N, int K, char* xq, char* wq, float* xs, float* ws) {
    Fp8Op o{};
    o.x = x; o.W = W; o.bias = bias; o.C = C; o.M = M; o.N = N; o.K = K; o.xq = xq; o.wq = wq; o.xs = xs; o.ws = ws;
    return o;
}
// ... on the scratch of s2v_op_linear_fp8, which s2v_op_linear_fp8_lora's starts with: xq [M][K], wq [N][K], xs [M], ws [N]
static Fp8Op fp8_op(const void* x, const void* W, const void* bias, void* C, int M, int N, int K, void* scratch) {
    char *xq = (char*)scratch, *wq = xq + (int64_t)M * K;
    float* xs = (float*)(wq + (int64_t)N * K);
    return fp8_op(x, W, bias, C, M, N, K, xq, wq, xs, xs + M);
}
static void fp8_op_adapter(Fp8Op& o, const float* A, const float* B, int rank, float scale, char* a_st, char* bs, char* t) {
    o.A = A; o.B = B; o.rank = rank; o.scale = scale; o.a_st = a_st; o.bs = bs; o.t = t;
}
static int launch_fp8_op(const Fp8Op& o, int epi, hipStream_t st) {
    const int M = o.M, N = o.N, K = o.K, R = (int)rup(o.rank, 64);
    if (!o.mx_s) S2V_TRY(launch_quant_rows_fp8(o.x, K, M, K, o.xq, o.xs, st));
    S2V_TRY(launch_quant_rows_fp8(o.W, K, N, K, o.wq, o.ws, st));
    GemmArgs g{};
    g.A = o.xq; g.lda = K; g.W = o.wq; g.ldw = K; g.bias = o.bias; g.C = o.C; g.ldc = N; g.M = M; g.N = N; g.K = K;
    g.a_rows_padded = M; g.w_rows_padded = N; g.a_scale = o.mx_s ? nullptr : o.xs; g.w_scale = o.ws;
    if (o.mx_s) { g.mx_a_s = o.mx_s; g.mx_rows = M; }
    if (o.mx_out_q) { g.mx_out_q = o.mx_out_q; g.mx_out_s = o.mx_out_s; g.mx_rows = M; }
    if (o.A) {
        S2V_TRY(launch_lora_pack_a(o.A, o.rank, R, K, o.a_st, K, S2V_BF16, st));
        S2V_TRY(launch_lora_pack_b(o.B, o.rank, R, N, o.scale, o.bs, R, S2V_BF16, st));
        LoraDownArgs d{};
        d.x = o.x; d.ldx = K; d.A = o.a_st; d.lda = K; d.out = o.t; d.ldo = R; d.M = M; d.N = R; d.K = K;
        if (o.mx_s) {
            d.x = o.xq; d.mx_s = o.mx_s; d.mx_rows = M;
            S2V_TRY(launch_lora_down_mx(d, st));
        } else {
            S2V_TRY(launch_lora_down(d, S2V_BF16, true, st));
        }
        g.lora_t = o.t; g.lora_ldt = R; g.lora_bs = o.bs; g.lora_r = R; g.lora_seg = 0;
    }
    return launch_gemm_fp8(g, epi, st);
}

// C = epilogue(dequant(quant_rows(A) . quant_rows(W)^T) + bias): both bf16 operands are quantised per row to e4m3 (dynamic
// per-token / per-output-channel scales) into `scratch` and multiplied on the fp8 matrix cores.  M, N multiples of 256, K of 128.
extern "C" int s2v_op_linear_fp8(const void* A, const void* W, const void* bias, void* C, int32_t M, int32_t N, int32_t K,
                                 int32_t epilogue, void* scratch, int64_t scratch_bytes, s2v_stream stream) {
    S2V_REQUIRE(A && W && C && scratch, "s2v_op_linear_fp8: null argument");
    S2V_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_BIAS_GELU, "s2v_op_linear_fp8: epilogue must be 0 or 1");
    S2V_REQUIRE(M % 256 == 0 && N % 256 == 0 && K % 128 == 0, "s2v_op_linear_fp8: M, N multiples of 256 and K of 128");
    const int64_t need = (int64_t)M * K + (int64_t)N * K + 4 * ((int64_t)M + N);
    S2V_REQUIRE(scratch_bytes >= need, "s2v_op_linear_fp8: scratch too small (M*K + N*K + 4*(M+N) bytes)");
    return launch_fp8_op(fp8_op(A, W, bias, C, M, N, K, scratch), epilogue, (hipStream_t)stream);
}

// FeedForward (attention.py:1237-1243) on the fp8 matrix cores as the fp8 engine runs it: x, W1, W2 quantised per row (e4m3, amax / 448);
// h = GELU(x W1^T + b1) either (mx = 1) left by the FF1 epilogue as MX e4m3 -- one power-of-two scale per 32 columns -- and read in
// place by the FF2, or (mx = 0) written in bf16 and quantised per row by a separate pass; out = h W2^T + b2, bf16.  Allocates its
// scratch and synchronises: a test / micro-benchmark entry point.
extern "C" int s2v_op_ff_fp8(const void* x, const void* w1, const void* b1, const void* w2, const void* b2, void* out, int32_t M, int32_t D,
                             int32_t F, int32_t mx, s2v_stream stream) {
    S2V_REQUIRE(x && w1 && w2 && out, "s2v_op_ff_fp8: null argument");
    S2V_REQUIRE(M % 256 == 0 && D % 256 == 0 && F % 256 == 0, "s2v_op_ff_fp8: M, D, F must be multiples of 256");
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)M * D + (size_t)F * D + (size_t)D * F + 4 * ((size_t)2 * M + F + D) + (size_t)M * F * 3 + (size_t)M * F / 32 + 4096;
    char* p = nullptr;
    S2V_CHECK_HIP(hipMalloc((void**)&p, bytes));
    char* xq = p; char* w1q = xq + (size_t)M * D; char* w2q = w1q + (size_t)F * D;
    float* xs = (float*)(w2q + (size_t)D * F); float* hs_row = xs + M; float* w1s = hs_row + M; float* w2s = w1s + F;
    char* hb = (char*)(w2s + D);                 // bf16 h (mx = 0)
    char* hq = hb + (size_t)M * F * 2;           // e4m3 h
    unsigned char* hsc = (unsigned char*)hq + (size_t)M * F;  // MX block scales
    Fp8Op f1 = fp8_op(x, w1, b1, hb, M, F, D, xq, w1q, xs, w1s), f2 = fp8_op(hb, w2, b2, out, M, D, F, hq, w2q, hs_row, w2s);
    if (mx) { f1.mx_out_q = (unsigned char*)hq; f1.mx_out_s = hsc; f2.mx_s = hsc; }
    int rc = launch_fp8_op(f1, EPI_BIAS_GELU, st);
    if (!rc) rc = launch_fp8_op(f2, EPI_BIAS, st);
    hipStreamSynchronize(st);
    hipFree(p);
    return rc;
}

// One adapted linear as the fp8 engines run it with S2V_LORA_FP8_BRANCH: s2v_op_linear_fp8's quantisation and GEMM with the adapter branch beside
// it (Fp8Op), T from the bf16 rows of x.  Everything lives in `scratch`; asynchronous.
extern "C" int s2v_op_linear_fp8_lora(const void* x, const void* W, const void* bias, const float* A, const float* B, int32_t rank, float scale, void* C,
                                      int32_t M, int32_t N, int32_t K, int32_t epilogue, void* scratch, int64_t scratch_bytes, s2v_stream stream) {
    S2V_REQUIRE(x && W && A && B && C && scratch, "s2v_op_linear_fp8_lora: null argument");
    S2V_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_BIAS_GELU, "s2v_op_linear_fp8_lora: epilogue must be 0 or 1");
    S2V_REQUIRE(M > 0 && N > 0 && K > 0 && M % 256 == 0 && N % 256 == 0 && K % 128 == 0, "s2v_op_linear_fp8_lora: M, N multiples of 256 and K of 128");
    S2V_REQUIRE(rank > 0 && rank <= 128, "s2v_op_linear_fp8_lora: rank must be 1 .. 128");
    const int64_t R = rup(rank, 64);
    const int64_t o_q = rup((int64_t)M * K + (int64_t)N * K + 4 * ((int64_t)M + N), 256);
    const int64_t need = o_q + 2 * R * ((int64_t)K + N + M);
    S2V_REQUIRE(scratch_bytes >= need, "s2v_op_linear_fp8_lora: scratch too small (M*K + N*K + 4*(M+N) rounded up to 256, + 2*R*(K+N+M) bytes, R = rank rounded up to 64)");
    char* a_st = (char*)scratch + o_q;          // A stack [R][K]
    char* bs = a_st + 2 * R * K;                // Bs [N][R]
    char* t = bs + 2 * R * N;                   // T [M][R]
    Fp8Op o = fp8_op(x, W, bias, C, M, N, K, scratch);
    fp8_op_adapter(o, A, B, rank, scale, a_st, bs, t);
    return launch_fp8_op(o, epilogue, (hipStream_t)stream);
}

// s2v_op_ff_fp8 with an adapter on both linears, as the fp8 engines run a block's FeedForward with S2V_LORA_FP8_BRANCH: FF1's branch reads the
// bf16 rows of x; FF2's reads (mx = 1) the MX image the FF1 epilogue left, dequantised exactly, or (mx = 0) the bf16 h.  `scratch` starts with
// what a test wants to look at: the image bytes [M][F], its block scales (GemmArgs::mx_a_s: [F / 128][M] dwords, rows permuted by mx_perm_row,
// byte b = block 4 kt + b) and, from the next multiple of 256 bytes on, FF2's T [M][R] bf16 (R = rank rounded up to 64).  Asynchronous.
extern "C" int s2v_op_ff_fp8_lora(const void* x, const void* w1, const void* b1, const void* w2, const void* b2, const float* A1, const float* B1,
                                  const float* A2, const float* B2, int32_t rank, float scale, void* out, int32_t M, int32_t D, int32_t F, int32_t mx,
                                  void* scratch, int64_t scratch_bytes, s2v_stream stream) {
    S2V_REQUIRE(x && w1 && w2 && out && A1 && B1 && A2 && B2 && scratch, "s2v_op_ff_fp8_lora: null argument");
    S2V_REQUIRE(M > 0 && D > 0 && F > 0 && M % 256 == 0 && D % 256 == 0 && F % 256 == 0, "s2v_op_ff_fp8_lora: M, D, F must be multiples of 256");
    S2V_REQUIRE(rank > 0 && rank <= 128, "s2v_op_ff_fp8_lora: rank must be 1 .. 128");
    hipStream_t st = (hipStream_t)stream;
    const int64_t R = rup(rank, 64), m = M, dd = D, f = F;
    int64_t off = 0;
    auto carve = [&](int64_t bytes) { int64_t o = off; off += rup(bytes, 256); return o; };
    off = m * f + m * f / 32;                          // image bytes + block scales, back to back
    off = rup(off, 256);
    const int64_t o_t2 = carve(m * R * 2), o_t1 = carve(m * R * 2);
    const int64_t o_xq = carve(m * dd), o_w1q = carve(f * dd), o_w2q = carve(dd * f);
    const int64_t o_xs = carve(m * 4), o_hrow = carve(m * 4), o_w1s = carve(f * 4), o_w2s = carve(dd * 4);
    const int64_t o_hb = carve(m * f * 2);
    const int64_t o_a1 = carve(R * dd * 2), o_bs1 = carve(f * R * 2), o_a2 = carve(R * f * 2), o_bs2 = carve(dd * R * 2);
    S2V_REQUIRE(scratch_bytes >= off, "s2v_op_ff_fp8_lora: scratch too small (4*M*F + M*D + 2*D*F + 2*R*(2*M + 2*D + 2*F) + 8*M + 4*(D + F) + 8192 bytes suffice)");
    char* p = (char*)scratch;
    unsigned char* hq = (unsigned char*)p;
    unsigned char* hsc = hq + m * f;
    char* hb = p + o_hb;
    Fp8Op f1 = fp8_op(x, w1, b1, hb, M, F, D, p + o_xq, p + o_w1q, (float*)(p + o_xs), (float*)(p + o_w1s));
    Fp8Op f2 = fp8_op(hb, w2, b2, out, M, D, F, (char*)hq, p + o_w2q, (float*)(p + o_hrow), (float*)(p + o_w2s));
    fp8_op_adapter(f1, A1, B1, rank, scale, p + o_a1, p + o_bs1, p + o_t1);
    fp8_op_adapter(f2, A2, B2, rank, scale, p + o_a2, p + o_bs2, p + o_t2);
    if (mx) { f1.mx_out_q = hq; f1.mx_out_s = hsc; f2.mx_s = hsc; }
    S2V_TRY(launch_fp8_op(f1, EPI_BIAS_GELU, st));
    return launch_fp8_op(f2, EPI_BIAS, st);
}

// Census of the attention kernel's deferred-maximum slow path since the last reset: slow = slow paths taken, total = (wave, KV tile) pairs run by
// the four-wave kernels (0 / 0 when only attn_pp ran).  Synchronises the device.  With attn_p_format 1 the threshold is 2^14 instead of 2^64: a
// caller that sees more than a fraction of a percent of slow paths on its data switches back with s2v_set_attn_p_format.
extern "C" int s2v_attn_slow_stats(s2v_ctx* c, uint64_t* slow, uint64_t* total, int32_t reset) {
    S2V_REQUIRE(c && slow && total, "s2v_attn_slow_stats: null argument");
    S2V_REQUIRE(c->attn_stats, "s2v_attn_slow_stats: an attention-weights context (S2V_CTX_ATTN_WEIGHTS) runs no attention");
    unsigned long long h[512];
    S2V_CHECK_HIP(hipDeviceSynchronize());
    S2V_CHECK_HIP(hipMemcpy(h, c->attn_stats, 4096, hipMemcpyDeviceToHost));
    uint64_t s = 0, t = 0;
    for (int i = 0; i < 256; ++i) { s += h[2 * i]; t += h[2 * i + 1]; }
    *slow = s; *total = t;
    if (reset) S2V_CHECK_HIP(hipMemset(c->attn_stats, 0, 4096));
    return 0;
}
// Change attn_p_format (include/s2v_hip.h, s2v_model_config) of a live context; a captured step is dropped and re-captured at its next use.
extern "C" int s2v_set_attn_p_format(s2v_ctx* c, int32_t fmt) {
    S2V_REQUIRE(c, "s2v_set_attn_p_format: null context");
    S2V_REQUIRE(fmt == 0 || fmt == 1, "s2v_set_attn_p_format: 0 (bf16) or 1 (fp16)");
    sc_invalidate(c);
    if (c->attn_p16 != (fmt == 1)) {
        S2V_CHECK_HIP(hipDeviceSynchronize());
        c->attn_p16 = fmt == 1;
        drop_graph(c);
    }
    return 0;
}

extern "C" int s2v_op_mod_gemv(const void* emb, const void* W, const void* bias, void* out, int32_t B, int32_t temb_dim,
                               int64_t rows, int32_t dtype, int32_t impl, s2v_stream stream) {
    S2V_REQUIRE(emb && W && out, "s2v_op_mod_gemv: null argument");
    S2V_REQUIRE(dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_F16, "s2v_op_mod_gemv: dtype must be f32, bf16 or f16");
    return launch_mod_gemv(emb, B, temb_dim, W, bias, rows, out, dtype, (hipStream_t)stream, impl == 1);
}

// The HBM-bound row kernels as operators (tests/test_gpu_norm_exact.py): each entry validates, fills the launcher's args struct and calls the
// launcher a context calls.  A row pitch or a parameter stride must keep every row 16-byte aligned: a multiple of `per16` elements.
static bool op_dtype_ok(int32_t dtype) { return dtype == S2V_DTYPE_BF16 || dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_F16; }
static int per16(int32_t dtype) { return dtype == S2V_DTYPE_F32 ? 4 : 8; }
extern "C" int s2v_op_ln_modulate(const void* x, int32_t ldx, void* y, int32_t ldy, const void* w, const void* b, float eps, const void* shift_vid,
                                  const void* scale_vid, const void* shift_txt, const void* scale_txt, const void* shift_ref, const void* scale_ref,
                                  int32_t mod_stride, int32_t B, int32_t Ntok, int32_t text_len, int32_t ref_len, int32_t D, void* q8, float* q8_scale,
                                  int32_t q8_keep_y, int32_t dtype, s2v_stream stream) {
    S2V_REQUIRE(op_dtype_ok(dtype), "s2v_op_ln_modulate: dtype must be f32, bf16 or f16");
    S2V_REQUIRE(x && w && b && shift_vid && scale_vid && shift_txt && scale_txt, "s2v_op_ln_modulate: null argument");
    S2V_REQUIRE((shift_ref == nullptr) == (scale_ref == nullptr), "s2v_op_ln_modulate: the reference set is a shift AND a scale, or neither");
    S2V_REQUIRE(q8 == nullptr || (dtype == S2V_DTYPE_BF16 && q8_scale != nullptr), "s2v_op_ln_modulate: the fp8 output needs bf16 rows and a scale vector");
    S2V_REQUIRE(y != nullptr || (q8 != nullptr && !q8_keep_y), "s2v_op_ln_modulate: y may be null only where the fp8 form does not keep the rows");
    S2V_REQUIRE(B > 0 && Ntok > 0 && (int64_t)B * Ntok <= INT32_MAX && text_len >= 0 && ref_len >= 0 && text_len + (int64_t)ref_len <= Ntok,
                "s2v_op_ln_modulate: B, Ntok > 0 and text_len + ref_len <= Ntok");
    const int v = per16(dtype);
    S2V_REQUIRE(D > 0 && D <= 4096 && D % 8 == 0, "s2v_op_ln_modulate: D must be <= 4096 and a multiple of 8");
    S2V_REQUIRE(ldx >= D && ldy >= D && mod_stride >= D && ldx % v == 0 && ldy % v == 0 && mod_stride % v == 0,
                "s2v_op_ln_modulate: ldx, ldy and mod_stride must cover D and keep rows 16-byte aligned");
    LnModArgs n{};
    n.x = x; n.ldx = ldx; n.y = y; n.ldy = ldy; n.w = w; n.b = b; n.eps = eps;
    n.shift_vid = shift_vid; n.scale_vid = scale_vid; n.shift_txt = shift_txt; n.scale_txt = scale_txt; n.mod_stride = mod_stride;
    n.B = B; n.Ntok = Ntok; n.text_len = text_len; n.D = D;
    n.shift_ref = shift_ref; n.scale_ref = scale_ref; n.ref_len = ref_len;
    n.q8 = q8; n.q8_scale = q8_scale; n.q8_keep_y = q8 != nullptr && q8_keep_y ? 1 : 0;
    return launch_ln_modulate(n, dtype, (hipStream_t)stream);
}
extern "C" int s2v_op_tail_norm(const void* x, int32_t ldx, void* y, int32_t ldy, const void* w1, const void* b1, const void* w2, const void* b2,
                                float eps, const void* shift, const void* scale, int32_t mod_stride, int32_t B, int32_t Ntok, int32_t row0, int32_t V,
                                int32_t D, int32_t dtype, s2v_stream stream) {
    S2V_REQUIRE(op_dtype_ok(dtype), "s2v_op_tail_norm: dtype must be f32, bf16 or f16");
    S2V_REQUIRE(x && y && w1 && b1 && w2 && b2 && shift && scale, "s2v_op_tail_norm: null argument");
    S2V_REQUIRE(B > 0 && Ntok > 0 && (int64_t)B * Ntok <= INT32_MAX && row0 >= 0 && V > 0 && row0 + (int64_t)V <= Ntok,
                "s2v_op_tail_norm: B, Ntok, V > 0 and rows [row0, row0 + V) inside a sample");
    const int v = per16(dtype);
    S2V_REQUIRE(D > 0 && D <= 4096 && D % 8 == 0, "s2v_op_tail_norm: D must be <= 4096 and a multiple of 8");
    S2V_REQUIRE(ldx >= D && ldy >= D && mod_stride >= D && ldx % v == 0 && ldy % v == 0 && mod_stride % v == 0,
                "s2v_op_tail_norm: ldx, ldy and mod_stride must cover D and keep rows 16-byte aligned");
    TailNormArgs t{};
    t.x = x; t.ldx = ldx; t.y = y; t.ldy = ldy; t.w1 = w1; t.b1 = b1; t.w2 = w2; t.b2 = b2; t.eps = eps;
    t.shift = shift; t.scale = scale; t.mod_stride = mod_stride; t.B = B; t.Ntok = Ntok; t.row0 = row0; t.V = V; t.D = D;
    return launch_tail_norm(t, dtype, (hipStream_t)stream);
}
extern "C" int s2v_op_qk_norm_rope(void* qkv, int32_t ld_qkv, int32_t B, int32_t H, int32_t Ntok, int32_t text_len, const void* nq_w, const void* nq_b,
                                   const void* nk_w, const void* nk_b, float eps, const float* cos_tab, const float* sin_tab, int32_t dtype,
                                   s2v_stream stream) {
    S2V_REQUIRE(op_dtype_ok(dtype), "s2v_op_qk_norm_rope: dtype must be f32, bf16 or f16");
    S2V_REQUIRE(qkv && nq_w && nq_b && nk_w && nk_b, "s2v_op_qk_norm_rope: null argument");
    S2V_REQUIRE((cos_tab == nullptr) == (sin_tab == nullptr), "s2v_op_qk_norm_rope: the rotary tables are a cosine AND a sine table, or neither");
    S2V_REQUIRE(B > 0 && H > 0 && H <= 4096 && Ntok > 0 && (int64_t)B * Ntok <= INT32_MAX && text_len >= 0 && text_len <= Ntok,
                "s2v_op_qk_norm_rope: B, H, Ntok > 0 and text_len <= Ntok");
    S2V_REQUIRE(ld_qkv >= 3 * H * 64 && ld_qkv % per16(dtype) == 0, "s2v_op_qk_norm_rope: ld_qkv must cover 3 * H * 64 and keep rows 16-byte aligned");
    QkNormRopeArgs q{};
    q.qkv = qkv; q.ld_qkv = ld_qkv; q.B = B; q.H = H; q.Ntok = Ntok; q.text_len = text_len;
    q.nq_w = nq_w; q.nq_b = nq_b; q.nk_w = nk_w; q.nk_b = nk_b; q.eps = eps; q.cos = cos_tab; q.sin = sin_tab;
    return launch_qk_norm_rope(q, dtype, (hipStream_t)stream);  // q.vt stays null: no V^T
}
extern "C" int s2v_op_v_transpose(const void* qkv, int32_t ld_qkv, int32_t B, int32_t H, int32_t Ntok, void* vt, int32_t ntok_pad, uint32_t* vt_amax,
                                  s2v_stream stream) {
    S2V_REQUIRE(qkv && vt, "s2v_op_v_transpose: null argument");
    S2V_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Ntok > 0, "s2v_op_v_transpose: B, H (<= 65535 each) and Ntok must be positive");
    S2V_REQUIRE(ld_qkv >= 3 * H * 64 && ld_qkv % 8 == 0, "s2v_op_v_transpose: ld_qkv must cover 3 * H * 64 and be a multiple of 8");
    S2V_REQUIRE(ntok_pad % 64 == 0 && ntok_pad >= Ntok, "s2v_op_v_transpose: ntok_pad must be a multiple of 64 covering Ntok");
    return launch_v_transpose(qkv, ld_qkv, B, H, Ntok, vt, ntok_pad, (hipStream_t)stream, vt_amax);
}

// attention with QK^T on the scaled fp8 MFMA as weight_format 2 runs it: q (times scale * log2 e) and k of the bf16 qkv rows become MX e4m3
// images in `scratch` (also returned to the caller for inspection: layout in kernels.h AttnArgs::q8 ... k8s, offsets below), V^T and P.V stay bf16.
static int op_attention_fp8qk(const void* qkv, void* vt_scratch, void* scratch, int64_t scratch_bytes, void* out, int32_t B, int32_t H,
                              int32_t Ntok, bool p16, s2v_stream stream) {
    S2V_REQUIRE(qkv && vt_scratch && scratch && out, "s2v_op_attention_fp8qk: null argument");
    const int D = H * 64;
    const int64_t ntok_pad = rup(Ntok, 64), BH = (int64_t)B * H;
    const int64_t oq8 = 0, oq8s = oq8 + rup(BH * Ntok * 64, 256), ok8 = oq8s + rup(BH * Ntok * 2, 256), ok8s = ok8 + rup(BH * ntok_pad * 64, 256);
    const int64_t oam = rup(ok8s + BH * ntok_pad * 4, 256);  // p16: the magnitude words of the fp16 V^T (AttnArgs::vt_amax) behind the images
    S2V_REQUIRE(scratch_bytes >= (p16 ? oam + BH * 4 : ok8s + BH * ntok_pad * 4),
                "s2v_op_attention_fp8qk: scratch too small (B*H*(66*Ntok + 68*ntok_pad) + 1024 bytes; fp16 P: 256 + 4*B*H more)");
    AttnArgs a{};
    a.qkv = qkv; a.ld_qkv = 3 * D; a.out = out; a.ld_out = D; a.B = B; a.H = H; a.Ntok = Ntok; a.scale = 0.125f;
    a.ntok_pad = (int)ntok_pad; a.vt = vt_scratch;
    char* w = (char*)scratch;
    a.q8 = (unsigned char*)(w + oq8); a.q8s = (unsigned short*)(w + oq8s); a.k8 = (unsigned char*)(w + ok8); a.k8s = (unsigned*)(w + ok8s);
    hipStream_t st = (hipStream_t)stream;
    if (p16) { a.p16 = 1; a.vt_amax = (const unsigned*)(w + oam); }
    S2V_TRY(launch_v_transpose(qkv, 3 * D, B, H, Ntok, vt_scratch, a.ntok_pad, st, p16 ? (unsigned*)(w + oam) : nullptr));
    S2V_TRY(launch_qk_quant_mx(qkv, 3 * D, B, H, Ntok, a.ntok_pad, a.scale * 1.4426950408889634f, (unsigned char*)a.q8, (unsigned short*)a.q8s,
                               (unsigned char*)a.k8, (unsigned*)a.k8s, st));
    return launch_attn_q4f(a, false, st);
}
extern "C" int s2v_op_attention_fp8qk(const void* qkv, void* vt_scratch, void* scratch, int64_t scratch_bytes, void* out, int32_t B, int32_t H,
                                      int32_t Ntok, s2v_stream stream) {
    return op_attention_fp8qk(qkv, vt_scratch, scratch, scratch_bytes, out, B, H, Ntok, false, stream);
}
// the same with P and V^T in fp16 (attn_p_format 1 under weight_format 2: attn_q4fh)
extern "C" int s2v_op_attention_fp8qk_p16(const void* qkv, void* vt_scratch, void* scratch, int64_t scratch_bytes, void* out, int32_t B, int32_t H,
                                          int32_t Ntok, s2v_stream stream) {
    return op_attention_fp8qk(qkv, vt_scratch, scratch, scratch_bytes, out, B, H, Ntok, true, stream);
}

extern "C" int s2v_op_attention(const void* qkv, void* vt_scratch, void* out, int32_t B, int32_t H, int32_t Ntok,
                                int32_t dtype, int32_t impl, s2v_stream stream) {
    S2V_REQUIRE(qkv && out, "s2v_op_attention: null argument");
    const int D = H * 64;
    AttnArgs a{};
    a.qkv = qkv; a.ld_qkv = 3 * D; a.out = out; a.ld_out = D; a.B = B; a.H = H; a.Ntok = Ntok; a.scale = 0.125f;
    a.ntok_pad = (int)rup(Ntok, 64);
    hipStream_t st = (hipStream_t)stream;
    if (impl == 0 || impl == 3 || impl == 4) {  // 3: as 0 with P / V^T in fp16 where the four-wave kernel runs (attn_p_format 1); 4: attn_q4h at any length
        S2V_REQUIRE(dtype == S2V_DTYPE_BF16 && vt_scratch, "s2v_op_attention: impl 0 / 3 / 4 are bf16 and need vt_scratch");
        a.vt = vt_scratch;
        a.p16 = (impl == 4 || (impl == 3 && attn_runs_q4(Ntok, false))) ? 1 : 0;
        if (a.p16) {  // operator level: one buffer of magnitude words per process, on the device of the first such call (restriction stated in s2v_hip.h)
            static unsigned* op_vt_amax = nullptr;
            S2V_REQUIRE((int64_t)B * H <= VT_AMAX_WORDS, "s2v_op_attention: B * H too large for the fp16 V^T");
            if (!op_vt_amax) S2V_CHECK_HIP(hipMalloc((void**)&op_vt_amax, sizeof(unsigned) * VT_AMAX_WORDS));
            a.vt_amax = op_vt_amax;
        }
        S2V_TRY(launch_v_transpose(qkv, 3 * D, B, H, Ntok, vt_scratch, a.ntok_pad, st, const_cast<unsigned*>(a.vt_amax)));
        if (impl == 4) return launch_attn_q4h(a, false, st);
        return launch_attn_bf16(a, st);
    }
    if (impl == 6) {  // fp16 on v_mfma_f32_32x32x16_f16 (what the fp16 engine runs); vt_scratch as for impl 0
        S2V_REQUIRE(dtype == S2V_DTYPE_F16 && vt_scratch, "s2v_op_attention: impl 6 is fp16 and needs vt_scratch");
        a.vt = vt_scratch;
        S2V_TRY(launch_v_transpose(qkv, 3 * D, B, H, Ntok, vt_scratch, a.ntok_pad, st));
        return launch_attn_f16(a, st);
    }
    if (impl == 5) {  // fp32 on the fp32 matrix pipe (what the fp32 engine runs)
        S2V_REQUIRE(dtype == S2V_DTYPE_F32 || dtype == S2V_DTYPE_F16, "s2v_op_attention: impl 5 is fp32 / fp16 only");
        return launch_attn_f32m(a, dtype, st);
    }
    a.valu_only = 1;
    return launch_attn_simple(a, dtype, st);
}
