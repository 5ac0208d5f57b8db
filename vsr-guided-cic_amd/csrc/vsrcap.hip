// libvsrcap.so - C ABI + per-timestep orchestration of the VSR captioning decoder on gfx950.
// Entry points are declared in include/vsrcap.h; reference behaviour cited there and in kernels.h.  GEMM routing (which kernel, tile and
// k plan a launch takes; the VSR_* routing knobs) lives in gemm_route.h, the kernel switch in gemm_dispatch.h, the problem lists of the
// step's launches (shared with the training forward) in step_gemms.h.
//
// One decoder timestep = 4 grouped fp32-MFMA GEMM launches + 5 small kernels, all on the caller's stream:
//   S1  [h2 | x | h1_old] -> LSTM1 gates (4H) | sentinel gate (H) | shift-gate image part (H)      gemm
//       k_lstm1                                                                                    pointwise
//   S2  h1_new -> [W1_hg | att_ha] ,  s_t -> [s_fc | att_sa]                                       gemm (4 problems)
//       k_attend (shift-gate vector and the S2 slab sums fused in)                                 pointwise / HBM-bound
//   S5  [h1_new | att | h2_old] -> LSTM2 gates (4H) ,  g_t -> att_ga                               gemm (2 problems)
//       k_lstm2
//   S6  h2_new -> vocabulary logits (V)                                                            gemm
//       k_vocab (log-sum-exp + arg-max / top-k / Gumbel sample / full row; the step's gate logits on the side), k_select_*
// (the training forward, train.inc.h, keeps k_gate2 separate and saves what the backward pass needs)
// The image-constant work (pooled descriptor and its projection, att_va(regions), row masks) is hoisted
// into vsr_prepare().  Beams never copy statics: rows index their image (row / beam) and their parent.
#include "../../include/vsrcap.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm_route.h"
#include "step_gemms.h"
#include "kernels.h"
#include "train_kernels.h"
#include "optim_kernels.h"

using namespace vsr;

static thread_local char g_err[512] = "";
static int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define LAUNCHCHK() HIPCHK(hipGetLastError())

struct Ctx {
    int B = 0, R0 = 0, L = 0, R = 0, beam = 1, Mmax = 0;
    int n_img = 0, Rb = 0;       // index-list region format: images and rows per image of the feature bank (0 = dense regions)
    const float* det = nullptr;
    const float* regions = nullptr;   // dense (B, L, R, D) region tensor, or the (n_img, Rb, D) feature bank
    const int* ridx = nullptr;   // (B, L, R) absolute bank row per slot entry (index-list format) or null
    bool rows_are_images = false;   // index-list format without a row -> image map: decoder row b owns bank rows [b Rb, (b + 1) Rb) (training needs this)
    int* ridx_buf = nullptr;
    float* bmask = nullptr;      // row masks of the rows att_va runs over (dense: = rmask)
    float* dmask = nullptr;      // row masks of the detection rows (pooled descriptor)
    float *vbar, *vproj, *vproj2, *P, *rmask;
    int *vlist, *nvalid_dev;     // non-padding region rows (ascending) and their number
    int* bcount;                 // per-256-row counts of the compaction
    int nvalid = 0;
    bool bounded = false;        // nvalid is the caller's row bound (vsr_set_valid_rows_bound), the real count lives in nvalid_dev[0]
    float* st[2][4];   // h1, c1, h2, c2 double-buffered
    int *slot[2], *word[2], *gate[2], *parent;
    float *s_t, *gpre, *g_t, *hA, *sa, *sent, *att, *zsum, *lg, *top_v;
    float* ga_slabs;             // att_ga(g_t) partial sums: kept apart from `scratch`, the vocabulary GEMM overwrites that first
    size_t ga_floats = 0, pre1_floats = 0;       // capacities of ga_slabs and pre1, as scratch_floats is scratch's
    int* top_i;
    float *seq[2], *mask[2];
    int *hist_parent, *hist_word, *hist_gate;
    float *hist_lpw, *hist_lpg;
    int *cap32, *forced_w32, *forced_g32;
    int64_t* tmp_i64;
    float* scratch;
    size_t scratch_floats = 0;
    // bf16 GEMM mode: bf16 images of the GEMMs' A operands, written by their producers next to the fp32 values (h1, h2 of both
    // state buffers, s_t, g_t, att); st16_ok[i]: the images of state buffer i match its fp32 content
    uint16_t* st16[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    uint16_t *s_t16 = nullptr, *g_t16 = nullptr, *att16 = nullptr;
    bool st16_ok[2] = {false, false};
    float* pre1 = nullptr;       // LSTM1/gate sums of the NEXT step, produced early (merged with the vocabulary GEMM)
    int pre1_ns = 0, pre1_nblk = 0, pre1_skip5 = 0;
    long long pre1_stride = 0;
};

struct TrainCtx;
static TrainCtx* new_train_ctx();
static void free_train_ctx(TrainCtx*);
static void invalidate_train_ctx(TrainCtx*);
struct SavedForwards;                 // the training forwards whose workspaces are still intact (train.inc.h)
static SavedForwards* new_saved_forwards();
static void free_saved_forwards(SavedForwards*);
static void drop_saved_forwards(SavedForwards*);                                            // all of them (a change of GEMM flavour / weights binding)
static void drop_saved_forwards_in(SavedForwards*, const void* lo, size_t bytes);           // those whose workspaces overlap [lo, lo + bytes)

struct vsr_handle : GemmState {         // (gemm_route.h: the GEMM flavours switched on, the operand images and the routing knobs `gk`)
    TrainCtx* tc = nullptr;
    SavedForwards* saved = nullptr;
    hipEvent_t bucket_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // recorded by vsr_train_backward after each gradient bucket
    bool buckets_recorded = false;
    long long gen_counter = 0;        // generations of the training forwards: strictly increasing per handle
    const char* ws_lo = nullptr;      // the workspace the current vsr_prepare*() carved (h->c points into it)
    size_t ws_bytes = 0;
    // the selection of step t inside the LSTM1 kernel of step t + 1 (kernels.h: k_select_lstm1_x2, k_select_simple_lstm1); VSR_FUSE_SELECT=0: a launch of its own
    int fuse_select = 3;              // bit 0: greedy / sampling / replay (k_select_simple_lstm1), bit 1: beam search (k_select_lstm1_x2)
    int bf16_a16 = 1;            // bf16 mode: the decode step's producers write bf16 images of the GEMM A operands (VSR_BF16_A16=0: off)
    vsr_dims d;
    vsr_weights w;
    bool bound = false, prepared = false;
    const int* vt_ptr = nullptr;
    const int* vt_ids = nullptr;
    int n_verbs = 0;
    const float* xproj = nullptr;     // decode cache: (V, 6H) projection of the embedding table, valid for the bound weights
    bool xproj_al8 = false;           // ... at an 8-byte aligned address: what k_select_lstm1_x2 needs (everything else it touches is the workspace's)
    long long rows_bound = 0;    // vsr_set_valid_rows_bound: > 0 = the caller's upper bound on the non-padding region rows; vsr_prepare*() then never waits for the host
    int attend_parts = 2, attend_limit = 256;        // workgroups per row of k_attend in launches of <= attend_limit / parts rows (VSR_ATTEND_PARTS, VSR_ATTEND_LIMIT)
    int adam_blocks = 0;         // grid budget of vsr_adam_step: the workgroups the device holds at once (set at its first call)
    int split_pre1 = 1;          // the h1 part of the next step's LSTM1 sums in the S5 launch, the h2 part with the vocabulary (run_step; VSR_SPLIT_PRE1=0: all of it with the vocabulary, as in rounds 2-5)
    Ctx c;
    hipEvent_t ev_count = nullptr;   // prepare(): the row count has reached the host
    int* host_back = nullptr;        // pinned landing place of that read-back (2 ints)
    GemmProfile prof;                // measurement (vsr_profile_*): every GEMM launch of the decoder is handed it
};

// ---------------------------------------------------------------------------------------------- workspace
struct Bump {
    char* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t n) {
        off = (off + 255) & ~size_t(255);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

static size_t carve(const vsr_handle* h, Ctx& c, char* base) {
    const vsr_dims& d = h->d;
    const size_t B = c.B, H = d.rnn_size, A = d.att_size, D = d.det_feat_size, T = d.seq_len;
    const size_t M = c.Mmax, rows = B * c.L * c.R;
    const size_t prows = c.Rb > 0 ? (size_t)c.n_img * c.Rb : rows;      // rows the hoisted att_va projection covers
    Bump b{base};
    c.vbar = b.take<float>(B * D);
    c.vproj = b.take<float>(B * 6 * H);
    c.vproj2 = b.take<float>(B * 4 * H);
    c.P = b.take<float>(prows * A);
    c.rmask = b.take<float>(rows);
    if (c.Rb > 0) {
        c.bmask = b.take<float>(prows);
        c.ridx_buf = b.take<int>(rows);
    } else {
        c.bmask = c.rmask;
        c.ridx_buf = nullptr;
    }
    c.dmask = b.take<float>((size_t)(c.Rb > 0 ? c.n_img : B) * c.R0);
    c.vlist = b.take<int>(prows);
    c.bcount = b.take<int>((prows + 255) / 256 + 1);
    c.nvalid_dev = b.take<int>(4);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 4; ++j) c.st[i][j] = b.take<float>(M * H);
    for (int i = 0; i < 2; ++i) {
        c.slot[i] = b.take<int>(M);
        c.word[i] = b.take<int>(M);
        c.gate[i] = b.take<int>(M);
        c.seq[i] = b.take<float>(M);
        c.mask[i] = b.take<float>(M * 2);
    }
    c.parent = b.take<int>(M);
    c.s_t = b.take<float>(M * H);
    c.gpre = b.take<float>(M * H);
    c.g_t = b.take<float>(M * H);
    c.hA = b.take<float>(M * A);
    c.sa = b.take<float>(M * A);
    c.sent = b.take<float>(M * D);
    c.att = b.take<float>(M * D);
    c.zsum = b.take<float>(M);
    c.lg = b.take<float>(M * 2);
    // The slab areas are sized by the layouts the launches are placed with (step_gemms.h): every group at GEMM_MAX_SLABS slabs.
    const SlabLayout l5 = s5_decode_slabs(d);      // decode S5: LSTM2 in scratch, att_ga in ga_slabs, the next step's LSTM1 sums in pre1
    c.ga_floats = slab_floats(l5, M, 1);
    c.ga_slabs = b.take<float>(c.ga_floats);
    c.top_v = b.take<float>(M * KMAX);
    c.top_i = b.take<int>(M * KMAX);
    c.hist_parent = b.take<int>(T * M);
    c.hist_word = b.take<int>(T * M);
    c.hist_gate = b.take<int>(T * M);
    c.hist_lpw = b.take<float>(T * M);
    c.hist_lpg = b.take<float>(T * M);
    c.cap32 = b.take<int>(T * M);
    c.forced_w32 = b.take<int>(T * M);
    c.forced_g32 = b.take<int>(T * M);
    c.tmp_i64 = b.take<int64_t>(T * M);
    // split-K slab scratch: the widest stage of a step (S1, S2, S5 as training packs it - decoding's takes less -, S6), the hoisted vbar
    // projections over the B images (the LSTM2 one is narrower) and att_va over the rows prepare() may project (the bank rows when indexed)
    size_t widest = std::max({slab_row_floats(lstm1_slabs(d)), slab_row_floats(s2_slabs(d)), slab_row_floats(s5_slabs(d)), slab_row_floats(vocab_slabs(d))});
    size_t stage = std::max(M * widest, B * slab_row_floats(lstm1_slabs(d)));
    c.scratch_floats = std::max(stage, std::max(rows, prows) * slab_row_floats(att_va_slabs(d))) * GEMM_MAX_SLABS;
    c.scratch = b.take<float>(c.scratch_floats);
    c.pre1_floats = slab_floats(l5, M, 2);
    c.pre1 = b.take<float>(c.pre1_floats);
    b.off = (b.off + 15) & ~size_t(15);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) c.st16[i][j] = b.take<uint16_t>(2 * ((M * H + 7) & ~size_t(7)));      // (bf16: 2 bytes per element; fp16 pairs: 4)
    c.s_t16 = b.take<uint16_t>(2 * ((M * H + 7) & ~size_t(7)));
    c.g_t16 = b.take<uint16_t>(2 * ((M * H + 7) & ~size_t(7)));
    c.att16 = b.take<uint16_t>(2 * ((M * D + 7) & ~size_t(7)));
    return (b.off + 255) & ~size_t(255);
}

// ------------------------------------------- GEMM launch (routing and planning: GemmBuilder::finish, gemm_route.h; the kernel switch: gemm_dispatch.h)
int vsr::GemmBuilder::launch(hipStream_t s, const GemmState* h, GemmProfile* p) {
    if (stale_h2) return fail("f16x2 flavour: a GEMM launch names a transposed operand of the training pass that only exists as an fp16-pair image but cannot take an f16x2 kernel (gemm mode / tile override changed since vsr_train_forward, or K / leading dimensions not multiples of 8)");
    if (stale_w) return fail("bf16 mode: a GEMM launch names a transposed operand that only exists as a bf16 image but cannot take the bf16 kernel (K / leading dimensions must be multiples of 8)");
    if (!h->gk.xcd_groups) a.xcd_chunk = 0;              // VSR_XCD_GROUPS=0: ceil(G / 8) workgroups per XCD whatever the m-groups (A/B)
    const bool prof = p && p->on && (p->seen++ % p->every) == 0 && p->ev_used + 2 <= p->ev.size();
    if (prof) (void)hipEventRecord(p->ev[p->ev_used], s);
    gemm_dispatch(route, a, s);
    if (prof) {
        (void)hipEventRecord(p->ev[p->ev_used + 1], s);
        p->ev_used += 2;
        p->flops += gemm_flops(a);
        p->bytes += gemm_bytes(a, route.kernel == GemmKernel::BF16W ? 2 : 4);      // (quirk kept: the all-DMA bf16 kernel, B16A, is accounted with 4-byte weights)
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
// dst (M, N), compact = the sum of ns compact (M, N) slabs: the finish kernel without an epilogue term
static void slab_sum_to(hipStream_t s, const float* slabs, int ns, int M, int N, float* dst) {
    const long long tot = (long long)M * N;
    hipLaunchKernelGGL((k_prod_finish<false, FIN_NONE>), dim3(cdiv(tot, 256)), dim3(256), 0, s, slabs, ns, tot, M, N, nullptr, SSP_ACT_NONE, nullptr, 0LL, dst,
                       (long long)N, nullptr, 0LL, nullptr, 1.f);
}
// Places the slab groups of a planned launch of M-row problems (step_gemms.h: place_slabs) in `areas` (the layout's area 0, 1, ..); the
// groups' views in pl.v are what the consumer kernels are given.  A group that does not fit its area fails under the launch's name.
static int place(GemmBuilder& g, int M, const SlabLayout& l, std::initializer_list<SlabArea> areas, SlabPlan& pl, const char* launch) {
    return place_slabs(g.a, M, l, areas.begin(), (int)areas.size(), pl) ? fail("%s: %s", launch, pl.err) : 0;
}
// The x part of the LSTM1 / gate pre-activations of o.M rows does not depend on the recurrence: one GEMM through the slabs of `scratch`
// -> dst (o.M, 6H).  The decode cache's chunks of vocabulary rows and the training forwards' input rows.
static int xproj_rows(vsr_handle* h, const StepOperands& o, SlabArea scratch, float* dst, hipStream_t s, const char* who) {
    GemmBuilder g;
    add_lstm1(g, h->d, h->w, o, L1_X);
    g.finish(h);
    SlabPlan pl;
    if (place(g, o.M, lstm1_slabs(h->d), {scratch}, pl, who)) return 1;
    if (g.launch(s, h, &h->prof)) return fail("%s gemm launch failed", who);
    slab_sum_to(s, pl.v[0].base, pl.v[0].n, o.M, 6 * h->d.rnn_size, dst);
    return 0;
}

// ---------------------------------------------------------------------------------------------- API: lifetime
extern "C" int vsr_abi_version(void) { return VSR_ABI_VERSION; }
extern "C" const char* vsr_last_error(void) { return g_err; }

extern "C" int vsr_create(const vsr_dims* dims, vsr_handle** out) {
    if (!dims || !out) return fail("vsr_create: null argument");
    const vsr_dims& d = *dims;
    if (d.seq_len <= 0 || d.vocab_size <= 0) return fail("vsr_create: seq_len and vocab_size must be positive");
    if (d.det_feat_size % 4 || d.input_encoding_size % 4 || d.rnn_size % 4 || d.att_size % 4)
        return fail("vsr_create: det_feat_size, input_encoding_size, rnn_size and att_size must be multiples of 4 "
                    "(16-byte vector loads); got %d %d %d %d", d.det_feat_size, d.input_encoding_size, d.rnn_size, d.att_size);
    if (d.bos_idx < 0 || d.bos_idx >= d.vocab_size) return fail("vsr_create: bos_idx out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("vsr_create: no HIP device");
    vsr_handle* h = new vsr_handle();
    h->d = d;
    h->tc = new_train_ctx();
    h->saved = new_saved_forwards();
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) h->gk.set_cus(prop.multiProcessorCount);
    h->gk.read_env();
    if (const char* e = getenv("VSR_FUSE_SELECT")) h->fuse_select = atoi(e);
    if (const char* e = getenv("VSR_BF16_A16")) h->bf16_a16 = atoi(e);
    if (const char* e = getenv("VSR_SPLIT_PRE1")) h->split_pre1 = atoi(e);
    if (const char* e = getenv("VSR_ATTEND_PARTS")) h->attend_parts = std::max(1, atoi(e));
    if (const char* e = getenv("VSR_ATTEND_LIMIT")) h->attend_limit = std::max(1, atoi(e));
    *out = h;
    return 0;
}

extern "C" void vsr_destroy(vsr_handle* h) {
    if (!h) return;
    for (hipEvent_t e : h->prof.ev) (void)hipEventDestroy(e);
    if (h->ev_count) (void)hipEventDestroy(h->ev_count);
    if (h->host_back) (void)hipHostFree(h->host_back);
    free_train_ctx(h->tc);
    free_saved_forwards(h->saved);
    for (hipEvent_t e : h->bucket_ev) if (e) (void)hipEventDestroy(e);
    delete h;
}

extern "C" int vsr_profile_begin_sampled(vsr_handle* h, int32_t every);
extern "C" int vsr_profile_begin(vsr_handle* h) { return vsr_profile_begin_sampled(h, 1); }

extern "C" int64_t vsr_profile_seen(const vsr_handle* h) { return h ? (int64_t)h->prof.seen : 0; }
extern "C" double vsr_profile_bytes(const vsr_handle* h) { return h ? h->prof.bytes : 0.0; }

extern "C" int vsr_profile_begin_sampled(vsr_handle* h, int32_t every) {
    if (!h) return fail("vsr_profile_begin: null handle");
    if (every < 1) return fail("vsr_profile_begin_sampled: every must be >= 1");
    GemmProfile& p = h->prof;
    p.every = every;
    p.seen = 0;
    const size_t want = 2 * 4096;
    while (p.ev.size() < want) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        p.ev.push_back(e);
    }
    p.ev_used = 0;
    p.flops = 0;
    p.bytes = 0;
    p.on = true;
    return 0;
}

extern "C" int vsr_profile_end(vsr_handle* h, void* stream, double* gemm_ms, int64_t* gemm_launches, double* gemm_flops) {
    if (!h || !h->prof.on) return fail("vsr_profile_end: profiling not active");
    GemmProfile& p = h->prof;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    double ms = 0;
    for (size_t i = 0; i + 1 < p.ev_used; i += 2) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, p.ev[i], p.ev[i + 1]));
        ms += t;
    }
    if (gemm_ms) *gemm_ms = ms;
    if (gemm_launches) *gemm_launches = (int64_t)(p.ev_used / 2);
    if (gemm_flops) *gemm_flops = p.flops;
    p.on = false;
    return 0;
}

// ---- derived from the weights: bound pointers -> flavour (bf16 copies | x3 switch | fp16-pair images) -> decode cache -> prepared statics.
// VOID_REFRESH: copies / images rebuilt in the same flavour: cache and statics are of older weights; the saved forwards stay (a training
// step refreshes, then differentiates).  VOID_FLAVOUR: flavour or weight pointers changed: a saved forward is not differentiated in another.
enum VoidLevel { VOID_REFRESH, VOID_FLAVOUR };
// the decode cache pointer and what vsr_beam asks of it (k_select_lstm1_x2 reads it 8 bytes at a time; nothing else it touches can be misaligned)
static void set_xproj(vsr_handle* h, const float* buf) {
    h->xproj = buf;
    h->xproj_al8 = buf && (reinterpret_cast<uintptr_t>(buf) & 7) == 0;
}
static void void_derived(vsr_handle* h, VoidLevel level) {
    set_xproj(h, nullptr);
    h->prepared = false;              // vsr_prepare*() again (check_ready says so)
    if (level == VOID_FLAVOUR) { invalidate_train_ctx(h->tc); drop_saved_forwards(h->saved); }
}

extern "C" int vsr_bind_weights(vsr_handle* h, const vsr_weights* w) {
    if (!h || !w) return fail("vsr_bind_weights: null argument");
    const float* const* p = reinterpret_cast<const float* const*>(w);
    for (size_t i = 0; i < sizeof(vsr_weights) / sizeof(float*); ++i)
        if (!p[i]) return fail("vsr_bind_weights: weight pointer %zu is null", i);
    h->w = *w;
    h->bound = true;
    void_derived(h, VOID_FLAVOUR);    // cache, statics and saved forwards were taken with the old tensors
    if (h->bf16_on) {                 // ... and so were the bf16 copies: back to fp32 until vsr_refresh_bf16_weights is called again
        h->bf16_on = false;
        h->img.clear_weights_bf16();
    }
    if (h->h2_on) {                   // ... and the fp16-pair images (vsr_refresh_h2_weights)
        h->h2_on = false;
        h->img.clear_h2();
    }
    return 0;
}

// ---- decode cache: xproj[v] = [W_ih1 ; W1_is ; W1_ig][:, x columns] . embed[v]  for every vocabulary row.
// Weight-only work hoisted out of the time loop AND out of the call: 6 of the 47.9 M MAC per row-step.
static const int XPROJ_CHUNK = 512;
extern "C" size_t vsr_decode_cache_floats(const vsr_handle* h) {
    if (!h) return 0;
    const size_t V = h->d.vocab_size, H = h->d.rnn_size;
    return V * 6 * H + slab_floats(lstm1_slabs(h->d), XPROJ_CHUNK) + 64;      // the cache, then a chunk's slabs
}
extern "C" int vsr_build_decode_cache(vsr_handle* h, float* buf, size_t n_floats, void* stream) {
    if (!h || !h->bound) return fail("vsr_build_decode_cache: weights not bound");
    if (!buf) { set_xproj(h, nullptr); return 0; }
    if (n_floats < vsr_decode_cache_floats(h)) return fail("vsr_build_decode_cache: buffer too small");
    hipStream_t s = (hipStream_t)stream;
    const int V = h->d.vocab_size, H = h->d.rnn_size, E = h->d.input_encoding_size;
    const SlabArea slabs{buf + (size_t)V * 6 * H, slab_floats(lstm1_slabs(h->d), XPROJ_CHUNK)};
    for (int v0 = 0; v0 < V; v0 += XPROJ_CHUNK) {
        StepOperands o;                       // the chunk's rows of the embedding table, ungathered
        o.M = std::min(XPROJ_CHUNK, V - v0);
        o.x = h->w.embed_weight + (size_t)v0 * E;
        if (xproj_rows(h, o, slabs, buf + (size_t)v0 * 6 * H, s, "decode cache")) return 1;
    }
    LAUNCHCHK();
    set_xproj(h, buf);
    return 0;
}

static void weight_sizes(const vsr_dims& d, size_t (&n)[ADAM_NT]) {          // elements of the 28 tensors, in the order of vsr_weights
    const size_t H = d.rnn_size, A = d.att_size, D = d.det_feat_size, E = d.input_encoding_size, V = d.vocab_size;
    const size_t in1 = (d.h2_first_lstm ? H : 0) + D + E, in2 = H + D + (d.img_second_lstm ? D : 0);
    const size_t c[ADAM_NT] = {V * E, H * in1, H, H * H, H, A * D, A * H, A, A * H, A, 4 * H * in1, 4 * H * H, 4 * H, 4 * H,
                               4 * H * in2, 4 * H * H, 4 * H, 4 * H, V * H, V, D * H, D, H * in1, H, H * H, H, A * H, A};
    for (int i = 0; i < ADAM_NT; ++i) n[i] = c[i];
}
static_assert(sizeof(vsr_weights) == ADAM_NT * sizeof(float*), "one table entry per tensor of vsr_weights");
// The 14 matrices the GEMMs multiply by, as tensors of vsr_weights: what the bf16 mode copies, the f16x2 flavour makes images of (exponent
// slot = position in this list) and the optimizer rewrites both for.  Sizes: weight_sizes
#define VSR_W(f) (int)(offsetof(vsr_weights, f) / sizeof(float*))
static const int GEMM_NW = 14;
static const int GEMM_MATRIX[GEMM_NW] = {VSR_W(W1_is_weight), VSR_W(W1_hs_weight), VSR_W(att_va_weight), VSR_W(att_ha_weight), VSR_W(att_sa_weight),
                                         VSR_W(lstm1_weight_ih), VSR_W(lstm1_weight_hh), VSR_W(lstm2_weight_ih), VSR_W(lstm2_weight_hh), VSR_W(out_fc_weight),
                                         VSR_W(s_fc_weight), VSR_W(W1_ig_weight), VSR_W(W1_hg_weight), VSR_W(att_ga_weight)};
#undef VSR_W
static void gemm_matrix_list(const vsr_dims& d, const vsr_weights& w, const float* (&ptr)[GEMM_NW], size_t (&n)[GEMM_NW]) {
    size_t all[ADAM_NT];
    weight_sizes(d, all);
    const float* const* W = reinterpret_cast<const float* const*>(&w);
    for (int i = 0; i < GEMM_NW; ++i) { ptr[i] = W[GEMM_MATRIX[i]]; n[i] = all[GEMM_MATRIX[i]]; }
}

// ---- bf16 throughput mode: bf16 copies of those matrices (fp32 stays the master copy)
extern "C" size_t vsr_bf16_weight_bytes(const vsr_handle* h) {
    if (!h) return 0;
    const float* p[GEMM_NW]; size_t n[GEMM_NW];
    vsr_weights none;                          // only the sizes are needed (the weights may be unbound)
    memset(&none, 0, sizeof(none));
    gemm_matrix_list(h->d, none, p, n);
    size_t tot = 0;
    for (int i = 0; i < GEMM_NW; ++i) tot += ((n[i] + 7) & ~size_t(7)) * sizeof(uint16_t);
    return tot + 256;
}
extern "C" int vsr_refresh_bf16_weights(vsr_handle* h, void* buffer, size_t bytes, void* stream) {
    if (!h) return fail("vsr_refresh_bf16_weights: null handle");
    if (!buffer) {                                          // back to the fp32 parity mode
        if (h->bf16_on) void_derived(h, VOID_FLAVOUR);
        h->bf16_on = false;
        h->img.clear_weights_bf16();                       // the weight copies only: the training workspace's twins stay registered
        return 0;
    }
    if (!h->bound) return fail("vsr_refresh_bf16_weights: weights not bound");
    const vsr_dims& d = h->d;
    if (d.det_feat_size % 8 || d.input_encoding_size % 8 || d.rnn_size % 8 || d.att_size % 8)
        return fail("vsr_refresh_bf16_weights: the bf16 mode needs det_feat_size, input_encoding_size, rnn_size and att_size to be "
                    "multiples of 8 (16-byte bf16 chunks); got %d %d %d %d", d.det_feat_size, d.input_encoding_size, d.rnn_size, d.att_size);
    if (bytes < vsr_bf16_weight_bytes(h)) return fail("vsr_refresh_bf16_weights: buffer too small");
    if (reinterpret_cast<uintptr_t>(buffer) & 15) return fail("vsr_refresh_bf16_weights: buffer must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const float* p[GEMM_NW]; size_t n[GEMM_NW];
    gemm_matrix_list(h->d, h->w, p, n);
    h->img.clear_weights_bf16();
    uint16_t* out = reinterpret_cast<uint16_t*>(buffer);
    for (int i = 0; i < GEMM_NW; ++i) {
        hipLaunchKernelGGL(k_f32_to_bf16, dim3(cdiv((long long)n[i], 8 * 256)), dim3(256), 0, s, p[i], out, (long long)n[i]);
        h->img.add_weight_bf16(p[i], n[i], out);
        out += (n[i] + 7) & ~size_t(7);
    }
    LAUNCHCHK();
    void_derived(h, h->bf16_on ? VOID_REFRESH : VOID_FLAVOUR);
    h->bf16_on = true;
    return 0;
}

// ---- f16x2 flavour (gemm_h2.h): fp16-pair images of the 14 weight matrices the GEMMs multiply by, their power-of-two scales, and the
// bounds of the A operands that depend on the weights only (embedding rows, the sentinel vector).  fp32 stays the master copy.
static const size_t H2_HEAD = 4096;      // bytes: exponent table | bound table | index scratch | from byte 1024: H2_NDYN dynamic slots (ints H2_DYN0 ..)
constexpr int H2_NDYN = 512;             // 64 blocks of 8: one block per timestep of the backward pass (bounds of its gradient operands), the last two for the whole-pass operands
static_assert(H2_DYN0 * 4 + H2_NDYN * 4 <= 4096, "dynamic slots inside the head");
extern "C" size_t vsr_h2_weight_bytes(const vsr_handle* h) {
    if (!h) return 0;
    const float* p[GEMM_NW]; size_t n[GEMM_NW];
    vsr_weights none;
    memset(&none, 0, sizeof(none));
    gemm_matrix_list(h->d, none, p, n);
    size_t tot = H2_HEAD;
    for (int i = 0; i < GEMM_NW; ++i) tot += ((n[i] + 7) & ~size_t(7)) * sizeof(float);
    tot += (((size_t)h->d.vocab_size * h->d.input_encoding_size + 7) & ~size_t(7)) * sizeof(float);      // the embedding table (an A operand: gemm_h2a.h)
    return tot + 256;
}
__global__ void k_h2_head_init(int* exps, unsigned* bounds, int* idx) {
    const int i = threadIdx.x;
    if (i < H2_NSLOT) {
        exps[i] = 0;
        bounds[i] = i == H2A_UNIT ? __float_as_uint(1.f) : 0u;
        idx[i] = i; idx[H2_NSLOT + i] = -1; idx[2 * H2_NSLOT + i] = i;       // k_h2_exps: slot i from bound i alone
    }
}
// exponents of the operands vsr_prepare*() measures: region rows (their max); the pooled descriptor (sum of <= R0 detection rows over a
// count >= 1, step :126-128: R0 x the detections' max - loose bounds cost nothing, fp16 subnormals are honoured); the attended vector
// (a convex combination of the sentinel and region rows, step :167-171): max(region max, sentinel bound)
// One 1024-thread block: it first folds the per-block maxima k_rowmask left (bm_regions, bm_det) into the two bounds (stored as the bit
// patterns of non-negative floats; a NaN counts as +inf).
__global__ __launch_bounds__(1024) void k_h2_prepare_exps(const float* __restrict__ bm_regions, long long n_regions, const float* __restrict__ bm_det,
                                                          long long n_det, unsigned* __restrict__ bounds, int R0, int* __restrict__ exps) {
    __shared__ float wm[2][16];
    const float r = block_max_1024(bm_regions, n_regions, wm[0]), dt = block_max_1024(bm_det, n_det, wm[1]);
    if (threadIdx.x != 0) return;
    bounds[H2A_REGION] = __float_as_uint(r);
    bounds[H2A_DET] = __float_as_uint(dt);
    const float sn = __uint_as_float(bounds[H2B_SENT]);
    exps[H2A_REGION] = h2_exp_of(r);
    exps[H2A_DET] = h2_exp_of(dt * (float)R0);
    exps[H2A_ATT] = h2_exp_of(fmaxf(r, sn));
}
// the launches of a refresh into the image buffer at `base`.  adam != null (vsr_adam_step): the optimizer's launch takes the place of the
// bound pass - it measures the tensors it has just written - and everything after it is the refresh's own tail
struct AdamLaunch { AdamMulti t; AdamHyper hy; };
static int h2_refresh_launches(vsr_handle* h, char* base, hipStream_t s, const AdamLaunch* adam) {
    const vsr_dims& d = h->d;
    const float* p[GEMM_NW]; size_t n[GEMM_NW];
    gemm_matrix_list(h->d, h->w, p, n);
    int* exps = reinterpret_cast<int*>(base);
    unsigned* bounds = reinterpret_cast<unsigned*>(base + 128);
    int* idx = reinterpret_cast<int*>(base + 256);          // 3 x H2_NSLOT ints of index lists for k_h2_exps
    hipLaunchKernelGGL(k_h2_head_init, dim3(1), dim3(64), 0, s, exps, bounds, idx);
    // bounds of the 14 matrices and of the embedding rows in one launch, the images in another (a training step refreshes them)
    static_assert(GEMM_NW + 1 <= H2_MT, "multi-tensor table");
    H2Multi mt;
    memset(&mt, 0, sizeof(mt));
    const long long ne = (long long)d.vocab_size * d.input_encoding_size;
    int blocks = 0;
    for (int i = 0; i <= GEMM_NW; ++i) {
        mt.src[i] = i < GEMM_NW ? p[i] : h->w.embed_weight;
        mt.n[i] = i < GEMM_NW ? (long long)n[i] : ne;
        mt.slot[i] = i < GEMM_NW ? i : (int)H2A_EMBED;
        mt.blk[i] = blocks;
        blocks += (int)std::max<long long>(1, std::min<long long>(256, cdiv(mt.n[i], 8192)));
    }
    mt.blk[GEMM_NW + 1] = blocks;
    mt.nt = GEMM_NW + 1;
    if (adam) hipLaunchKernelGGL(k_adam_multi, dim3(adam->t.blk[ADAM_NT]), dim3(256), 0, s, adam->t, adam->hy, bounds);
    else hipLaunchKernelGGL(k_absmax_multi, dim3(blocks), dim3(256), 0, s, mt, bounds);
    // |sentinel| = |s_fc s_t + b| <= max_d (sum_j |W_dj| + |b_d|) since |s_t| < 1                                   (step :155)
    hipLaunchKernelGGL(k_row_l1_max, dim3(cdiv(d.det_feat_size, L1MAX_ROWS)), dim3(256), 0, s, h->w.s_fc_weight, h->w.s_fc_bias, d.det_feat_size, d.rnn_size, bounds + H2B_SENT);
    hipLaunchKernelGGL(k_h2_exps, dim3(1), dim3(64), 0, s, bounds, idx, idx + H2_NSLOT, idx + 2 * H2_NSLOT, (int)H2A_REGION, exps);   // slots 0 .. 15
    h->img.clear_weights_h2();
    float* out = reinterpret_cast<float*>(base + H2_HEAD);
    H2Multi mc;
    memset(&mc, 0, sizeof(mc));
    long long off = 0;
    blocks = 0;
    for (int i = 0; i < GEMM_NW; ++i) {
        const size_t n8 = (n[i] + 7) & ~size_t(7);
        mc.src[i] = p[i]; mc.n[i] = (long long)n8; mc.dst_off[i] = off; mc.slot[i] = i; mc.blk[i] = blocks;
        blocks += cdiv((long long)n8, 8 * 256);
        h->img.add_weight_h2(p[i], n[i], out + off, i);
        off += (long long)n8;
    }
    {   // the embedding table: an A operand (gathered rows) of the all-DMA kernel, scaled by its own bound class
        const size_t n8 = ((size_t)ne + 7) & ~size_t(7);
        mc.src[GEMM_NW] = h->w.embed_weight; mc.n[GEMM_NW] = (long long)n8; mc.dst_off[GEMM_NW] = off; mc.slot[GEMM_NW] = H2A_EMBED; mc.blk[GEMM_NW] = blocks;
        blocks += cdiv((long long)n8, 8 * 256);
        h->img.add_weight_h2(h->w.embed_weight, (size_t)ne, out + off, H2A_EMBED);
        off += (long long)n8;
    }
    mc.blk[GEMM_NW + 1] = blocks;
    mc.nt = GEMM_NW + 1;
    hipLaunchKernelGGL(k_f32_to_h2_multi, dim3(blocks), dim3(256), 0, s, mc, reinterpret_cast<uint32_t*>(out), exps);
    LAUNCHCHK();
    h->h2_exps = exps; h->h2_bounds = bounds;
    return 0;
}
extern "C" int vsr_refresh_h2_weights(vsr_handle* h, void* buffer, size_t bytes, void* stream) {
    if (!h) return fail("vsr_refresh_h2_weights: null handle");
    if (!buffer) {                                          // back to f32x3 for every launch
        if (h->h2_on) void_derived(h, VOID_FLAVOUR);
        h->h2_on = false;
        h->img.clear_h2();
        return 0;
    }
    if (!h->bound) return fail("vsr_refresh_h2_weights: weights not bound");
    const vsr_dims& d = h->d;
    if (d.det_feat_size % 8 || d.input_encoding_size % 8 || d.rnn_size % 8 || d.att_size % 8)
        return fail("vsr_refresh_h2_weights: the f16x2 flavour needs det_feat_size, input_encoding_size, rnn_size and att_size to be "
                    "multiples of 8 (whole 8-element groups of the fp16-pair images); got %d %d %d %d", d.det_feat_size, d.input_encoding_size, d.rnn_size, d.att_size);
    if (bytes < vsr_h2_weight_bytes(h)) return fail("vsr_refresh_h2_weights: buffer too small");
    if (reinterpret_cast<uintptr_t>(buffer) & 255) return fail("vsr_refresh_h2_weights: buffer must be 256-byte aligned");
    if (h2_refresh_launches(h, reinterpret_cast<char*>(buffer), (hipStream_t)stream, nullptr)) return 1;
    void_derived(h, h->h2_on ? VOID_REFRESH : VOID_FLAVOUR);      // (the bounds of the region / detection operands are measured by vsr_prepare*())
    h->h2_on = true;
    return 0;
}

// ---- the optimizer step (optim_kernels.h): Adam on the 28 bound tensors and, in the same pass, what the flavour derives from them
extern "C" int vsr_adam_step(vsr_handle* h, const vsr_weights* params, const vsr_weights* grads, const vsr_weights* exp_avg,
                             const vsr_weights* exp_avg_sq, const vsr_adam_args* a, void* stream) {
    if (!h || !params || !grads || !exp_avg || !exp_avg_sq || !a) return fail("vsr_adam_step: null argument");
    if (!h->bound) return fail("vsr_adam_step: weights not bound");
    if (memcmp(params, &h->w, sizeof(vsr_weights)) != 0)
        return fail("vsr_adam_step: params are not the 28 tensors bound to this handle (vsr_bind_weights): the step writes through the bound pointers and rebuilds what the handle derives from them");
    if (a->step < 1) return fail("vsr_adam_step: step is the 1-based count of this step, got %d", a->step);
    if (!(a->lr >= 0) || !(a->eps >= 0) || !(a->weight_decay >= 0) || !(a->beta1 >= 0 && a->beta1 < 1) || !(a->beta2 >= 0 && a->beta2 < 1))
        return fail("vsr_adam_step: lr, eps, weight_decay must be >= 0 and the betas in [0, 1)");
    float* const* P = reinterpret_cast<float* const*>(params);
    const float* const* G = reinterpret_cast<const float* const*>(grads);
    float* const* M = reinterpret_cast<float* const*>(exp_avg);
    float* const* V = reinterpret_cast<float* const*>(exp_avg_sq);
    size_t n[ADAM_NT];
    weight_sizes(h->d, n);
    bool matrix[ADAM_NT] = {};           // one of the 14 matrices the GEMMs multiply by
    for (int j = 0; j < GEMM_NW; ++j) matrix[GEMM_MATRIX[j]] = true;
    if (!h->adam_blocks) {               // one resident round of workgroups: a second, partial round would be the tail of the launch
        int per_cu = 0, dev = 0, cus = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_adam_multi, 256, 0));
        HIPCHK(hipGetDevice(&dev));
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        h->adam_blocks = std::max(ADAM_NT, std::min(ADAM_MAX_BLOCKS, per_cu * cus));
    }
    AdamLaunch L;
    memset(&L, 0, sizeof(L));
    size_t total = 0;
    for (int i = 0; i < ADAM_NT; ++i) total += n[i];
    int blocks = 0;
    for (int i = 0; i < ADAM_NT; ++i) {
        if (!M[i] || !V[i]) return fail("vsr_adam_step: moment pointer %d is null", i);
        L.t.p[i] = P[i]; L.t.g[i] = G[i]; L.t.m[i] = M[i]; L.t.v[i] = V[i]; L.t.n[i] = (long long)n[i];
        L.t.slot[i] = -1;
        // what the flavour derives from tensor i: the refreshes registered it (params are the bound tensors; a bind would have switched the flavour off)
        const ImageRange* im = h->img.weight_at(P[i]);
        if (h->h2_on && im && im->h2) L.t.slot[i] = im->slot;       // (a matrix's position in gemm_matrix_list, or H2A_EMBED)
        if (h->bf16_on && matrix[i]) {
            if (!im || !im->b16) return fail("vsr_adam_step: internal: the bf16 copy of tensor %d of vsr_weights (a GEMM matrix) is not registered", i);
            L.t.b16[i] = const_cast<uint16_t*>(im->b16);
        }
        // blocks by the tensor's share of the elements, at least one, no more than it has 16-byte groups for; grid-stride covers the rest
        L.t.blk[i] = blocks;
        const long long share = (long long)((double)n[i] / (double)total * h->adam_blocks);
        blocks += (int)std::max<long long>(1, std::min<long long>(share, cdiv((long long)n[i], 4 * 256)));
    }
    L.t.blk[ADAM_NT] = blocks;
    // torch's: both corrections in double, handed to the kernel as fp32; the step size a double quotient rounded once
    const float bc1 = (float)(1.0 - std::pow(a->beta1, (double)a->step));
    L.hy.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(a->beta2, (double)a->step));
    L.hy.step_size = (float)(a->lr / (double)bc1);
    L.hy.beta1 = a->beta1; L.hy.beta2 = a->beta2; L.hy.eps = a->eps; L.hy.wd = a->weight_decay;
    hipStream_t s = (hipStream_t)stream;
    if (h->h2_on) {
        if (h2_refresh_launches(h, reinterpret_cast<char*>(h->h2_exps), s, &L)) return 1;      // (the exponent table is the head of the image buffer)
    } else {
        hipLaunchKernelGGL(k_adam_multi, dim3(blocks), dim3(256), 0, s, L.t, L.hy, (unsigned*)nullptr);
        LAUNCHCHK();
    }
    // what a refresh voids (vsr_bind_weights has the rules); with no flavour product the fp32 kernels read the weights live: only the
    // decode cache is of the old weights
    if (h->has_weight_images()) void_derived(h, VOID_REFRESH);
    else set_xproj(h, nullptr);
    return 0;
}

// fp32 GEMM flavour: 0 = exact k-ordered fma chain (v_mfma_f32_32x32x2_f32) for every launch,
// 1 (default since round 3) = "f32x3" for launches of more than 192 rows: each fp32 operand split into three bf16 terms, six bf16
// MFMAs per product, fp32 accumulation (gemm_f32x3.h).  Every reference fixture is checked in both (tests/conftest.py).
extern "C" int vsr_set_gemm_mode(vsr_handle* h, int32_t mode) {
    if (!h) return fail("vsr_set_gemm_mode: null handle");
    if (mode != 0 && mode != 1) return fail("vsr_set_gemm_mode: mode %d not in {0, 1}", mode);
    if (h->x3_on != (mode == 1)) void_derived(h, VOID_FLAVOUR);
    h->x3_on = mode == 1;
    return 0;
}

extern "C" int vsr_set_valid_rows_bound(vsr_handle* h, int64_t max_valid_rows) {
    if (!h) return fail("vsr_set_valid_rows_bound: null handle");
    if (max_valid_rows < 0) return fail("vsr_set_valid_rows_bound: negative bound");
    h->rows_bound = max_valid_rows;
    return 0;
}

extern "C" int vsr_set_verb_table(vsr_handle* h, const int32_t* row_ptr, const int32_t* vocab_ids, int32_t n_verbs) {
    if (!h) return fail("vsr_set_verb_table: null handle");
    h->vt_ptr = row_ptr;
    h->vt_ids = vocab_ids;
    h->n_verbs = row_ptr ? n_verbs : 0;
    return 0;
}

extern "C" size_t vsr_workspace_bytes(const vsr_handle* h, int32_t B, int32_t R0, int32_t L, int32_t R, int32_t beam) {
    if (!h || B <= 0 || L <= 0 || R <= 0 || beam <= 0) return 0;
    Ctx c;
    c.B = B; c.R0 = R0; c.L = L; c.R = R; c.beam = beam; c.Mmax = B * beam;
    return carve(h, c, nullptr);
}

extern "C" size_t vsr_workspace_bytes_indexed(const vsr_handle* h, int32_t B, int32_t R0, int32_t n_img, int32_t Rb, int32_t L,
                                              int32_t R, int32_t beam) {
    if (!h || B <= 0 || L <= 0 || R <= 0 || beam <= 0 || n_img <= 0 || Rb <= 0) return 0;
    Ctx c;
    c.B = B; c.R0 = R0; c.L = L; c.R = R; c.beam = beam; c.Mmax = B * beam; c.n_img = n_img; c.Rb = Rb;
    return carve(h, c, nullptr);
}

// ---------------------------------------------------------------------------------------------- prepare
// Both region formats.  Dense: regions = (B, L, R, D).  Index lists: regions = feature bank (n_img, Rb, D),
// slot_idx = (B, L, R) rows of image row_img[b]'s bank (-1 = padding), det = (n_img, R0, D).
static int prepare_impl(vsr_handle* h, const float* det, int B, int R0, const float* regions, int n_img, int Rb,
                        const int* row_img, const int* slot_idx, int L, int R, int beam, void* workspace,
                        size_t workspace_bytes, void* stream, const char* who) {
    if (!h || !h->bound) return fail("%s: weights not bound", who);
    if (!det || !regions || !workspace) return fail("%s: null tensor", who);
    if (B <= 0 || R0 <= 0 || L <= 0 || R <= 0) return fail("%s: empty batch / regions", who);
    if (beam < 1 || beam > VSR_MAX_BEAM) return fail("%s: beam size %d not in [1, %d]", who, beam, VSR_MAX_BEAM);
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail("%s: workspace must be 16-byte aligned", who);
    const bool indexed = slot_idx != nullptr;
    if (indexed && (n_img <= 0 || Rb <= 0)) return fail("%s: empty feature bank", who);
    hipStream_t s = (hipStream_t)stream;
    const vsr_dims& d = h->d;
    const vsr_weights& w = h->w;
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size;
    Ctx& c = h->c;
    c.B = B; c.R0 = R0; c.L = L; c.R = R; c.beam = beam; c.Mmax = B * beam;
    c.n_img = indexed ? n_img : 0; c.Rb = indexed ? Rb : 0;
    c.det = det; c.regions = regions;
    const size_t need = carve(h, c, reinterpret_cast<char*>(workspace));
    if (need > workspace_bytes) return fail("%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    c.ridx = c.ridx_buf;
    c.rows_are_images = indexed && row_img == nullptr && n_img == B;
    h->prepared = false;
    // h->c is rewritten: the CURRENT saved forward (if any) goes with it unless it lives in another workspace - forwards saved in
    // workspaces this call does not touch stay differentiable (vsr_train_select)
    invalidate_train_ctx(h->tc);
    drop_saved_forwards_in(h->saved, workspace, need);
    h->ws_lo = reinterpret_cast<const char*>(workspace); h->ws_bytes = need;

    // region-row masks, then the list of NON-PADDING rows att_va has to run over (att_va(0) = 0).  Their count has to
    // reach the host to size that launch: the one place where this library waits, and it waits for an EVENT behind the
    // copy, with the pooled descriptor and its projections queued after it, so the GPU has work while the host wakes up.
    // (The index-list format reports its out-of-range count through the same read-back.)
    const long long rows = (long long)B * L * R;                         // slot entries
    const long long prows = indexed ? (long long)n_img * Rb : rows;      // rows att_va runs over
    // f16x2 flavour: the bounds of the region / detection operands are measured in the passes that read them anyway (per-block maxima
    // into the idle GEMM scratch, folded by one block); exponents of the region rows, the pooled descriptor and the attended vector
    const bool h2b = h->measures_h2_bounds();         // (h2_on alone, unlike the routing: needed under bf16_on too - GemmState says why)
    float* bm_regions = h2b ? c.scratch : nullptr;
    float* bm_det = h2b ? c.scratch + cdiv(prows, 4) : nullptr;
    if (h2b && (size_t)(cdiv(prows, 4) + cdiv((long long)(indexed ? n_img : B) * R0, 4)) > c.scratch_floats) return fail("%s: scratch too small for the operand bounds", who);
    // one launch masks the region rows and the detection rows (the pooled descriptor's, below) and clears the device counters:
    // [0] row count, [1] bad slot indices, [2] bad word / slot / verb ids, [3] rows beyond a caller's bound
    const long long drows = (long long)(indexed ? n_img : B) * R0;
    {
        RowMaskArgs a;
        a.X[0] = regions; a.rows[0] = prows; a.mask[0] = c.bmask; a.blockmax[0] = bm_regions;
        a.X[1] = det; a.rows[1] = drows; a.mask[1] = c.dmask; a.blockmax[1] = bm_det;
        a.nblk0 = (int)cdiv(prows, 4); a.zero4 = c.nvalid_dev;
        hipLaunchKernelGGL(k_rowmask, dim3(cdiv(prows, 4) + cdiv(drows, 4)), dim3(256), 0, s, a, D);
    }
    if (indexed) {
        hipLaunchKernelGGL(k_index_rows, dim3(cdiv(rows, 256)), dim3(256), 0, s, slot_idx, row_img, c.bmask, B, L * R, Rb, n_img,
                           c.ridx_buf, c.rmask, c.nvalid_dev + 1);
    }
    {
        const int nb = (int)cdiv(prows, 256);
        hipLaunchKernelGGL(k_compact_count, dim3(nb), dim3(256), 0, s, c.bmask, (int)prows, c.bcount);
        hipLaunchKernelGGL(k_compact_write, dim3(nb), dim3(256), 0, s, c.bmask, (int)prows, c.bcount, c.vlist, c.nvalid_dev);
    }
    LAUNCHCHK();
    // A caller that knows an upper bound on the non-padding rows (vsr_set_valid_rows_bound: the eval script builds its region tensors on
    // the host and has the count for free) gets NO read-back: the list is padded to the bound on the device, the projection is sized by it.
    const long long bound = h->rows_bound > 0 ? std::min(h->rows_bound, prows) : 0;
    int* back = nullptr;
    if (bound > 0) {
        hipLaunchKernelGGL(k_pad_row_list, dim3(cdiv(bound, 256)), dim3(256), 0, s, c.vlist, c.nvalid_dev, (int)bound);
        LAUNCHCHK();
    } else {
        if (!h->host_back) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->host_back), 2 * sizeof(int), hipHostMallocDefault));
        back = h->host_back;                                             // pinned: the copy does not block this thread
        HIPCHK(hipMemcpyAsync(back, c.nvalid_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        if (!h->ev_count) HIPCHK(hipEventCreateWithFlags(&h->ev_count, hipEventDisableTiming));
        HIPCHK(hipEventRecord(h->ev_count, s));
    }

    // pooled descriptor
    if (h2b)
        hipLaunchKernelGGL(k_h2_prepare_exps, dim3(1), dim3(1024), 0, s, bm_regions, (long long)cdiv(prows, 4), bm_det, (long long)cdiv(drows, 4),
                           h->h2_bounds, R0, h->h2_exps);
    // (one wave per block: B x D / 256 blocks, enough of them to fill the chip at 100 images)
    hipLaunchKernelGGL(k_pool, dim3(B, cdiv(D, 256)), dim3(64), 0, s, det, indexed ? row_img : nullptr, c.dmask, R0, D, c.vbar);
    LAUNCHCHK();

    // hoisted vbar projections: columns [voff, voff + D) of the LSTM1 / gate input weights
    const SlabArea scratch{c.scratch, c.scratch_floats};
    SlabPlan pl;
    {
        GemmBuilder g;
        add_vproj(g, d, w, c.vbar, B);
        g.finish(h);
        if (place(g, B, lstm1_slabs(d), {scratch}, pl, "vproj")) return 1;
        if (g.launch(s, h, &h->prof)) return fail("vproj gemm launch failed");
        const SlabView& v = pl.v[0];
        hipLaunchKernelGGL(k_vproj_finish, dim3(cdiv(v.stride, 256)), dim3(256), 0, s, v.base, v.n, v.stride, B, H,
                           w.lstm1_bias_ih, w.lstm1_bias_hh, w.W1_is_bias, w.W1_hs_bias, w.W1_ig_bias, w.W1_hg_bias, c.vproj);
        LAUNCHCHK();
    }
    if (d.img_second_lstm) {
        GemmBuilder g;
        add_vproj2(g, d, w, c.vbar, B);
        g.finish(h);
        if (place(g, B, vproj2_slabs(d), {scratch}, pl, "vproj2")) return 1;
        if (g.launch(s, h, &h->prof)) return fail("vproj2 gemm launch failed");
        slab_sum_to(s, pl.v[0].base, pl.v[0].n, B, 4 * H, c.vproj2);
        LAUNCHCHK();
    }
    c.bounded = bound > 0;
    if (bound > 0) {
        c.nvalid = (int)bound;         // (bad slot indices of the index-list format join the bad-id count: vsr_bad_ids)
        // a bound that is too small: the rows vlist[bound .. n) get no projection.  Their P rows are ZEROED (att_va = 0, a defined result)
        // instead of keeping whatever the workspace held, and their number is in vsr_bad_ids()'s count
        if (prows > bound)
            hipLaunchKernelGGL(k_zero_rows_beyond, dim3((unsigned)std::min<long long>(prows - bound, 2048)), dim3(128), 0, s, c.vlist, c.nvalid_dev, (int)bound, A, c.P);
    } else {
        HIPCHK(hipEventSynchronize(h->ev_count));
        c.nvalid = back[0];
        if (indexed && back[1] != 0) return fail("%s: %d slot entries index outside the feature bank [-1, %d) or name an image outside [0, %d)", who, back[1], Rb, n_img);
    }
    if (c.nvalid > 0) {
        GemmBuilder g;
        add_att_va(g, d, w, regions, c.vlist, c.nvalid);
        g.finish(h);
        if (place_slabs(g.a, c.nvalid, att_va_slabs(d), &scratch, 1, pl)) return fail("%s: att_va slabs over %d rows: %s", who, c.nvalid, pl.err);
        if (g.launch(s, h, &h->prof)) return fail("att_va gemm launch failed");
        const SlabView& v = pl.v[0];
        hipLaunchKernelGGL(k_slab_reduce_scatter, dim3(cdiv(v.stride, 4 * 256)), dim3(256), 0, s, v.base, v.n, v.stride, c.nvalid, A, c.vlist, c.P,
                           bound > 0 ? c.nvalid_dev : (const int*)nullptr);
        LAUNCHCHK();
    }
    h->prepared = true;
    return 0;
}

extern "C" int vsr_prepare(vsr_handle* h, const float* det, int32_t B, int32_t R0, const float* regions, int32_t L,
                           int32_t R, int32_t beam, void* workspace, size_t workspace_bytes, void* stream) {
    return prepare_impl(h, det, B, R0, regions, 0, 0, nullptr, nullptr, L, R, beam, workspace, workspace_bytes, stream, "vsr_prepare");
}

extern "C" int vsr_prepare_indexed(vsr_handle* h, const float* det, int32_t n_img, int32_t R0, const float* bank, int32_t Rb,
                                   const int32_t* row_img, int32_t B, const int32_t* slot_idx, int32_t L, int32_t R,
                                   int32_t beam, void* workspace, size_t workspace_bytes, void* stream) {
    if (!slot_idx) return fail("vsr_prepare_indexed: null slot index list");
    return prepare_impl(h, det, B, R0, bank, n_img, Rb, row_img, slot_idx, L, R, beam, workspace, workspace_bytes, stream,
                        "vsr_prepare_indexed");
}

extern "C" int vsr_row_mask(const float* rows, int64_t n_rows, int32_t D, float* mask, void* stream) {
    if (!rows || !mask || n_rows <= 0 || D <= 0 || (D & 3)) return fail("vsr_row_mask: bad arguments");
    RowMaskArgs a;
    memset(&a, 0, sizeof(a));
    a.X[0] = rows; a.rows[0] = (long long)n_rows; a.mask[0] = mask; a.nblk0 = (int)cdiv(n_rows, 4);
    hipLaunchKernelGGL(k_rowmask, dim3(cdiv(n_rows, 4)), dim3(256), 0, (hipStream_t)stream, a, D);
    LAUNCHCHK();
    return 0;
}

extern "C" int vsr_reorder_slots(const int32_t* slot_idx, const int32_t* rank, const float* verbs, const float* bank_mask,
                                 const int32_t* row_img, int32_t N, int32_t L, int32_t R, int32_t Rb, int32_t* slot_out,
                                 float* verbs_out, void* stream) {
    if (!slot_idx || !rank || !slot_out || N <= 0 || L <= 0 || R <= 0 || Rb <= 0) return fail("vsr_reorder_slots: bad arguments");
    if (verbs && !verbs_out) return fail("vsr_reorder_slots: verbs given without an output");
    hipLaunchKernelGGL(k_reorder_slots, dim3(N), dim3(64), (size_t)L * sizeof(int), (hipStream_t)stream, slot_idx, rank, verbs,
                       bank_mask, row_img, L, R, Rb, slot_out, verbs_out);
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- one timestep
struct StepIO {
    int t = 0, M = 0, rpi = 1, cur = 0;
    const int* parent = nullptr;       // state-row gather (beam parents) or null
    const int* word_prev = nullptr;    // (M) int32
    const int* slot = nullptr;         // (M) int32 or null -> fixed_slot
    int fixed_slot = 0;
    int vmode = VM_TOPK, K = 1;
    int gs = 0;                        // > 0: greedy baseline rows in a sampling launch (kernels.h, k_vocab): rows with row % gs == 0
    float* full_out = nullptr; long long full_stride = 0;
    const int* forced = nullptr;
    uint64_t seed = 0;
    const float* verbs = nullptr; int gt = 0;
    float* lg_out = nullptr; long long lg_stride = 2;
    float* alpha_out = nullptr;
    bool s1_from_prev = false;   // this step's LSTM1 sums are already in c.pre1 (computed over the parent rows)
    // the selection of the PREVIOUS step, still to be made: it rides in this step's LSTM1 kernel (k_select_lstm1_x2 / k_select_simple_lstm1;
    // only with s1_from_prev).  sel_images: images of the beam selection (its parents are sel_beam->cb rows per image).
    const SelBeamArgs* sel_beam = nullptr;
    const SelSimpleArgs* sel_simple = nullptr;
    bool s1_for_next = false;    // compute the next step's LSTM1 sums together with this step's vocabulary GEMM
};

// Workgroups per row of k_attend.  Launches of <= 128 rows: two workgroups per row (each forms half of the attended vector's columns): every
// row's ~370 KB then come in through two CUs' ingest instead of one while the other half of the chip idles (k_attend, nparts; VSR_ATTEND_PARTS=1: off)
static int attend_parts(const vsr_handle* h, int M) {
    const int np = h->attend_parts;
    return (np > 1 && M * np <= h->attend_limit && h->d.det_feat_size % (4 * np) == 0) ? np : 1;
}
// ... and of k_attend_bwd (NT threads): a part also takes A / parts of the A columns, and its threads are those columns x whole row groups
static int attend_bwd_parts(const vsr_handle* h, int M, int NT) {
    const int np = attend_parts(h, M), A = h->d.att_size;
    return (np > 1 && A % np == 0 && NT % (A / np) == 0) ? np : 1;
}
static void launch_attend(vsr_handle* h, hipStream_t s, const Gate2Args& g2, int M, int rpi, const int* slot, int fixed_slot, const float* hA,
                          const float* sa, const float* sent, float* att, float* alpha_out, uint16_t* att16, const int* att_exp) {
    const Ctx& c = h->c;
    const int A = h->d.att_size, D = h->d.det_feat_size, np = attend_parts(h, M);
    const size_t smem = (size_t)(2 * A + D + c.R + 1 + 8 + 2 * c.R) * sizeof(float);      // hA | sa | sentinel | z | red | region rows | region mask
    auto go = [&](auto NT) {
        hipLaunchKernelGGL(k_attend<decltype(NT)::value>, dim3(cdiv(M * np, 8) * 8), dim3(decltype(NT)::value), smem, s, g2, hA, sa, sent, c.P, c.regions,
                           c.rmask, c.ridx, slot, fixed_slot, rpi, M, c.L, c.R, A, D, h->w.att_a_weight, h->w.att_s_weight, att, c.zsum, alpha_out, att16, att_exp, np);
    };
    if (D >= 2048) go(std::integral_constant<int, 512>{}); else go(std::integral_constant<int, 256>{});
}
// k_vocab over the io.M rows of `logits` (ns slabs): K = io.K exactly (fewer selection rounds than rounding up to a power of two); 512
// threads per row from V = 4096 up
static void launch_vocab(vsr_handle* h, hipStream_t s, const StepIO& io, const float* logits, int ns, long long stride, const GateLogitArgs& gate) {
    const Ctx& c = h->c;
    const int V = h->d.vocab_size;
    const VocabLaunch vl = vocab_launch_rule(V);             // threads per row, combined logits row staged in LDS or not (kernels.h)
    with_const_1to8(io.K, [&](auto KK) {
        auto go = [&](auto NT) {
            hipLaunchKernelGGL((k_vocab<decltype(KK)::value, decltype(NT)::value>), dim3(io.M), dim3(decltype(NT)::value), vl.lds_bytes, s, logits, ns, stride,
                               h->w.out_fc_bias, io.M, V, io.vmode, c.top_v, c.top_i, io.full_out, io.full_stride, io.forced, io.seed, (uint32_t)io.t, io.verbs,
                               io.slot, io.rpi, c.L, io.gt, h->vt_ptr, h->vt_ids, h->n_verbs, vl.lds_row, gate, c.nvalid_dev + 2, io.gs);
        };
        if (vl.nt == 512) go(std::integral_constant<int, 512>{}); else go(std::integral_constant<int, 256>{});
    });
}

static int run_step(vsr_handle* h, const StepIO& io, hipStream_t s) {
    const vsr_dims& d = h->d;
    const vsr_weights& w = h->w;
    Ctx& c = h->c;
    const int H = d.rnn_size, A = d.att_size;
    const int M = io.M;
    float* const* so = c.st[io.cur];          // old state
    float* const* sn = c.st[io.cur ^ 1];      // new state
    float *c1o = so[1], *c2o = so[3];
    float *h1n = sn[0], *c1n = sn[1], *h2n = sn[2], *c2n = sn[3];
    // bf16 images of the A operands (bf16 mode): the producers below write them, the GEMM segments name them
    // ... or fp16-pair images (f16x2 flavour, gemm_h2a.h): isc = the scale of the unit-bounded ones (2^15), the attended vector's from the table
    const bool sh2 = h->writes_h2_a_images();         // (also with VSR_GEMM_TILE forced, when no launch reads them: not needed, kept)
    const bool sh = (h->bf16() && h->bf16_a16) || sh2;
    const float isc = sh2 ? 32768.f : 0.f;
    const int* att_exp = sh2 ? h->h2_exps + H2A_ATT : nullptr;
    const bool sh_old = sh && c.st16_ok[io.cur];
    uint16_t *h1n16 = sh ? c.st16[io.cur ^ 1][0] : nullptr, *h2n16 = sh ? c.st16[io.cur ^ 1][1] : nullptr;
    uint16_t *s_t16 = sh ? c.s_t16 : nullptr, *g_t16 = sh ? c.g_t16 : nullptr, *att16 = sh ? c.att16 : nullptr;
    StepOperands o;                           // what the step's GEMMs multiply (step_gemms.h)
    o.M = M; o.parent = io.parent; o.x = w.embed_weight; o.word = io.word_prev;
    o.h1_old = so[0]; o.h2_old = so[2]; o.h1_new = h1n; o.h2_new = h2n; o.s_t = c.s_t; o.g_t = c.g_t; o.att = c.att;
    o.h1_old16 = sh_old ? c.st16[io.cur][0] : nullptr; o.h2_old16 = sh_old ? c.st16[io.cur][1] : nullptr;
    o.h1_new16 = h1n16; o.h2_new16 = h2n16; o.s_t16 = s_t16; o.g_t16 = g_t16; o.att16 = att16;
    const SlabArea scratch{c.scratch, c.scratch_floats}, ga{c.ga_slabs, c.ga_floats}, pre1{c.pre1, c.pre1_floats};
    SlabPlan pl;                              // the slab groups of the launch in hand (step_gemms.h)

    // ---- S1
    if (io.s1_from_prev && io.sel_beam) {
        const SelBeamArgs& sb = *io.sel_beam;
        // two units per lane, 8-byte accesses: H % 4 == 0 (vsr_create), the workspace is 16-byte aligned and carved at 256 bytes, and
        // vsr_beam leaves a selection pending only over a decode cache at an 8-byte aligned address (xproj_al8)
        const int nslice = cdiv(H, 2 * SL_UB);
        with_const_1to8(sb.beam, [&](auto KK) {
            constexpr int K = decltype(KK)::value;
            hipLaunchKernelGGL(k_select_lstm1_x2<K>, dim3(sb.B * nslice), dim3((K + 1) * 64), 0, s, sb, c.pre1, c.pre1_ns, c.pre1_stride,
                               c.vproj, c1o, H, nslice, h1n, c1n, c.s_t, c.gpre, h->xproj, c.pre1_nblk, h1n16, s_t16, isc, c.pre1_skip5);
        });
    } else if (io.s1_from_prev && io.sel_simple) {
        hipLaunchKernelGGL(k_select_simple_lstm1, dim3(cdiv((long long)M * H, 256)), dim3(256), 0, s, *io.sel_simple, c.pre1, c.pre1_ns, c.pre1_stride,
                           c.vproj, c1o, M, H, h1n, c1n, c.s_t, c.gpre, h->xproj, c.pre1_nblk, h1n16, s_t16, isc, c.pre1_skip5, io.rpi);
    } else if (io.s1_from_prev) {
        hipLaunchKernelGGL(k_lstm1, dim3(cdiv((long long)M * H, 256)), dim3(256), 0, s, c.pre1, c.pre1_ns, c.pre1_stride, c.vproj, io.rpi,
                           io.parent, c1o, M, H, h1n, c1n, c.s_t, c.gpre, h->xproj, io.word_prev, c.pre1_nblk, 1, h1n16, s_t16, isc, c.pre1_skip5);
    } else {
        // the state parts from step 1 on; the embedding part unless it comes from the decode cache
        // (nothing to multiply at step 0 over a decode cache: no launch, and a view without slabs)
        GemmBuilder g;
        const int nblk = add_lstm1(g, d, w, o, (io.t > 0 ? L1_H2 | L1_H1 : 0) | (h->xproj ? 0 : L1_X));
        if (g.a.nprob > 0) g.finish(h);
        if (place(g, M, lstm1_slabs(d, g.a.nprob), {scratch}, pl, "S1")) return 1;
        if (g.a.nprob > 0 && g.launch(s, h, &h->prof)) return fail("S1 gemm launch failed");
        const SlabView& v = pl.v[0];
        hipLaunchKernelGGL(k_lstm1, dim3(cdiv((long long)M * H, 256)), dim3(256), 0, s, v.base, v.n, v.stride, c.vproj, io.rpi,
                           io.parent, c1o, M, H, h1n, c1n, c.s_t, c.gpre, h->xproj, io.word_prev, nblk, 0, h1n16, s_t16, isc);
    }
    // ---- S2
    {
        GemmBuilder g;
        add_s2(g, d, w, o);
        g.finish(h);
        if (place(g, M, s2_slabs(d), {scratch}, pl, "S2")) return 1;
        if (g.launch(s, h, &h->prof)) return fail("S2 gemm launch failed");
        // k_gate2's work (g_t, hA, s_a, sentinel from the S2 slabs) is done by the attention kernel's row blocks themselves
        const SlabView &va = pl.v[0], &vb = pl.v[1];
        const Gate2Args g2{va.base, vb.base, va.n, va.stride, vb.stride, c.gpre, c1n, w.s_fc_bias, H, c.g_t, c.hA, g_t16, isc};
        launch_attend(h, s, g2, M, io.rpi, io.slot, io.fixed_slot, c.hA, c.sa, c.sent, c.att, io.alpha_out, att16, att_exp);
    }
    // ---- S5 and S6 are planned together, before either is launched.
    // S6 = the vocabulary problem + (s1_for_next) the LSTM1 / gate sums of step t+1 over THIS step's rows: they depend on (h2, h1) only (the
    // word enters through the decode cache, the beam re-indexing through k_lstm1's parent gather), so they ride in the same launch as the
    // vocabulary projection: 3 GEMM launches per timestep instead of 4, and a longer stream-K range per workgroup.
    // Round 6 (split_pre1): the h1 part of those sums (h1_new . [W_hh1 ; W1_hs]) rides in S5 instead: S5's k-aligned plan left 56 of 256 CUs
    // idle (64 LSTM2 tiles x 3 pieces + 8 att_ga tiles), and without these K = H tiles the vocabulary launch is UNIFORM (every tile K = H:
    // one k-aligned piece per tile, no slabs at all).  Measured on the beam-5 shapes (tools/gemm_bench GEMM_REPACK=1, profiles/r06_e_*):
    // 148-153 -> 133 us for the two launches.  The composition, its slab counts and the re-plan when the two parts would not fit pre1's
    // 8 slabs: plan_s56 (step_gemms.h).
    Step56 p56;
    plan_s56(h, d, w, o, io.t > 0, io.s1_for_next, io.s1_for_next && h->split_pre1 && d.h2_first_lstm, p56);
    // ---- S5
    GateLogitArgs gate_args;
    SlabView h1_part;                         // the h1 part of the next step's LSTM1 sums in pre1 (no slabs without the split)
    {
        GemmBuilder& g = p56.g5;
        if (place(g, M, s5_decode_slabs(d, g.a.nprob, p56.ns_h1), {scratch, ga, pre1}, pl, "S5")) return 1;
        const SlabView &v = pl.v[0], &vg = pl.v[1];
        h1_part = pl.v[2];
        c.pre1_skip5 = h1_part.n;
        if (g.launch(s, h, &h->prof)) return fail("S5 gemm launch failed");
        hipLaunchKernelGGL(k_lstm2, dim3(cdiv((long long)M * H, 256)), dim3(256), 0, s, v.base, v.n, v.stride, w.lstm2_bias_ih,
                           w.lstm2_bias_hh, d.img_second_lstm ? c.vproj2 : nullptr, io.rpi, io.parent, c2o, M, H, h2n, c2n, h2n16, isc);
        // the gate logits (z_g, log_softmax([z_g, zsum]), step :185-188) are nobody's input before the selection: the
        // vocabulary kernel's row blocks compute them on the side instead of a launch of their own
        // (att_ga has a quarter of LSTM2's K: fewer stream-K pieces per tile, fewer slabs for the gate logits to add)
        gate_args = GateLogitArgs{vg.base, vg.n, vg.stride, c.hA, w.att_g_weight, c.zsum, io.verbs, io.slot, io.rpi, c.L, M, A,
                                  io.lg_out, io.lg_stride};
    }
    // ---- S6
    {
        GemmBuilder& g = p56.g6;
        c.pre1_ns = (g.a.nprob > 1 ? p56.ns_pre1 : g.a.nslab) + c.pre1_skip5; c.pre1_nblk = p56.nblk6;
        if (c.pre1_ns > GEMM_MAX_SLABS) return fail("S6: the LSTM1 sums of the next step would need %d slabs (%d fit)", c.pre1_ns, GEMM_MAX_SLABS);
        // the vocabulary tiles (K = H) are cut into fewer pieces than the LSTM1 tiles (K = 2 H) they share the launch with: k_vocab
        // adds only the slabs they wrote (60 -> 40 MB of logits per beam-5 step); the LSTM1 sums go behind the slabs the S5 launch
        // above wrote the h1 part into
        if (place(g, M, s6_slabs(d, g.a.nprob, p56.ns_pre1), {scratch, area_behind(pre1, h1_part)}, pl, "S6")) return 1;
        c.pre1_stride = pl.v[1].stride;
        if (g.launch(s, h, &h->prof)) return fail("S6 gemm launch failed");
        launch_vocab(h, s, io, pl.v[0].base, pl.v[0].n, pl.v[0].stride, gate_args);
    }
    c.st16_ok[io.cur ^ 1] = sh;               // the new state's bf16 images exist iff this step wrote them
    LAUNCHCHK();
    return 0;
}

static int check_ready(vsr_handle* h, const char* who) {
    if (!h) return fail("%s: null handle", who);
    if (!h->bound) return fail("%s: weights not bound", who);
    if (!h->prepared) return fail("%s: vsr_prepare() has not been called", who);
    return 0;
}

static int zero_state(vsr_handle* h, int M, hipStream_t s) {
    Ctx& c = h->c;
    const size_t n = (size_t)M * h->d.rnn_size * sizeof(float);
    // the four state arrays of buffer 0 are consecutive in the workspace (carve): one range; the images of the zero h1 / h2 (bf16 or
    // fp16 pairs: up to 4 bytes per element); the initial rows - one launch
    const size_t n_st = ((size_t)(reinterpret_cast<char*>(c.st[0][3]) - reinterpret_cast<char*>(c.st[0][0])) + n) / 4;
    hipLaunchKernelGGL(k_zero_state, dim3((unsigned)std::min<size_t>(cdiv((long long)n_st, 4 * 256), 2048)), dim3(256), 0, s,
                       reinterpret_cast<uint32_t*>(c.st[0][0]), n_st, reinterpret_cast<uint32_t*>(c.st16[0][0]),
                       reinterpret_cast<uint32_t*>(c.st16[0][1]), n / 4, c.slot[0], c.word[0], h->d.bos_idx, M);
    c.st16_ok[0] = true;
    c.st16_ok[1] = false;
    LAUNCHCHK();
    return 0;
}

// Number of out-of-range ids (words outside [0, V), slots outside [0, L), gates outside {0, 1}, gt verbs outside [0, V)) the
// calls since the last vsr_prepare*() / vsr_bad_ids() were handed.  Such ids are clamped on the device (no out-of-bounds
// access); the reference would raise (nn.Embedding / tensor indexing).  Synchronises the stream; resets the count.
extern "C" int vsr_bad_ids(vsr_handle* h, int32_t* count, void* stream) {
    if (!h || !count) return fail("vsr_bad_ids: null argument");
    if (!h->prepared) { *count = 0; return 0; }
    hipStream_t s = (hipStream_t)stream;
    int v[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(v, h->c.nvalid_dev + 2, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemsetAsync(h->c.nvalid_dev + 2, 0, 2 * sizeof(int), s));
    *count = v[0] + v[1];              // [1]: non-padding region rows beyond the caller's bound (vsr_set_valid_rows_bound) - they got no projection
    return 0;
}

// ---------------------------------------------------------------------------------------------- greedy / sampling
// rpi rows per image (vsr_sample_rows: several independent samples of every image): the rows of an image are adjacent and read its
// statics as beams do (row / rpi) - nothing is copied; there are no parent pointers, every row is its own history
// gs = rpi > 1 (vsr_sample_rows_baseline): the first row of every image is its greedy baseline -> base_w / base_g (images, T); the other
// rpi - 1 are its samples: the caller's forced ids and outputs are the (images x (rpi - 1), T) tensors of the call without baseline rows
static int decode_simple(vsr_handle* h, int vmode, uint64_t seed, const int64_t* forced_w, const int64_t* forced_g,
                         const float* verbs, int gt, int64_t* words, int64_t* gates, float* lp_w, float* lp_g, hipStream_t s, int rpi = 1,
                         int gs = 0, int64_t* base_w = nullptr, int64_t* base_g = nullptr) {
    Ctx& c = h->c;
    const int B = c.B * rpi, T = h->d.seq_len;          // (B: decoder rows)
    const int Bf = gs > 0 ? c.B * (gs - 1) : B;         // rows of the forced ids
    if (verbs && vmode != VM_TOPK) return fail("verb forcing is only defined for greedy / beam decoding");
    if (zero_state(h, B, s)) return 1;
    if (vmode == VM_FORCED) {
        for (int t = 0; t < T; ++t) {
            hipLaunchKernelGGL(k_i64_to_i32, dim3(cdiv(Bf, 256)), dim3(256), 0, s, forced_w + t, (long long)T, c.forced_w32 + (size_t)t * Bf, Bf, h->d.vocab_size, c.nvalid_dev + 2);
            hipLaunchKernelGGL(k_i64_to_i32, dim3(cdiv(Bf, 256)), dim3(256), 0, s, forced_g + t, (long long)T, c.forced_g32 + (size_t)t * Bf, Bf, 2, c.nvalid_dev + 2);
        }
    }
    // The selection of step t is per row and tiny: where the next step's LSTM1 kernel starts from cached sums (decode cache) it makes the
    // selection itself (k_select_simple_lstm1) and k_select_simple is not launched for that step (VSR_FUSE_SELECT=0: always launched).
    SelSimpleArgs pending{};
    bool have_pending = false;
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        StepIO io;
        io.t = t; io.M = B; io.rpi = rpi; io.cur = cur;
        io.word_prev = c.word[cur]; io.slot = c.slot[cur];
        io.sel_simple = have_pending ? &pending : nullptr;
        io.vmode = vmode; io.gs = gs;
        io.forced = (vmode == VM_FORCED) ? c.forced_w32 + (size_t)t * Bf : nullptr;
        io.seed = seed; io.verbs = verbs; io.gt = gt; io.lg_out = c.lg;
        io.s1_from_prev = t > 0 && h->xproj != nullptr;
        io.s1_for_next = t + 1 < T && h->xproj != nullptr;
        if (run_step(h, io, s)) return 1;
        const SelSimpleArgs sa{vmode, c.top_v, c.top_i, c.lg, (vmode == VM_FORCED) ? c.forced_g32 + (size_t)t * Bf : nullptr, seed, (uint32_t)t,
                               c.slot[cur], c.L, B, T, c.word[cur ^ 1], c.gate[cur ^ 1], c.slot[cur ^ 1], words, gates, lp_w, lp_g,
                               gs, base_w, base_g};
        have_pending = (h->fuse_select & 1) && t + 1 < T && h->xproj != nullptr;       // (the next step is then s1_from_prev)
        if (have_pending) pending = sa;
        else hipLaunchKernelGGL(k_select_simple, dim3(cdiv(B, 256)), dim3(256), 0, s, sa);
        LAUNCHCHK();
    }
    return 0;
}

extern "C" int vsr_greedy(vsr_handle* h, const float* verbs, int32_t gt, int64_t* words, int64_t* gates, void* stream) {
    if (check_ready(h, "vsr_greedy")) return 1;
    if (!words || !gates) return fail("vsr_greedy: null output");
    return decode_simple(h, VM_TOPK, 0, nullptr, nullptr, verbs, gt, words, gates, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int vsr_sample(vsr_handle* h, uint64_t seed, const int64_t* forced_words, const int64_t* forced_gates,
                          int64_t* words, int64_t* gates, float* lp_words, float* lp_gates, void* stream) {
    if (check_ready(h, "vsr_sample")) return 1;
    if (!words || !gates || !lp_words || !lp_gates) return fail("vsr_sample: null output");
    if ((forced_words == nullptr) != (forced_gates == nullptr)) return fail("vsr_sample: forced_words and forced_gates go together");
    return decode_simple(h, forced_words ? VM_FORCED : VM_SAMPLE, seed, forced_words, forced_gates, nullptr, 0, words, gates,
                         lp_words, lp_gates, (hipStream_t)stream);
}

extern "C" int vsr_sample_rows(vsr_handle* h, int32_t rows_per_image, uint64_t seed, const int64_t* forced_words, const int64_t* forced_gates,
                               int64_t* words, int64_t* gates, float* lp_words, float* lp_gates, void* stream) {
    if (check_ready(h, "vsr_sample_rows")) return 1;
    if (rows_per_image < 1 || rows_per_image > h->c.beam) return fail("vsr_sample_rows: rows_per_image %d not in [1, the prepared beam %d]", rows_per_image, h->c.beam);
    if (!words || !gates || !lp_words || !lp_gates) return fail("vsr_sample_rows: null output");
    if ((forced_words == nullptr) != (forced_gates == nullptr)) return fail("vsr_sample_rows: forced_words and forced_gates go together");
    return decode_simple(h, forced_words ? VM_FORCED : VM_SAMPLE, seed, forced_words, forced_gates, nullptr, 0, words, gates,
                         lp_words, lp_gates, (hipStream_t)stream, rows_per_image);
}

extern "C" int vsr_sample_rows_baseline(vsr_handle* h, int32_t rows_per_image, uint64_t seed, const int64_t* forced_words,
                                        const int64_t* forced_gates, int64_t* words, int64_t* gates, float* lp_words, float* lp_gates,
                                        int64_t* base_words, int64_t* base_gates, void* stream) {
    if (check_ready(h, "vsr_sample_rows_baseline")) return 1;
    const int K = rows_per_image;
    if (K < 1) return fail("vsr_sample_rows_baseline: rows_per_image %d < 1", K);
    if (K + 1 > h->c.beam)
        return fail("vsr_sample_rows_baseline: %d samples + the baseline row per image exceed the prepared beam %d", K, h->c.beam);
    if (!words || !gates || !lp_words || !lp_gates || !base_words || !base_gates) return fail("vsr_sample_rows_baseline: null output");
    if ((forced_words == nullptr) != (forced_gates == nullptr)) return fail("vsr_sample_rows_baseline: forced_words and forced_gates go together");
    return decode_simple(h, forced_words ? VM_FORCED : VM_SAMPLE, seed, forced_words, forced_gates, nullptr, 0, words, gates,
                         lp_words, lp_gates, (hipStream_t)stream, K + 1, K + 1, base_words, base_gates);
}

// ---------------------------------------------------------------------------------------------- beam search
extern "C" int vsr_beam(vsr_handle* h, int32_t beam, int32_t out_size, int64_t eos_word, int64_t eos_gate, const float* verbs,
                        int32_t gt, int64_t* words, int64_t* gates, float* lp_words, float* lp_gates, float* scores, void* stream) {
    if (check_ready(h, "vsr_beam")) return 1;
    Ctx& c = h->c;
    if (beam < 1 || beam > c.beam) return fail("vsr_beam: beam %d exceeds the prepared beam %d", beam, c.beam);
    if (out_size < 1 || out_size > beam) return fail("vsr_beam: out_size %d not in [1, beam]", out_size);
    if (!words || !gates) return fail("vsr_beam: null output");
    hipStream_t s = (hipStream_t)stream;
    const int B = c.B, T = h->d.seq_len;
    const int K = beam;
    if (zero_state(h, B, s)) return 1;
    // The beam selection of step t rides in the LSTM1 kernel of step t + 1 (k_select_lstm1_x2) wherever that kernel starts from cached sums
    // (decode cache); the last step's, and every step's with VSR_FUSE_SELECT=0 or over a decode cache that is not 8-byte aligned, is a
    // launch of its own (k_select_beam, then k_lstm1: the same values).
    SelBeamArgs pending{};
    bool have_pending = false;
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        const int cb = t == 0 ? 1 : beam;
        const int M = B * cb;
        StepIO io;
        io.sel_beam = have_pending ? &pending : nullptr;
        io.t = t; io.M = M; io.rpi = cb; io.cur = cur;
        io.parent = t == 0 ? nullptr : c.parent; io.word_prev = c.word[cur]; io.slot = c.slot[cur];
        io.K = K; io.verbs = verbs; io.gt = gt; io.lg_out = c.lg;
        io.s1_from_prev = t > 0 && h->xproj != nullptr;
        io.s1_for_next = t + 1 < T && h->xproj != nullptr;
        if (run_step(h, io, s)) return 1;
        const SelBeamArgs sa{t, cb, beam, c.L, eos_word, eos_gate, c.top_v, c.top_i, c.lg, c.slot[cur], c.word[cur], c.gate[cur], c.seq[cur],
                             c.seq[cur ^ 1], c.mask[cur], c.mask[cur ^ 1], c.word[cur ^ 1], c.gate[cur ^ 1], c.slot[cur ^ 1], c.parent,
                             c.hist_parent, c.hist_word, c.hist_gate, c.hist_lpw, c.hist_lpg, B};
        have_pending = (h->fuse_select & 2) && t + 1 < T && h->xproj_al8;       // (the next step is then s1_from_prev)
        if (have_pending) pending = sa;
        else with_const_1to8(K, [&](auto KK) { hipLaunchKernelGGL((k_select_beam<decltype(KK)::value>), dim3(B), dim3(64), 0, s, sa); });
        LAUNCHCHK();
    }
    hipLaunchKernelGGL(k_backtrack, dim3(B), dim3(64), (size_t)3 * T * beam * sizeof(int), s, T, B, beam, out_size, c.seq[T & 1], c.hist_parent, c.hist_word,
                       c.hist_gate, c.hist_lpw, c.hist_lpg, words, gates, lp_words, lp_gates, scores);
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- teacher forcing
extern "C" int vsr_xe_forward(vsr_handle* h, const int64_t* captions, int32_t T, float* logp_words, float* logp_gates, void* stream) {
    if (check_ready(h, "vsr_xe_forward")) return 1;
    Ctx& c = h->c;
    if (!captions || !logp_words || !logp_gates) return fail("vsr_xe_forward: null tensor");
    if (T < 1 || T > c.L) return fail("vsr_xe_forward: captions have %d steps but prepare() saw %d region slots (need 1 <= T <= L: step t reads slot t)", T, c.L);
    if (T > h->d.seq_len) return fail("vsr_xe_forward: T %d exceeds seq_len %d (workspace is sized by seq_len)", T, h->d.seq_len);
    hipStream_t s = (hipStream_t)stream;
    const int B = c.B, V = h->d.vocab_size;
    if (zero_state(h, B, s)) return 1;
    for (int t = 0; t < T; ++t)
        hipLaunchKernelGGL(k_i64_to_i32, dim3(cdiv(B, 256)), dim3(256), 0, s, captions + t, (long long)T, c.cap32 + (size_t)t * B, B, V, c.nvalid_dev + 2);
    for (int t = 0; t < T; ++t) {
        StepIO io;
        io.t = t; io.M = B; io.cur = t & 1;
        io.word_prev = c.cap32 + (size_t)t * B; io.fixed_slot = t;           // (no slot list: step t reads slot t)
        io.vmode = VM_FULL; io.full_out = logp_words + (size_t)t * V; io.full_stride = (long long)T * V;
        io.lg_out = logp_gates + (size_t)t * 2; io.lg_stride = (long long)T * 2;
        if (run_step(h, io, s)) return 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- single step
__global__ void k_step_slots(int t, const int64_t* slot_in, const int64_t* prev_gate, int L, int M, int* slot32, int64_t* slot_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    long long k = slot_in[i];
    if (t > 0) {
        k += prev_gate[i];
        k = k < 0 ? 0 : (k > L - 1 ? L - 1 : k);
    }
    slot32[i] = (int)k;
    slot_out[i] = k;
}

extern "C" int vsr_step(vsr_handle* h, int32_t t, int32_t rows_per_image, const int64_t* prev_words, const int64_t* prev_gates,
                        const float* h1, const float* c1, const float* h2, const float* c2, const int64_t* slot,
                        float* h1_out, float* c1_out, float* h2_out, float* c2_out, int64_t* slot_out,
                        const float* verbs, int32_t gt, float* logp_words, float* logp_gates, void* stream) {
    if (check_ready(h, "vsr_step")) return 1;
    Ctx& c = h->c;
    if (rows_per_image < 1 || rows_per_image > c.beam) return fail("vsr_step: rows_per_image %d exceeds the prepared beam %d", rows_per_image, c.beam);
    if (t > 0 && (!prev_words || !prev_gates)) return fail("vsr_step: previous outputs required for t > 0");
    hipStream_t s = (hipStream_t)stream;
    const int M = c.B * rows_per_image, H = h->d.rnn_size, V = h->d.vocab_size;
    const size_t n = (size_t)M * H * sizeof(float);
    const float* in[4] = {h1, c1, h2, c2};
    float* out[4] = {h1_out, c1_out, h2_out, c2_out};
    for (int j = 0; j < 4; ++j) HIPCHK(hipMemcpyAsync(c.st[0][j], in[j], n, hipMemcpyDeviceToDevice, s));
    c.st16_ok[0] = false;                     // the caller's state has no bf16 image
    // (not tied to gemm_tile: with VSR_GEMM_TILE forced the count is still taken though no launch scales the states by the unit bound - not needed, kept)
    if (h->f16x2()) {                         // f16x2: the hidden states are unit-class GEMM operands (include/vsrcap.h, limits of the flavour)
        const long long ne = (long long)M * H;
        hipLaunchKernelGGL(k_count_outside_unit, dim3(cdiv(ne, 256)), dim3(256), 0, s, h1, ne, c.nvalid_dev + 2);
        hipLaunchKernelGGL(k_count_outside_unit, dim3(cdiv(ne, 256)), dim3(256), 0, s, h2, ne, c.nvalid_dev + 2);
    }
    hipLaunchKernelGGL(k_step_slots, dim3(cdiv(M, 256)), dim3(256), 0, s, t, slot, prev_gates, c.L, M, c.slot[0], slot_out);
    if (t == 0) hipLaunchKernelGGL(k_fill_i32, dim3(cdiv(M, 256)), dim3(256), 0, s, c.word[0], h->d.bos_idx, M);
    else hipLaunchKernelGGL(k_i64_to_i32, dim3(cdiv(M, 256)), dim3(256), 0, s, prev_words, 1LL, c.word[0], M, V, c.nvalid_dev + 2);
    StepIO io;
    io.t = 1;  // state segments are always live here (the caller may pass a non-zero state at t == 0)
    io.M = M; io.rpi = rows_per_image;
    io.word_prev = c.word[0]; io.slot = c.slot[0];
    io.vmode = VM_FULL; io.full_out = logp_words; io.full_stride = V;
    io.verbs = verbs; io.gt = gt; io.lg_out = logp_gates;
    if (run_step(h, io, s)) return 1;
    for (int j = 0; j < 4; ++j) HIPCHK(hipMemcpyAsync(out[j], c.st[1][j], n, hipMemcpyDeviceToDevice, s));
    return 0;
}

// ---------------------------------------------------------------------------------------------- training path
#include "products.h"
#include "train.inc.h"
#include "cider.inc.h"
#include "ssp.inc.h"

static TrainCtx* new_train_ctx() { return new TrainCtx(); }
static void free_train_ctx(TrainCtx* t) { delete t; }
static void invalidate_train_ctx(TrainCtx* t) { if (t) t->valid = false; }
