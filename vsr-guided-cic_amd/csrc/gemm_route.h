// GEMM routing: which kernel, tile and k plan a grouped launch takes.  Host only: GemmBuilder::finish() reads the handle's GemmState
// (flavours switched on, operand images, knobs), calls no HIP function and leaves a GemmRoute (gemm_dispatch.h) plus the planned GemmArgs.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm_dispatch.h"

namespace vsr {

// An operand that exists as an image beside its fp32 buffer [lo, hi), or instead of it
struct ImageRange {
    enum Owner { WEIGHTS, TRAIN };       // the bound weights (set by the refreshes) | the transposed W operands of the current training workspace
    const float* lo; const float* hi;
    Owner owner;
    const uint16_t* b16;                 // bf16 copy (gemm_bf16.h), or null
    const float* h2;                     // fp16-pair image (gemm_h2.h), or null ...
    int slot;                            // ... and the slot of its scale exponent (H2Slot)
    bool holds(const float* p) const { return p >= lo && p < hi; }
    const float* h2_at(const float* p) const { return h2 + (p - lo); }
};

// THE registry of operand images: GemmBuilder::finish(), the transposing kernels of the training pass and the optimizer find an operand's
// image by the address of its fp32 buffer.  The entry points (vsrcap.hip, train.inc.h) change it through the named operations only.
// A lookup prefers the weights' ranges: a training range may outlive the memory it was registered for.
struct OperandImages {
    std::vector<ImageRange> r;
    bool train_h2_only = false;          // the running backward pass writes ONLY the fp16-pair images of the training ranges (train.inc.h: h2b)

    // ---- the weights' images (vsr_bind_weights, vsr_refresh_*_weights, vsr_adam_step)
    void clear_weights_bf16() { drop(ImageRange::WEIGHTS, true, false); }       // (the training ranges keep their twins: see clear_h2)
    void add_weight_bf16(const float* p, size_t n, const uint16_t* b) { weight(p, n).b16 = b; }
    void clear_weights_h2() { drop(ImageRange::WEIGHTS, false, true); }
    void add_weight_h2(const float* p, size_t n, const float* img, int slot) { ImageRange& x = weight(p, n); x.h2 = img; x.slot = slot; }   // (the embedding table too: an A operand)
    // Leaving the f16x2 flavour (bind, refresh(NULL)) also forgets the training ranges' fp16-pair images, leaving the bf16 mode keeps their
    // twins.  Kept as it was: both transitions invalidate the training context, and the next forward or select registers anew, but
    // stale_w (below) scans the twins for launches of the decoder too, so dropping them could in principle be observed
    void clear_h2() { clear_weights_h2(); drop(ImageRange::TRAIN, false, true); }
    // ---- the training workspace's.  register_train (train_begin, vsr_train_select: `ops` is the list carve_train built out of train_operands)
    // replaces the registrations of the workspace before it; no entry point calls clear_train on its own (tools/route_host does)
    void clear_train() { drop(ImageRange::TRAIN, true, true); train_h2_only = false; }
    void register_train(const std::vector<ImageRange>& ops) { clear_train(); r.insert(r.end(), ops.begin(), ops.end()); }
    void mark_train_image_only(bool on) { train_h2_only = on; }

    // ---- lookups
    const uint16_t* bf16_of(const float* p) const {
        const ImageRange* x = find(p, true, [](const ImageRange& q) { return q.b16 != nullptr; });
        return x ? x->b16 + (p - x->lo) : nullptr;
    }
    const ImageRange* h2_of(const float* p) const { return find(p, true, [](const ImageRange& q) { return q.h2 != nullptr; }); }
    // A operands are looked up among the weights' ranges only (the embedding table): the training ranges describe W operands
    const ImageRange* h2_of_weight(const float* p) const { return find(p, false, [](const ImageRange& q) { return q.h2 != nullptr; }); }
    int h2_slot_of(const float* p) const { const ImageRange* x = h2_of(p); return x ? x->slot : 0; }
    // p lies in a training range that exists ONLY as an image: its bf16 twin (bf16 mode) / its fp16-pair image (while a backward pass says so)
    bool only_bf16(const float* p) const { return train(p, [](const ImageRange& q) { return q.b16 != nullptr; }); }
    bool only_h2(const float* p) const { return train_h2_only && train(p, [](const ImageRange& q) { return q.h2 != nullptr; }); }
    // the range registered for the weight tensor that begins at p (vsr_adam_step), or null
    const ImageRange* weight_at(const float* p) const {
        for (const ImageRange& x : r)
            if (x.owner == ImageRange::WEIGHTS && x.lo == p) return &x;
        return nullptr;
    }

private:
    ImageRange& weight(const float* p, size_t n) {
        for (ImageRange& x : r)
            if (x.owner == ImageRange::WEIGHTS && x.lo == p && x.hi == p + n) return x;
        r.push_back(ImageRange{p, p + n, ImageRange::WEIGHTS, nullptr, nullptr, 0});
        return r.back();
    }
    void drop(ImageRange::Owner o, bool bf16, bool h2) {          // forgets the images of a kind; a range without any goes
        for (ImageRange& x : r)
            if (x.owner == o) { if (bf16) x.b16 = nullptr; if (h2) x.h2 = nullptr; }
        r.erase(std::remove_if(r.begin(), r.end(), [](const ImageRange& x) { return !x.b16 && !x.h2; }), r.end());
    }
    template <class F> const ImageRange* find(const float* p, bool with_train, F&& has) const {
        const ImageRange* hit = nullptr;
        for (const ImageRange& x : r)
            if (x.holds(p) && has(x)) {
                if (x.owner == ImageRange::WEIGHTS) return &x;
                if (with_train && !hit) hit = &x;
            }
        return hit;
    }
    template <class F> bool train(const float* p, F&& has) const {
        for (const ImageRange& x : r)
            if (x.owner == ImageRange::TRAIN && x.holds(p) && has(x)) return true;
        return false;
    }
};

// f16x2 flavour: slots of the scale-exponent table (device ints at the head of the image buffer; a twin table of float bounds next to it).
// 0..13: the 14 weight matrices; then the bounds of the A operands a GEMM segment can name (GemmBuilder::seg's a_cls)
enum H2Slot { H2A_NONE = -1, H2A_EMBED = 14, H2A_UNIT = 15, H2A_REGION = 16, H2A_DET = 17, H2A_ATT = 18, H2B_SENT = 19, H2_NSLOT = 32 };

// Routing knobs: defaults, the slot counts of the device (set_cus) and their VSR_* environment overrides (read_env)
struct GemmKnobs {
    // f16x2 streaming kernel: launches of at most h2s_max rows (VSR_H2S_MAX / _SLOTS / _MIN / _NS).  Measured end to end in one run
    // (profiles/r04_e_h2s_routing.txt): 80 - greedy (M = 100, then on the 128 x 128 tile) 660 k tokens/s against 632 k at 128, the 13-image shard
    // (M = 65) 2.61 ms either way; 48 - greedy 668 k, the shard 2.75 ms
    int h2s_max = 80, h2s_slots = 512, h2s_min = 8, h2s_ns = 1;
    int h2_aligned_min = 4;      // shortest k-aligned piece of the f16x2 kernels, in 32-wide k-tiles (VSR_H2_ALIGNED_MIN) ...
    int h2_aligned_min_small = 8;   // ... and in launches whose rows fit ONE m-tile (<= 128 rows: greedy decoding, the per-step GEMMs of training; VSR_H2_ALIGNED_MIN_SMALL).
                                    // Round 6: 8 instead of 4 there - pieces of 4 k-tiles cost more in their flush than in their k loop: XE +2.4 %, greedy +1.1 %
                                    // (profiles/r06_t_*).  For the wide launches 8 was REJECTED by the flip-rate fixture (one caption of 1 024 flipped in the default flavour).
    double aligned_eff_min = 0.75;    // wide launches: k-aligned pieces when they keep at least this share of the CUs busy, stream-K ranges otherwise (VSR_ALIGNED_EFF, percent)
    // the producers of the decoder's A operands (h1, h2, s_t, g_t, the attended vector) write fp16-pair images next to the fp32 values
    // and launches whose A operands all have one take the all-DMA kernel (gemm_h2a.h); VSR_H2_AIMG=0: in-kernel split of fp32 A only
    bool h2_aimg = true;
    int h2_mfma = 16;                 // MFMA shape of the all-DMA kernel's multipliers: 16 (v_mfma_f32_16x16x32_f16) or 32 (32x32x16; VSR_H2_MFMA=32)
    bool b16_dma = true;              // bf16 mode: launches whose A operands all have bf16 images take the all-DMA kernel (VSR_B16_DMA=0: register-staged)
    int gemm_slots_bf16 = 256;         // ONE 16-wave workgroup per CU (108 KB of LDS: two 128+256-row x 64-k bf16 buffers; 147 KB for f32x3)
    int gemm_slots = 1024;       // resident 64x64 GEMM workgroups to fill: 256 CUs x 4 (36.9 KB LDS each)
    int gemm_slots_small = 768;  // 64x64 tiles (M <= 192): 3 per CU measured best (greedy 473 k vs 461 k tokens/s at 4 per CU)
    int gemm_min_iters = 8;
    int gemm_x3_min_rows = 193;  // f32x3 flavour: launches of at least this many rows take the 128 x 256 tile (VSR_X3_MIN_ROWS)
    int x3_skinny = 1;           // ... launches of r16_max < rows <= 128 the 128 x 128 tile (one m-tile holds every row; VSR_X3_SKINNY=0: exact kernels)
    // k-aligned pieces (gemm_plan_aligned) or stream-K ranges.  VSR_X3_ALIGNED=<wide><skinny> as two digits; wide: 0 never, 1 whenever the
    // tiles fit the CUs, 2 (default) per launch by its efficiency (plan_mfma128) and always from 1024 rows up.  Measured end to
    // end: beam-5 (M = 500) 265.7 k tokens/s with stream-K ranges everywhere against 256.5 k with aligned pieces everywhere; XE step
    // (its wide launches have 2000 rows) 9.52 k against 9.40 k samples/s; greedy (M = 100) 572 k with aligned pieces against 550 k
    int x3_aligned_wide = 2, x3_aligned_skinny = 1;
    int x3_aligned_min = 4;      // shortest k-aligned piece of the f32x3 kernels, in 32-wide k-tiles
    // f32x3 launches of at most x3s_max rows: the weight-streaming kernel (gemm_x3s.h) when its k-aligned plan exists.  Measured over
    // the four step GEMMs (tools/gemm_bench, one 16-column strip per wave, two workgroups per CU): M = 13: 53 us against 65 (rows-16
    // kernel); M = 32: 61 against 76; M = 65: 99 against 107 (128 x 128 tile); M = 100: 123 against 112 - so up to 80 rows.
    // VSR_X3S_MAX=0 turns it off.
    int x3s_max = 80, x3s_slots = 512, x3s_min = 8;
    int gemm_slots_r16 = 256;    // rows-16 kernel: ONE 8-wave workgroup per CU (two waves per SIMD)
    // Problems with at most this many rows take the rows-16 kernel (VSR_GEMM_R16_MAX=0 disables it).  Measured end to end on
    // one MI355X: at M = 100 it is level with the 64x64 kernel inside a GEMM (61.5 vs 60.6 TF/s) but its tiles are cut into
    // 7-8 stream-K pieces instead of 4-6, and the consumers' extra slab reads cost more than its 11 %-instead-of-28 %
    // padding saves (greedy 459 k vs 481 k tokens/s, XE step 6.8 k vs 7.4 k samples/s).  Below 64 rows (a data-parallel
    // shard of 12-13 images and its 65 beam rows, small eval batches) the 64-row tiles are mostly padding and the rows-16 kernel wins
    // (M = 13: 19.5 vs 13.2 TF/s over the four step GEMMs; beam-5 over a 13-image shard, M = 65: 3.48 vs 3.81 ms per call).
    int gemm_r16_max = 40;
    int bf16_p_fp32 = 1;         // bf16 mode: the hoisted att_va(regions) GEMM of vsr_prepare*() stays fp32-equivalent (VSR_BF16_P_FP32=0: bf16 like the rest)
    int gemm_aligned = 1;        // 128 x 256 kernels: k-aligned pieces (gemm_plan_aligned) when the tiles fit the CUs; VSR_GEMM_ALIGNED=0: stream-K always
    int gemm_aligned_min = 8;    // shortest piece, in 64-wide k-tiles (VSR_GEMM_ALIGNED_MIN)
    int xcd_groups = 0;          // VSR_XCD_GROUPS=1: k-aligned plans deal whole m-groups of tiles to an XCD (gemm_plan_aligned).  Measured: 2 % less fabric traffic on the wide kernel, 1.3 % SLOWER end to end (profiles/r06_d_xcd_group_dealing_ab.txt): off
    int gemm_tile = 0;           // 0 = by M; VSR_GEMM_TILE=64 | 12864 | 128 forces 64x64 / 128x64 / 128x128

    void set_cus(int cus) {
        gemm_slots = cus * 4; gemm_slots_small = cus * 3; gemm_slots_r16 = cus; gemm_slots_bf16 = cus;
        x3s_slots = cus * 2; h2s_slots = cus * 2;
    }
    void read_env() {
        const int ANY = INT_MIN, TOP = INT_MAX;
        const struct { const char* name; int* v; int lo, hi; } tab[] = {
            {"VSR_X3_MIN_ROWS", &gemm_x3_min_rows, ANY, TOP}, {"VSR_X3_SKINNY", &x3_skinny, ANY, TOP},
            {"VSR_X3S_MAX", &x3s_max, ANY, 128}, {"VSR_H2S_MAX", &h2s_max, ANY, 128},     // (the streaming kernels hold every row in ONE m-tile)
            {"VSR_H2S_SLOTS", &h2s_slots, 1, TOP}, {"VSR_H2S_MIN", &h2s_min, 1, TOP},
            {"VSR_H2_ALIGNED_MIN", &h2_aligned_min, 1, TOP}, {"VSR_H2_ALIGNED_MIN_SMALL", &h2_aligned_min_small, 1, TOP},
            {"VSR_X3S_SLOTS", &x3s_slots, 1, TOP}, {"VSR_X3S_MIN", &x3s_min, 1, TOP}, {"VSR_X3_ALIGNED_MIN", &x3_aligned_min, 1, TOP},
            {"VSR_GEMM_SLOTS_BF16", &gemm_slots_bf16, 1, TOP}, {"VSR_GEMM_SLOTS_R16", &gemm_slots_r16, 1, TOP},
            {"VSR_GEMM_R16_MAX", &gemm_r16_max, ANY, TOP}, {"VSR_GEMM_ALIGNED", &gemm_aligned, ANY, TOP},
            {"VSR_BF16_P_FP32", &bf16_p_fp32, ANY, TOP}, {"VSR_GEMM_ALIGNED_MIN", &gemm_aligned_min, 1, TOP},
            {"VSR_GEMM_SLOTS", &gemm_slots, 1, TOP}, {"VSR_GEMM_SLOTS_SMALL", &gemm_slots_small, 1, TOP},
            {"VSR_GEMM_TILE", &gemm_tile, ANY, TOP}, {"VSR_XCD_GROUPS", &xcd_groups, ANY, TOP}, {"VSR_GEMM_MIN_ITERS", &gemm_min_iters, 1, TOP}};
        for (const auto& t : tab)
            if (const char* e = getenv(t.name)) *t.v = std::min(std::max(atoi(e), t.lo), t.hi);
        if (const char* e = getenv("VSR_H2S_NS")) h2s_ns = atoi(e) == 2 ? 2 : 1;
        if (const char* e = getenv("VSR_H2_AIMG")) h2_aimg = atoi(e) != 0;
        if (const char* e = getenv("VSR_H2_MFMA")) h2_mfma = atoi(e) == 32 ? 32 : 16;
        if (const char* e = getenv("VSR_B16_DMA")) b16_dma = atoi(e) != 0;
        if (const char* e = getenv("VSR_ALIGNED_EFF")) aligned_eff_min = atoi(e) / 100.0;
        if (const char* e = getenv("VSR_X3_ALIGNED")) { x3_aligned_wide = atoi(e) / 10; x3_aligned_skinny = atoi(e) % 10; }
    }
};

// The kernels a launch is offered first (GemmState::flavour(); the names of vsrcap/derived.py's table)
enum class Flavour { F32, F32X3, F16X2, BF16 };

// What routing reads of a handle (vsr_handle derives from it)
struct GemmState {
    // bf16 throughput mode (gemm_bf16.h): off unless vsr_refresh_bf16_weights() has been given a buffer
    bool bf16_on = false;
    // f16x2 flavour (gemm_h2.h): on once vsr_refresh_h2_weights() has been given a buffer, and only together with x3_on (a launch
    // that does not qualify - an operand without an image / a bound, sizes that are not multiples of 8 - takes the f32x3 kernels)
    bool h2_on = false;
    bool x3_on = true;                // launches of >= gemm_x3_min_rows rows: fp32 products through three bf16 terms per operand (gemm_x3.h); fp32 operands, no copies.  vsr_set_gemm_mode(h, 0): exact fma chain everywhere
    GemmKnobs gk;
    OperandImages img;
    int* h2_exps = nullptr;           // device: H2_NSLOT scale exponents ...
    unsigned* h2_bounds = nullptr;    // ... and the bounds they come from (bit patterns of non-negative floats)

    // THE flavour rule.  The three switches are what the C ABI sets, and it allows states Python never asks for: with both kinds of
    // images on, bf16 is offered first and a launch it does not take falls to the f16x2 kernels; h2_on without x3_on is F32 with images nobody reads.
    // Every reader of the flavour goes through flavour() or one of the predicates below; none spells a conjunction of the switches.
    Flavour flavour() const { return bf16_on ? Flavour::BF16 : !x3_on ? Flavour::F32 : h2_on ? Flavour::F16X2 : Flavour::F32X3; }
    bool bf16() const { return flavour() == Flavour::BF16; }
    bool f16x2() const { return flavour() == Flavour::F16X2; }
    // launches of this state route to the f16x2 kernels (when their operands qualify).  finish() and the backward pass's h2b must agree on it:
    // the backward writes ONLY images for launches that finish() then has to route there.  (Under bf16_on too: see flavour())
    bool routes_f16x2() const { return h2_on && x3_on && gk.gemm_tile == 0; }
    // a training workspace carries fp16-pair images of its W operands (carve_train), which a backward pass may make the only copy (finish(): stale_h2).
    // Without x3_on too: the workspace's size does not depend on vsr_set_gemm_mode
    bool train_h2_images() const { return h2_on && !bf16_on; }
    // the producers of the decoder's A operands write fp16-pair images beside the fp32 values (run_step, train_a_images).  Not tied to gemm_tile:
    // with VSR_GEMM_TILE forced the images are written and no launch reads them - not needed, a diagnostic knob's cost
    bool writes_h2_a_images() const { return f16x2() && gk.h2_aimg; }
    // vsr_prepare*() measures the bounds of the region / detection operands.  h2_on alone: needed under bf16_on (launches fall through to
    // the f16x2 kernels), not needed without x3_on, where the passes that carry the measurement are the same
    bool measures_h2_bounds() const { return h2_on; }
    bool has_weight_images() const { return h2_on || bf16_on; }      // something derived from the weights' values exists (vsr_adam_step)
};

// What vsr_profile_* measures.  GemmBuilder::launch times and counts a launch that is handed one (the decoder's); the ordering models hand none.
struct GemmProfile {
    bool on = false;
    std::vector<hipEvent_t> ev;      // pool, pairs (start, stop)
    size_t ev_used = 0;
    double flops = 0, bytes = 0;
    int every = 1;                   // time every every-th GEMM launch (1 = all of them)
    long long seen = 0;              // GEMM launches since vsr_profile_begin*
};

// every segment of every problem of a launch
template <class F> inline void for_each_seg(GemmArgs& a, F&& f) {
    for (int i = 0; i < a.nprob; ++i)
        for (int sg = 0; sg < a.p[i].nseg; ++sg) f(a.p[i].seg[sg]);
}
template <class P> inline bool all_segs(const GemmArgs& a, P&& pred) {
    for (int i = 0; i < a.nprob; ++i)
        for (int sg = 0; sg < a.p[i].nseg; ++sg)
            if (!pred(a.p[i].seg[sg])) return false;
    return true;
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// efficiency of a k-aligned plan: work units over (slots x longest piece); 1 = every CU busy for the whole launch
inline double aligned_eff(const GemmArgs& g, int slots) {
    int T = 1;
    for (int i = 0; i < g.nprob; ++i) T = std::max(T, (g.p[i].ktiles + g.p[i].split - 1) / g.p[i].split);
    return (double)g.total_iters / ((double)slots * T);
}

// The planner of the 128-row MFMA tiles (f32x3 and f16x2 kernels; k-tiles of BK).  small: the rows fit ONE m-tile and the launch takes
// 128 x 128 tiles - k-aligned pieces of at least min_small k-tiles when small_aligned, else stream-K ranges.  Otherwise the wide rule
// below with pieces of at least min_wide.  Plans `a`, sets tn (64-column units) and returns the slab count; trial plans are made on copies.
inline int plan_mfma128(GemmArgs& a, int& tn, const GemmKnobs& k, int maxM, bool small, int BK, int min_wide, int min_small, bool small_aligned, int slots) {
    if (small) {
        tn = 2;
        if (small_aligned)
            if (const int ns = gemm_plan_aligned(a, slots, min_small, 128, 128, BK)) return ns;
        return gemm_plan(a, slots, 4, 128, 128, BK);
    }
    // Wide launches: stream-K ranges keep every CU busy but cut a tile into 3-5 pieces (slabs every consumer has to add);
    // k-aligned pieces share their k-windows in L2 and write exactly `split` slabs, but leave CUs idle when tiles x split
    // does not fill the chip.  Measured on the beam-5 step shapes (tools/gemm_bench, M = 500): S2 (64 tiles of K = 1000)
    // 42 us / 5 slabs with stream-K ranges, 35 us / 2 slabs with k-aligned halves of 128 x 128 tiles; S5 125 us / 5 slabs
    // vs 124 us / 3 slabs (efficiency 0.76); S1 120 vs 137 us (0.74); the vocabulary GEMM 82 vs 88 us (0.63).
    if (k.x3_aligned_wide != 0) {             // (quirk kept: VSR_X3_ALIGNED's wide digit steers the f16x2 wide planner too)
        const bool force = k.x3_aligned_wide == 1 || maxM >= 1024;
        GemmArgs a22 = a, a21 = a;
        const int ns22 = gemm_plan_aligned(a22, slots, min_wide, 128, 256, BK);
        int tiles22 = 0;
        for (int i = 0; i < a.nprob; ++i) tiles22 += ((a.p[i].M + 127) / 128) * ((a.p[i].N + 255) / 256);
        if (tiles22 <= 64 && maxM < 1024) {              // a small launch: halves of narrow tiles fill the chip with fewer slabs
            const int ns21 = gemm_plan_aligned(a21, slots, min_wide, 128, 128, BK);
            if (ns21 && aligned_eff(a21, slots) >= 0.95 && (!ns22 || ns21 < ns22)) { a = a21; tn = 2; return ns21; }
        }
        if (ns22 && (force || aligned_eff(a22, slots) >= k.aligned_eff_min)) { a = a22; tn = 4; return ns22; }
    }
    tn = 4;
    return gemm_plan(a, slots, 4, 128, 256, BK);
}

struct GemmBuilder {
    GemmArgs a;
    GemmBuilder() { memset(&a, 0, sizeof(a)); }
    GemmProb& prob(int M, int N, float* C, int ldc) {
        GemmProb& p = a.p[a.nprob++];
        p.M = M; p.N = N; p.C = C; p.ldc = ldc; p.nseg = 0;
        return p;
    }
    // a_cls: which bound the A operand obeys (H2Slot; the f16x2 kernels scale A by it); H2A_NONE: the launch cannot take them
    static void seg(GemmProb& p, const float* A, int lda, const int* idx, const float* W, int ldw, int K, const uint16_t* A16 = nullptr, int a_cls = H2A_NONE) {
        if (K <= 0) return;
        GemmSeg& s = p.seg[p.nseg++];
        s.A = A; s.lda = lda; s.a_idx = idx; s.W = W; s.ldw = ldw; s.K = K; s.A16 = A16;
        s.exp_idx = a_cls;               // (finish() turns it into (a slot << 16) | w slot when the launch takes the f16x2 kernels)
    }
    GemmRoute route;        // set by finish()
    bool keep_fp32 = false; // bf16 mode: this launch stays fp32-equivalent (f32x3 kernels): the hoisted att_va(regions) projection, whose
                            // outputs are summed RAW over up to 36 rows into the shift logit (step :187) - bf16 rounding adds up coherently there
    bool a_image_only = false;   // f16x2 flavour: an A operand exists ONLY as an fp16-pair image (GemmSeg::A16; the training pass's transposed gradients): the launch must take the all-DMA kernel
    bool stale_h2 = false;  // f16x2 flavour: a W operand exists only as an fp16-pair image (a transposed operand of the training pass) but the launch does not take an f16x2 kernel
    bool stale_w = false;   // bf16 mode: a W operand exists only as a bf16 image but the launch does not qualify for the bf16 kernel

    // a streaming kernel (one m-tile of mt 16-row tiles, bn-column blocks, k-aligned pieces only), planned on a copy: 0 = its plan does not exist
    int try_stream(GemmKernel kernel, int maxM, int slots, int min_piece, int bn, int BK) {
        GemmArgs as = a;
        const int ns = gemm_plan_aligned(as, slots, min_piece, 128, bn, BK);
        if (ns) { a = as; route.kernel = kernel; route.tm = 0; route.tn = bn / 64; route.mt = (maxM + 15) / 16; }
        return ns;
    }

    // picks the kernel (route) and plans the launch; returns the slab count; the caller then sets every problem's C / slab_stride
    int finish(const GemmState* h) {
        const GemmKnobs& k = h->gk;
        route = GemmRoute();
        int maxM = 0;
        for (int i = 0; i < a.nprob; ++i) maxM = std::max(maxM, a.p[i].M);
        const bool kept_fp32 = keep_fp32 && k.bf16_p_fp32;      // (a knob of the bf16 mode: only read together with bf16())
        if (h->bf16() && !kept_fp32) {
            // bf16 mode: every W operand of the launch must have a bf16 copy (and 16-byte-aligned 8-element chunks);
            // a launch that does not qualify runs on the fp32 kernel
            const bool ok = all_segs(a, [&](const GemmSeg& S) {
                const uint16_t* w16 = h->img.bf16_of(S.W);
                return w16 && (S.K % 8 == 0) && (S.ldw % 8 == 0) && (S.lda % 4 == 0) && aligned16(w16) && aligned16(S.A);
            });
            // the transposing kernels of the training pass write ONLY the bf16 image of such an operand: the fp32 kernel
            // would read a stale buffer.  (Does not happen for sizes the mode accepts: every K / leading dimension is a
            // multiple of 8.)
            if (!ok) for_each_seg(a, [&](const GemmSeg& S) { stale_w = stale_w || h->img.only_bf16(S.W); });
            if (ok) {
                route.a16 = true;
                for_each_seg(a, [&](GemmSeg& S) {
                    S.W = reinterpret_cast<const float*>(h->img.bf16_of(S.W));
                    route.a16 = route.a16 && S.A16 && (S.lda % 8 == 0) && aligned16(S.A16);
                });
                route.kernel = (route.a16 && k.b16_dma) ? GemmKernel::B16A : GemmKernel::BF16W;   // both operands are images: the all-DMA kernel (gemm_b16a.h)
                // launches whose rows fit one m-tile: 128 x 128 tiles (twice the tiles, half the k pieces per tile), as for f32x3
                const bool narrow = k.x3_skinny && maxM <= 128;
                route.tm = 2; route.tn = narrow ? 2 : 4;
                if (k.gemm_aligned)
                    if (const int ns = gemm_plan_aligned(a, k.gemm_slots_bf16, narrow ? 2 : k.gemm_aligned_min, 128, 64 * route.tn, B16_BK)) return ns;
                return gemm_plan(a, k.gemm_slots_bf16, 4, 128, 64 * route.tn, B16_BK);
            }
        }
        if (h->routes_f16x2()) {
            // f16x2 (gemm_h2.h): every W operand has an fp16-pair image (window starts and leading dimensions in whole 8-element
            // groups), every A operand a bound class
            const bool ok = all_segs(a, [&](const GemmSeg& S) {
                const ImageRange* r = h->img.h2_of(S.W);
                return r && S.exp_idx >= 0 && (S.K % 8 == 0) && (S.ldw % 8 == 0) && (S.lda % 4 == 0) && ((S.W - r->lo) % 8 == 0) && aligned16(S.A);
            });
            if (ok) {             // (every path below returns: the operands are rewritten in place)
                for_each_seg(a, [&](GemmSeg& S) {
                    const ImageRange* r = h->img.h2_of(S.W);
                    S.exp_idx = (S.exp_idx << 16) | r->slot;
                    S.W = r->h2_at(S.W);
                });
                a.exps = h->h2_exps;
                // all-DMA kernel (gemm_h2a.h): every A operand has an fp16-pair image too - written by its producer (GemmSeg::A16 in this
                // flavour) or a registered one (the embedding table)
                const bool aimg = k.h2_aimg && all_segs(a, [&](const GemmSeg& S) {
                    const ImageRange* ra = S.A16 ? nullptr : h->img.h2_of_weight(S.A);
                    return (S.lda % 8 == 0) && (S.A16 ? (reinterpret_cast<uintptr_t>(S.A16) & 31) == 0
                                                      : (ra && ra->slot == (S.exp_idx >> 16) && (S.A - ra->lo) % 8 == 0));
                });
                if (maxM <= k.h2s_max && maxM <= 128 && !(a_image_only && aimg))
                    if (const int ns = try_stream(GemmKernel::H2S, maxM, k.h2s_slots, k.h2s_min, h2s_bn(k.h2s_ns), H2_BK)) return ns;
                route.kernel = aimg ? GemmKernel::H2A : GemmKernel::H2;
                route.tm = 2; route.mf = k.h2_mfma;
                if (aimg)
                    for_each_seg(a, [&](GemmSeg& S) {
                        if (S.A16) S.A = reinterpret_cast<const float*>(S.A16);
                        else S.A = h->img.h2_of_weight(S.A)->h2_at(S.A);
                    });
                return plan_mfma128(a, route.tn, k, maxM, maxM <= 128, H2_BK, k.h2_aligned_min, k.h2_aligned_min_small, true, k.gemm_slots_bf16);
            }
        }
        // from here on the launch reads fp32 operands: the transposing kernels of an f16x2 backward pass wrote ONLY the images of theirs
        if (h->train_h2_images()) for_each_seg(a, [&](const GemmSeg& S) { stale_h2 = stale_h2 || h->img.only_h2(S.W); });
        if ((h->x3_on || (h->bf16() && kept_fp32)) && k.gemm_tile == 0) {
            // f32x3 (gemm_x3.h): 128 x 256 tiles from 193 rows up; 128 x 128 tiles for launches whose rows fit ONE m-tile (greedy
            // decoding, sampling, the per-step GEMMs of the training pass at batch 100, a shard of a strong-scaled decode): the
            // number of tiles is then the number of n-tiles, which 256-wide tiles would have to cut into ~10 k pieces each.
            // Measured over the four step GEMMs (tools/gemm_bench): M = 100: 112 us against 160 us for the exact 64 x 64 kernel;
            // M = 65: 107 against 120 (rows-16) / 154; M = 13: 100 against 64 for the rows-16 kernel, which keeps the shortest launches.
            const bool ok = all_segs(a, [](const GemmSeg& S) { return (S.K % 4 == 0) && (S.ldw % 4 == 0) && (S.lda % 4 == 0) && aligned16(S.W) && aligned16(S.A); });
            const bool wide = ok && maxM >= k.gemm_x3_min_rows;
            // weight-streaming kernel: 64-column blocks x k-aligned pieces, two workgroups per CU
            if (ok && !wide && k.x3_skinny && maxM <= k.x3s_max)
                if (const int ns = try_stream(GemmKernel::X3S, maxM, k.x3s_slots, k.x3s_min, x3s_bn(1), X3_BK)) return ns;
            const bool skinny = ok && !wide && k.x3_skinny && maxM <= 128 && maxM > k.gemm_r16_max;
            if (wide || skinny) {
                route.kernel = GemmKernel::X3; route.tm = 2;
                return plan_mfma128(a, route.tn, k, maxM, skinny, X3_BK, k.x3_aligned_min, k.x3_aligned_min, k.x3_aligned_skinny != 0, k.gemm_slots_bf16);
            }
        }
        if (k.gemm_tile == 0 && maxM <= k.gemm_r16_max) {
            // short problems: every row of an m-tile in one workgroup, rows in units of 16 (M = 100 -> 112, not 128)
            const int tiles = (maxM + 127) / 128;
            route.kernel = GemmKernel::F32_R16;
            route.tm = 0; route.tn = 2; route.mt = (((maxM + tiles - 1) / tiles) + 15) / 16;
            return gemm_plan(a, k.gemm_slots_r16, 4, 16 * route.mt, 128);
        }
        // resident workgroups per CU: 4 at 36.9 KB LDS (64x64), 2 at 55.3 KB (128x64) or 73.7 KB (128x128).
        // 128x128 for M >= 1024 (weight-gradient GEMMs: one tile per workgroup, 130 TF/s at long K);
        // 128x64 is the default for tall problems: as fast as 128x128 in the GEMM itself (91.8 vs 93.7 TF/s) but its
        // tiles are cut into ~3 stream-K pieces instead of ~5, so every consumer kernel reads 40 % fewer slab bytes.
        const int t = k.gemm_tile;
        const bool by_m = t != 128 && t != 12864 && t != 64;
        route.tm = (t == 128 || t == 12864 || (by_m && maxM > 192)) ? 2 : 1;
        route.tn = (t == 128 || (by_m && maxM >= 1024)) ? 2 : 1;
        return gemm_plan(a, route.tm == 2 ? k.gemm_slots / 2 : k.gemm_slots_small, k.gemm_min_iters, 64 * route.tm, 64 * route.tn);
    }
    int launch(hipStream_t s, const GemmState* h, GemmProfile* prof);        // (vsrcap.hip: gemm_dispatch(), inside prof's events when prof is given)
};

}  // namespace vsr
