// What a decoder timestep multiplies: the problem lists of its grouped GEMM launches (S1 / S2 / S5 / S6 of vsrcap.hip's header), ONCE for
// the decode step (run_step) and the training forward (vsr_train_forward, train.inc.h); at the end those of the training backward's step.  Host only: free functions that append problems to a
// GemmBuilder (gemm_route.h).  The order of the problems numbers the tiles and the order of a problem's segments is the summation order:
// both are part of the result's bits (tests/test_gpu_flip_rate.py has rejected a reorder).  Slab layout - which problems share a slab array,
// tight counts, which buffer a group's slabs land in - is stated next to each list as a SlabLayout (the *_slabs functions) and applied by
// place_slabs after finish(), which does not read C: the add_* functions leave C null.  The workspace sizes (carve, carve_train,
// vsr_decode_cache_floats) are computed from the same layouts (slab_floats).  tools/step_slabs_host.hip drives all of it on the CPU.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "../../include/vsrcap.h"
#include "gemm_route.h"

namespace vsr {

// ---- slab placement.  A slab GROUP is a run of consecutive problems of a planned launch that write column windows of ONE slab array
// (n, M, width): every problem has ldc = width and their columns are consecutive from 0 in problem order (LSTM1: 4H | H | H).  A layout
// lists the groups of a launch in problem order; groups of the same area are packed one behind the other.
constexpr int SLABS_LAUNCH = -2, SLABS_TIGHT = -1;    // SlabGroup::count: the launch's count, the largest gemm_tight_slabs of the group's problems; >= 0: that many
struct SlabGroup { int first, n, width, count, area; };    // problems [first, first + n); n = 0: absent (its view has no slabs).  area: index into place_slabs' areas
struct SlabLayout {
    int ng = 0;
    SlabGroup g[GEMM_MAX_PROB];
    SlabLayout& add(int n, int width, int count = SLABS_LAUNCH, int area = 0) {
        g[ng] = SlabGroup{ng ? g[ng - 1].first + g[ng - 1].n : 0, n, width, count, area};
        ++ng;
        return *this;
    }
};
struct SlabArea { float* base; size_t floats; };
struct SlabView { float* base; int n; long long stride; };      // what a group's consumer kernel is given
struct SlabPlan {
    SlabView v[GEMM_MAX_PROB];            // per group of the layout
    char err[200] = "";
    int refuse(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, sizeof(err), fmt, ap);
        va_end(ap);
        return 1;
    }
};
// floats per row and slab that the layout's groups take in an area, and what that area needs at M rows when every group has GEMM_MAX_SLABS slabs
inline size_t slab_row_floats(const SlabLayout& l, int area = 0) {
    size_t w = 0;
    for (int k = 0; k < l.ng; ++k)
        if (l.g[k].area == area) w += (size_t)l.g[k].width;
    return w;
}
inline size_t slab_floats(const SlabLayout& l, size_t M, int area = 0) { return M * slab_row_floats(l, area) * GEMM_MAX_SLABS; }
// the rest of `a` behind the slabs of v (decode S6's LSTM1 sums follow those the S5 launch wrote into pre1)
inline SlabArea area_behind(const SlabArea& a, const SlabView& v) {
    float* const end = v.base + v.stride * v.n;
    return SlabArea{end, a.floats - (size_t)(end - a.base)};
}
inline int tight_slabs(const GemmArgs& a, int first, int n) {
    int ns = 0;
    for (int i = first; i < first + n; ++i) ns = std::max(ns, gemm_tight_slabs(a, i));
    return ns;
}
// Sets C / slab_stride / nslab of every problem of the planned launch `a` (M rows each; nprob = 0: a launch that is not made) and leaves
// the groups' views in pl.v; `areas` holds narea areas.  Host arithmetic only.  Returns non-zero with pl.err set when the layout does not describe the launch or a
// group would end outside its area.
inline int place_slabs(GemmArgs& a, int M, const SlabLayout& l, const SlabArea* areas, int narea, SlabPlan& pl) {
    size_t used[GEMM_MAX_PROB] = {};      // per area
    int next = 0;
    for (int k = 0; k < l.ng; ++k) {
        const SlabGroup& G = l.g[k];
        if (G.first != next || G.n < 0 || G.first + G.n > a.nprob) return pl.refuse("slab group %d names problems %d .. %d of a launch of %d", k, G.first, G.first + G.n - 1, a.nprob);
        if (G.area < 0 || G.area >= narea || G.area >= GEMM_MAX_PROB) return pl.refuse("slab group %d names area %d of %d", k, G.area, narea);
        next += G.n;
        const int tight = tight_slabs(a, G.first, G.n);
        const int n = G.n == 0 ? 0 : (G.count == SLABS_LAUNCH ? a.nslab : (G.count == SLABS_TIGHT ? tight : G.count));
        if (n < tight) return pl.refuse("slab group %d is given %d slabs, its tiles write %d", k, n, tight);
        const long long stride = (long long)M * G.width;
        float* const base = areas[G.area].base + used[G.area];
        int col = 0;
        for (int i = G.first; i < G.first + G.n; ++i) {
            GemmProb& p = a.p[i];
            if (p.M != M || p.ldc != G.width) return pl.refuse("problem %d (%d rows, ldc %d) is not a window of slab group %d (%d rows, width %d)", i, p.M, p.ldc, k, M, G.width);
            p.C = base + col; p.slab_stride = stride; p.nslab = n;
            col += p.N;
        }
        if (col > G.width) return pl.refuse("the problems of slab group %d have %d columns, its slabs %d", k, col, G.width);
        used[G.area] += (size_t)stride * n;
        if (used[G.area] > areas[G.area].floats) return pl.refuse("slab group %d ends at %zu floats of an area of %zu", k, used[G.area], areas[G.area].floats);
        pl.v[k] = SlabView{base, n, stride};
    }
    if (next != a.nprob) return pl.refuse("the slab layout covers %d problems of a launch of %d", next, a.nprob);
    return 0;
}

// The A operands of one step: fp32 values, their 16-bit images (bf16, or fp16 pairs in the f16x2 flavour; null = none) and the row gathers
struct StepOperands {
    int M = 0;                                            // rows
    const float *h1_old = nullptr, *h2_old = nullptr;     // state before the step (rows gathered through `parent`) ...
    const float *h1_new = nullptr, *h2_new = nullptr;     // ... and after it
    const float *s_t = nullptr, *g_t = nullptr, *att = nullptr;
    const uint16_t *h1_old16 = nullptr, *h2_old16 = nullptr, *h1_new16 = nullptr, *h2_new16 = nullptr;
    const uint16_t *s_t16 = nullptr, *g_t16 = nullptr, *att16 = nullptr;
    const int* parent = nullptr;                          // beam parents or null
    const float* x = nullptr;                             // (., E) input embeddings: the embedding table gathered through `word`, or gathered rows (word = null)
    const int* word = nullptr;
};

// LSTM1 gates (4H) | sentinel gate (H) | shift-gate image part (H): {W_ih1, W1_is, W1_ig} x {W_hh1, W1_hs, -}, one slab group of width 6H.
// parts: which K segments a problem gets, always in the order h2, x, h1 (the h2 part only exists with h2_first_lstm).  L1_NEXT: the
// sums of the NEXT step - the state parts read this step's new state, ungathered.  A problem without a segment is skipped.
// Returns nblk, the gate blocks k_lstm1 has to add slabs for (4 / 5 / 6: through the last problem appended; 0 = none).
enum Lstm1Parts { L1_H2 = 1, L1_X = 2, L1_H1 = 4, L1_NEXT = 8 };
inline int add_lstm1(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const StepOperands& o, int parts) {
    const int H = d.rnn_size, E = d.input_encoding_size;
    const int xoff = (d.h2_first_lstm ? H : 0) + d.det_feat_size, in1 = xoff + E;
    const float* Wih[3] = {w.lstm1_weight_ih, w.W1_is_weight, w.W1_ig_weight};
    const float* Whh[3] = {w.lstm1_weight_hh, w.W1_hs_weight, nullptr};
    const int Nn[3] = {4 * H, H, H};
    const bool next = parts & L1_NEXT;
    const float *h1 = next ? o.h1_new : o.h1_old, *h2 = next ? o.h2_new : o.h2_old;
    const uint16_t *h1_16 = next ? o.h1_new16 : o.h1_old16, *h2_16 = next ? o.h2_new16 : o.h2_old16;
    const int* rows = next ? nullptr : o.parent;
    int nblk = 0;
    for (int i = 0; i < 3; ++i) {
        const bool has_h2 = (parts & L1_H2) && d.h2_first_lstm, has_x = parts & L1_X, has_h1 = (parts & L1_H1) && Whh[i];
        if (!has_h2 && !has_x && !has_h1) continue;
        GemmProb& p = g.prob(o.M, Nn[i], nullptr, 6 * H);
        if (has_h2) GemmBuilder::seg(p, h2, H, rows, Wih[i], in1, H, h2_16, H2A_UNIT);
        if (has_x) GemmBuilder::seg(p, o.x, E, o.word, Wih[i] + xoff, in1, E, nullptr, H2A_EMBED);
        if (has_h1) GemmBuilder::seg(p, h1, H, rows, Whh[i], H, H, h1_16, H2A_UNIT);
        nblk = i + 4;
    }
    return nblk;
}
// the nprob problems of an add_lstm1 list (a launch of its own: S1, the x projections of the decode cache and of training, the hoisted
// vbar projection, whose consumers sum the launch's count; as the tail of S5 / S6: tight, in `pre1`)
inline SlabLayout lstm1_slabs(const vsr_dims& d, int nprob = 3, int count = SLABS_LAUNCH, int area = 0) {
    return SlabLayout().add(nprob, 6 * d.rnn_size, count, area);
}

// S2: h1_new -> [W1_hg | att_ha] (ldc H + A),  s_t -> [s_fc | att_sa] (ldc D + A): two slab groups, the second packed behind the first
inline void add_s2(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const StepOperands& o) {
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size;
    GemmProb& p0 = g.prob(o.M, H, nullptr, H + A);
    GemmBuilder::seg(p0, o.h1_new, H, nullptr, w.W1_hg_weight, H, H, o.h1_new16, H2A_UNIT);
    GemmProb& p1 = g.prob(o.M, A, nullptr, H + A);
    GemmBuilder::seg(p1, o.h1_new, H, nullptr, w.att_ha_weight, H, H, o.h1_new16, H2A_UNIT);
    GemmProb& p2 = g.prob(o.M, D, nullptr, D + A);
    GemmBuilder::seg(p2, o.s_t, H, nullptr, w.s_fc_weight, H, H, o.s_t16, H2A_UNIT);
    GemmProb& p3 = g.prob(o.M, A, nullptr, D + A);
    GemmBuilder::seg(p3, o.s_t, H, nullptr, w.att_sa_weight, H, H, o.s_t16, H2A_UNIT);
}
inline SlabLayout s2_slabs(const vsr_dims& d) {
    return SlabLayout().add(2, d.rnn_size + d.att_size).add(2, d.det_feat_size + d.att_size);
}

// S5: [h1_new | att | h2_old] -> LSTM2 gates (ldc 4H; the h2 segment from step 1 on),  g_t -> att_ga (ldc A)
inline void add_s5(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const StepOperands& o, bool with_h2) {
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size, in2 = H + D + (d.img_second_lstm ? D : 0);
    GemmProb& p0 = g.prob(o.M, 4 * H, nullptr, 4 * H);
    GemmBuilder::seg(p0, o.h1_new, H, nullptr, w.lstm2_weight_ih, in2, H, o.h1_new16, H2A_UNIT);
    GemmBuilder::seg(p0, o.att, D, nullptr, w.lstm2_weight_ih + H, in2, D, o.att16, H2A_ATT);
    if (with_h2) GemmBuilder::seg(p0, o.h2_old, H, o.parent, w.lstm2_weight_hh, H, H, o.h2_old16, H2A_UNIT);
    GemmProb& p1 = g.prob(o.M, A, nullptr, A);
    GemmBuilder::seg(p1, o.g_t, H, nullptr, w.att_ga_weight, H, H, o.g_t16, H2A_UNIT);
}
// Training: both groups in area 0 with the launch's count (k_fwd_tail reads them side by side).  Decoding: every consumer reads its group
// on its own, so each is tight - LSTM2 in area 0 (k_lstm2), att_ga in area 1 (`ga_slabs`: the vocabulary GEMM overwrites area 0 before
// k_vocab forms the gate logits), and the h1 part of the next step's LSTM1 sums that the split composition appends in area 2 (`pre1`)
// with the ns_h1 slabs plan_s56 counted: the next step's LSTM1 kernel is told that number
inline SlabLayout s5_slabs(const vsr_dims& d) { return SlabLayout().add(1, 4 * d.rnn_size).add(1, d.att_size); }
inline SlabLayout s5_decode_slabs(const vsr_dims& d, int nprob = 2, int ns_h1 = 0) {
    return SlabLayout().add(1, 4 * d.rnn_size, SLABS_TIGHT).add(1, d.att_size, SLABS_TIGHT, 1).add(nprob - 2, 6 * d.rnn_size, ns_h1, 2);
}

// the vocabulary problem: h2_new (optionally gathered through `rows`) -> logits (ldc V)
inline void add_vocab(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const StepOperands& o, const int* rows = nullptr) {
    const int H = d.rnn_size, V = d.vocab_size;
    GemmProb& p0 = g.prob(o.M, V, nullptr, V);
    GemmBuilder::seg(p0, o.h2_new, H, rows, w.out_fc_weight, H, H, o.h2_new16, H2A_UNIT);
}
// Training: the launch's count.  Decoding (S6): tight - the vocabulary tiles (K = H) are cut into fewer pieces than the LSTM1 tiles of the
// next step (K = 2 H) that share the launch; those go to area 1, the rest of `pre1` behind what S5 wrote there, with plan_s56's ns_pre1 slabs
inline SlabLayout vocab_slabs(const vsr_dims& d) { return SlabLayout().add(1, d.vocab_size); }
inline SlabLayout s6_slabs(const vsr_dims& d, int nprob = 1, int ns_pre1 = 1) {
    return SlabLayout().add(1, d.vocab_size, SLABS_TIGHT).add(nprob - 1, 6 * d.rnn_size, ns_pre1, 1);
}

// S5 and S6 of a decode step are planned together, before either is launched.  S6 = the vocabulary problem + (for_next) the LSTM1 / gate
// sums of step t + 1 over THIS step's rows; split: their h1 part rides in S5 instead.  Both parts land in the GEMM_MAX_SLABS slabs of
// `pre1` - S5's in the leading ns_h1, S6's ns_pre1 behind them: when the two plans would not fit (the exact-fp32 flavour cuts its
// 64 x 64 tiles into up to 8 stream-K pieces) both launches are planned again without the split.
struct Step56 {
    GemmBuilder g5, g6;
    int ns_h1 = 0, ns_pre1 = 1, nblk6 = 0;     // slabs of the h1 part (S5) and of the rest (S6) of the next step's sums; their gate blocks (add_lstm1)
    bool replanned = false;
};
inline void plan_s56(const GemmState* st, const vsr_dims& d, const vsr_weights& w, const StepOperands& o, bool with_h2, bool for_next, bool want_split, Step56& p) {
    auto plan = [&](bool split) {
        p.g5 = GemmBuilder(); p.g6 = GemmBuilder();
        add_s5(p.g5, d, w, o, with_h2);
        if (split) add_lstm1(p.g5, d, w, o, L1_NEXT | L1_H1);
        add_vocab(p.g6, d, w, o);
        p.nblk6 = for_next ? add_lstm1(p.g6, d, w, o, L1_NEXT | L1_H2 | (split ? 0 : L1_H1)) : 0;
        p.g5.finish(st); p.g6.finish(st);
        // the LSTM1 / gate problems write (and k_lstm1 adds) only the slabs THEIR tiles can meet - all of a launch's get the largest of
        // their counts, k_lstm1 takes one count for its six gate blocks
        p.ns_h1 = tight_slabs(p.g5.a, 2, p.g5.a.nprob - 2);
        p.ns_pre1 = std::max(1, tight_slabs(p.g6.a, 1, p.g6.a.nprob - 1));
    };
    plan(want_split);
    p.replanned = p.ns_h1 > 0 && p.ns_h1 + p.ns_pre1 > GEMM_MAX_SLABS;
    if (p.replanned) plan(false);
}

// ---- the image-constant launches hoisted into vsr_prepare*(): the pooled descriptor's columns [voff, voff + D) of the LSTM1 / gate input
// weights (the list and slab group of add_lstm1), its columns of the LSTM2 input weights (img_second_lstm), att_va over the non-padding
// region rows (gathered through vlist; keep_fp32: gemm_route.h)
inline void add_vproj(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const float* vbar, int B) {
    const int H = d.rnn_size, D = d.det_feat_size, voff = d.h2_first_lstm ? H : 0, in1 = voff + D + d.input_encoding_size;
    GemmProb& p0 = g.prob(B, 4 * H, nullptr, 6 * H);
    GemmBuilder::seg(p0, vbar, D, nullptr, w.lstm1_weight_ih + voff, in1, D, nullptr, H2A_DET);
    GemmProb& p1 = g.prob(B, H, nullptr, 6 * H);
    GemmBuilder::seg(p1, vbar, D, nullptr, w.W1_is_weight + voff, in1, D, nullptr, H2A_DET);
    GemmProb& p2 = g.prob(B, H, nullptr, 6 * H);
    GemmBuilder::seg(p2, vbar, D, nullptr, w.W1_ig_weight + voff, in1, D, nullptr, H2A_DET);
}
inline void add_vproj2(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const float* vbar, int B) {
    const int H = d.rnn_size, D = d.det_feat_size, in2 = H + 2 * D;
    GemmProb& p0 = g.prob(B, 4 * H, nullptr, 4 * H);
    GemmBuilder::seg(p0, vbar, D, nullptr, w.lstm2_weight_ih + H + D, in2, D, nullptr, H2A_DET);
}
inline SlabLayout vproj2_slabs(const vsr_dims& d) { return SlabLayout().add(1, 4 * d.rnn_size); }
inline void add_att_va(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const float* regions, const int* vlist, int nvalid) {
    const int A = d.att_size, D = d.det_feat_size;
    g.keep_fp32 = true;
    GemmProb& p0 = g.prob(nvalid, A, nullptr, A);
    GemmBuilder::seg(p0, regions, D, vlist, w.att_va_weight, D, D, nullptr, H2A_REGION);
}
inline SlabLayout att_va_slabs(const vsr_dims& d) { return SlabLayout().add(1, d.att_size); }

// ---- the training backward's step: its three grouped data-gradient GEMMs against the TRANSPOSED weights (train.inc.h, train_backward_step).
// The step's gradient rows, the transposed weights and the exponent slots of the gradients (H2A_NONE: the launch cannot take the f16x2
// kernels).  Every problem is a slab group of its own, packed in the training scratch with the launch's count.  Problem order and segment
// order are part of the bits here too.
struct BwdStepOperands {
    int M = 0;
    const float *dpre1 = nullptr, *dpre2 = nullptr;       // (M, 6H) [LSTM1 gates | sentinel gate | dq], (M, 4H)
    const float *dhA = nullptr, *dsent = nullptr, *dsa = nullptr, *dga = nullptr;
    const float *wT_ih1 = nullptr, *wT_is = nullptr, *wT_ig = nullptr, *wT_hh1 = nullptr, *wT_hs = nullptr, *wT_ih2 = nullptr, *wT_hh2 = nullptr;
    const float *wT_hg = nullptr, *wT_ha = nullptr, *wT_sfc = nullptr, *wT_sa = nullptr, *wT_ga = nullptr;
    int s_dpre1 = H2A_NONE, s_dpre2 = H2A_NONE, s_dq = H2A_NONE, s_dhA = H2A_NONE, s_dsent = H2A_NONE, s_dsa = H2A_NONE, s_dga = H2A_NONE;
};
// GEMM 1: dpre2 -> [dh1_a | datt (| dvbar)] (N = H + D: the first rows of W_ih2^T), dpre2 -> the hh part of the dh2 carry, dga -> dg_t
inline void add_bwd1(GemmBuilder& g, const vsr_dims& d, const BwdStepOperands& o) {
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size;
    GemmProb& p0 = g.prob(o.M, H + D, nullptr, H + D);
    GemmBuilder::seg(p0, o.dpre2, 4 * H, nullptr, o.wT_ih2, 4 * H, 4 * H, nullptr, o.s_dpre2);
    GemmProb& p1 = g.prob(o.M, H, nullptr, H);
    GemmBuilder::seg(p1, o.dpre2, 4 * H, nullptr, o.wT_hh2, 4 * H, 4 * H, nullptr, o.s_dpre2);
    GemmProb& p2 = g.prob(o.M, H, nullptr, H);
    GemmBuilder::seg(p2, o.dga, A, nullptr, o.wT_ga, A, A, nullptr, o.s_dga);
}
// GEMM 2: [dq | dhA] -> dh1_b,  [dsent | dsa] -> ds_t
inline void add_bwd2(GemmBuilder& g, const vsr_dims& d, const BwdStepOperands& o) {
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size;
    GemmProb& p0 = g.prob(o.M, H, nullptr, H);
    GemmBuilder::seg(p0, o.dpre1 + 5 * H, 6 * H, nullptr, o.wT_hg, H, H, nullptr, o.s_dq);
    GemmBuilder::seg(p0, o.dhA, A, nullptr, o.wT_ha, A, A, nullptr, o.s_dhA);
    GemmProb& p1 = g.prob(o.M, H, nullptr, H);
    GemmBuilder::seg(p1, o.dsent, D, nullptr, o.wT_sfc, D, D, nullptr, o.s_dsent);
    GemmBuilder::seg(p1, o.dsa, A, nullptr, o.wT_sa, A, A, nullptr, o.s_dsa);
}
// GEMM 3: dpre1 -> the dh1 carry, then (h2_first_lstm) the LSTM1-input part of the dh2 carry: rows 0 .. H-1 of W_ih1^T / W1_is^T / W1_ig^T = their h2 columns
inline void add_bwd3(GemmBuilder& g, const vsr_dims& d, const BwdStepOperands& o) {
    const int H = d.rnn_size;
    GemmProb& p1 = g.prob(o.M, H, nullptr, H);
    GemmBuilder::seg(p1, o.dpre1, 6 * H, nullptr, o.wT_hh1, 4 * H, 4 * H, nullptr, o.s_dpre1);
    GemmBuilder::seg(p1, o.dpre1 + 4 * H, 6 * H, nullptr, o.wT_hs, H, H, nullptr, o.s_dpre1);
    if (d.h2_first_lstm) {
        GemmProb& p0 = g.prob(o.M, H, nullptr, H);
        GemmBuilder::seg(p0, o.dpre1, 6 * H, nullptr, o.wT_ih1, 4 * H, 4 * H, nullptr, o.s_dpre1);
        GemmBuilder::seg(p0, o.dpre1 + 4 * H, 6 * H, nullptr, o.wT_is, H, H, nullptr, o.s_dpre1);
        GemmBuilder::seg(p0, o.dpre1 + 5 * H, 6 * H, nullptr, o.wT_ig, H, H, nullptr, o.s_dq);
    }
}
// GEMM 1 is read by k_bwd_mid, GEMM 2 by k_bwd_tail.  GEMM 3's slabs stay live until the NEXT step's k_bwd_head (which runs before that
// step's GEMM 1 overwrites them); nprob = 0: no launch (step 0, and before the first step) - both views then have no slabs
inline SlabLayout bwd1_slabs(const vsr_dims& d) { return SlabLayout().add(1, d.rnn_size + d.det_feat_size).add(1, d.rnn_size).add(1, d.rnn_size); }
inline SlabLayout bwd2_slabs(const vsr_dims& d) { return SlabLayout().add(1, d.rnn_size).add(1, d.rnn_size); }
inline SlabLayout bwd3_slabs(const vsr_dims& d, int nprob) { return SlabLayout().add(nprob > 0, d.rnn_size).add(nprob > 1, d.rnn_size); }

}  // namespace vsr
