// What a decoder timestep multiplies: the problem lists of its grouped GEMM launches (S1 / S2 / S5 / S6 of vsrcap.hip's header), ONCE for
// the decode step (run_step) and the training forward (vsr_train_forward, train.inc.h); at the end those of the training backward's step.  Host only: free functions that append problems to a
// GemmBuilder (gemm_route.h).  The order of the problems numbers the tiles and the order of a problem's segments is the summation order:
// both are part of the result's bits (tests/test_gpu_flip_rate.py has rejected a reorder).  Slab layout - tight counts, which buffer a
// problem's slabs land in - is the caller's: finish() does not read C, so a caller patches C / slab_stride / nslab after planning.
#pragma once
#include "../../include/vsrcap.h"
#include "gemm_route.h"

namespace vsr {

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

// LSTM1 gates (4H) | sentinel gate (H) | shift-gate image part (H): {W_ih1, W1_is, W1_ig} x {W_hh1, W1_hs, -} into dst + {0, 4H, 5H}, ldc 6H.
// parts: which K segments a problem gets, always in the order h2, x, h1 (the h2 part only exists with h2_first_lstm).  L1_NEXT: the
// sums of the NEXT step - the state parts read this step's new state, ungathered.  A problem without a segment is skipped.
// Returns nblk, the gate blocks k_lstm1 has to add slabs for (4 / 5 / 6: through the last problem appended; 0 = none).
enum Lstm1Parts { L1_H2 = 1, L1_X = 2, L1_H1 = 4, L1_NEXT = 8 };
inline int add_lstm1(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const StepOperands& o, float* dst, int parts) {
    const int H = d.rnn_size, E = d.input_encoding_size;
    const int xoff = (d.h2_first_lstm ? H : 0) + d.det_feat_size, in1 = xoff + E;
    const float* Wih[3] = {w.lstm1_weight_ih, w.W1_is_weight, w.W1_ig_weight};
    const float* Whh[3] = {w.lstm1_weight_hh, w.W1_hs_weight, nullptr};
    const int Nn[3] = {4 * H, H, H}, off[3] = {0, 4 * H, 5 * H};
    const bool next = parts & L1_NEXT;
    const float *h1 = next ? o.h1_new : o.h1_old, *h2 = next ? o.h2_new : o.h2_old;
    const uint16_t *h1_16 = next ? o.h1_new16 : o.h1_old16, *h2_16 = next ? o.h2_new16 : o.h2_old16;
    const int* rows = next ? nullptr : o.parent;
    int nblk = 0;
    for (int i = 0; i < 3; ++i) {
        const bool has_h2 = (parts & L1_H2) && d.h2_first_lstm, has_x = parts & L1_X, has_h1 = (parts & L1_H1) && Whh[i];
        if (!has_h2 && !has_x && !has_h1) continue;
        GemmProb& p = g.prob(o.M, Nn[i], dst + off[i], 6 * H);
        if (has_h2) GemmBuilder::seg(p, h2, H, rows, Wih[i], in1, H, h2_16, H2A_UNIT);
        if (has_x) GemmBuilder::seg(p, o.x, E, o.word, Wih[i] + xoff, in1, E, nullptr, H2A_EMBED);
        if (has_h1) GemmBuilder::seg(p, h1, H, rows, Whh[i], H, H, h1_16, H2A_UNIT);
        nblk = i + 4;
    }
    return nblk;
}

// S2: h1_new -> [W1_hg | att_ha] (slabs at c2a, ldc H + A),  s_t -> [s_fc | att_sa] (placed by place_s2 once the slab count is known)
inline void add_s2(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const StepOperands& o, float* c2a) {
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size;
    GemmProb& p0 = g.prob(o.M, H, c2a, H + A);
    GemmBuilder::seg(p0, o.h1_new, H, nullptr, w.W1_hg_weight, H, H, o.h1_new16, H2A_UNIT);
    GemmProb& p1 = g.prob(o.M, A, c2a + H, H + A);
    GemmBuilder::seg(p1, o.h1_new, H, nullptr, w.att_ha_weight, H, H, o.h1_new16, H2A_UNIT);
    GemmProb& p2 = g.prob(o.M, D, nullptr, D + A);
    GemmBuilder::seg(p2, o.s_t, H, nullptr, w.s_fc_weight, H, H, o.s_t16, H2A_UNIT);
    GemmProb& p3 = g.prob(o.M, A, nullptr, D + A);
    GemmBuilder::seg(p3, o.s_t, H, nullptr, w.att_sa_weight, H, H, o.s_t16, H2A_UNIT);
}
// ... after finish(): the ns slabs of the second pair follow the ns slabs of the first.  Returns c2b, the second pair's base.
struct S2Layout { float* c2b; long long stride_a, stride_b; };
inline S2Layout place_s2(GemmBuilder& g, const vsr_dims& d, int M, float* c2a, int ns) {
    const S2Layout l{c2a + (long long)M * (d.rnn_size + d.att_size) * ns, (long long)M * (d.rnn_size + d.att_size), (long long)M * (d.det_feat_size + d.att_size)};
    g.a.p[0].slab_stride = g.a.p[1].slab_stride = l.stride_a;
    g.a.p[2].C = l.c2b; g.a.p[3].C = l.c2b + d.det_feat_size;
    g.a.p[2].slab_stride = g.a.p[3].slab_stride = l.stride_b;
    return l;
}

// S5: [h1_new | att | h2_old] -> LSTM2 gates (slabs at dst, ldc 4H; the h2 segment from step 1 on),  g_t -> att_ga (placed by the caller)
inline void add_s5(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const StepOperands& o, float* dst, bool with_h2) {
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size, in2 = H + D + (d.img_second_lstm ? D : 0);
    GemmProb& p0 = g.prob(o.M, 4 * H, dst, 4 * H);
    GemmBuilder::seg(p0, o.h1_new, H, nullptr, w.lstm2_weight_ih, in2, H, o.h1_new16, H2A_UNIT);
    GemmBuilder::seg(p0, o.att, D, nullptr, w.lstm2_weight_ih + H, in2, D, o.att16, H2A_ATT);
    if (with_h2) GemmBuilder::seg(p0, o.h2_old, H, o.parent, w.lstm2_weight_hh, H, H, o.h2_old16, H2A_UNIT);
    GemmProb& p1 = g.prob(o.M, A, nullptr, A);
    GemmBuilder::seg(p1, o.g_t, H, nullptr, w.att_ga_weight, H, H, o.g_t16, H2A_UNIT);
}

// the vocabulary problem: h2_new (optionally gathered through `rows`) -> logits (slabs at dst, ldc V)
inline void add_vocab(GemmBuilder& g, const vsr_dims& d, const vsr_weights& w, const StepOperands& o, float* dst, const int* rows = nullptr) {
    const int H = d.rnn_size, V = d.vocab_size;
    GemmProb& p0 = g.prob(o.M, V, dst, V);
    GemmBuilder::seg(p0, o.h2_new, H, rows, w.out_fc_weight, H, H, o.h2_new16, H2A_UNIT);
}

// ---- the training backward's step: its three grouped data-gradient GEMMs against the TRANSPOSED weights (train.inc.h, train_backward_step).
// The step's gradient rows, the transposed weights and the exponent slots of the gradients (H2A_NONE: the launch cannot take the f16x2
// kernels).  C is left null: every problem's slabs are placed by the caller.  Problem order and segment order are part of the bits here too.
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

}  // namespace vsr
