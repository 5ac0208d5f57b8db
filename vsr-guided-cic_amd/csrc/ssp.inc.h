// C ABI of the two ordering models that feed the decoder in the eval loop; included at the end of vsrcap.hip.
// Reference: coco_scripts/eval_coco.py:127-221 calls S_SSP.generate (batch size 1) once per (caption, verb) and
// SinkhornNet + munkres once per repeated role, each with host round trips; here ALL sequences / items of a loader batch go
// through one call each, and the results (role orders, assignments) stay on the device: vsr_rank_captions (at the end of this
// file, kernels in rank_kernels.h) turns them into the (N, L) rank tensor vsr_reorder_slots consumes without a read-back.
// vsrcap/evalbatch.py: rank_captions is the same flow with the integer bookkeeping on the host.
// Each model has ONE forward on the host: ssp_layer is the transformer layer of vsr_ssp_generate (encoder and every decode step) and of
// vsr_ssp_train_forward, sinkhorn_layers the five layers of assign, rank and the Sinkhorn training forward.  What training differentiates
// is what inference runs by construction, not by copies kept alike.
#include "ssp_kernels.h"
#include "rank_kernels.h"
#include "train_batch_kernels.h"

struct vsr_ssp {
    GemmState cfg;                   // GEMM launch configuration only (stream-K slots, tile choice); fp32
    vsr_ssp_weights w;
    vsr_sinkhorn_weights sw;
    bool has_ssp = false, has_sh = false;
};

extern "C" int vsr_ssp_create(vsr_ssp** out) {
    if (!out) return fail("vsr_ssp_create: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("vsr_ssp_create: no HIP device");
    vsr_ssp* e = new vsr_ssp();
    e->cfg.x3_on = false;            // the ordering models stay on the exact fp32 chain (their fixtures pin integer-truncated log-probs)
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) e->cfg.gk.set_cus(prop.multiProcessorCount);
    *out = e;
    return 0;
}
extern "C" void vsr_ssp_destroy(vsr_ssp* e) { delete e; }

extern "C" int vsr_ssp_bind(vsr_ssp* e, const vsr_ssp_weights* w, const vsr_sinkhorn_weights* sw) {
    if (!e) return fail("vsr_ssp_bind: null handle");
    if (w) {
        if (!w->sr_embed || !w->v_embed || !w->fc_w || !w->exp_w || w->n_verbs <= 0) return fail("vsr_ssp_bind: incomplete S-SSP weights");
        e->w = *w;
        e->has_ssp = true;
    }
    if (sw) {
        if (!sw->W1_txt_w || !sw->W_fc_w || sw->N < 2 || sw->N > 16 || sw->n_iters < 0 || !(sw->tau > 0.f)) return fail("vsr_ssp_bind: bad Sinkhorn weights (2 <= N <= 16)");
        e->sw = *sw;
        e->has_sh = true;
    }
    return 0;
}

struct SspWs {
    float *x, *y, *q, *k, *v, *ctx, *x1, *ff, *prior, *pk[3], *pv[3], *last, *logits, *scratch;
    int *roles32, *remain, *tokens;
    size_t scratch_floats;
};
static size_t carve_ssp(int S, char* base, SspWs& w) {
    const size_t R = (size_t)S * (SSP_LEN + 1), H = SSP_H;
    Bump b{base};
    w.x = b.take<float>(R * H); w.y = b.take<float>(R * H); w.q = b.take<float>(R * H); w.k = b.take<float>(R * H);
    w.v = b.take<float>(R * H); w.ctx = b.take<float>(R * H); w.x1 = b.take<float>(R * H); w.ff = b.take<float>(R * SSP_FF);
    w.prior = b.take<float>((size_t)S * SSP_LEN * H);
    for (int l = 0; l < 3; ++l) { w.pk[l] = b.take<float>((size_t)S * SSP_LEN * H); w.pv[l] = b.take<float>((size_t)S * SSP_LEN * H); }
    w.last = b.take<float>((size_t)S * H); w.logits = b.take<float>((size_t)S * SSP_ROLES);
    w.roles32 = b.take<int>((size_t)S * SSP_LEN); w.remain = b.take<int>((size_t)S * SSP_LEN); w.tokens = b.take<int>(R);
    w.scratch_floats = R * SSP_FF * GEMM_MAX_SLABS;
    w.scratch = b.take<float>(w.scratch_floats);
    return (b.off + 255) & ~size_t(255);
}
extern "C" size_t vsr_ssp_workspace_bytes(int32_t S) {
    if (S <= 0) return 0;
    SspWs w;
    return carve_ssp(S, nullptr, w);
}

// ---------------------------------------------------------------------------------------------- the dense products
// Inference, SinkhornNet's and S-SSP's training passes describe each product as a Prod and hand it to run_products (products.h), on the
// exact fp32 kernels; their launches are not part of any GEMM profile.
static ProdRun ssp_run(const vsr_ssp* e, hipStream_t s, float* scratch, size_t scratch_floats, const int* hdr, float scale, const char* pass) {
    return ProdRun{&e->cfg, nullptr, s, scratch, scratch_floats, hdr, scale, pass};
}

// ---------------------------------------------------------------------------------------------- the S-SSP layer
// Where a layer's intermediates land: the training tape's entries, or a view of the inference workspace (ssp_ws_view) whose xhat / rstd / P
// are null - which selects the plain kernels: inference writes no tape data.
struct SspLnTape { float *y, *xhat, *rstd; };
// lnA / lnC / lnF: the LayerNorm in front of the self attention / cross attention (decoder only) / feed-forward.  pk set: a decoder layer
struct SspLayerTape { SspLnTape lnA, lnC, lnF; float *q, *k, *v, *P1, *ctx1, *q2, *pk, *pv, *P2, *ctx2, *ff; };
static SspLayerTape ssp_ws_view(const SspWs& ws, int dec_layer /* -1: an encoder layer */) {
    SspLayerTape v{};
    v.lnA.y = v.lnC.y = v.lnF.y = ws.y;
    v.q = v.q2 = ws.q; v.k = ws.k; v.v = ws.v; v.ctx1 = v.ctx2 = ws.ctx; v.ff = ws.ff;
    if (dec_layer >= 0) { v.pk = ws.pk[dec_layer]; v.pv = ws.pv[dec_layer]; }
    return v;
}
static void layernorm(hipStream_t s, const float* x, const float* w, const float* b, int rows, const SspLnTape& t) {
    if (t.xhat) hipLaunchKernelGGL(k_layernorm512_train, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, w, b, rows, t.y, t.xhat, t.rstd);
    else hipLaunchKernelGGL(k_layernorm512, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, w, b, rows, t.y);
}
// ctx (S, Tq, 512) = multi-head attention of q (S, Tq) on k / v (S, Tk).  P set: the softmax weights are taped and the site's keep bytes applied
static void ssp_mha(const ProdRun& run, const float* q, const float* k, const float* v, int S, int Tq, int Tk, const int* mask_tok, int ld_tok, float* ctx, float* P,
                    const uint8_t* keep) {
    if (P) hipLaunchKernelGGL(k_ssp_mha_train, dim3(S, SSP_HEADS), dim3(64), 0, run.s, q, k, v, Tq, Tk, mask_tok, ld_tok, ctx, P, keep, run.scale);
    else hipLaunchKernelGGL(k_ssp_mha, dim3(S, SSP_HEADS), dim3(64), 0, run.s, q, k, v, Tq, Tk, mask_tok, ld_tok, ctx);
}
// keys / values of a decoder layer's cross attention: the prior (Re rows) through the layer's (self-)attention K / V projections
// (sort_modules.py:88 re-uses self.attention for the cross attention), one launch
static int ssp_cross_kv(const ProdRun& run, const vsr_ssp_layer& ly, const float* prior, int Re, float* pk, float* pv) {
    Prod kv[2] = {lin(Re, SSP_H, SSP_H, prior, SSP_H, ly.Wk, ly.bk, pk), lin(Re, SSP_H, SSP_H, prior, SSP_H, ly.Wv, ly.bv, pv)};
    return run_products(run, kv, 2);
}
// One pre-LN layer of either stack for S sequences of T positions: THE layer of generate (encoder, every decode step) and of the training forward.
// The input is in x and so is the output on return; x1 is the other row buffer (the two are exchanged when the result falls into it).
//   mask_tok  the decoder's self-attention mask tokens (leading dimension ld_tok), or null
//   prior     decoder: the encoder's output, projected to lt.pk / lt.pv here, after the q2 product; null: the caller has filled them
//   keep      the keep bytes of the layer's dropout sites in order (4 encoder, 6 decoder), each null without dropout; run.scale = 1 / (1 - p)
static const uint8_t* const SSP_NO_DROPOUT[6] = {};
static int ssp_layer(const ProdRun& run, const vsr_ssp_layer& ly, const SspLayerTape& lt, int S, int T, const int* mask_tok, int ld_tok, const float* prior,
                     const uint8_t* const* keep, float*& x, float*& x1) {
    const int H = SSP_H, R = S * T;
    const bool dec = lt.pk != nullptr;
    // ---- self attention: x1 = drop(Wo ctx1 + bo) + x, ctx1 = mha(q, k, v = W yA + b), yA = LN(x); the three projections in one launch
    layernorm(run.s, x, ly.ln1_w, ly.ln1_b, R, lt.lnA);
    Prod qkv[3] = {lin(R, H, H, lt.lnA.y, H, ly.Wq, ly.bq, lt.q), lin(R, H, H, lt.lnA.y, H, ly.Wk, ly.bk, lt.k), lin(R, H, H, lt.lnA.y, H, ly.Wv, ly.bv, lt.v)};
    if (run_products(run, qkv, 3)) return 1;
    ssp_mha(run, lt.q, lt.k, lt.v, S, T, T, mask_tok, ld_tok, lt.ctx1, lt.P1, keep[0]);
    if (run_product(run, lin(R, H, H, lt.ctx1, H, ly.Wo, ly.bo, x1, SSP_ACT_NONE, x, keep[1]))) return 1;
    keep += 2;
    if (dec) {
        // ---- cross attention: x = drop(Wo ctx2 + bo) + x1, ctx2 = mha(q2 = Wq yC + bq, pk, pv), yC = LN(x1): the SAME projections (sort_modules.py:87)
        layernorm(run.s, x1, ly.ln2_w, ly.ln2_b, R, lt.lnC);
        if (run_product(run, lin(R, H, H, lt.lnC.y, H, ly.Wq, ly.bq, lt.q2))) return 1;
        if (prior && ssp_cross_kv(run, ly, prior, S * SSP_LEN, lt.pk, lt.pv)) return 1;
        ssp_mha(run, lt.q2, lt.pk, lt.pv, S, T, SSP_LEN, nullptr, 0, lt.ctx2, lt.P2, keep[0]);
        if (run_product(run, lin(R, H, H, lt.ctx2, H, ly.Wo, ly.bo, x, SSP_ACT_NONE, x1, keep[1]))) return 1;
        std::swap(x, x1);                                                                             // (x1 names the feed-forward's input again)
        keep += 2;
    }
    // ---- feed-forward: x = drop(W2 ff + b2) + x1, ff = drop(relu(W1 yF + b1)), yF = LN(x1)
    layernorm(run.s, x1, dec ? ly.ln3_w : ly.ln2_w, dec ? ly.ln3_b : ly.ln2_b, R, lt.lnF);
    if (run_product(run, lin(R, SSP_FF, H, lt.lnF.y, H, ly.W1, ly.b1, lt.ff, SSP_ACT_RELU, nullptr, keep[0]))) return 1;
    return run_product(run, lin(R, H, SSP_FF, lt.ff, SSP_FF, ly.W2, ly.b2, x, SSP_ACT_NONE, x1, keep[1]));
}

// S_SSP.generate(mode='not-normal') (sort_model.py:105-183) for S sequences at once.
//   verbs (S) int64 (taken % 10000 as in :108), roles (S, 10) int32 role ids, 0 = padding (the reference's verb_det_seqs_sr)
//   pred (S, 10) int32: roles in generated order, 0 beyond; logp (S, 10) fp32: log-prob of each pick (the reference returns these
//   truncated to integers - its buffer inherits the integer dtype of the role tensor, :121 - and its callers ignore them)
extern "C" int vsr_ssp_generate(vsr_ssp* e, const int64_t* verbs, const int32_t* roles, int32_t S, int32_t* pred, float* logp, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (!e || !e->has_ssp) return fail("vsr_ssp_generate: S-SSP weights not bound");
    if (!verbs || !roles || !pred || !logp || !workspace || S <= 0) return fail("vsr_ssp_generate: bad arguments");
    SspWs ws;
    if (carve_ssp(S, reinterpret_cast<char*>(workspace), ws) > workspace_bytes) return fail("vsr_ssp_generate: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const vsr_ssp_weights& w = e->w;
    const int H = SSP_H, L = SSP_LEN;
    const ProdRun run = ssp_run(e, s, ws.scratch, ws.scratch_floats, nullptr, 1.f, "ssp");
    hipLaunchKernelGGL(k_ssp_init, dim3(cdiv(S * (L + 1), 256)), dim3(256), 0, s, roles, S, ws.remain, ws.tokens, pred, logp);
    // ---- encoder (sort_modules.py:50-62): embeddings -> fc_feat -> 3 pre-LN layers -> LN
    int R = S * L;
    hipLaunchKernelGGL(k_ssp_embed, dim3(R), dim3(128), 0, s, roles, L, L, w.sr_embed, verbs, w.v_embed, w.n_verbs, S, ws.y);
    if (run_product(run, lin(R, H, H, ws.y, H, w.fc_w, w.fc_b, ws.x))) return 1;
    for (int l = 0; l < 3; ++l)
        if (ssp_layer(run, w.enc[l], ssp_ws_view(ws, -1), S, L, nullptr, 0, nullptr, SSP_NO_DROPOUT, ws.x, ws.x1)) return 1;
    layernorm(s, ws.x, w.enc_ln_w, w.enc_ln_b, R, SspLnTape{ws.prior, nullptr, nullptr});
    // the cross attention's keys / values are constant over the decode steps: projected once, here
    for (int l = 0; l < 3; ++l)
        if (ssp_cross_kv(run, w.dec[l], ws.prior, R, ws.pk[l], ws.pv[l])) return 1;
    LAUNCHCHK();
    // ---- decoder: step t re-runs the stack on [bos, picks 0..t-1] as the reference does (:154-160) and picks among the remaining roles
    for (int t = 0; t < L; ++t) {
        const int T = t + 1;
        hipLaunchKernelGGL(k_ssp_embed, dim3(S * T), dim3(128), 0, s, ws.tokens, L + 1, T, w.sr_embed, (const int64_t*)nullptr, (const float*)nullptr, 0, S, ws.x);
        for (int l = 0; l < 3; ++l)
            if (ssp_layer(run, w.dec[l], ssp_ws_view(ws, l), S, T, ws.tokens, L + 1, nullptr, SSP_NO_DROPOUT, ws.x, ws.x1)) return 1;
        hipLaunchKernelGGL(k_ssp_last, dim3(S), dim3(128), 0, s, ws.x, T, ws.last);
        layernorm(s, ws.last, w.dec_ln_w, w.dec_ln_b, S, SspLnTape{ws.y, nullptr, nullptr});
        if (run_product(run, lin(S, SSP_ROLES, H, ws.y, H, w.exp_w, w.exp_b, ws.logits))) return 1;
        hipLaunchKernelGGL(k_ssp_select, dim3(S), dim3(64), 0, s, ws.logits, roles, ws.remain, t, S, ws.tokens, pred, logp);
        LAUNCHCHK();
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- SinkhornNet
// The outputs of SinkhornNet's five layers and of k_sh_cat for R = Q N rows: t1 (R, 128), v1 (R, 512), v2 (R, 128), cat (R, 260), f1 (R, 256),
// th (R, N; tanh applied).  The training tape keeps them; inference only passes through them.
struct ShActs { float *t1, *v1, *v2, *cat, *f1, *th; };
static void carve_sh_acts(Bump& b, size_t R, int N, ShActs& a) {
    a.t1 = b.take<float>(R * 128); a.v1 = b.take<float>(R * 512); a.v2 = b.take<float>(R * 128); a.cat = b.take<float>(R * 260);
    a.f1 = b.take<float>(R * 256); a.th = b.take<float>(R * N);
}
struct ShWs { ShActs a; float* scratch; size_t scratch_floats; };
static size_t carve_sh_ws(int Q, int N, char* base, ShWs& w) {
    const size_t R = (size_t)Q * N;
    Bump b{base};
    carve_sh_acts(b, R, N, w.a);
    w.scratch_floats = R * 512 * GEMM_MAX_SLABS;
    w.scratch = b.take<float>(w.scratch_floats);
    return (b.off + 255) & ~size_t(255);
}
extern "C" size_t vsr_sinkhorn_workspace_bytes(int32_t Q, int32_t N) {
    if (Q <= 0 || N <= 0) return 0;
    ShWs w;
    return carve_sh_ws(Q, N, nullptr, w);
}
// The five layers of SinkhornNet for Q items: seq (Q, N, 2352) -> a.th (Q, N, N).  The ONE forward of vsr_sinkhorn_assign, vsr_rank_captions
// and vsr_sinkhorn_train_forward: with the Sinkhorn arithmetic they also share (sinkhorn_normalise), the training forward's tr has assign's bits.
static int sinkhorn_layers(const ProdRun& c, const vsr_sinkhorn_weights& w, const float* seq, int Q, const ShActs& a) {
    const int N = w.N, R = Q * N;
    if (run_product(c, lin(R, 128, 300, seq, SH_ROW, w.W1_txt_w, w.W1_txt_b, a.t1, SSP_ACT_RELU))) return 1;
    if (run_product(c, lin(R, 512, 2048, seq + 300, SH_ROW, w.W1_vis_w, w.W1_vis_b, a.v1, SSP_ACT_RELU))) return 1;
    if (run_product(c, lin(R, 128, 512, a.v1, 512, w.W2_vis_w, w.W2_vis_b, a.v2, SSP_ACT_RELU))) return 1;
    hipLaunchKernelGGL(k_sh_cat, dim3(cdiv((long long)R * 260, 256)), dim3(256), 0, c.s, a.t1, a.v2, seq, R, a.cat);
    if (run_product(c, lin(R, 256, 260, a.cat, 260, w.W_fc_pos_w, w.W_fc_pos_b, a.f1, SSP_ACT_RELU))) return 1;
    return run_product(c, lin(R, N, 256, a.f1, 256, w.W_fc_w, w.W_fc_b, a.th, SSP_ACT_TANH));
}
// SinkhornNet.forward (sinkhorn_network.py:39-51) + the assignment of eval_coco.py:185-189 for Q items at once.
//   seq (Q, N, 2352) fp32 rows [300 | 2048 | 4]; tr (Q, N, N) fp32 or NULL: the doubly-normalised matrix; assign (Q, N) int32:
//   assign[q][i] = column chosen for row i of tr[q]^T (the munkres result "(i, assign)" of :187).
extern "C" int vsr_sinkhorn_assign(vsr_ssp* e, const float* seq, int32_t Q, float* tr, int32_t* assign, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!e || !e->has_sh) return fail("vsr_sinkhorn_assign: Sinkhorn weights not bound");
    if (!seq || !assign || !workspace || Q <= 0) return fail("vsr_sinkhorn_assign: bad arguments");
    const vsr_sinkhorn_weights& w = e->sw;
    ShWs ws;
    if (carve_sh_ws(Q, w.N, reinterpret_cast<char*>(workspace), ws) > workspace_bytes) return fail("vsr_sinkhorn_assign: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (sinkhorn_layers(ssp_run(e, s, ws.scratch, ws.scratch_floats, nullptr, 1.f, "sinkhorn forward"), e->sw, seq, Q, ws.a)) return 1;
    hipLaunchKernelGGL(k_sinkhorn_assign, dim3(Q), dim3(64), 0, s, ws.a.th, w.N, w.n_iters, w.tau, tr, assign);
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- SinkhornNet training
// coco_scripts/train_sinkhorn.py:137-215 calls the net once per (image, caption, verb, repeated role) at batch size 1 and adds the
// losses on the host; here ONE forward, ONE fused location loss and ONE backward serve all Q items of a loader batch.
//   forward   sinkhorn_layers and the Sinkhorn arithmetic of vsr_sinkhorn_assign (tr is bit-identical to assign's), the layers' outputs
//             written into the caller's TAPE; no assignment
//   backward  k_sinkhorn_bwd (ssp_kernels.h: the divisor tape), then the five layers: ReLU masks from the taped outputs, bias
//             gradients by the ordered column sums of the decoder's training pass (k_colsum), dW = dY^T X and dX = dY W as NT
//             products on transposed copies (k_transpose_multi), all on the exact fp32 kernels.  No gradient flows to seq, so
//             the two input layers have no dX product (the 2048-wide one is the largest of the pass).
// The k extent of the dW products is R = Q N, any integer: the transposed copies have the leading dimension Rp = R rounded up to 4
// (what gemm_f32.h asks of K and the leading dimensions) and k_transpose_* zero the padding columns.  d_pre and W_fc^T are padded
// to Np = N rounded up to 4 in the same way.
// The tape's size is a function of (Q, N) alone, so each item has room for 2 x SH_TRAIN_MAX_ITERS divisor rows whatever n_iters is
// bound.  The forward RECORDS its n_iters and tau in the tape's header and packs the divisors at the stride 2 n_iters N; the
// backward takes both from the header, never from the binding, so it differentiates the forward that wrote the tape even when
// the object was re-bound in between (k_sinkhorn_bwd clamps the header's n_iters to the slot: a tape no forward wrote cannot
// send it out of bounds).
constexpr int SH_TRAIN_MAX_ITERS = 64;

struct ShTape { int* hdr; ShActs a; float *tr, *div; };
static size_t carve_sh_tape(int Q, int N, char* base, ShTape& t) {
    const size_t R = (size_t)Q * N;
    Bump b{base};
    t.hdr = b.take<int>(SH_TAPE_HDR_INTS);
    carve_sh_acts(b, R, N, t.a);
    t.tr = b.take<float>(R * N);
    t.div = b.take<float>((size_t)Q * 2 * SH_TRAIN_MAX_ITERS * N);
    return (b.off + 255) & ~size_t(255);
}
struct ShTrainWs {
    float *dpre, *df1, *dcat, *dv1;                              // gradients of the pre-activations (ReLU / tanh already applied)
    float *wfcT, *wposT, *w2T;                                   // W^T of the three layers that pass a gradient down
    float *dpreT, *f1T, *df1T, *catT, *dt1T, *txtT, *dv2T, *v1T, *dv1T, *visT;      // (columns, Rp) operands of the dW products
    float* scratch;
    size_t scratch_floats;
};
static size_t carve_sh_train(int Q, int N, char* base, ShTrainWs& w) {
    const size_t R = (size_t)Q * N, Rp = (R + 3) & ~size_t(3), Np = ((size_t)N + 3) & ~size_t(3);
    Bump b{base};
    w.dpre = b.take<float>(R * Np); w.df1 = b.take<float>(R * 256); w.dcat = b.take<float>(R * 256); w.dv1 = b.take<float>(R * 512);
    w.wfcT = b.take<float>(256 * Np); w.wposT = b.take<float>(260 * 256); w.w2T = b.take<float>(512 * 128);
    w.dpreT = b.take<float>(N * Rp); w.f1T = b.take<float>(256 * Rp); w.df1T = b.take<float>(256 * Rp); w.catT = b.take<float>(260 * Rp);
    w.dt1T = b.take<float>(128 * Rp); w.txtT = b.take<float>(300 * Rp); w.dv2T = b.take<float>(128 * Rp); w.v1T = b.take<float>(512 * Rp);
    w.dv1T = b.take<float>(512 * Rp); w.visT = b.take<float>(2048 * Rp);
    w.scratch_floats = std::max<size_t>((size_t)512 * 2048, R * 512) * GEMM_MAX_SLABS;       // the forward's need (R x 512, every slab) and W1_vis's gradient in as many
    w.scratch = b.take<float>(w.scratch_floats);
    return (b.off + 255) & ~size_t(255);
}
extern "C" size_t vsr_sinkhorn_tape_bytes(int32_t Q, int32_t N) {
    if (Q <= 0 || N < 2 || N > 16) return 0;
    ShTape t;
    return carve_sh_tape(Q, N, nullptr, t);
}
extern "C" size_t vsr_sinkhorn_train_workspace_bytes(int32_t Q, int32_t N) {
    if (Q <= 0 || N < 2 || N > 16) return 0;
    ShTrainWs w;
    return carve_sh_train(Q, N, nullptr, w);
}

extern "C" int vsr_sinkhorn_train_forward(vsr_ssp* e, const float* seq, int32_t Q, float* tr, void* tape, size_t tape_bytes, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    if (!e || !e->has_sh) return fail("vsr_sinkhorn_train_forward: Sinkhorn weights not bound");
    if (!seq || !tr || !tape || !workspace || Q <= 0) return fail("vsr_sinkhorn_train_forward: bad arguments");
    const vsr_sinkhorn_weights& w = e->sw;
    if (w.n_iters > SH_TRAIN_MAX_ITERS) return fail("vsr_sinkhorn_train_forward: n_iters %d exceeds the training cap of %d (the tape's divisor rows)", w.n_iters, SH_TRAIN_MAX_ITERS);
    const int N = w.N;
    if ((long long)Q * N * 2352 > INT_MAX) return fail("vsr_sinkhorn_train_forward: Q %d too large", Q);
    ShTape t;
    ShTrainWs tw;
    if (carve_sh_tape(Q, N, reinterpret_cast<char*>(tape), t) > tape_bytes) return fail("vsr_sinkhorn_train_forward: tape too small");
    if (carve_sh_train(Q, N, reinterpret_cast<char*>(workspace), tw) > workspace_bytes) return fail("vsr_sinkhorn_train_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (sinkhorn_layers(ssp_run(e, s, tw.scratch, tw.scratch_floats, nullptr, 1.f, "sinkhorn forward"), e->sw, seq, Q, t.a)) return 1;
    hipLaunchKernelGGL(k_sinkhorn_train_fwd, dim3(Q), dim3(64), 0, s, t.a.th, N, w.n_iters, w.tau, tr, t.tr, t.div, t.hdr);
    LAUNCHCHK();
    return 0;
}

extern "C" int vsr_sinkhorn_loc_loss(const float* tr, const float* tr_locs, const float* gt_locs, int32_t Q, int32_t N, float scale, float* loss_items,
                                     float* d_tr, void* stream) {
    if (!tr || !tr_locs || !gt_locs || !loss_items || Q <= 0 || N < 2 || N > 16) return fail("vsr_sinkhorn_loc_loss: bad arguments (2 <= N <= 16)");
    hipLaunchKernelGGL(k_sinkhorn_loc_loss, dim3(Q), dim3(64), 0, (hipStream_t)stream, tr, tr_locs, gt_locs, N, scale, loss_items, d_tr);
    LAUNCHCHK();
    return 0;
}

extern "C" int vsr_sinkhorn_train_backward(vsr_ssp* e, const float* seq, int32_t Q, const void* tape, size_t tape_bytes, const float* d_tr,
                                           const vsr_sinkhorn_grads* g, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !e->has_sh) return fail("vsr_sinkhorn_train_backward: Sinkhorn weights not bound");
    if (!seq || !tape || !d_tr || !g || !workspace || Q <= 0) return fail("vsr_sinkhorn_train_backward: bad arguments");
    if (!g->W1_txt_w || !g->W1_txt_b || !g->W1_vis_w || !g->W1_vis_b || !g->W2_vis_w || !g->W2_vis_b || !g->W_fc_pos_w || !g->W_fc_pos_b || !g->W_fc_w || !g->W_fc_b)
        return fail("vsr_sinkhorn_train_backward: all ten gradient pointers are required");
    const vsr_sinkhorn_weights& w = e->sw;
    const int N = w.N, R = Q * N, Rp = (R + 3) & ~3, Np = (N + 3) & ~3;
    if ((long long)Q * N * 2352 > INT_MAX) return fail("vsr_sinkhorn_train_backward: Q %d too large", Q);
    ShTape t;
    ShTrainWs ws;
    if (carve_sh_tape(Q, N, reinterpret_cast<char*>(const_cast<void*>(tape)), t) > tape_bytes) return fail("vsr_sinkhorn_train_backward: tape too small");
    if (carve_sh_train(Q, N, reinterpret_cast<char*>(workspace), ws) > workspace_bytes) return fail("vsr_sinkhorn_train_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const ProdRun run = ssp_run(e, s, ws.scratch, ws.scratch_floats, nullptr, 1.f, "sinkhorn backward");
    // dst (m, n; leading dimension ldd) = A (m, k) . W (n, k)^T; relu_y: masked by the ReLU whose output it is.  The unmasked ones have
    // no epilogue and are written in place where no tile is split.
    auto product = [&](int m, int n, int k, const float* A, int lda, const float* W, int ldw, float* dst, int ldd, const float* relu_y = nullptr, int ldy = 0) {
        Prod p = prod1(m, n, k, A, lda, W, ldw, dst, ldd);
        p.relu_y = relu_y; p.ldy = ldy; p.in_place = !relu_y;
        return run_product(run, p);
    };
    hipLaunchKernelGGL(k_sinkhorn_bwd, dim3(Q), dim3(64), 0, s, t.hdr, SH_TRAIN_MAX_ITERS, t.tr, t.div, t.a.th, d_tr, N, ws.dpre, Np);
    // everything that can be transposed before the first product: the three weights, the taped activations, the input's two column blocks
    TransBatch tb;
    auto tr_add = [&](const float* in, long long ld_in, int rows, int cols, float* out, long long ld_out) { tb.add(s, 0, nullptr, in, ld_in, rows, cols, out, ld_out, nullptr, 0); };
    tr_add(w.W_fc_w, 256, N, 256, ws.wfcT, Np);
    tr_add(w.W_fc_pos_w, 260, 256, 260, ws.wposT, 256);
    tr_add(w.W2_vis_w, 512, 128, 512, ws.w2T, 128);
    tr_add(ws.dpre, Np, R, N, ws.dpreT, Rp);
    tr_add(t.a.f1, 256, R, 256, ws.f1T, Rp);
    tr_add(t.a.cat, 260, R, 260, ws.catT, Rp);
    tr_add(seq, 2352, R, 300, ws.txtT, Rp);
    tr_add(t.a.v1, 512, R, 512, ws.v1T, Rp);
    tr_add(seq + 300, 2352, R, 2048, ws.visT, Rp);
    tb.flush(s);
    // W_fc
    colsum(s, ws.scratch, ws.dpre, Np, R, N, g->W_fc_b);
    if (product(N, 256, Rp, ws.dpreT, Rp, ws.f1T, Rp, g->W_fc_w, 256)) return 1;
    if (product(R, 256, Np, ws.dpre, Np, ws.wfcT, Np, ws.df1, 256, t.a.f1, 256)) return 1;
    // W_fc_pos: its input is [t1 | v2 | pos]; the first 256 columns carry a gradient further down, both behind a ReLU
    tr_add(ws.df1, 256, R, 256, ws.df1T, Rp);
    tb.flush(s);
    colsum(s, ws.scratch, ws.df1, 256, R, 256, g->W_fc_pos_b);
    if (product(256, 260, Rp, ws.df1T, Rp, ws.catT, Rp, g->W_fc_pos_w, 260)) return 1;
    if (product(R, 256, 256, ws.df1, 256, ws.wposT, 256, ws.dcat, 256, t.a.cat, 260)) return 1;
    // W1_txt and W2_vis
    tr_add(ws.dcat, 256, R, 128, ws.dt1T, Rp);
    tr_add(ws.dcat + 128, 256, R, 128, ws.dv2T, Rp);
    tb.flush(s);
    colsum(s, ws.scratch, ws.dcat, 256, R, 128, g->W1_txt_b);
    colsum(s, ws.scratch, ws.dcat + 128, 256, R, 128, g->W2_vis_b);
    if (product(128, 300, Rp, ws.dt1T, Rp, ws.txtT, Rp, g->W1_txt_w, 300)) return 1;
    if (product(128, 512, Rp, ws.dv2T, Rp, ws.v1T, Rp, g->W2_vis_w, 512)) return 1;
    if (product(R, 512, 128, ws.dcat + 128, 256, ws.w2T, 128, ws.dv1, 512, t.a.v1, 512)) return 1;
    // W1_vis
    tr_add(ws.dv1, 512, R, 512, ws.dv1T, Rp);
    tb.flush(s);
    colsum(s, ws.scratch, ws.dv1, 512, R, 512, g->W1_vis_b);
    if (product(512, 2048, Rp, ws.dv1T, Rp, ws.visT, Rp, g->W1_vis_w, 2048)) return 1;
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- S-SSP training
// S_SSP.forward (sort_model.py:80-103) for S sequences: ONE forward that ends in the loss (a device float) and ONE hand-written backward.
//   forward   k_ssp_train_prep, the embeddings, the encoder, the decoder teacher-forced in one pass over [bos, gt_0 .. gt_9] (Rd = 11 S
//             rows), expander_nn, k_ssp_kl_loss / k_ssp_loss_finish.  The products are inference's (run_products) with the dropout bytes
//             as one more epilogue term.
//   tape      per LayerNorm its output, the normalised rows and 1 / std; per attention q, k, v, the softmax WEIGHTS before dropout (taped,
//             not recomputed: at most 8 x 11 x 11 floats per sequence and layer) and the context; the feed-forward hidden AFTER ReLU and
//             dropout (its sign pattern is both masks); the encoder's summed embeddings; logp.  `prior` is the encoder LayerNorm's output.
//   backward  k_ssp_kl_bwd, then the layers in reverse.  Per linear layer: the bias gradient by the ordered column sums (k_colsum), dW = dY^T X
//             and dX = dY W as NT products on transposed copies (TransBatch), k dimension padded to Rp = rows rounded up to 4 with zeroed
//             padding columns.  What the reference adds up by re-using a module is ONE product with several k segments: the decoder's
//             attention.linear_{Q,K,V,O} serve the self AND the cross attention (d W_q = dq^T y1 + dq2^T y2, ...), the three projections of
//             one input give d y1 = dq W_q + dk W_k + dv W_v, and the three decoder layers accumulate into d prior.
//             cross_attention.* is never used and has no gradient.  Every sum has a fixed order: two runs give the same bits.
// The backward trusts the tape's header, not its caller, for p and for whether masks were applied; a header that does not carry the call's
// S and mask mode turns every gradient into NaN (k_ssp_kl_bwd).
constexpr int SSP_TRAIN_MAX_S = 32768;            // Rd x 2048 elements and every row index stay far inside int

static void ssp_sites(int S, SspSites& st) {
    const long long Te = SSP_LEN, Td = SSP_TD, H = SSP_H, F = SSP_FF, NH = SSP_HEADS, s = S;
    long long n[SSP_SITES];
    int i = 0;
    n[i++] = s * H; n[i++] = s * Te * H;
    for (int l = 0; l < 3; ++l) { n[i++] = s * NH * Te * Te; n[i++] = s * Te * H; n[i++] = s * Te * F; n[i++] = s * Te * H; }
    n[i++] = s * Td * H;
    for (int l = 0; l < 3; ++l) { n[i++] = s * NH * Td * Td; n[i++] = s * Td * H; n[i++] = s * NH * Td * Te; n[i++] = s * Td * H; n[i++] = s * Td * F; n[i++] = s * Td * H; }
    long long off = 0;
    for (i = 0; i < SSP_SITES; ++i) { st.off[i] = off; st.n[i] = n[i]; off += (n[i] + 15) & ~15LL; }
    st.off[SSP_SITES] = off;
}
extern "C" size_t vsr_ssp_mask_bytes(int32_t S) {
    if (S <= 0 || S > SSP_TRAIN_MAX_S) return 0;
    SspSites st;
    ssp_sites(S, st);
    return (size_t)st.off[SSP_SITES];
}
extern "C" size_t vsr_ssp_mask_offset(int32_t S, int32_t site) {
    if (S <= 0 || S > SSP_TRAIN_MAX_S || site < 0 || site >= SSP_SITES) return 0;
    SspSites st;
    ssp_sites(S, st);
    return (size_t)st.off[site];
}
extern "C" int vsr_ssp_dropout_masks(uint64_t seed, float p, int32_t S, uint8_t* masks, void* stream) {
    if (!masks || S <= 0 || S > SSP_TRAIN_MAX_S || !(p >= 0.f && p < 1.f)) return fail("vsr_ssp_dropout_masks: bad arguments (1 <= S <= %d, 0 <= p < 1)", SSP_TRAIN_MAX_S);
    if (!aligned16(masks)) return fail("vsr_ssp_dropout_masks: the mask buffer must start on a 16-byte boundary");      // (the kernel stores whole words)
    SspSites st;
    ssp_sites(S, st);
    hipLaunchKernelGGL(k_ssp_dropout_masks, dim3(cdiv(st.off[SSP_SITES] / 4, 256)), dim3(256), 0, (hipStream_t)stream, st, seed, p, masks);
    LAUNCHCHK();
    return 0;
}

struct SspTape { int* hdr; float* emb; SspLayerTape enc[3], dec[3]; SspLnTape encln, decln; float* logp; };
static size_t carve_ssp_tape(int S, char* base, SspTape& t) {
    const size_t Re = (size_t)S * SSP_LEN, Rd = (size_t)S * SSP_TD, H = SSP_H;
    Bump b{base};
    auto ln = [&](SspLnTape& l, size_t R) { l.y = b.take<float>(R * H); l.xhat = b.take<float>(R * H); l.rstd = b.take<float>(R); };
    t.hdr = b.take<int>(SSP_TAPE_HDR_INTS);
    t.emb = b.take<float>(Re * H);
    for (int l = 0; l < 3; ++l) {
        SspLayerTape& e = t.enc[l];
        memset(&e, 0, sizeof(e));
        ln(e.lnA, Re); ln(e.lnF, Re);
        e.q = b.take<float>(Re * H); e.k = b.take<float>(Re * H); e.v = b.take<float>(Re * H);
        e.P1 = b.take<float>((size_t)S * SSP_HEADS * SSP_LEN * SSP_LEN); e.ctx1 = b.take<float>(Re * H); e.ff = b.take<float>(Re * SSP_FF);
    }
    ln(t.encln, Re);
    for (int l = 0; l < 3; ++l) {
        SspLayerTape& d = t.dec[l];
        ln(d.lnA, Rd); ln(d.lnC, Rd); ln(d.lnF, Rd);
        d.q = b.take<float>(Rd * H); d.k = b.take<float>(Rd * H); d.v = b.take<float>(Rd * H);
        d.P1 = b.take<float>((size_t)S * SSP_HEADS * SSP_TD * SSP_TD); d.ctx1 = b.take<float>(Rd * H);
        d.q2 = b.take<float>(Rd * H); d.pk = b.take<float>(Re * H); d.pv = b.take<float>(Re * H);
        d.P2 = b.take<float>((size_t)S * SSP_HEADS * SSP_TD * SSP_LEN); d.ctx2 = b.take<float>(Rd * H); d.ff = b.take<float>(Rd * SSP_FF);
    }
    ln(t.decln, Rd);
    t.logp = b.take<float>(Rd * SSP_ROLES);
    return (b.off + 255) & ~size_t(255);
}

constexpr int SSP_LOGIT_LD = (SSP_ROLES + 3) & ~3;        // d logits and expander_nn^T: the 26 classes as a k dimension, padded to 28
struct SspTrainWs {
    int *verbs32, *roles, *gt, *tok;
    float *r[10], *ddec;             // (Rd, 512) rows: the residual stream of the forward, the gradients of the backward
    float *dff;                      // (Rd, 2048)
    float *logits, *row_loss, *dlog; // (Rd, 26), (Rd), (Rd, 28)
    float *dprior, *dpk, *dpv;       // (Re, 512)
    float *dbk1, *dbk2;              // (S, 512): k_ssp_mha_bwd's per-sequence sums of dk (self, cross) for linear_K's bias
    float *t512[10], *t2048[2];      // transposed activations / gradients (columns, Rp)
    float *tE[3];                    // (512, Rep): d pk^T, d pv^T, prior^T
    float *wT[4];                    // transposed weights of the block at hand, up to 2048 x 512 each
    float *part;                     // two k_colsum tables
    float *scratch;
    size_t scratch_floats;
};
static size_t carve_ssp_train(int S, char* base, SspTrainWs& w) {
    const size_t Re = (size_t)S * SSP_LEN, Rd = (size_t)S * SSP_TD, H = SSP_H, Rp = (Rd + 3) & ~size_t(3), Rep = (Re + 3) & ~size_t(3);
    Bump b{base};
    w.verbs32 = b.take<int>(S); w.roles = b.take<int>(Re); w.gt = b.take<int>(Re); w.tok = b.take<int>(Rd);
    for (auto& p : w.r) p = b.take<float>(Rd * H);
    w.ddec = b.take<float>(Rd * H);
    w.dff = b.take<float>(Rd * SSP_FF);
    w.logits = b.take<float>(Rd * SSP_ROLES); w.row_loss = b.take<float>(Rd); w.dlog = b.take<float>(Rd * SSP_LOGIT_LD);
    w.dprior = b.take<float>(Re * H); w.dpk = b.take<float>(Re * H); w.dpv = b.take<float>(Re * H);
    w.dbk1 = b.take<float>((size_t)S * H); w.dbk2 = b.take<float>((size_t)S * H);
    for (auto& p : w.t512) p = b.take<float>(H * Rp);
    for (auto& p : w.t2048) p = b.take<float>((size_t)SSP_FF * Rp);
    for (auto& p : w.tE) p = b.take<float>(H * Rep);
    for (auto& p : w.wT) p = b.take<float>((size_t)SSP_FF * H);
    w.part = b.take<float>((size_t)2 * COLSUM_CHUNKS * SSP_FF);
    w.scratch_floats = std::max<size_t>(Rd * SSP_FF, (size_t)SSP_FF * H) * GEMM_MAX_SLABS;      // every slab of the widest activation / of W1's gradient
    w.scratch = b.take<float>(w.scratch_floats);
    return (b.off + 255) & ~size_t(255);
}
extern "C" size_t vsr_ssp_tape_bytes(int32_t S) {
    if (S <= 0 || S > SSP_TRAIN_MAX_S) return 0;
    SspTape t;
    return carve_ssp_tape(S, nullptr, t);
}
// TEST ONLY: byte offset, in the tape, of a layer's feed-forward hidden (rows x 2048 fp32, after ReLU and dropout): > 0 there is the
// gate the forward applied, which a test needs to put its reference on the same side of a ReLU kink.  The tape's layout is otherwise private.
extern "C" size_t vsr_ssp_tape_ff_offset(int32_t S, int32_t decoder, int32_t layer) {
    if (S <= 0 || S > SSP_TRAIN_MAX_S || layer < 0 || layer > 2) return 0;
    SspTape t;
    char* base = reinterpret_cast<char*>(uintptr_t(4096));
    carve_ssp_tape(S, base, t);
    return (size_t)(reinterpret_cast<char*>(decoder ? t.dec[layer].ff : t.enc[layer].ff) - base);
}
extern "C" size_t vsr_ssp_train_workspace_bytes(int32_t S) {
    if (S <= 0 || S > SSP_TRAIN_MAX_S) return 0;
    SspTrainWs w;
    return carve_ssp_train(S, nullptr, w);
}

static int ssp_train_args(const char* who, vsr_ssp* e, const void* verbs, const void* roles, const void* gt, int32_t S, const void* tape, const void* ws) {
    if (!e || !e->has_ssp) return fail("%s: S-SSP weights not bound", who);
    if (!verbs || !roles || !gt || !tape || !ws || S <= 0 || S > SSP_TRAIN_MAX_S) return fail("%s: bad arguments (1 <= S <= %d)", who, SSP_TRAIN_MAX_S);
    if (e->w.n_verbs > INT_MAX / SSP_H) return fail("%s: verb table too large", who);
    return 0;
}

extern "C" int vsr_ssp_train_forward(vsr_ssp* e, const int64_t* verbs, const int32_t* roles, const int32_t* gt, int32_t S, const uint8_t* masks, float p,
                                     const float* one_hot, float* loss, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (ssp_train_args("vsr_ssp_train_forward", e, verbs, roles, gt, S, tape, workspace)) return 1;
    if (!one_hot || !loss) return fail("vsr_ssp_train_forward: bad arguments");
    if (masks && !(p >= 0.f && p < 1.f)) return fail("vsr_ssp_train_forward: dropout p %g outside [0, 1)", (double)p);
    if (masks && !aligned16(masks)) return fail("vsr_ssp_train_forward: the mask buffer must start on a 16-byte boundary");
    SspTape t;
    SspTrainWs ws;
    if (carve_ssp_tape(S, reinterpret_cast<char*>(tape), t) > tape_bytes) return fail("vsr_ssp_train_forward: tape too small");
    if (carve_ssp_train(S, reinterpret_cast<char*>(workspace), ws) > workspace_bytes) return fail("vsr_ssp_train_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const vsr_ssp_weights& w = e->w;
    const int H = SSP_H, Re = S * SSP_LEN, Rd = S * SSP_TD;
    const float p_applied = masks ? p : 0.f, scale = 1.0f / (1.0f - p_applied);
    SspSites st;
    ssp_sites(S, st);
    auto keep = [&](int site) -> const uint8_t* { return masks ? masks + st.off[site] : nullptr; };
    const ProdRun run = ssp_run(e, s, ws.scratch, ws.scratch_floats, nullptr, scale, "ssp training");
    hipLaunchKernelGGL(k_ssp_train_prep, dim3(cdiv(Rd, 256)), dim3(256), 0, s, verbs, roles, gt, S, (int)w.n_verbs, ws.verbs32, ws.roles, ws.gt, ws.tok);
    // a layer's dropout sites are consecutive from site0, in the order ssp_layer takes them
    auto layer = [&](const vsr_ssp_layer& ly, const SspLayerTape& lt, int T, const int* mask_tok, int site0, const float* prior) {
        const uint8_t* k[6] = {};
        for (int i = 0; i < (lt.pk ? 6 : 4); ++i) k[i] = keep(site0 + i);
        return ssp_layer(run, ly, lt, S, T, mask_tok, SSP_TD, prior, k, ws.r[0], ws.r[1]);
    };
    // ---- encoder
    hipLaunchKernelGGL(k_ssp_embed_train, dim3(Re), dim3(128), 0, s, ws.roles, SSP_LEN, w.sr_embed, ws.verbs32, w.v_embed, keep(1), keep(0), scale, t.emb);
    Prod fc = lin(Re, H, H, t.emb, H, w.fc_w, w.fc_b, ws.r[0]);
    if (run_product(run, fc)) return 1;
    for (int l = 0; l < 3; ++l)
        if (layer(w.enc[l], t.enc[l], SSP_LEN, nullptr, 2 + 4 * l, nullptr)) return 1;
    layernorm(s, ws.r[0], w.enc_ln_w, w.enc_ln_b, Re, t.encln);
    LAUNCHCHK();
    // ---- decoder
    hipLaunchKernelGGL(k_ssp_embed_train, dim3(Rd), dim3(128), 0, s, ws.tok, SSP_TD, w.sr_embed, (const int*)nullptr, (const float*)nullptr, keep(14),
                       (const uint8_t*)nullptr, scale, ws.r[0]);
    for (int l = 0; l < 3; ++l)
        if (layer(w.dec[l], t.dec[l], SSP_TD, ws.tok, 15 + 6 * l, t.encln.y)) return 1;
    layernorm(s, ws.r[0], w.dec_ln_w, w.dec_ln_b, Rd, t.decln);
    // ---- loss
    Prod ex = lin(Rd, SSP_ROLES, H, t.decln.y, H, w.exp_w, w.exp_b, ws.logits);
    if (run_product(run, ex)) return 1;
    hipLaunchKernelGGL(k_ssp_kl_loss, dim3(cdiv(Rd, 4)), dim3(256), 0, s, ws.logits, ws.gt, one_hot, Rd, t.logp, ws.row_loss);
    hipLaunchKernelGGL(k_ssp_loss_finish, dim3(1), dim3(256), 0, s, ws.row_loss, ws.gt, one_hot, S, p_applied, masks ? 1 : 0, loss, t.hdr);
    LAUNCHCHK();
    return 0;
}

extern "C" int vsr_ssp_train_backward(vsr_ssp* e, const int64_t* verbs, const int32_t* roles, const int32_t* gt, int32_t S, const uint8_t* masks, const void* tape,
                                      size_t tape_bytes, const float* d_loss, const vsr_ssp_grads* g, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    if (ssp_train_args("vsr_ssp_train_backward", e, verbs, roles, gt, S, tape, workspace)) return 1;
    if (!d_loss || !g) return fail("vsr_ssp_train_backward: bad arguments");
    if (masks && !aligned16(masks)) return fail("vsr_ssp_train_backward: the mask buffer must start on a 16-byte boundary");
    if (g->n_verbs != e->w.n_verbs) return fail("vsr_ssp_train_backward: the v_embed gradient has %lld rows, the bound table %lld", (long long)g->n_verbs, (long long)e->w.n_verbs);
    {
        bool all = g->sr_embed && g->v_embed && g->fc_w && g->fc_b && g->enc_ln_w && g->enc_ln_b && g->dec_ln_w && g->dec_ln_b && g->exp_w && g->exp_b;
        for (int l = 0; l < 3; ++l)
            for (int d = 0; d < 2; ++d) {
                const vsr_ssp_layer_grads& ly = d ? g->dec[l] : g->enc[l];
                all = all && ly.ln1_w && ly.ln1_b && ly.ln2_w && ly.ln2_b && (!d || (ly.ln3_w && ly.ln3_b)) && ly.Wq && ly.bq && ly.Wk && ly.bk && ly.Wv && ly.bv &&
                      ly.Wo && ly.bo && ly.W1 && ly.b1 && ly.W2 && ly.b2;
            }
        if (!all) return fail("vsr_ssp_train_backward: every gradient pointer that has a weight is required");
    }
    SspTape t;
    SspTrainWs ws;
    if (carve_ssp_tape(S, reinterpret_cast<char*>(const_cast<void*>(tape)), t) > tape_bytes) return fail("vsr_ssp_train_backward: tape too small");
    if (carve_ssp_train(S, reinterpret_cast<char*>(workspace), ws) > workspace_bytes) return fail("vsr_ssp_train_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const vsr_ssp_weights& w = e->w;
    const int H = SSP_H, F = SSP_FF, Re = S * SSP_LEN, Rd = S * SSP_TD, Rdp = (Rd + 3) & ~3, Rep = (Re + 3) & ~3, LD = SSP_LOGIT_LD;
    SspSites st;
    ssp_sites(S, st);
    auto keep = [&](int site) -> const uint8_t* { return masks ? masks + st.off[site] : nullptr; };
    const ProdRun run = ssp_run(e, s, ws.scratch, ws.scratch_floats, t.hdr, 1.f, "ssp training");
    TransBatch tb;
    auto tr_add = [&](const float* in, int ld_in, int rows, int cols, float* out, int ld_out) { tb.add(s, 0, nullptr, in, ld_in, rows, cols, out, ld_out, nullptr, 0); };
    // the gradient of x where y = drop(x) (site) and dy is given: dy itself without masks, else a masked copy in `buf`
    auto undrop = [&](const float* dy, int site, long long n, float* buf) -> const float* {
        if (!masks) return dy;
        hipLaunchKernelGGL(k_ssp_drop_bwd, dim3(cdiv(n / 4, 256)), dim3(256), 0, s, dy, keep(site), t.hdr, n, buf);
        return buf;
    };
    // out = the column sums of X (R, C) (+ those of X2 (R2, C)): the second use of a shared bias
    auto bias_sum = [&](const float* X, int R, int C, float* out, const float* X2 = nullptr, int R2 = 0) { colsum(s, ws.part, X, C, R, C, out, nullptr, X2, R2); };
    auto ln_bwd = [&](const float* dy, const float* gamma, const SspLnTape& lt, const float* add, int R, float* dx, float* dgamma, float* dbeta) {
        hipLaunchKernelGGL(k_layernorm512_bwd, dim3(cdiv(R, 4)), dim3(256), 0, s, dy, gamma, lt.xhat, lt.rstd, add, R, dx, ws.r[9]);
        bias_sum(ws.r[9], R, H, dgamma);
        bias_sum(dy, R, H, dbeta);
    };
    hipLaunchKernelGGL(k_ssp_train_prep, dim3(cdiv(Rd, 256)), dim3(256), 0, s, verbs, roles, gt, S, (int)w.n_verbs, ws.verbs32, ws.roles, ws.gt, ws.tok);

    // ---- loss and expander_nn: d logits -> ws.r[2] = d (decoder LayerNorm output) -> ws.r[0] = d (last decoder layer's output)
    hipLaunchKernelGGL(k_ssp_kl_bwd, dim3(cdiv((long long)Rd * LD, 256)), dim3(256), 0, s, t.logp, ws.gt, t.hdr, S, masks ? 1 : 0, d_loss, Rd, LD, ws.dlog);
    tr_add(ws.dlog, LD, Rd, SSP_ROLES, ws.t512[0], Rdp);
    tr_add(t.decln.y, H, Rd, H, ws.t512[1], Rdp);
    tr_add(w.exp_w, H, SSP_ROLES, H, ws.wT[0], LD);
    tr_add(t.encln.y, H, Re, H, ws.tE[2], Rep);                      // prior^T: the k operand of the three layers' cross-attention d W_k, d W_v
    tb.flush(s);
    bias_sum(ws.dlog, Rd, LD, ws.r[9]);                     // (28 columns; the first 26 are the bias gradient)
    HIPCHK(hipMemcpyAsync(g->exp_b, ws.r[9], SSP_ROLES * sizeof(float), hipMemcpyDeviceToDevice, s));
    {
        Prod pw = prod1(SSP_ROLES, H, Rdp, ws.t512[0], Rdp, ws.t512[1], Rdp, g->exp_w);
        Prod px = prod1(Rd, H, LD, ws.dlog, LD, ws.wT[0], LD, ws.r[2]);
        if (run_product(run, pw) || run_product(run, px)) return 1;
    }
    ln_bwd(ws.r[2], w.dec_ln_w, t.decln, nullptr, Rd, ws.r[0], g->dec_ln_w, g->dec_ln_b);

    // one layer of either stack, backwards: d (layer output) in ws.r[0] -> d (layer input) in ws.r[0]
    //   r[0] A: the running gradient   r[1] B   r[2] Y, r[5] C, r[6] D, r[7] E: products   r[3] Z, r[4] Z2: masked copies   r[8] Q2   r[9]: dy x^
    auto layer_bwd = [&](const vsr_ssp_layer& ly, const vsr_ssp_layer_grads& gl, const SspLayerTape& lt, int R, int Rp, int T, bool dec, int site0, bool first_dec) -> int {
        float *A = ws.r[0], *B = ws.r[1], *Y = ws.r[2], *Z = ws.r[3], *Z2 = ws.r[4], *C = ws.r[5], *D = ws.r[6], *E = ws.r[7], *Q2 = ws.r[8];
        const int site_ff = site0 + (dec ? 4 : 2);
        const long long n = (long long)R * H;
        // ---- feed-forward: out = drop(W2 ff + b2) + h, ff = drop(relu(W1 yF + b1)), yF = LN(h)
        const float* dz2 = undrop(A, site_ff + 1, n, Z);
        tr_add(dz2, H, R, H, ws.t512[0], Rp);
        tr_add(lt.ff, F, R, F, ws.t2048[0], Rp);
        tr_add(lt.lnF.y, H, R, H, ws.t512[1], Rp);
        tr_add(ly.W2, F, H, F, ws.wT[0], H);
        tr_add(ly.W1, H, F, H, ws.wT[1], F);
        tb.flush(s);
        bias_sum(dz2, R, H, gl.b2);
        Prod pw2 = prod1(H, F, Rp, ws.t512[0], Rp, ws.t2048[0], Rp, gl.W2);
        Prod pff = prod1(R, F, H, dz2, H, ws.wT[0], H, ws.dff);
        pff.relu_y = lt.ff;                                                                           // d (W1 yF + b1): relu and the site's dropout in one
        if (run_product(run, pw2) || run_product(run, pff)) return 1;
        tr_add(ws.dff, F, R, F, ws.t2048[1], Rp);
        tb.flush(s);
        bias_sum(ws.dff, R, F, gl.b1);
        Prod pw1 = prod1(F, H, Rp, ws.t2048[1], Rp, ws.t512[1], Rp, gl.W1);
        Prod pyf = prod1(R, H, F, ws.dff, F, ws.wT[1], F, Y);
        if (run_product(run, pw1) || run_product(run, pyf)) return 1;
        ln_bwd(Y, dec ? ly.ln3_w : ly.ln2_w, lt.lnF, A, R, B, dec ? gl.ln3_w : gl.ln2_w, dec ? gl.ln3_b : gl.ln2_b);       // B = d h
        // the four attention weights, transposed once for both uses
        tr_add(ly.Wo, H, H, H, ws.wT[0], H);
        tr_add(ly.Wq, H, H, H, ws.wT[1], H);
        tr_add(ly.Wk, H, H, H, ws.wT[2], H);
        tr_add(ly.Wv, H, H, H, ws.wT[3], H);
        const float* dzo2 = nullptr;
        if (dec) {
            // ---- cross attention: h = drop(Wo ctx2 + bo) + h1, ctx2 = mha(q2 = Wq yC + bq, pk = Wk prior + bk, pv = Wv prior + bv), yC = LN(h1)
            dzo2 = undrop(B, site0 + 3, n, Z2);
            tr_add(dzo2, H, R, H, ws.t512[0], Rp);
            tr_add(lt.ctx2, H, R, H, ws.t512[1], Rp);
            tb.flush(s);
            Prod pc = prod1(R, H, H, dzo2, H, ws.wT[0], H, Y);
            if (run_product(run, pc)) return 1;
            hipLaunchKernelGGL(k_ssp_mha_bwd, dim3(S, SSP_HEADS), dim3(64), 0, s, lt.q2, lt.pk, lt.pv, lt.P2, keep(site0 + 2), t.hdr, Y, T, SSP_LEN, (const int*)nullptr, 0,
                               Q2, ws.dpk, ws.dpv, ws.dbk2);
            tr_add(Q2, H, R, H, ws.t512[2], Rp);
            tr_add(lt.lnC.y, H, R, H, ws.t512[3], Rp);
            tr_add(ws.dpk, H, Re, H, ws.tE[0], Rep);
            tr_add(ws.dpv, H, Re, H, ws.tE[1], Rep);
            tb.flush(s);
            Prod pyc = prod1(R, H, H, Q2, H, ws.wT[1], H, C);
            Prod pp = prod1(Re, H, H, ws.dpk, H, ws.wT[2], H, ws.dprior);
            pp.seg[1] = ProdSeg{ws.dpv, H, ws.wT[3], H, H}; pp.nseg = 2;
            pp.residual = first_dec ? nullptr : ws.dprior;                                            // the three layers accumulate into d prior
            if (run_product(run, pyc) || run_product(run, pp)) return 1;
            ln_bwd(C, ly.ln2_w, lt.lnC, B, R, A, gl.ln2_w, gl.ln2_b);                                   // A = d h1
        } else {
            tb.flush(s);
            std::swap(A, B);                                                                          // A = d h1 here too
        }
        // ---- self attention: h1 = drop(Wo ctx1 + bo) + x, ctx1 = mha(q, k, v = W yA + b), yA = LN(x)
        const float* dzo1 = undrop(A, site0 + 1, n, Z);
        tr_add(dzo1, H, R, H, ws.t512[4], Rp);
        tr_add(lt.ctx1, H, R, H, ws.t512[5], Rp);
        tb.flush(s);
        bias_sum(dzo1, R, H, gl.bo, dzo2, R);
        Prod pc1 = prod1(R, H, H, dzo1, H, ws.wT[0], H, Y);
        Prod pwo = prod1(H, H, Rp, ws.t512[4], Rp, ws.t512[5], Rp, gl.Wo);
        if (dec) { pwo.seg[1] = ProdSeg{ws.t512[0], Rp, ws.t512[1], Rp, Rp}; pwo.nseg = 2; }
        if (run_product(run, pc1) || run_product(run, pwo)) return 1;
        hipLaunchKernelGGL(k_ssp_mha_bwd, dim3(S, SSP_HEADS), dim3(64), 0, s, lt.q, lt.k, lt.v, lt.P1, keep(site0), t.hdr, Y, T, T, dec ? ws.tok : (const int*)nullptr, SSP_TD,
                           C, D, E, ws.dbk1);
        tr_add(C, H, R, H, ws.t512[6], Rp);
        tr_add(D, H, R, H, ws.t512[7], Rp);
        tr_add(E, H, R, H, ws.t512[8], Rp);
        tr_add(lt.lnA.y, H, R, H, ws.t512[9], Rp);
        tb.flush(s);
        bias_sum(C, R, H, gl.bq, dec ? Q2 : nullptr, R);
        bias_sum(ws.dbk1, S, H, gl.bk, dec ? ws.dbk2 : nullptr, S);                           // (k_ssp_mha_bwd: summed per sequence in fp64)
        bias_sum(E, R, H, gl.bv, dec ? ws.dpv : nullptr, Re);
        Prod pw[3] = {prod1(H, H, Rp, ws.t512[6], Rp, ws.t512[9], Rp, gl.Wq), prod1(H, H, Rp, ws.t512[7], Rp, ws.t512[9], Rp, gl.Wk),
                         prod1(H, H, Rp, ws.t512[8], Rp, ws.t512[9], Rp, gl.Wv)};
        if (dec) {
            pw[0].seg[1] = ProdSeg{ws.t512[2], Rp, ws.t512[3], Rp, Rp}; pw[0].nseg = 2;
            pw[1].seg[1] = ProdSeg{ws.tE[0], Rep, ws.tE[2], Rep, Rep}; pw[1].nseg = 2;
            pw[2].seg[1] = ProdSeg{ws.tE[1], Rep, ws.tE[2], Rep, Rep}; pw[2].nseg = 2;
        }
        if (run_products(run, pw, 3)) return 1;
        Prod pya = prod1(R, H, H, C, H, ws.wT[1], H, Y);
        pya.seg[1] = ProdSeg{D, H, ws.wT[2], H, H}; pya.seg[2] = ProdSeg{E, H, ws.wT[3], H, H}; pya.nseg = 3;
        if (run_product(run, pya)) return 1;
        ln_bwd(Y, ly.ln1_w, lt.lnA, A, R, B, gl.ln1_w, gl.ln1_b);                                       // B = d x
        if (B != ws.r[0]) std::swap(ws.r[0], ws.r[1]);
        return 0;
    };
    for (int l = 2; l >= 0; --l)
        if (layer_bwd(w.dec[l], g->dec[l], t.dec[l], Rd, Rdp, SSP_TD, true, 15 + 6 * l, l == 2)) return 1;
    LAUNCHCHK();
    std::swap(ws.r[0], ws.ddec);                 // d (decoder embeddings) waits for the embedding kernel while the encoder's pass uses the row buffers
    const float* d_dec = ws.ddec;
    // ---- encoder: d prior -> its LayerNorm -> the layers -> fc_feat -> the embeddings
    ln_bwd(ws.dprior, w.enc_ln_w, t.encln, nullptr, Re, ws.r[0], g->enc_ln_w, g->enc_ln_b);
    for (int l = 2; l >= 0; --l)
        if (layer_bwd(w.enc[l], g->enc[l], t.enc[l], Re, Rep, SSP_LEN, false, 2 + 4 * l, false)) return 1;
    tr_add(ws.r[0], H, Re, H, ws.t512[0], Rep);
    tr_add(t.emb, H, Re, H, ws.t512[1], Rep);
    tr_add(w.fc_w, H, H, H, ws.wT[0], H);
    tb.flush(s);
    bias_sum(ws.r[0], Re, H, g->fc_b);
    {
        Prod pw = prod1(H, H, Rep, ws.t512[0], Rep, ws.t512[1], Rep, g->fc_w);
        Prod px = prod1(Re, H, H, ws.r[0], H, ws.wT[0], H, ws.r[2]);
        if (run_product(run, pw) || run_product(run, px)) return 1;
    }
    hipLaunchKernelGGL(k_ssp_sr_embed_bwd, dim3(SSP_ROLES, H / 64), dim3(256), 0, s, ws.roles, ws.r[2], keep(1), Re, ws.tok, d_dec, keep(14), Rd, t.hdr, g->sr_embed);
    hipLaunchKernelGGL(k_ssp_v_embed_bwd, dim3((int)w.n_verbs), dim3(128), 0, s, ws.verbs32, ws.r[2], keep(0), t.hdr, S, g->v_embed);
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- caption ranking on the device
// eval_coco.py:141-221 for the N caption rows of a loader batch as one stream of launches: integer annotations in,
// the (N, L) rank tensor of vsr_reorder_slots out, no read-back.  S-SSP runs on the PADDED job slots S = N MV (an inactive slot has
// verb 0 and no roles: k_ssp_init emits nothing for it) and SinkhornNet on Q = max_items items (an unused item is all zero rows).
// The items go through SinkhornNet's five layers (vsr_sinkhorn_assign's own: sinkhorn_layers) in chunks of RANK_SH_CHUNK (max_items rounded
// up to whole chunks): every GEMM launch then has the same shape whatever max_items is, so an item's assignment - down to how a tie
// between two identical padding rows falls, which follows the last bit of the stream-K GEMMs and with it the launch's row count - does
// not depend on the bound the caller chose.  The Sinkhorn iterations and the assignment (k_sinkhorn_assign, one wave per item, 0.37 ms
// whether it has 128 items or 2432: its time is lane 0's serial Kuhn-Munkres) run ONCE over all items.
constexpr int RANK_SH_CHUNK = 128;
static int rank_qcap(int N, int MV, int max_items) { return max_items > 0 ? max_items : N * MV * RANK_L; }
static int rank_qpad(int Qcap) { return (int)(((long long)Qcap + RANK_SH_CHUNK - 1) / RANK_SH_CHUNK * RANK_SH_CHUNK); }
static size_t carve_rank_plan(int N, int MV, char* base, RankPlan& p) {
    const size_t S = (size_t)N * MV;
    Bump b{base};
    p.hdr = b.take<int32_t>(RANK_HDR_INTS); p.item_cnt = b.take<int32_t>(S); p.item_off = b.take<int32_t>(S); p.jobs = b.take<RankJob>(S);
    return (b.off + 255) & ~size_t(255);
}
static int rank_shape(const char* who, int N, int L, int MV, int MS, int N_sink, int max_items) {
    if (N <= 0 || max_items < 0) return fail("%s: bad arguments (N %d, max_items %d)", who, N, max_items);
    if (!rank_limits_ok(L, MV, MS, N_sink))
        return fail("%s: outside the limits L == %d, 1 <= MV <= %d, MS >= MV, %d <= N_sink <= %d (got L %d, MV %d, MS %d, N_sink %d)", who, RANK_L, RANK_MAX_MV,
                    RANK_MIN_SINK, RANK_MAX_SINK, L, MV, MS, N_sink);
    if ((long long)N * MV * RANK_L > INT_MAX / 64 || max_items > INT_MAX / 64)         // job and item row indices (x 10, x N_sink) stay inside int
        return fail("%s: N %d / max_items %d too large", who, N, max_items);
    return 0;
}
extern "C" size_t vsr_rank_plan_bytes(int32_t N, int32_t MV, int32_t max_items) {
    if (N <= 0 || MV < 1 || MV > RANK_MAX_MV || max_items < 0 || max_items > INT_MAX / 64 || (long long)N * MV * RANK_L > INT_MAX / 64) return 0;
    RankPlan p;
    return carve_rank_plan(N, MV, nullptr, p);
}

// Qfill >= Qcap: rows of item_gather to fill (those beyond Qcap with -1: the tail of the last Sinkhorn chunk)
static int rank_plan_launch(const int32_t* control_verb, const int32_t* det_seqs_v, const int32_t* det_seqs_sr, int N, int L, int MV, int MS, int N_sink, int64_t n_verbs,
                            int Qcap, int Qfill, int64_t* job_verbs, int32_t* job_roles, int32_t* item_gather, const RankPlan& p, hipStream_t s) {
    const int S = N * MV;
    hipLaunchKernelGGL(k_rank_jobs, dim3(cdiv(S, 64)), dim3(64), 0, s, control_verb, det_seqs_v, det_seqs_sr, N, L, MV, MS, N_sink, Qcap, (long long)n_verbs, p,
                       job_verbs, job_roles);
    hipLaunchKernelGGL(k_rank_items, dim3(1), dim3(256), 0, s, p, S, L, MV, N_sink, Qcap, Qfill, item_gather);
    LAUNCHCHK();
    return 0;
}

extern "C" int vsr_rank_plan(const int32_t* control_verb, const int32_t* det_seqs_v, const int32_t* det_seqs_sr, int32_t N, int32_t L, int32_t MV, int32_t MS,
                             int32_t N_sink, int64_t n_verbs, int32_t max_items, int64_t* job_verbs, int32_t* job_roles, int32_t* item_gather, void* plan,
                             size_t plan_bytes, void* stream) {
    if (!control_verb || !det_seqs_v || !det_seqs_sr || !job_verbs || !job_roles || !item_gather || !plan || n_verbs <= 0) return fail("vsr_rank_plan: bad arguments");
    if (rank_shape("vsr_rank_plan", N, L, MV, MS, N_sink, max_items)) return 1;
    RankPlan p;
    if (carve_rank_plan(N, MV, reinterpret_cast<char*>(plan), p) > plan_bytes) return fail("vsr_rank_plan: plan buffer too small");
    const int Qcap = rank_qcap(N, MV, max_items);
    return rank_plan_launch(control_verb, det_seqs_v, det_seqs_sr, N, L, MV, MS, N_sink, n_verbs, Qcap, Qcap, job_verbs, job_roles, item_gather, p, (hipStream_t)stream);
}

extern "C" int vsr_rank_finish(const void* plan, size_t plan_bytes, const int32_t* pred, const int32_t* assign, int32_t N, int32_t L, int32_t MV, int32_t N_sink,
                               int32_t* rank, int32_t* status, void* stream) {
    if (!plan || !pred || !assign || !rank || !status) return fail("vsr_rank_finish: bad arguments");
    if (rank_shape("vsr_rank_finish", N, L, MV, MV, N_sink, 0)) return 1;
    RankPlan p;
    if (carve_rank_plan(N, MV, reinterpret_cast<char*>(const_cast<void*>(plan)), p) > plan_bytes) return fail("vsr_rank_finish: plan buffer too small");
    hipLaunchKernelGGL(k_rank_finish, dim3(N), dim3(64), 0, (hipStream_t)stream, p, pred, assign, N, L, MV, N_sink, rank, status);
    LAUNCHCHK();
    return 0;
}

struct RankWs { char* plan; size_t plan_bytes; int64_t* job_verbs; int32_t *job_roles, *item_gather, *pred, *assign; float *logp, *seq, *fc; char *ssp, *sh; size_t ssp_bytes, sh_bytes; };
static size_t carve_rank_ws(int N, int MV, int Qcap, int N_sink, char* base, RankWs& w) {
    const size_t S = (size_t)N * MV, R = (size_t)rank_qpad(Qcap) * N_sink;
    Bump b{base};
    w.plan_bytes = vsr_rank_plan_bytes(N, MV, 0);
    w.plan = b.take<char>(w.plan_bytes);
    w.job_verbs = b.take<int64_t>(S); w.job_roles = b.take<int32_t>(S * RANK_L); w.pred = b.take<int32_t>(S * RANK_L); w.logp = b.take<float>(S * RANK_L);
    w.item_gather = b.take<int32_t>(R); w.assign = b.take<int32_t>(R); w.seq = b.take<float>(R * SH_ROW); w.fc = b.take<float>(R * N_sink);
    w.ssp_bytes = vsr_ssp_workspace_bytes((int32_t)S); w.ssp = b.take<char>(w.ssp_bytes);
    w.sh_bytes = vsr_sinkhorn_workspace_bytes(RANK_SH_CHUNK, N_sink); w.sh = b.take<char>(w.sh_bytes);
    return (b.off + 255) & ~size_t(255);
}
extern "C" size_t vsr_rank_workspace_bytes(int32_t N, int32_t MV, int32_t max_items, int32_t N_sink) {
    if (!vsr_rank_plan_bytes(N, MV, max_items) || N_sink < RANK_MIN_SINK || N_sink > RANK_MAX_SINK) return 0;
    RankWs w;
    return carve_rank_ws(N, MV, rank_qcap(N, MV, max_items), N_sink, nullptr, w);
}

extern "C" int vsr_rank_captions(vsr_ssp* e, const int32_t* control_verb, const int32_t* det_seqs_v, const int32_t* det_seqs_sr, int32_t N, int32_t L, int32_t MV,
                                 int32_t MS, int32_t N_sink, int64_t n_verbs, const float* seqs_perm, int32_t max_items, int32_t* rank, int32_t* status,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !e->has_ssp || !e->has_sh) return fail("vsr_rank_captions: the S-SSP and the Sinkhorn weights must both be bound on this object");
    if (!seqs_perm || !rank || !status || !workspace) return fail("vsr_rank_captions: bad arguments");
    if (rank_shape("vsr_rank_captions", N, L, MV, MS, N_sink, max_items)) return 1;
    if (N_sink != e->sw.N || n_verbs != e->w.n_verbs)
        return fail("vsr_rank_captions: N_sink %d / n_verbs %lld differ from the bound models' (%d, %lld)", N_sink, (long long)n_verbs, e->sw.N, (long long)e->w.n_verbs);
    const int S = N * MV, Qcap = rank_qcap(N, MV, max_items);
    RankWs w;
    if (carve_rank_ws(N, MV, Qcap, N_sink, reinterpret_cast<char*>(workspace), w) > workspace_bytes) return fail("vsr_rank_captions: workspace too small");
    RankPlan p;
    carve_rank_plan(N, MV, w.plan, p);
    hipStream_t s = (hipStream_t)stream;
    const int Qpad = rank_qpad(Qcap);
    if (rank_plan_launch(control_verb, det_seqs_v, det_seqs_sr, N, L, MV, MS, N_sink, n_verbs, Qcap, Qpad, w.job_verbs, w.job_roles, w.item_gather, p, s)) return 1;
    const long long n_rows = (long long)Qpad * N_sink;
    hipLaunchKernelGGL(k_rank_gather, dim3((int)std::min<long long>(2048, cdiv(n_rows, 4))), dim3(256), 0, s, seqs_perm, w.item_gather, n_rows, (long long)N * L, w.seq);
    LAUNCHCHK();
    if (vsr_ssp_generate(e, w.job_verbs, w.job_roles, S, w.pred, w.logp, w.ssp, w.ssp_bytes, stream)) return 1;
    ShWs sh;
    if (carve_sh_ws(RANK_SH_CHUNK, N_sink, w.sh, sh) > w.sh_bytes) return fail("vsr_rank_captions: Sinkhorn slot of the workspace too small");
    const ProdRun run = ssp_run(e, s, sh.scratch, sh.scratch_floats, nullptr, 1.f, "sinkhorn forward");
    for (int q = 0; q < Qpad; q += RANK_SH_CHUNK) {
        sh.a.th = w.fc + (size_t)q * N_sink * N_sink;
        if (sinkhorn_layers(run, e->sw, w.seq + (size_t)q * N_sink * SH_ROW, RANK_SH_CHUNK, sh.a)) return 1;
    }
    hipLaunchKernelGGL(k_sinkhorn_assign, dim3(Qpad), dim3(64), 0, s, w.fc, N_sink, e->sw.n_iters, e->sw.tau, (float*)nullptr, w.assign);
    LAUNCHCHK();
    return vsr_rank_finish(w.plan, w.plan_bytes, w.pred, w.assign, N, L, MV, N_sink, rank, status, stream);
}

// ---------------------------------------------------------------------------------------------- training batches on the device
// train_region_sort.py:133-179 and train_sinkhorn.py:144-205 for the N caption rows of a loader batch: integer
// annotations in; the rows of S_SSP.forward and the item tables of SinkhornNet.loc_loss out, compacted in the reference's loop order
// (captions, verb columns, ascending role), with their counts in a 16-byte tensor that is the caller's ONE read-back.  Two launches on
// the caller's stream, no read-back and no allocation here.  The tables are integers and a few floats (under 300 KB at N MV 10 items),
// so max_items = 0 - the static maximum - costs nothing worth a bound; the feature rows are gathered afterwards (vsr_gather_rows) for
// the items that exist.
static size_t carve_tb_plan(int N, int MV, char* base, TbPlan& p) {
    const size_t S = (size_t)N * MV;
    Bump b{base};
    p.row_off = b.take<int32_t>(S); p.item_off = b.take<int32_t>(S); p.jobs = b.take<TbJob>(S);
    return (b.off + 255) & ~size_t(255);
}
extern "C" size_t vsr_train_batch_plan_bytes(int32_t N, int32_t MV) {
    if (N <= 0 || MV < 1 || MV > RANK_MAX_MV || (long long)N * MV * RANK_L > INT_MAX / 64) return 0;
    TbPlan p;
    return carve_tb_plan(N, MV, nullptr, p);
}

extern "C" int vsr_train_batch_plan(const int32_t* control_verb, const int32_t* det_seqs_v, const int32_t* det_seqs_sr, const int32_t* gt_seqs_v,
                                    const int32_t* gt_seqs_sr, int32_t Lg, const int32_t* idx_list, int32_t N, int32_t L, int32_t MV, int32_t MS, int32_t N_sink,
                                    int64_t n_verbs, int32_t max_items, int64_t* verbs, int32_t* det_roles, int32_t* gt_roles, int32_t* item_gather, float* tr_locs,
                                    float* gt_locs, int32_t* item_key, int32_t* counts, int32_t* status, void* plan, size_t plan_bytes, void* stream) {
    if (!control_verb || !det_seqs_v || !det_seqs_sr || !verbs || !det_roles || !counts || !status || !plan || n_verbs <= 0)
        return fail("vsr_train_batch_plan: bad arguments");
    if (!gt_seqs_v != !gt_seqs_sr || (gt_seqs_v && !gt_roles)) return fail("vsr_train_batch_plan: gt_seqs_v, gt_seqs_sr and gt_roles go together");
    if (idx_list && (!item_gather || !tr_locs || !gt_locs || !item_key)) return fail("vsr_train_batch_plan: idx_list needs the four item tables");
    if (!!item_gather != !!tr_locs || !!item_gather != !!gt_locs || !!item_gather != !!item_key)
        return fail("vsr_train_batch_plan: the four item tables go together");
    if (rank_shape("vsr_train_batch_plan", N, L, MV, MS, N_sink, max_items)) return 1;
    if (gt_seqs_v && Lg < 1) return fail("vsr_train_batch_plan: Lg %d < 1", Lg);
    TbPlan p;
    if (carve_tb_plan(N, MV, reinterpret_cast<char*>(plan), p) > plan_bytes) return fail("vsr_train_batch_plan: plan buffer too small");
    const int S = N * MV, Qcap = rank_qcap(N, MV, max_items);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tb_jobs, dim3(cdiv(S, 64)), dim3(64), 0, s, control_verb, det_seqs_v, det_seqs_sr, gt_seqs_v, gt_seqs_sr, idx_list, N, L, gt_seqs_v ? Lg : 1,
                       MV, MS, N_sink, (long long)n_verbs, p);
    TbOut o{verbs, det_roles, gt_roles, item_gather, tr_locs, gt_locs, item_key, counts, status};
    hipLaunchKernelGGL(k_tb_compact, dim3(1), dim3(256), 0, s, p, idx_list, N, L, MV, N_sink, Qcap, o);
    LAUNCHCHK();
    return 0;
}

extern "C" int vsr_gather_rows(const float* rows, int64_t n_src_rows, int32_t D, const int32_t* gather, int64_t n_out_rows, float* out, void* stream) {
    if (!rows || !gather || !out || n_src_rows <= 0 || n_out_rows < 0 || n_src_rows > INT_MAX || n_out_rows > INT_MAX) return fail("vsr_gather_rows: bad arguments");
    if (D < 4 || D % 4) return fail("vsr_gather_rows: D %d must be a positive multiple of 4", D);
    if (n_out_rows == 0) return 0;
    const dim3 grid((int)std::min<long long>(2048, cdiv((long long)n_out_rows, 4LL)));
    if (D == SH_ROW)
        hipLaunchKernelGGL(k_rank_gather, grid, dim3(256), 0, (hipStream_t)stream, rows, gather, (long long)n_out_rows, (long long)n_src_rows, out);
    else
        hipLaunchKernelGGL(k_tb_gather, grid, dim3(256), 0, (hipStream_t)stream, rows, gather, (long long)n_out_rows, (long long)n_src_rows, D / 4, out);
    LAUNCHCHK();
    return 0;
}
