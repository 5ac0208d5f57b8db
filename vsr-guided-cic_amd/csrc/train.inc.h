// Training path of libvsrcap.so: teacher-forced (or sample-replayed) forward that saves activations, and the
// hand-written BPTT backward.  Included at the end of vsrcap.hip.
//
// Reference: coco_scripts/train.py:103-113 (XE: model(...) -> NLL losses -> loss.backward()) and :151-178 (SCST:
// sample_rl log-probs -> loss.backward()); the graph autograd differentiates there is step :117-190 unrolled T times.
//
// Backward structure (B rows, T steps, rows of the "all-steps" matrices ordered (t, b)):
//   phase 0  dlogits for all steps (log_softmax backward) and dh2_vocab = dlogits . W_out        one big GEMM
//   phase A  t = T-1 .. 0: pointwise backward kernels + 3 grouped GEMMs per step against TRANSPOSED weights
//            (data gradients only): dpre2_t, dpre1_t, d[hg|hA]_t, d[sent|sa]_t, dga_t, dP rows, state carries
//   phase B  all weight gradients as big GEMMs with the reduction over the T*B rows:
//            dW[n][k] = sum_rows dY^T[n][row] * X^T[k][row]   (both operands transposed once per call)
// so every matrix product of the backward pass runs on the same stream-K fp32-MFMA kernel as the forward pass.
// Stated once: the transposed operands (train_operands), a step's slices of the saved arrays (train_step_slices), the step's grouped
// GEMMs (step_gemms.h), the 28 gradients with their producers and buckets (train_grad_table), the ordered column sum of every bias
// gradient here and in the ordering models (colsum_partials / colsum_finish / colsum, one finishing kernel).

constexpr int VSR_GRAD_BUCKETS = 5;
// f16x2 backward: the "dynamic" slots of the exponent table (from H2_DYN0), where the producers of the gradient operands fold max |x|.
// Block tt of DYN_PER_STEP slots belongs to step tt (DY_*); the last two blocks hold the whole-pass slots (DW_*): DW_step + DY_x is the
// max over the steps of DY_x (k_h2_dyn_fold)
constexpr int DYN_PER_STEP = 8, DYN_MAX_T = H2_NDYN / DYN_PER_STEP - 2;
enum { DY_dpre2, DY_dga, DY_dq, DY_dhA, DY_dsent, DY_dsa, DY_dpre1, DY_N };
enum { DW_dlogits = DYN_MAX_T * DYN_PER_STEP, DW_dP, DW_dpre1sum, DW_dpre2sum, DW_dpre1all, DW_N, DW_step = (DYN_MAX_T + 1) * DYN_PER_STEP };
static_assert(DY_N <= DYN_PER_STEP && DW_N <= DW_step && DW_step + DYN_PER_STEP == H2_NDYN && DYN_MAX_T == 62,
              "the per-step blocks, then one block of whole-pass slots, then the block of the per-step maxima: k_h2_dyn_fold");

struct TrainCtx {                      // (plain data + one vector, `images`: copied into SavedForwards)
    bool valid = false;
    const char* tws_lo = nullptr;      // the training workspace this forward was carved into
    size_t tws_bytes = 0;
    int* h2_stash = nullptr;           // f16x2: the per-batch exponents / bounds of the handle's table as they were for THIS forward (8 ints)
    long long generation = 0;          // bumped by every vsr_train_forward: identifies the saved forward a backward belongs to
    int B = 0, T = 0, TB = 0, TBp = 0, Bp = 0, RLp = 0;       // B: decoder ROWS (= images x rpi); Bp: the IMAGES, padded (K of the v-bar products)
    int rpi = 1;                       // rows per image (vsr_train_forward_rows): rows b rpi .. b rpi + rpi - 1 share image b's statics
    // a TAPE (vsr_train_tape_begin): a forward taken one step per call.  tape_max = the steps its workspace was carved for (0: a whole
    // forward), tape_steps = the steps taken; T / TB / TBp and logp_w / logp_g are those of the steps taken once it is sealed
    int tape_max = 0, tape_steps = 0;
    bool sealed = false;
    // a SPARSE forward (vsr_train_forward_selected): no (B,T,V) tensor exists - the (t, b) log_softmax rows are in `dlogits` (stride
    // up8(V)), the validated targets in tgt32 (the storage of rows_bt, which such a forward does not gather through), logp_w is null.
    // vsr_train_backward_selected turns the rows into dlogits in place and marks the forward consumed: it cannot be differentiated twice
    bool sparse = false, consumed = false;
    int* tgt32 = nullptr;
    // ... with row statistics (vsr_train_forward_selected_stats): the caller's (rows, T) entropy output, held like logp_g - the backward of
    // an entropy gradient reads H from it.  Null: a plain sparse forward (or a dense one)
    const float* ent = nullptr;
    float* dP_rows = nullptr;          // rpi > 1: the rows' (R, A) contributions to dP of the current step (k_attend_bwd -> k_dP_rows_sum)
    const float* logp_w = nullptr;     // caller's (B,T,V) output of the forward, needed by the backward
    const float* logp_g = nullptr;     // (B,T,2)
    float *h1s, *c1s, *h2s, *c2s;      // (T+1, B, H): slot 0 = zeros
    float *gates1, *gates2, *s_ts, *g_ts, *hAs, *sas, *gas, *sents, *atts, *alphas, *x_all;
    int *word32, *slot32, *rows_bt;
    float *dlogits, *dh2_voc, *dpre1, *dpre2, *dhA_all, *dsent_all, *dsa_all, *dga_all, *dwa_rows, *dws_rows, *dwg_rows, *dP;
    float* dP_bank = nullptr;        // index-list regions: dP summed over the slot entries that name each bank row
    float *dalpha;
    float *datt, *dtc, *dh_tot, *dzsum, *dh1_c, *dh2_c, *dc1_c[2], *dc2_c[2], *dpre1sum, *dpre2sum, *dx_all;
    float *wT_ih1, *wT_is, *wT_ig, *wT_hh1, *wT_hs, *wT_ih2, *wT_hh2, *wT_hg, *wT_ha, *wT_sfc, *wT_sa, *wT_ga, *wT_out;
    float *tX_h2prev, *tX_x, *tX_h1prev, *tX_h1, *tX_att, *tX_st, *tX_gt, *tX_h2, *tX_vbar, *tX_reg;
    float *tY_dpre1, *tY_dpre2, *tY_dlogits, *tY_dhA, *tY_dsent, *tY_dsa, *tY_dga, *tY_dpre1sum, *tY_dpre2sum, *tY_dP;
    float* xproj_all;            // (T B, 6H): embedding rows through the x columns of the LSTM1 / gate input weights
    float* scratch;
    size_t scratch_floats = 0;
    // Every transposed operand that a GEMM takes as W (transposed weights, transposed activations of the weight-gradient products), as
    // the registry takes it (OperandImages::register_train; entry i = operand i of train_operands): its bf16 twin, which the transposing
    // kernels write instead of the fp32 buffer in the bf16 mode, and in the f16x2 flavour its fp16-pair image (gemm_h2.h) in h2img,
    // written likewise (transpose()); slot = exponent slot of the values (the weight's own, or the class of the activation)
    std::vector<ImageRange> images;
    float* h2img = nullptr;
    // ... and the forward pass's A operands are written as fp16-pair images by their producers (kernels.h img_store; gemm_h2a.h takes them):
    // h1 / h2 of every step (T + 1 slots like the fp32 saves), s_t / g_t / the attended vector of the current step
    uint16_t *h1s16 = nullptr, *h2s16 = nullptr, *s_t16 = nullptr, *g_t16 = nullptr, *att16 = nullptr;
};

static inline size_t up4(size_t x) { return (x + 7) & ~size_t(7); }   // K paddings: multiples of 8 (16-byte bf16 chunks; fp32 needs 4)

// One transposed operand of the backward pass: buf (C, ld_out) = src (R, C; leading dimension ld_in) transposed.  THE description of the
// buffer: carve_train takes it (and, for a W operand, its bf16 twin and its fp16-pair image with exponent slot `slot`) by size(), the
// backward transposes by R / C / ld, the gradient table (train_grad_table) names its operands by entry.
struct TOperand {
    float* TrainCtx::* buf; const float* src; int R, C; long long ld_in, ld_out; int slot;
    size_t size() const { return (size_t)C * (size_t)ld_out; }
};
// The 13 transposed weights, the 10 transposed activations (both W operands), then the 10 transposed gradients (the A operands of the
// weight-gradient products): the order of the workspace and of the batched transposes.
enum { TW_ih1, TW_is, TW_ig, TW_hh1, TW_hs, TW_ih2, TW_hh2, TW_hg, TW_ha, TW_sfc, TW_sa, TW_ga, TW_out,
       TX_h2prev, TX_x, TX_h1prev, TX_h1, TX_att, TX_st, TX_gt, TX_h2, TX_vbar, TX_reg,
       TY_dpre1, TY_dpre2, TY_dlogits, TY_dhA, TY_dsent, TY_dsa, TY_dga, TY_dpre1sum, TY_dpre2sum, TY_dP, N_TOPS };
constexpr int N_TW = TX_h2prev, N_TWX = TY_dpre1;       // [0, N_TW) weights, [N_TW, N_TWX) activations, [N_TWX, N_TOPS) gradients
// Reads B / rpi / TB / TBp / Bp / RLp of `t`: for a sealed tape those of the steps taken (its buffers were carved for tape_max).  The
// sources in the workspace are null while it is only being sized.  TX_reg and TY_dP are sized here (RLp) and transposed through the list
// of the non-padding rows (R = 0 here: the backward sets their R / ld_out to the rows it gathers).  A gradient's slot is its DYNAMIC
// slot (DW_*: relative to H2_DYN0, and only while the backward runs on the f16x2 kernels)
static void train_operands(const vsr_handle* h, const TrainCtx& t, TOperand (&o)[N_TOPS]) {
    const vsr_dims& d = h->d;
    const vsr_weights& w = h->w;
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size, E = d.input_encoding_size, V = d.vocab_size;
    const int in1 = (d.h2_first_lstm ? H : 0) + D + E, in2 = H + D + (d.img_second_lstm ? D : 0), Bi = t.B / t.rpi;
    const size_t BH = (size_t)t.B * H;
    // (N, K) weight -> (K, ld_out >= N); the transposed matrix has the bound of the matrix: its slot (0..13, the order of gemm_matrix_list)
    auto W = [&](int i, float* TrainCtx::* buf, const float* src, int N, int K, long long ld_out) { o[i] = TOperand{buf, src, N, K, K, ld_out, h->img.h2_slot_of(src)}; };
    W(TW_ih1, &TrainCtx::wT_ih1, w.lstm1_weight_ih, 4 * H, in1, 4 * H); W(TW_is, &TrainCtx::wT_is, w.W1_is_weight, H, in1, H); W(TW_ig, &TrainCtx::wT_ig, w.W1_ig_weight, H, in1, H);
    W(TW_hh1, &TrainCtx::wT_hh1, w.lstm1_weight_hh, 4 * H, H, 4 * H); W(TW_hs, &TrainCtx::wT_hs, w.W1_hs_weight, H, H, H);
    W(TW_ih2, &TrainCtx::wT_ih2, w.lstm2_weight_ih, 4 * H, in2, 4 * H); W(TW_hh2, &TrainCtx::wT_hh2, w.lstm2_weight_hh, 4 * H, H, 4 * H);
    W(TW_hg, &TrainCtx::wT_hg, w.W1_hg_weight, H, H, H); W(TW_ha, &TrainCtx::wT_ha, w.att_ha_weight, A, H, A); W(TW_sfc, &TrainCtx::wT_sfc, w.s_fc_weight, D, H, D);
    W(TW_sa, &TrainCtx::wT_sa, w.att_sa_weight, A, H, A); W(TW_ga, &TrainCtx::wT_ga, w.att_ga_weight, A, H, A);
    W(TW_out, &TrainCtx::wT_out, w.out_fc_weight, V, H, (long long)up4(V));      // (K of the dh2_vocab GEMM: a multiple of 8)
    // (R, C) matrix, leading dimension ld_in -> (C, R padded); slot: the class of the activation / the dynamic slot of the gradient
    auto X = [&](int i, float* TrainCtx::* buf, const float* src, size_t skip, int R, int C, long long ld_in, long long ld_out, int slot) {
        o[i] = TOperand{buf, src ? src + skip : nullptr, R, C, ld_in, ld_out, slot};
    };
    X(TX_h2prev, &TrainCtx::tX_h2prev, t.h2s, 0, t.TB, H, H, t.TBp, H2A_UNIT); X(TX_x, &TrainCtx::tX_x, t.x_all, 0, t.TB, E, E, t.TBp, H2A_EMBED);   // state slots 0 .. T-1: entering step t
    X(TX_h1prev, &TrainCtx::tX_h1prev, t.h1s, 0, t.TB, H, H, t.TBp, H2A_UNIT); X(TX_h1, &TrainCtx::tX_h1, t.h1s, BH, t.TB, H, H, t.TBp, H2A_UNIT);
    X(TX_att, &TrainCtx::tX_att, t.atts, 0, t.TB, D, D, t.TBp, H2A_ATT); X(TX_st, &TrainCtx::tX_st, t.s_ts, 0, t.TB, H, H, t.TBp, H2A_UNIT);
    X(TX_gt, &TrainCtx::tX_gt, t.g_ts, 0, t.TB, H, H, t.TBp, H2A_UNIT); X(TX_h2, &TrainCtx::tX_h2, t.h2s, BH, t.TB, H, H, t.TBp, H2A_UNIT);
    X(TX_vbar, &TrainCtx::tX_vbar, h->c.vbar, 0, Bi, D, D, t.Bp, H2A_DET);     // per IMAGE
    X(TX_reg, &TrainCtx::tX_reg, h->c.regions, 0, 0, D, D, t.RLp, H2A_REGION);
    // rows (t, b) of every step; dpre1 is ONE image (all six column blocks), dlogits' rows are padded to up8(V)
    X(TY_dpre1, &TrainCtx::tY_dpre1, t.dpre1, 0, t.TB, 6 * H, 6 * H, t.TBp, DW_dpre1all); X(TY_dpre2, &TrainCtx::tY_dpre2, t.dpre2, 0, t.TB, 4 * H, 4 * H, t.TBp, DW_step + DY_dpre2);
    X(TY_dlogits, &TrainCtx::tY_dlogits, t.dlogits, 0, t.TB, V, (long long)up4(V), t.TBp, DW_dlogits);
    X(TY_dhA, &TrainCtx::tY_dhA, t.dhA_all, 0, t.TB, A, A, t.TBp, DW_step + DY_dhA); X(TY_dsent, &TrainCtx::tY_dsent, t.dsent_all, 0, t.TB, D, D, t.TBp, DW_step + DY_dsent);
    X(TY_dsa, &TrainCtx::tY_dsa, t.dsa_all, 0, t.TB, A, A, t.TBp, DW_step + DY_dsa); X(TY_dga, &TrainCtx::tY_dga, t.dga_all, 0, t.TB, A, A, t.TBp, DW_step + DY_dga);
    // per IMAGE: the sums over an image's rows and steps (the gradients of the hoisted v-bar projections)
    X(TY_dpre1sum, &TrainCtx::tY_dpre1sum, t.dpre1sum, 0, Bi, 6 * H, 6 * H, t.Bp, DW_dpre1sum); X(TY_dpre2sum, &TrainCtx::tY_dpre2sum, t.dpre2sum, 0, Bi, 4 * H, 4 * H, t.Bp, DW_dpre2sum);
    // dP per slot entry, or (index lists) summed per bank row first
    X(TY_dP, &TrainCtx::tY_dP, h->c.ridx ? t.dP_bank : t.dP, 0, 0, A, A, t.RLp, DW_dP);
}

static size_t carve_train(const vsr_handle* h, TrainCtx& t, char* base) {
    const vsr_dims& d = h->d;
    const Ctx& c = h->c;
    const size_t B = t.B, T = t.T, H = d.rnn_size, A = d.att_size, D = d.det_feat_size, E = d.input_encoding_size, V = d.vocab_size;
    const size_t in1 = (d.h2_first_lstm ? H : 0) + D + E, in2 = H + D + (d.img_second_lstm ? D : 0);
    const size_t Bi = B / t.rpi;       // images: what the per-image arrays (dP, the v-bar side) are sized by
    const size_t TB = T * B, TBp = up4(TB), Bp = up4(Bi), RL = (size_t)c.B * c.L * c.R, R1 = c.R + 1;
    // rows att_va's weight gradient runs over: the slot entries (dense regions) or the feature-bank rows (index lists)
    const size_t PR = c.Rb > 0 ? (size_t)c.n_img * c.Rb : RL, RLp = up4(std::max(RL, PR));
    t.TB = (int)TB; t.TBp = (int)TBp; t.Bp = (int)Bp; t.RLp = (int)RLp;
    Bump b{base};
    t.h1s = b.take<float>((T + 1) * B * H); t.c1s = b.take<float>((T + 1) * B * H);
    t.h2s = b.take<float>((T + 1) * B * H); t.c2s = b.take<float>((T + 1) * B * H);
    t.gates1 = b.take<float>(TB * 6 * H); t.gates2 = b.take<float>(TB * 4 * H);
    t.s_ts = b.take<float>(TB * H); t.g_ts = b.take<float>(TB * H);
    t.hAs = b.take<float>(TB * A); t.sas = b.take<float>(TB * A); t.gas = b.take<float>(TB * A);
    t.sents = b.take<float>(TB * D); t.atts = b.take<float>(TB * D); t.alphas = b.take<float>(TB * R1);
    t.x_all = b.take<float>(TB * E);
    t.word32 = b.take<int>(TB); t.slot32 = b.take<int>(TB); t.rows_bt = b.take<int>(TB);
    t.h2_stash = b.take<int>(8);
    t.dlogits = b.take<float>(TB * up4(V)); t.dh2_voc = b.take<float>(TB * H);
    t.dpre1 = b.take<float>(TB * 6 * H); t.dpre2 = b.take<float>(TB * 4 * H);
    t.dhA_all = b.take<float>(TB * A); t.dsent_all = b.take<float>(TB * D); t.dsa_all = b.take<float>(TB * A); t.dga_all = b.take<float>(TB * A);
    t.dwa_rows = b.take<float>(TB * A); t.dws_rows = b.take<float>(TB * A); t.dwg_rows = b.take<float>(TB * A);
    t.dP = b.take<float>(RL * A);
    t.dP_bank = c.Rb > 0 ? b.take<float>(PR * A) : nullptr;
    t.dP_rows = t.rpi > 1 ? b.take<float>(B * c.R * A) : nullptr;
    t.datt = b.take<float>(B * D); t.dtc = b.take<float>(B * H);
    t.dh_tot = b.take<float>(B * H); t.dzsum = b.take<float>(B); t.dalpha = b.take<float>(B * R1);
    t.dh1_c = b.take<float>(B * H); t.dh2_c = b.take<float>(B * H);
    for (int i = 0; i < 2; ++i) { t.dc1_c[i] = b.take<float>(B * H); t.dc2_c[i] = b.take<float>(B * H); }
    t.dpre1sum = b.take<float>(Bi * 6 * H); t.dpre2sum = b.take<float>(Bi * 4 * H); t.dx_all = b.take<float>(TB * E); t.xproj_all = b.take<float>(TB * 6 * H);
    // the transposed operands (train_operands): the fp32 buffer of each, bf16 twin and fp16-pair image of a W operand, all sized and slotted by its entry
    TOperand ops[N_TOPS];
    train_operands(h, t, ops);
    t.images.clear();
    auto take = [&](int lo, int hi) { for (int i = lo; i < hi; ++i) t.*ops[i].buf = b.take<float>(ops[i].size()); };
    auto twins = [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i) t.images.push_back(ImageRange{t.*ops[i].buf, t.*ops[i].buf + ops[i].size(), ImageRange::TRAIN, b.take<uint16_t>(ops[i].size()), nullptr, ops[i].slot});
    };
    take(0, N_TW);
    twins(0, N_TW);
    b.off = (b.off + 255) & ~size_t(255);
    take(N_TW, N_TOPS);               // (the gradients are A operands: no twins, no registered images)
    twins(N_TW, N_TWX);
    t.h2img = nullptr;
    if (h->train_h2_images()) {
        size_t off = 0;
        for (int i = 0; i < N_TWX; ++i) off += up4(ops[i].size());
        b.off = (b.off + 255) & ~size_t(255);
        t.h2img = b.take<float>(off);
        off = 0;
        for (int i = 0; i < N_TWX; ++i) { t.images[i].h2 = t.h2img + off; off += up4(ops[i].size()); }
        b.off = (b.off + 255) & ~size_t(255);
        t.h1s16 = b.take<uint16_t>(2 * (T + 1) * B * H); t.h2s16 = b.take<uint16_t>(2 * (T + 1) * B * H);
        t.s_t16 = b.take<uint16_t>(2 * B * H); t.g_t16 = b.take<uint16_t>(2 * B * H); t.att16 = b.take<uint16_t>(2 * B * D);
    } else {
        t.h1s16 = t.h2s16 = t.s_t16 = t.g_t16 = t.att16 = nullptr;
    }
    // GEMM slab scratch: every slab of the largest product of the training path (products.h), and of the step launches placed in it, by
    // their layouts (step_gemms.h): the x projection and the vocabulary projection over T B rows.  The backward step's GEMM 1 stays at
    // B (in2 + 2H): its layout (bwd1_slabs) takes B (3H + D), which that equals, or with img_second_lstm exceeds by B D (kept: no size
    // changes); GEMM 2 and 3 take B 2H, less than GEMM 1.
    size_t big = std::max({4 * H * in1, V * H, 4 * H * in2, A * D, TB * H, TB * E, D * H, B * (in2 + 2 * H), H * in1, TB * slab_row_floats(vocab_slabs(d)),
                           TB * slab_row_floats(lstm1_slabs(d))});
    t.scratch_floats = big * GEMM_MAX_SLABS;
    t.scratch = b.take<float>(t.scratch_floats);
    return (b.off + 255) & ~size_t(255);
}

// whole-pass bounds from the per-step ones (DW_step + j: max over the steps; DW_dpre1sum / DW_dpre2sum: the sums over t of dpre1 / dpre2 rows)
// (nsum: rows one sum runs over - the T steps of a row, times the rows of an image when several share its statics)
__global__ void k_h2_dyn_fold(int* __restrict__ dyn, int T, int nsum) {
    const int j = threadIdx.x;
    if (j >= DYN_PER_STEP) return;
    int m = 0;
    for (int tt = 0; tt < T; ++tt) m = max(m, dyn[tt * DYN_PER_STEP + j]);
    dyn[DW_step + j] = m;
    if (j == DY_dpre2) dyn[DW_dpre2sum] = __float_as_int(__int_as_float(m) * (float)nsum);
    if (j == DY_dpre1) {
        int m2 = 0;
        for (int tt = 0; tt < T; ++tt) m2 = max(m2, dyn[tt * DYN_PER_STEP + DY_dq]);
        dyn[DW_dpre1sum] = __float_as_int(fmaxf(__int_as_float(m), __int_as_float(m2)) * (float)nsum);
        dyn[DW_dpre1all] = max(m, m2);                                      // all six column blocks of dpre1 (its transpose is one image)
    }
}

// THE deterministic two-stage column sum (bias gradients) of the decoder's and the ordering models' (ssp.inc.h) backward passes.
// colsum_partials: table[chunk][c] = the sum of that chunk of X's rows (R rows, C columns, leading dimension ld); COLSUM_CHUNKS x C floats.
// colsum_finish: out[c] (and out2[c]) = the ordered sum of the partials of columns [c0, c0 + n) of a table of C columns; two: of TWO tables, one
// after the other in memory and in the sum.  Several finishes may share a table (the gradient table's column windows of dpre1).
static void colsum_partials(hipStream_t s, const float* X, long long ld, int R, int C, float* table) {
    hipLaunchKernelGGL(k_colsum, dim3(cdiv(C, 64), COLSUM_CHUNKS), dim3(256), 0, s, X, ld, R, C, table);
}
static void colsum_finish(hipStream_t s, const float* table, int C, int c0, int n, float* out, float* out2 = nullptr, bool two = false) {
    hipLaunchKernelGGL(two ? k_colsum_finish<2> : k_colsum_finish<1>, dim3(cdiv(n, 256)), dim3(256), 0, s, table, C, c0, n, out, out2);
}
// the pair for a whole matrix, through `part` (the idle slab scratch, or S-SSP's own two tables); X2 (R2, C; compact): the second use of one bias
static void colsum(hipStream_t s, float* part, const float* X, long long ld, int R, int C, float* out, float* out2 = nullptr, const float* X2 = nullptr, int R2 = 0) {
    colsum_partials(s, X, ld, R, C, part);
    if (X2) colsum_partials(s, X2, C, R2, C, part + (size_t)COLSUM_CHUNKS * C);
    colsum_finish(s, part, C, 0, C, out, out2, X2 != nullptr);
}
// up to ZERO_MT buffers zeroed by one launch (sizes in bytes, multiples of 16; pointers 16-byte aligned)
struct ZeroList {
    ZeroMulti z; int blocks = 0;
    ZeroList() { memset(&z, 0, sizeof(z)); }
    void add(void* p, size_t bytes) {
        if (!p || bytes == 0) return;
        z.p[z.nt] = p; z.n16[z.nt] = (long long)(bytes / 16); z.blk[z.nt] = blocks;
        blocks += (int)std::max<long long>(1, std::min<long long>(2048, (long long)(bytes / 16 + 1023) / 1024));
        z.blk[++z.nt] = blocks;
    }
    int launch(hipStream_t s) {
        if (z.nt == 0) return 0;
        hipLaunchKernelGGL(k_zero_multi, dim3(blocks), dim3(256), 0, s, z);
        return hipGetLastError() == hipSuccess ? 0 : 1;
    }
};
// out = in^T (rows optionally gathered through `list`).  A buffer that a GEMM takes as W receives ONLY its image - the registered bf16
// twin in the bf16 mode, the fp16-pair image of the f16x2 flavour when the backward pass runs on those kernels (h2img) - and the fp32
// buffer `out` then only lends its address
// self_slot >= 0: `out` itself receives the image (an A operand: a transposed gradient, scaled by the bound in that slot of the table)
// (batch: transposes without a row list may be COLLECTED and launched together - TransBatch::flush - in the order they were added)
struct TransBatch {
    TransMulti m; int kind = -1, blocks = 0; const int* exps = nullptr;
    TransBatch() { memset(&m, 0, sizeof(m)); }
    void flush(hipStream_t s) {
        if (m.nt == 0) return;
        if (kind == 2) hipLaunchKernelGGL((k_transpose_multi<2>), dim3(blocks), dim3(256), 0, s, m, exps);
        else if (kind == 1) hipLaunchKernelGGL((k_transpose_multi<1>), dim3(blocks), dim3(256), 0, s, m, exps);
        else hipLaunchKernelGGL((k_transpose_multi<0>), dim3(blocks), dim3(256), 0, s, m, exps);
        memset(&m, 0, sizeof(m)); kind = -1; blocks = 0;
    }
    void add(hipStream_t s, int k, const int* ex, const float* in, long long ld_in, int R, int C, float* out, long long ld_out, uint16_t* img, int slot) {
        if (m.nt == TR_MT || (m.nt > 0 && k != kind)) flush(s);
        kind = k; exps = ex;
        const int i = m.nt++;
        m.in[i] = in; m.ld_in[i] = ld_in; m.R[i] = R; m.C[i] = C; m.out[i] = out; m.ld_out[i] = ld_out; m.out16[i] = img; m.slot[i] = slot;
        m.blk[i] = blocks;
        blocks += cdiv(C, 64) * cdiv(R, 64);
        m.blk[i + 1] = blocks;
    }
};
// where a transpose's output goes: kind 0 = the fp32 buffer, 1 = its bf16 twin, 2 = an fp16-pair image scaled by exps[slot] - the registered
// one of a W operand (h2img), else `out` itself when the caller names a slot (self_slot >= 0) and the buffer can hold an image in place
struct TransDst { int kind; uint16_t* img; int slot; const int* exps; };
static TransDst trans_dst(const vsr_handle* h, float* out, long long ld_out, bool h2img, int self_slot) {
    if (uint16_t* tw = h->bf16() ? const_cast<uint16_t*>(h->img.bf16_of(out)) : nullptr) return TransDst{1, tw, 0, nullptr};
    if (h2img) {
        if (const ImageRange* r2 = h->img.h2_of(out)) return TransDst{2, reinterpret_cast<uint16_t*>(const_cast<float*>(r2->h2_at(out))), r2->slot, h->h2_exps};
        if (self_slot >= 0 && ld_out % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 31) == 0) return TransDst{2, reinterpret_cast<uint16_t*>(out), self_slot, h->h2_exps};
    }
    return TransDst{0, nullptr, 0, nullptr};
}
static void transpose(vsr_handle* h, hipStream_t s, const float* in, long long ld_in, int R, int C, float* out, long long ld_out,
                      const int* list = nullptr, bool h2img = false, int self_slot = -1, const int* rlimit = nullptr, TransBatch* tb = nullptr) {
    const TransDst d = trans_dst(h, out, ld_out, h2img, self_slot);
    if (tb && !list) { tb->add(s, d.kind, d.exps, in, ld_in, R, C, out, ld_out, d.img, d.slot); return; }
    auto go = [&](auto GATHER, auto IMG) {
        hipLaunchKernelGGL((k_transpose_t<decltype(GATHER)::value, decltype(IMG)::value>), dim3(cdiv(C, 64), cdiv(R, 64)), dim3(256), 0, s, in, ld_in, list, R, C,
                           out, ld_out, d.img, d.exps, d.slot, list ? rlimit : (const int*)nullptr);
    };
    auto kind = [&](auto GATHER) {
        if (d.kind == 2) go(GATHER, std::integral_constant<int, 2>{});
        else if (d.kind == 1) go(GATHER, std::integral_constant<int, 1>{});
        else go(GATHER, std::integral_constant<int, 0>{});
    };
    if (list) kind(std::true_type{}); else kind(std::false_type{});
}

// ---------------------------------------------------------------------------------------------- more than one live forward
// The reference runs under eager autograd: two forwards and then (l1 + l2).backward(), or a decode between a forward and its backward,
// just work (CaptioningModel.py:22-36).  Here a forward's saved state is the pair (Ctx, TrainCtx) of pointers into TWO caller buffers:
// the vsr_prepare*() workspace and the training workspace.  Every vsr_train_forward files a copy of that pair under its generation; a
// later vsr_prepare*() / vsr_train_forward drops the copies whose buffers it is about to overwrite (address overlap) and keeps the
// rest.  A caller that gives its second forward OTHER buffers can therefore still differentiate the first: vsr_train_select() makes a
// filed forward the handle's current one again (pointers, image registrations, the per-batch rows of the f16x2 exponent table).
struct SavedForward { Ctx c; TrainCtx t; const char* ws_lo; size_t ws_bytes; };
struct SavedForwards { std::vector<SavedForward> v; };
static SavedForwards* new_saved_forwards() { return new SavedForwards(); }
static void free_saved_forwards(SavedForwards* s) { delete s; }
static void drop_saved_forwards(SavedForwards* s) { if (s) s->v.clear(); }
static bool ranges_overlap(const char* a, size_t na, const char* b, size_t nb) { return a && b && a < b + nb && b < a + na; }
static void drop_saved_forwards_in(SavedForwards* s, const void* lo, size_t bytes) {
    if (!s) return;
    const char* p = reinterpret_cast<const char*>(lo);
    for (size_t i = s->v.size(); i-- > 0;)
        if (ranges_overlap(p, bytes, s->v[i].ws_lo, s->v[i].ws_bytes) || ranges_overlap(p, bytes, s->v[i].t.tws_lo, s->v[i].t.tws_bytes))
            s->v.erase(s->v.begin() + i);
}
// the images of a training workspace's transposed operands: the GEMM builder finds them by address
static void register_train_images(vsr_handle* h, const TrainCtx& t) { h->img.register_train(t.images); }
// rows of the f16x2 exponent / bound tables that vsr_prepare*() fills per batch (H2A_REGION, H2A_DET, H2A_ATT): dir 0 = table -> stash
__global__ void k_h2_stash(int* __restrict__ exps, unsigned* __restrict__ bounds, int* __restrict__ stash, int dir) {
    const int i = threadIdx.x;
    if (i >= 3) return;
    if (dir == 0) { stash[i] = exps[H2A_REGION + i]; stash[4 + i] = (int)bounds[H2A_REGION + i]; }
    else { exps[H2A_REGION + i] = stash[i]; bounds[H2A_REGION + i] = (unsigned)stash[4 + i]; }
}
static_assert(H2A_DET == H2A_REGION + 1 && H2A_ATT == H2A_REGION + 2, "k_h2_stash walks three consecutive slots");

extern "C" int vsr_train_select(vsr_handle* h, int64_t generation, void* stream) {
    if (!h || !h->tc) return fail("vsr_train_select: null handle");
    if (generation <= 0) return fail("vsr_train_select: generation %lld", (long long)generation);
    if (h->tc->valid && h->tc->generation == generation && h->prepared) return 0;
    for (const SavedForward& sf : h->saved->v)
        if (sf.t.generation == generation) {
            h->c = sf.c;
            *h->tc = sf.t;
            h->tc->valid = true;
            h->ws_lo = sf.ws_lo; h->ws_bytes = sf.ws_bytes;
            h->prepared = true;
            register_train_images(h, *h->tc);
            if (h->measures_h2_bounds() && h->tc->h2_stash) hipLaunchKernelGGL(k_h2_stash, dim3(1), dim3(64), 0, (hipStream_t)stream, h->h2_exps, h->h2_bounds, h->tc->h2_stash, 1);
            LAUNCHCHK();
            return 0;
        }
    return fail("vsr_train_select: the forward pass of generation %lld is gone (a later vsr_prepare*() / vsr_train_forward was given its "
                "workspaces, or the GEMM flavour / the weight binding changed)", (long long)generation);
}

extern "C" size_t vsr_train_workspace_bytes_rows(const vsr_handle* h, int32_t B, int32_t rows_per_image, int32_t T) {
    if (!h || !h->prepared || B != h->c.B || T <= 0 || rows_per_image < 1 || rows_per_image > VSR_MAX_BEAM) return 0;
    TrainCtx t;
    t.rpi = rows_per_image; t.B = B * rows_per_image; t.T = T;
    return carve_train(h, t, nullptr);
}
extern "C" size_t vsr_train_workspace_bytes(const vsr_handle* h, int32_t B, int32_t T) { return vsr_train_workspace_bytes_rows(h, B, 1, T); }

// ---------------------------------------------------------------------------------------------- forward with saves
// f16x2 flavour: fp16-pair images of the A operands (all-DMA kernel); BH elements of 4 bytes per state slot
static bool train_a_images(const vsr_handle* h, const TrainCtx& t) {
    return h->writes_h2_a_images() && t.h1s16 && (t.B * h->d.rnn_size) % 8 == 0;
}
// Begins a saved forward of K rows per image and T steps in the caller's buffer: carves it, drops the forwards filed in it, registers the
// images of its transposed operands and zeroes the states of step 0.  `who`: the public function, for the messages
static int train_begin(vsr_handle* h, TrainCtx& t, int K, int T, void* train_ws, size_t bytes, const char* who, hipStream_t s) {
    t.valid = false;
    t.rpi = K; t.B = h->c.B * K; t.T = T;
    const size_t need = carve_train(h, t, reinterpret_cast<char*>(train_ws));
    if (need > bytes) return fail("%s: training workspace too small (%zu < %zu)", who, bytes, need);
    drop_saved_forwards_in(h->saved, train_ws, need);       // forwards filed in THIS buffer are overwritten now
    t.tws_lo = reinterpret_cast<const char*>(train_ws); t.tws_bytes = need;
    register_train_images(h, t);                           // the bf16 twins / fp16-pair images of this workspace's transposed operands
    const size_t BH = (size_t)t.B * h->d.rnn_size;
    ZeroList zl;                                           // the zero states of step 0 (and their images): one launch
    zl.add(t.h1s, BH * sizeof(float)); zl.add(t.c1s, BH * sizeof(float)); zl.add(t.h2s, BH * sizeof(float)); zl.add(t.c2s, BH * sizeof(float));
    if (train_a_images(h, t)) { zl.add(t.h1s16, BH * 2 * sizeof(uint16_t)); zl.add(t.h2s16, BH * 2 * sizeof(uint16_t)); }
    if (zl.launch(s)) return fail("%s: zero launch failed", who);
    return 0;
}
// the per-batch rows of the f16x2 exponent table as they are now -> the forward's stash (vsr_train_select restores from there)
static void train_stash(vsr_handle* h, TrainCtx& t, hipStream_t s) {
    if (h->measures_h2_bounds()) hipLaunchKernelGGL(k_h2_stash, dim3(1), dim3(64), 0, s, h->h2_exps, h->h2_bounds, t.h2_stash, 0);
}
// Files the forward under a new generation: from here on vsr_train_select can make it the handle's current one again
static int train_file(vsr_handle* h, TrainCtx& t, hipStream_t s) {
    t.valid = true;
    t.generation = ++h->gen_counter;
    train_stash(h, t, s);
    LAUNCHCHK();
    h->saved->v.push_back(SavedForward{h->c, t, h->ws_lo, h->ws_bytes});
    return 0;
}
// The x part of the LSTM1 / gate pre-activations of o.M rows does not depend on the recurrence: one GEMM -> dst (o.M, 6H)
static int train_xproj(vsr_handle* h, TrainCtx& t, const StepOperands& o, float* dst, hipStream_t s) {
    if (xproj_rows(h, o, SlabArea{t.scratch, t.scratch_floats}, dst, s, "train x-projection")) return 1;
    LAUNCHCHK();
    return 0;
}
// S6 of o.M rows (gathered through `rows` when given): logits = h2 . out_fc^T as slabs in t.scratch -> v (at most ns_max of them when that
// is given); the caller's head kernel (launch_vocab, k_vocab_select) sums them
static int train_vocab_gemm(vsr_handle* h, TrainCtx& t, const StepOperands& o, const int* rows, int ns_max, SlabView& v, hipStream_t s) {
    GemmBuilder g;
    add_vocab(g, h->d, h->w, o, rows);
    const int ns = g.finish(h);
    if (ns_max && ns > ns_max) return fail("train S6: the vocabulary projection's %d slabs are more than its head kernel sums (%d)", ns, ns_max);
    SlabPlan pl;
    if (place(g, o.M, vocab_slabs(h->d), {SlabArea{t.scratch, t.scratch_floats}}, pl, "train S6")) return 1;
    if (g.launch(s, h, &h->prof)) return fail("train S6 gemm launch failed");
    v = pl.v[0];
    return 0;
}
// ... and the dense head over them: whole log_softmax rows -> out (o.M, V)
static int train_vocab_full(vsr_handle* h, TrainCtx& t, const StepOperands& o, const int* rows, float* out, hipStream_t s) {
    SlabView v;
    if (train_vocab_gemm(h, t, o, rows, 0, v, s)) return 1;
    const GateLogitArgs no_gate{nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0, 0, 0, nullptr, 0};
    StepIO io;                                         // (K = 1, no gate logits)
    io.M = o.M; io.vmode = VM_FULL; io.full_out = out; io.full_stride = h->d.vocab_size;
    launch_vocab(h, s, io, v.base, v.n, v.stride, no_gate);
    LAUNCHCHK();
    return 0;
}
// K rows per image -> the "rows share an image" template flag and the K the kernel is given: f(std::bool_constant<(K > 1)>, K).  K = 1
// launches the kernels of the one-row-per-image path (the <false> instances) with 1
template <class F> static inline void with_shared_rows(int K, F&& f) {
    if (K > 1) f(std::true_type{}, K); else f(std::false_type{}, 1);
}
// Step tt's slices of the saved arrays (rows (t, b)) and of the backward's all-steps gradients: THE place that knows the layouts.
// Shared by the forward step, the tape step and the backward step.  im: the forward keeps 16-bit images of its A operands (else null)
struct StepSlices {
    float *h1o, *c1o, *h2o, *c2o;          // state entering the step (slot tt) ...
    float *h1n, *c1n, *h2n, *c2n;          // ... and leaving it (slot tt + 1)
    float *g1, *g2, *s_t, *g_t, *hA, *sa, *ga, *sent, *att, *alpha, *x, *xproj;
    int *word, *slot;
    uint16_t *h1o16, *h2o16, *h1n16, *h2n16, *s_t16, *g_t16, *att16;
    float *dh2_voc, *dpre1, *dpre2, *dhA, *dsent, *dsa, *dga, *dwa, *dws, *dwg;
};
static StepSlices train_step_slices(const vsr_handle* h, const TrainCtx& t, int tt, bool im = false) {
    const vsr_dims& d = h->d;
    const size_t B = t.B, BH = B * d.rnn_size, BA = B * d.att_size, BD = B * d.det_feat_size, BE = B * d.input_encoding_size, o = tt, n = tt + 1;
    StepSlices q;
    q.h1o = t.h1s + o * BH; q.c1o = t.c1s + o * BH; q.h2o = t.h2s + o * BH; q.c2o = t.c2s + o * BH;
    q.h1n = t.h1s + n * BH; q.c1n = t.c1s + n * BH; q.h2n = t.h2s + n * BH; q.c2n = t.c2s + n * BH;
    q.g1 = t.gates1 + o * BH * 6; q.g2 = t.gates2 + o * BH * 4; q.s_t = t.s_ts + o * BH; q.g_t = t.g_ts + o * BH;
    q.hA = t.hAs + o * BA; q.sa = t.sas + o * BA; q.ga = t.gas + o * BA;
    q.sent = t.sents + o * BD; q.att = t.atts + o * BD; q.alpha = t.alphas + o * B * (h->c.R + 1);
    q.x = t.x_all + o * BE; q.xproj = t.xproj_all + o * BH * 6;
    q.word = t.word32 + o * B; q.slot = t.slot32 + o * B;
    q.h1o16 = im ? t.h1s16 + o * BH * 2 : nullptr; q.h2o16 = im ? t.h2s16 + o * BH * 2 : nullptr;
    q.h1n16 = im ? t.h1s16 + n * BH * 2 : nullptr; q.h2n16 = im ? t.h2s16 + n * BH * 2 : nullptr;
    q.s_t16 = im ? t.s_t16 : nullptr; q.g_t16 = im ? t.g_t16 : nullptr; q.att16 = im ? t.att16 : nullptr;     // (of the current step only)
    q.dh2_voc = t.dh2_voc + o * BH; q.dpre1 = t.dpre1 + o * BH * 6; q.dpre2 = t.dpre2 + o * BH * 4;
    q.dhA = t.dhA_all + o * BA; q.dsent = t.dsent_all + o * BD; q.dsa = t.dsa_all + o * BA; q.dga = t.dga_all + o * BA;
    q.dwa = t.dwa_rows + o * BA; q.dws = t.dws_rows + o * BA; q.dwg = t.dwg_rows + o * BA;
    return q;
}
// Step tt of the unroll: state slot tt -> slot tt + 1, the step's saves, its gate log-probs into lg_out (row stride lg_stride).  The body
// of vsr_train_forward's loop over the steps; a tape (vsr_train_tape_step) takes the same step one call at a time.
static int train_forward_step(vsr_handle* h, TrainCtx& t, int K, int tt, bool im, float* lg_out, long long lg_stride, hipStream_t s) {
    Ctx& c = h->c;
    const vsr_dims& d = h->d;
    const vsr_weights& w = h->w;
    const int B = t.B, H = d.rnn_size, A = d.att_size, D = d.det_feat_size;
    const float isc = im ? 32768.f : 0.f;                  // (2^15: the exponent of the unit-bounded class)
    const int* att_exp = im ? h->h2_exps + H2A_ATT : nullptr;
    const StepSlices q = train_step_slices(h, t, tt, im);
    StepOperands o;
    o.M = B;
    o.h1_old = q.h1o; o.h2_old = q.h2o; o.h1_new = q.h1n; o.h2_new = q.h2n; o.s_t = q.s_t; o.g_t = q.g_t; o.att = q.att;
    o.h1_old16 = q.h1o16; o.h2_old16 = q.h2o16; o.h1_new16 = q.h1n16; o.h2_new16 = q.h2n16; o.s_t16 = q.s_t16; o.g_t16 = q.g_t16; o.att16 = q.att16;
    const SlabArea scratch{c.scratch, c.scratch_floats};   // (the step's launches go through the decode workspace's scratch)
    SlabPlan pl;
    {   // S1: the recurrent parts only (h2, h1 of the previous step); nothing to multiply at step 0: no launch, a view without slabs
        GemmBuilder g;
        if (tt > 0) { add_lstm1(g, d, w, o, L1_H2 | L1_H1); g.finish(h); }
        if (place(g, B, lstm1_slabs(d, g.a.nprob), {scratch}, pl, "train S1")) return 1;
        if (tt > 0 && g.launch(s, h, &h->prof)) return fail("train S1 gemm launch failed");
        const int nblk = d.h2_first_lstm ? 6 : 5;      // without h2 in the input the shift-gate block has no recurrent part
        const SlabView& v = pl.v[0];
        with_shared_rows(K, [&](auto SH, int k) {
            hipLaunchKernelGGL(k_lstm1_train<decltype(SH)::value>, dim3(cdiv((long long)B * H, 256)), dim3(256), 0, s, v.base, v.n, v.stride, c.vproj,
                               q.xproj, q.c1o, B, H, q.h1n, q.c1n, q.s_t, c.gpre, q.g1, nblk, q.h1n16, q.s_t16, isc, k);
        });
    }
    {   // S2
        GemmBuilder g;
        add_s2(g, d, w, o);
        g.finish(h);
        if (place(g, B, s2_slabs(d), {scratch}, pl, "train S2")) return 1;
        if (g.launch(s, h, &h->prof)) return fail("train S2 gemm launch failed");
        // (Round 5: k_gate2's work inside the attention kernel's row blocks, as in decoding, with the sentinel / s_a / the shift gate stored
        // on the way for the backward pass: measured at no gain - 10.99-11.06 k against 10.85-11.10 k samples/s, profiles/r05_h_* - and not kept.)
        const long long n = (long long)B * (H + A + D + A);
        const SlabView &va = pl.v[0], &vb = pl.v[1];
        hipLaunchKernelGGL(k_gate2, dim3(cdiv(n, 256)), dim3(256), 0, s, va.base, vb.base, va.n, va.stride, vb.stride, c.gpre, q.c1n, w.s_fc_bias,
                           B, H, A, D, q.g_t, q.hA, q.sent, q.sa, q.g1, q.g_t16, isc);
    }
    launch_attend(h, s, Gate2Args{}, B, K, q.slot, 0, q.hA, q.sa, q.sent, q.att, q.alpha, q.att16, att_exp);
    {   // S5
        GemmBuilder g;
        add_s5(g, d, w, o, tt > 0);
        g.finish(h);
        if (place(g, B, s5_slabs(d), {scratch}, pl, "train S5")) return 1;
        if (g.launch(s, h, &h->prof)) return fail("train S5 gemm launch failed");
        const SlabView &v = pl.v[0], &vg = pl.v[1];
        GateLogitArgs gl{vg.base, vg.n, vg.stride, q.hA, w.att_g_weight, c.zsum, nullptr, q.slot, K, c.L, B, A,
                         lg_out, lg_stride};
        gl.ga_out = q.ga;
        const int gblocks = B;
        with_shared_rows(K, [&](auto SH, int k) {
            hipLaunchKernelGGL(k_fwd_tail<decltype(SH)::value>, dim3(gblocks + cdiv((long long)B * H, 256)), dim3(256), 0, s, gl, gblocks, v.base, v.n, v.stride,
                               w.lstm2_bias_ih, w.lstm2_bias_hh, d.img_second_lstm ? c.vproj2 : nullptr, q.c2o, B, H, q.h2n, q.c2n, q.g2, q.h2n16, isc, k);
        });
    }
    LAUNCHCHK();
    return 0;
}
// K = rows per image: M = B K decoder rows, rows b K .. b K + K - 1 are image b's (the order of repeat_interleave(K, 0)).  Whatever is
// per image - the hoisted projections, P, the region rows, masks and index lists - is read through row / K, as the beams of the decode
// path do; K = 1 launches the kernels of the one-row-per-image path (the <false> instantiations).
// targets != null: the sparse head (vsr_train_forward_selected) - logp_words is then the (rows, T) tensor of the targets' log-probs
// logp_mean / entropy != null (both or neither): the sparse head with row statistics (vsr_train_forward_selected_stats)
// rows_call: one of the rows_per_image entry points, which take any K up to the prepared beam - K = 1 under a larger beam too (the replay
// of one sample per image drawn next to its greedy baseline row, vsr_sample_rows_baseline); vsr_train_forward itself asks for beam = 1
static int train_forward_impl(vsr_handle* h, int K, const int64_t* word_in, const int64_t* slots, int32_t T, float* logp_words,
                              float* logp_gates, void* train_ws, size_t train_ws_bytes, void* stream, const int64_t* targets = nullptr,
                              bool rows_call = false, float* logp_mean = nullptr, float* entropy = nullptr) {
    const char* who = entropy ? "vsr_train_forward_selected_stats" : targets ? "vsr_train_forward_selected" : "vsr_train_forward";
    if (check_ready(h, who)) return 1;
    if (!word_in || !logp_words || !logp_gates || !train_ws) return fail("%s: null tensor", who);
    Ctx& c = h->c;
    if (K == 1 && !rows_call && c.beam != 1 && c.Mmax != c.B) return fail("vsr_train_forward: prepare() must be called with beam = 1");
    if (K < 1 || K > c.beam) return fail("vsr_train_forward_rows: rows_per_image %d not in [1, the prepared beam %d] (the workspace of vsr_prepare*() is sized by the beam)", K, c.beam);
    // index-list regions (vsr_prepare_indexed) train too, with one decoder row per image (the XE / SCST batches of train.py: every
    // sample brings its own detections): the backward pass sums dP over the entries of a row that name the same bank row
    if (c.ridx && !c.rows_are_images) return fail("vsr_train_forward: index-list regions with a row -> image map (row_img) are a decode-side format; training needs one row per image (row_img = NULL)");
    if (!slots && (T < 1 || T > c.L)) return fail("vsr_train_forward: without a slot trace step t reads slot t: need 1 <= T <= L (T %d, L %d)", T, c.L);
    hipStream_t s = (hipStream_t)stream;
    const vsr_dims& d = h->d;
    const vsr_weights& w = h->w;
    const int B = c.B * K, H = d.rnn_size, E = d.input_encoding_size, V = d.vocab_size;      // (B: decoder rows)
    TrainCtx& t = *h->tc;
    t.tape_max = t.tape_steps = 0; t.sealed = false;
    t.sparse = targets != nullptr; t.consumed = false;
    if (train_begin(h, t, K, T, train_ws, train_ws_bytes, "vsr_train_forward", s)) return 1;
    t.tgt32 = t.sparse ? t.rows_bt : nullptr;
    t.ent = entropy;
    const int TB = T * B;
    const size_t BH = (size_t)B * H;
    const bool im = train_a_images(h, t);
    StepOperands all;                                     // the operands of the two launches over all T B rows (step_gemms.h)
    all.M = TB;
    // (with images: the rows are gathered from the embedding table's image by the GEMM itself)
    all.x = im ? w.embed_weight : t.x_all; all.word = im ? t.word32 : nullptr;
    all.h2_new = t.h2s; all.h2_new16 = im ? t.h2s16 : nullptr;
    hipLaunchKernelGGL(k_train_indices, dim3(cdiv(TB, 256)), dim3(256), 0, s, word_in, slots, T, B, V, c.L, t.word32, t.slot32, t.rows_bt, c.nvalid_dev + 2);
    hipLaunchKernelGGL(k_gather_rows, dim3(cdiv((long long)TB * E, 256)), dim3(256), 0, s, w.embed_weight, t.word32, TB, E, t.x_all);
    LAUNCHCHK();
    if (train_xproj(h, t, all, t.xproj_all, s)) return 1;      // every step's x part at once: M = T B

    for (int tt = 0; tt < T; ++tt)
        if (train_forward_step(h, t, K, tt, im, logp_gates + (size_t)tt * 2, (long long)T * 2, s)) return 1;
    if (t.sparse) {
        // S6 for all steps at once, sparse head: the rows in their natural (t, b) order (state slots 1 .. T: nothing to gather), then
        // k_vocab_select: the log_softmax rows stay in t.dlogits, the targets' entries go to the caller's (rows, T) tensor
        all.h2_new = t.h2s + BH; all.h2_new16 = im ? t.h2s16 + BH * 2 : nullptr;
        SlabView v;
        if (train_vocab_gemm(h, t, all, nullptr, GEMM_MAX_SLABS, v, s)) return 1;        // (k_vocab_select sums at most that many slabs: slab_sum)
        const int lds_row = V <= VOCAB_LDS_MAX ? 1 : 0;
        const size_t vsm = lds_row ? (size_t)V * sizeof(float) : 0;
        const int Vp = (int)up4(V);
        auto select = [&](auto NT, auto ST) {              // the instance: threads per row, with / without the row statistics
            constexpr int nt = decltype(NT)::value;
            hipLaunchKernelGGL((k_vocab_select<nt, decltype(ST)::value>), dim3(TB), dim3(nt), vsm, s, v.base, v.n, v.stride, w.out_fc_bias, B, T, V, Vp,
                               lds_row, targets, t.dlogits, logp_words, t.tgt32, c.nvalid_dev + 2, logp_mean, entropy);
        };
        using N512 = std::integral_constant<int, 512>; using N256 = std::integral_constant<int, 256>;
        if (V >= 4096) { if (entropy) select(N512{}, std::true_type{}); else select(N512{}, std::false_type{}); }
        else           { if (entropy) select(N256{}, std::true_type{}); else select(N256{}, std::false_type{}); }
        LAUNCHCHK();
    } else {   // S6 for all steps at once: logits = h2[(b, t)] . out_fc^T (M = T B rows gathered in (b, t) order, so that the
        // (B, T, V) log-prob tensor is written row by row), then one log_softmax launch
        if (train_vocab_full(h, t, all, t.rows_bt, logp_words, s)) return 1;
    }
    t.logp_w = t.sparse ? nullptr : logp_words;
    t.logp_g = logp_gates;
    return train_file(h, t, s);
}
extern "C" int vsr_train_forward(vsr_handle* h, const int64_t* word_in, const int64_t* slots, int32_t T, float* logp_words,
                                 float* logp_gates, void* train_ws, size_t train_ws_bytes, void* stream) {
    return train_forward_impl(h, 1, word_in, slots, T, logp_words, logp_gates, train_ws, train_ws_bytes, stream);
}
extern "C" int vsr_train_forward_rows(vsr_handle* h, int32_t rows_per_image, const int64_t* word_in, const int64_t* slots, int32_t T,
                                      float* logp_words, float* logp_gates, void* train_ws, size_t train_ws_bytes, void* stream) {
    if (rows_per_image < 1 || rows_per_image > VSR_MAX_BEAM) return fail("vsr_train_forward_rows: rows_per_image %d not in [1, %d]", rows_per_image, VSR_MAX_BEAM);
    return train_forward_impl(h, rows_per_image, word_in, slots, T, logp_words, logp_gates, train_ws, train_ws_bytes, stream, nullptr, true);
}
// The sparse head: targets (rows, T) int64 (a word id, or -1 = not selected) -> logp_sel (rows, T); the gate head stays dense
extern "C" int vsr_train_forward_selected(vsr_handle* h, int32_t rows_per_image, const int64_t* word_in, const int64_t* slots,
                                          const int64_t* targets, int32_t T, float* logp_sel, float* logp_gates, void* train_ws,
                                          size_t train_ws_bytes, void* stream) {
    if (rows_per_image < 1 || rows_per_image > VSR_MAX_BEAM) return fail("vsr_train_forward_selected: rows_per_image %d not in [1, %d]", rows_per_image, VSR_MAX_BEAM);
    if (!targets) return fail("vsr_train_forward_selected: null targets (the dense head is vsr_train_forward / vsr_train_forward_rows)");
    return train_forward_impl(h, rows_per_image, word_in, slots, T, logp_sel, logp_gates, train_ws, train_ws_bytes, stream, targets, true);
}
// ... plus the row statistics of every (row, step): logp_mean, entropy (rows, T); entropy is held until the backward like logp_gates
extern "C" int vsr_train_forward_selected_stats(vsr_handle* h, int32_t rows_per_image, const int64_t* word_in, const int64_t* slots,
                                                const int64_t* targets, int32_t T, float* logp_sel, float* logp_mean, float* entropy,
                                                float* logp_gates, void* train_ws, size_t train_ws_bytes, void* stream) {
    if (rows_per_image < 1 || rows_per_image > VSR_MAX_BEAM) return fail("vsr_train_forward_selected_stats: rows_per_image %d not in [1, %d]", rows_per_image, VSR_MAX_BEAM);
    if (!targets) return fail("vsr_train_forward_selected_stats: null targets (the dense head is vsr_train_forward / vsr_train_forward_rows)");
    if (!logp_mean || !entropy) return fail("vsr_train_forward_selected_stats: null tensor");
    return train_forward_impl(h, rows_per_image, word_in, slots, T, logp_sel, logp_gates, train_ws, train_ws_bytes, stream, targets, true, logp_mean, entropy);
}

// ---------------------------------------------------------------------------------------------- tape: the forward, one step per call
// ControllableCaptioningModel.step under autograd (controllable_captioning.py:117-190) is the unroll of CaptioningModel.forward (:22-36)
// taken by the caller one step at a time.  A tape is that unroll saved as a training forward: begin carves the workspace for max_steps and
// files a forward of 0 steps, every step appends what train_forward_step saves for it, seal sets T to the steps taken and points the
// saved forward at the caller's stacked (B, T, .) log-probs.  vsr_train_select / vsr_train_backward then see an ordinary forward.
// One row per image (K = 1), zero initial state.

// the (b, t)-ordered list of the saved state rows for the T steps taken (what k_train_indices lays out for a whole forward)
__global__ void k_tape_rows_bt(int T, int B, int* __restrict__ rows_bt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * B) return;
    const int tt = i / B, b = i - tt * B;
    rows_bt[b * T + tt] = (tt + 1) * B + b;
}

// makes the tape of `generation` the handle's current forward (as vsr_train_select does for a backward) and checks that it is one
static int tape_current(vsr_handle* h, int64_t generation, const char* who, void* stream) {
    if (!h || !h->tc) return fail("%s: null handle", who);
    if (!h->bound) return fail("%s: weights not bound", who);
    if (vsr_train_select(h, generation, stream)) return 1;         // (fails when the tape's buffers were handed out again)
    if (!h->tc->tape_max) return fail("%s: generation %lld is a whole forward, not a tape", who, (long long)generation);
    return 0;
}
static void tape_refile(vsr_handle* h, const TrainCtx& t) {
    for (SavedForward& sf : h->saved->v)
        if (sf.t.generation == t.generation) sf.t = t;
}

extern "C" int vsr_train_tape_begin(vsr_handle* h, int32_t max_steps, void* train_ws, size_t train_ws_bytes, void* stream) {
    if (check_ready(h, "vsr_train_tape_begin")) return 1;
    if (!train_ws) return fail("vsr_train_tape_begin: null workspace");
    Ctx& c = h->c;
    if (c.beam != 1 && c.Mmax != c.B) return fail("vsr_train_tape_begin: prepare() must be called with beam = 1 (a tape has one row per image)");
    if (c.ridx && !c.rows_are_images) return fail("vsr_train_tape_begin: index-list regions with a row -> image map (row_img) are a decode-side format; training needs one row per image (row_img = NULL)");
    if (max_steps < 1 || max_steps > h->d.seq_len) return fail("vsr_train_tape_begin: max_steps %d not in [1, seq_len %d]", max_steps, h->d.seq_len);
    hipStream_t s = (hipStream_t)stream;
    TrainCtx& t = *h->tc;
    if (train_begin(h, t, 1, max_steps, train_ws, train_ws_bytes, "vsr_train_tape_begin", s)) return 1;
    t.tape_max = max_steps; t.tape_steps = 0; t.sealed = false;
    t.sparse = t.consumed = false; t.tgt32 = nullptr; t.ent = nullptr;
    t.logp_w = t.logp_g = nullptr;
    // (filed - and the exponent rows stashed - now, not only at the seal: a vsr_prepare*() of another batch may come between two steps,
    // and vsr_train_select restores from here)
    return train_file(h, t, s);
}

extern "C" int vsr_train_tape_step(vsr_handle* h, int64_t generation, const int64_t* word_in, const int64_t* slots, float* logp_words,
                                   float* logp_gates, float* h1_out, float* c1_out, float* h2_out, float* c2_out, void* stream) {
    if (tape_current(h, generation, "vsr_train_tape_step", stream)) return 1;
    if (!word_in || !slots || !logp_words || !logp_gates || !h1_out || !c1_out || !h2_out || !c2_out) return fail("vsr_train_tape_step: null tensor");
    TrainCtx& t = *h->tc;
    if (t.sealed) return fail("vsr_train_tape_step: the tape of generation %lld has been sealed", (long long)generation);
    if (t.tape_steps >= t.tape_max) return fail("vsr_train_tape_step: the tape already holds the %d steps it was begun for", t.tape_max);
    hipStream_t s = (hipStream_t)stream;
    Ctx& c = h->c;
    const vsr_dims& d = h->d;
    const vsr_weights& w = h->w;
    const int B = t.B, H = d.rnn_size, E = d.input_encoding_size, V = d.vocab_size, tt = t.tape_steps;
    const size_t BH = (size_t)B * H;
    const bool im = train_a_images(h, t);
    const StepSlices q = train_step_slices(h, t, tt, im);  // (x: the weight-gradient phase reads the rows of every step)
    // (T = 1, no row list: the step's (B) ids -> the step's rows of the (T, B) int32 copies, counted and clamped as for a whole forward)
    hipLaunchKernelGGL(k_train_indices, dim3(cdiv(B, 256)), dim3(256), 0, s, word_in, slots, 1, B, V, c.L, q.word, q.slot, (int*)nullptr, c.nvalid_dev + 2);
    hipLaunchKernelGGL(k_gather_rows, dim3(cdiv((long long)B * E, 256)), dim3(256), 0, s, w.embed_weight, q.word, B, E, q.x);
    LAUNCHCHK();
    StepOperands o;                                        // this step's M = B rows of the two launches a whole forward makes over all T B
    o.M = B;
    o.x = im ? w.embed_weight : q.x; o.word = im ? q.word : nullptr;
    o.h2_new = q.h2n; o.h2_new16 = q.h2n16;
    if (train_xproj(h, t, o, q.xproj, s)) return 1;
    if (train_forward_step(h, t, 1, tt, im, logp_gates, 2, s)) return 1;
    if (train_vocab_full(h, t, o, nullptr, logp_words, s)) return 1;      // the new h2 (state slot tt + 1) -> the caller's (B, V) log-probs
    const float* src[4] = {t.h1s, t.c1s, t.h2s, t.c2s};
    float* dst[4] = {h1_out, c1_out, h2_out, c2_out};
    for (int j = 0; j < 4; ++j) HIPCHK(hipMemcpyAsync(dst[j], src[j] + (size_t)(tt + 1) * BH, BH * sizeof(float), hipMemcpyDeviceToDevice, s));
    t.tape_steps = tt + 1;
    tape_refile(h, t);
    return 0;
}

extern "C" int vsr_train_tape_seal(vsr_handle* h, int64_t generation, const float* logp_words, const float* logp_gates, void* stream) {
    if (tape_current(h, generation, "vsr_train_tape_seal", stream)) return 1;
    if (!logp_words || !logp_gates) return fail("vsr_train_tape_seal: null tensor");
    TrainCtx& t = *h->tc;
    if (t.tape_steps < 1) return fail("vsr_train_tape_seal: the tape holds no step");
    hipStream_t s = (hipStream_t)stream;
    const int T = t.tape_steps, TB = T * t.B;
    t.T = T; t.TB = TB; t.TBp = (int)up4((size_t)TB);       // (<= what the workspace was carved for: tape_steps <= tape_max)
    hipLaunchKernelGGL(k_tape_rows_bt, dim3(cdiv(TB, 256)), dim3(256), 0, s, T, t.B, t.rows_bt);
    t.logp_w = logp_words;
    t.logp_g = logp_gates;
    t.sealed = true;
    train_stash(h, t, s);
    LAUNCHCHK();
    tape_refile(h, t);
    return 0;
}

// Identity of the saved forward pass (0 = none).  The training workspace holds ONE forward at a time: a caller that keeps
// several autograd nodes alive compares the value it got after its forward with the current one before differentiating.
extern "C" int64_t vsr_train_generation(const vsr_handle* h) { return (h && h->tc && h->tc->valid) ? (int64_t)h->tc->generation : 0; }

// dlogits in (t, b) row order from the (B, T, V) tensors
__global__ __launch_bounds__(256) void k_dlogits_tb(const float* __restrict__ logp, const float* __restrict__ dlogp, int B, int T, int V,
                                                    int Vp, float* __restrict__ dlogits, int* bm) {
    __shared__ float red[4];
    const int tt = blockIdx.x / B, b = blockIdx.x % B;
    const long long src = ((long long)b * T + tt) * V, dst = (long long)blockIdx.x * Vp;
    const int tid = threadIdx.x;
    // 16 bytes per lane where the rows allow it (V a multiple of 4: every row of the (B, T, V) tensors starts 16-byte aligned)
    const bool vec = (V & 3) == 0 && (Vp & 3) == 0 && ((reinterpret_cast<uintptr_t>(logp) | reinterpret_cast<uintptr_t>(dlogp) | reinterpret_cast<uintptr_t>(dlogits)) & 15) == 0;
    float s = 0.f;
    if (vec) {
        for (int v = tid * 4; v < V; v += 1024) {
            const float4 g = *reinterpret_cast<const float4*>(dlogp + src + v);
            s += (g.x + g.y) + (g.z + g.w);
        }
    } else {
        for (int v = tid; v < V; v += 256) s += dlogp[src + v];
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const float tot = (red[0] + red[1]) + (red[2] + red[3]);
    float mx = 0.f;
    if (vec) {
        for (int v = tid * 4; v < Vp; v += 1024) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (v < V) {
                const float4 g = *reinterpret_cast<const float4*>(dlogp + src + v), l = *reinterpret_cast<const float4*>(logp + src + v);
                o = make_float4(g.x - expf(l.x) * tot, g.y - expf(l.y) * tot, g.z - expf(l.z) * tot, g.w - expf(l.w) * tot);
            }
            *reinterpret_cast<float4*>(dlogits + dst + v) = o;
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
        }
    } else {
        for (int v = tid; v < Vp; v += 256) {
            const float o = v < V ? dlogp[src + v] - expf(logp[src + v]) * tot : 0.f;
            dlogits[dst + v] = o;
            mx = fmaxf(mx, fabsf(o));
        }
    }
    if (bm) block_absmax_to(mx, bm);
}

__global__ void k_sum_over_t(const float* __restrict__ X, int T, long long per_t, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_t) return;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += X[t * per_t + i];
    out[i] = s;
}

// several rows per image: out[image] = sum over the image's K rows, in ascending row order, of each row's sum over t (X: (T, M, C))
__global__ void k_sum_over_t_rows(const float* __restrict__ X, int T, int K, int C, long long per_t, long long n_out, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const long long img = i / C, col = i % C;
    float s = 0.f;
    for (int j = 0; j < K; ++j)
        for (int t = 0; t < T; ++t) s += X[t * per_t + (img * K + j) * C + col];
    out[i] = s;
}

// ---------------------------------------------------------------------------------------------- backward
// the 28 gradients, in the field order of vsr_weights
enum { g_embed, g_Wis, g_bis, g_Whs, g_bhs, g_Wva, g_Wha, g_wa, g_Wsa, g_ws, g_Wih1, g_Whh1, g_bih1, g_bhh1, g_Wih2, g_Whh2, g_bih2,
       g_bhh2, g_Wout, g_bout, g_Wsfc, g_bsfc, g_Wig, g_big, g_Whg, g_bhg, g_Wga, g_wg, N_GRADS };
static_assert(N_GRADS * sizeof(float*) == sizeof(vsr_weights), "one gradient per field of vsr_weights");

// One row of THE table of the weight gradients (train_grad_table): what produces a gradient (or one column window of it) and in which
// bucket.  Phase B of the backward walks the rows in order and records a bucket's event where the walk leaves the bucket;
// vsr_train_bucket_map reads the buckets off the same rows.  Adding a gradient, or moving one to another bucket, is an edit of its rows.
struct GradRow {
    enum Kind { PROD, COLSUM, EMBED };
    enum { ALONE = -1 };
    enum Pre { PRE_NONE, PRE_DPRE2SUM, PRE_VA };
    int kind, g, bucket;
    bool on;                   // the configuration has this row (the bucket map counts it either way)
    // PROD: G[g] + col (leading dimension ldd) = rows [r0, r0 + M) of the transposed gradient `ty` x the transposed activation `tx`
    // (train_operands entries: K = their padded row count, N = tx's columns, exponent slot and image-in-place of A = ty's)
    int ty, r0, M, tx, col, ldd;
    int slot;                  // the dynamic slot of these rows where ty is NOT one image of one bound (-1: ty's own)
    int launch;                // adjacent products with the same id share a run_products launch; ALONE: one of its own.  Which products share a
                               // launch decides tiles and slabs, i.e. the bits
    int pre;                   // code that stays code, run before the product: the sum over t and its transpose (PRE_DPRE2SUM); a memset
                               // INSTEAD of the product when no region row is valid (PRE_VA)
    // COLSUM: G[g] (and G[g2], the second bias of a pair; -1: none) = the sums of columns [c0, c0 + n) of src (T B rows, C columns,
    // leading dimension ld).  Adjacent rows of one src share the partial-sum launch
    int g2, ld, C, c0, n;
    float* TrainCtx::* src;
    // EMBED: the data-gradient GEMM dx, a memset and k_embed_grad_rows - code in the walk
};
// The rows, in the order phase B issues them.  Reads only the sizes and the two flags of `d`: buckets and order do not depend on them.
static std::vector<GradRow> train_grad_table(const vsr_dims& d) {
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size, E = d.input_encoding_size, V = d.vocab_size, Vp = (int)up4((size_t)V);
    const bool h2in = d.h2_first_lstm, img2 = d.img_second_lstm;
    const int voff = h2in ? H : 0, xoff = voff + D, in1 = xoff + E, in2 = H + D + (img2 ? D : 0);
    const int ALONE = GradRow::ALONE;
    std::vector<GradRow> v;
    v.reserve(40);
    int b = 0;
    auto prod = [&](int g, int col, int ldd, int ty, int r0, int M, int tx, int launch, int slot = -1, bool on = true, int pre = GradRow::PRE_NONE) {
        GradRow r{};
        r.kind = GradRow::PROD; r.g = g; r.g2 = -1; r.bucket = b; r.on = on;
        r.ty = ty; r.r0 = r0; r.M = M; r.tx = tx; r.col = col; r.ldd = ldd; r.slot = slot; r.launch = launch; r.pre = pre;
        v.push_back(r);
    };
    auto bias = [&](int g, int g2, float* TrainCtx::* src, int ld, int C, int c0, int n) {
        GradRow r{};
        r.kind = GradRow::COLSUM; r.g = g; r.g2 = g2; r.bucket = b; r.on = true; r.src = src; r.ld = ld; r.C = C; r.c0 = c0; r.n = n;
        v.push_back(r);
    };
    // dpre1's column blocks [LSTM1 gates | sentinel gate] and [dq] have bounds of their own where its transpose is not one image
    const int sP1 = DW_step + DY_dpre1, sQ = DW_step + DY_dq;
    // ---- bucket 0: lstm_cell_1.weight_ih / W1_is / W1_ig: row blocks [0,4H), [4H,5H), [5H,6H) of dpre1^T against [h2_prev | vbar | x].
    // (grouped launches, round 6: the two 4H-row products are 256 whole tiles together, the four H-row ones share a launch - without the
    // h2 columns the three x parts share one; the three short-K image-constant parts share one)
    b = 0;
    const int gi[3] = {g_Wih1, g_Wis, g_Wig}, r0[3] = {0, 4 * H, 5 * H}, nr[3] = {4 * H, H, H}, sl[3] = {sP1, sP1, sQ};
    for (int i = 0; i < 3; ++i) {
        const int l = h2in && i > 0 ? 1 : 0;
        prod(gi[i], 0, in1, TY_dpre1, r0[i], nr[i], TX_h2prev, l, sl[i], h2in);
        prod(gi[i], xoff, in1, TY_dpre1, r0[i], nr[i], TX_x, l, sl[i]);
    }
    for (int i = 0; i < 3; ++i) prod(gi[i], voff, in1, TY_dpre1sum, r0[i], nr[i], TX_vbar, 2);
    // ---- bucket 1: lstm_cell_2 (the attended-vector part is 256 whole tiles on its own; the h1 part and weight_hh are 256 together)
    b = 1;
    prod(g_Wih2, 0, in2, TY_dpre2, 0, 4 * H, TX_h1, 0);
    prod(g_Whh2, 0, H, TY_dpre2, 0, 4 * H, TX_h2prev, 0);
    prod(g_Wih2, H, in2, TY_dpre2, 0, 4 * H, TX_att, ALONE);
    prod(g_Wih2, H + D, in2, TY_dpre2sum, 0, 4 * H, TX_vbar, ALONE, -1, img2, GradRow::PRE_DPRE2SUM);
    bias(g_bih2, g_bhh2, &TrainCtx::dpre2, 4 * H, 4 * H, 0, 4 * H);
    // ---- bucket 2: out_fc and the embedding
    b = 2;
    prod(g_Wout, 0, H, TY_dlogits, 0, V, TX_h2, ALONE);
    bias(g_bout, -1, &TrainCtx::dlogits, Vp, V, 0, V);
    { GradRow r{}; r.kind = GradRow::EMBED; r.g = g_embed; r.g2 = -1; r.bucket = b; r.on = true; v.push_back(r); }
    // ---- bucket 3: the recurrent LSTM1 / sentinel-gate weights, all LSTM1 / gate biases, s_fc, att_va
    b = 3;
    prod(g_Whh1, 0, H, TY_dpre1, 0, 4 * H, TX_h1prev, 0, sP1);           // (with W1_hs and s_fc: 224 whole tiles in one launch)
    prod(g_Whs, 0, H, TY_dpre1, 4 * H, H, TX_h1prev, 0, sP1);
    prod(g_Wsfc, 0, H, TY_dsent, 0, D, TX_st, 0);
    // the six LSTM1 / gate bias gradients are column sums of ONE matrix (dpre1, 6H columns): one partial-sum launch, three finishing launches
    // that write both members of a pair (same per-column arithmetic as three separate sums: bit-identical)
    bias(g_bih1, g_bhh1, &TrainCtx::dpre1, 6 * H, 6 * H, 0, 4 * H);
    bias(g_bis, g_bhs, &TrainCtx::dpre1, 6 * H, 6 * H, 4 * H, H);
    bias(g_big, g_bhg, &TrainCtx::dpre1, 6 * H, 6 * H, 5 * H, H);
    bias(g_bsfc, -1, &TrainCtx::dsent_all, D, D, 0, D);
    prod(g_Wva, 0, D, TY_dP, 0, A, TX_reg, ALONE, -1, true, GradRow::PRE_VA);      // dP^T (A, NV) x regions^T (D, NV) over the non-padding rows
    // ---- bucket 4 (the tail, 3.5 M floats): W1_hg, att_ha, att_sa, att_ga and the three score vectors
    b = 4;
    prod(g_Whg, 0, H, TY_dpre1, 5 * H, H, TX_h1, 0, sQ);
    prod(g_Wha, 0, H, TY_dhA, 0, A, TX_h1, 0);
    prod(g_Wsa, 0, H, TY_dsa, 0, A, TX_st, 0);
    prod(g_Wga, 0, H, TY_dga, 0, A, TX_gt, 0);
    bias(g_wa, -1, &TrainCtx::dwa_rows, A, A, 0, A);
    bias(g_ws, -1, &TrainCtx::dws_rows, A, A, 0, A);
    bias(g_wg, -1, &TrainCtx::dwg_rows, A, A, 0, A);
    return v;
}

// out (images, C) = the sum over t - and over an image's K rows, ascending - of X (T, B, C)
static void sum_over_t(hipStream_t s, const float* X, int T, int K, int B, int C, float* out) {
    const long long per_t = (long long)B * C, n_out = per_t / K;
    if (K > 1) hipLaunchKernelGGL(k_sum_over_t_rows, dim3(cdiv(n_out, 256)), dim3(256), 0, s, X, T, K, C, per_t, n_out, out);
    else hipLaunchKernelGGL(k_sum_over_t, dim3(cdiv(per_t, 256)), dim3(256), 0, s, X, T, per_t, out);
}

// What the steps of one backward pass share
struct BwdPass {
    const float* dlg = nullptr;    // the gradient of the gate log-probs (B, T, 2)
    int* dyn = nullptr;            // the dynamic slots of the exponent table when the pass runs on the f16x2 kernels, else null
    int cb = 0;                    // which of the two cell-carry buffers holds the carries of step tt + 1
    SlabView dh1_3{}, dh2_3{};     // slabs of the later step's GEMM 3 waiting in t.scratch (consumed by k_bwd_head; bwd_gemm3)
    int slot(int i) const { return dyn ? H2_DYN0 + i : (int)H2A_NONE; }
    int* ptr(int i) const { return dyn ? dyn + i : nullptr; }
};
// GEMM 3 of a step (o = null: none - step 0, and before the first step) and where its slabs wait in t.scratch for the NEXT step's k_bwd_head
static int bwd_gemm3(vsr_handle* h, TrainCtx& t, const BwdStepOperands* o, BwdPass& p, hipStream_t s) {
    GemmBuilder g;
    if (o) { add_bwd3(g, h->d, *o); g.finish(h); }
    SlabPlan pl;
    if (place(g, t.B, bwd3_slabs(h->d, g.a.nprob), {SlabArea{t.scratch, t.scratch_floats}}, pl, "bwd gemm 3")) return 1;
    p.dh1_3 = pl.v[0]; p.dh2_3 = pl.v[1];
    if (o && g.launch(s, h, &h->prof)) return fail("bwd gemm 3 launch failed");
    return 0;
}
// Step tt of the reverse-time loop: k_bwd_head, GEMM 1, k_bwd_mid, k_dalpha, k_attend_bwd, GEMM 2, k_bwd_tail, GEMM 3 (data gradients
// only; the GEMMs' problem lists are step_gemms.h's).  Mirrors train_forward_step.
static int train_backward_step(vsr_handle* h, TrainCtx& t, int tt, BwdPass& p, hipStream_t s) {
    Ctx& c = h->c;
    const vsr_dims& d = h->d;
    const vsr_weights& w = h->w;
    const int B = t.B, T = t.T, K = t.rpi, Bi = B / K, H = d.rnn_size, A = d.att_size, D = d.det_feat_size, R1 = c.R + 1, cb = p.cb;
    const size_t BH = (size_t)B * H;
    const SlabArea scratch{t.scratch, t.scratch_floats};
    SlabPlan pl;
    const StepSlices q = train_step_slices(h, t, tt);
    const int y = tt * DYN_PER_STEP;                   // the step's block of dynamic slots
    BwdStepOperands o;
    o.M = B;
    o.dpre1 = q.dpre1; o.dpre2 = q.dpre2; o.dhA = q.dhA; o.dsent = q.dsent; o.dsa = q.dsa; o.dga = q.dga;
    o.wT_ih1 = t.wT_ih1; o.wT_is = t.wT_is; o.wT_ig = t.wT_ig; o.wT_hh1 = t.wT_hh1; o.wT_hs = t.wT_hs; o.wT_ih2 = t.wT_ih2; o.wT_hh2 = t.wT_hh2;
    o.wT_hg = t.wT_hg; o.wT_ha = t.wT_ha; o.wT_sfc = t.wT_sfc; o.wT_sa = t.wT_sa; o.wT_ga = t.wT_ga;
    o.s_dpre1 = p.slot(y + DY_dpre1); o.s_dpre2 = p.slot(y + DY_dpre2); o.s_dq = p.slot(y + DY_dq); o.s_dhA = p.slot(y + DY_dhA);
    o.s_dsent = p.slot(y + DY_dsent); o.s_dsa = p.slot(y + DY_dsa); o.s_dga = p.slot(y + DY_dga);
    {   // gate log-probs -> dga, dhA (first writer), dzsum;  carries of step tt + 1 + vocabulary part -> LSTM2 backward
        BwdHeadArgs a;
        a.lg = t.logp_g + (size_t)tt * 2; a.dlg = p.dlg + (size_t)tt * 2; a.lg_stride = (long long)T * 2;
        a.ga = q.ga; a.hA = q.hA; a.w_g = w.att_g_weight; a.A = A;
        a.dga = q.dga; a.dhA = q.dhA; a.dzsum = t.dzsum; a.dwg_rows = q.dwg; a.gblocks = B;
        a.s_h1 = p.dh1_3.base; a.s_h2 = d.h2_first_lstm ? p.dh2_3.base : nullptr; a.nslab3 = p.dh1_3.n; a.stride3 = p.dh1_3.stride;
        a.dh1_c = t.dh1_c; a.dh2_c = t.dh2_c; a.dh2_voc = q.dh2_voc;
        a.dc_next = t.dc2_c[cb]; a.gates2 = q.g2; a.c2 = q.c2n; a.c2_prev = tt > 0 ? q.c2o : nullptr;
        a.M = B; a.H = H; a.dpre2 = q.dpre2; a.dc_prev = t.dc2_c[cb ^ 1];
        a.bm_dga = p.ptr(y + DY_dga); a.bm_dpre2 = p.ptr(y + DY_dpre2);
        hipLaunchKernelGGL(k_bwd_head, dim3(a.gblocks + cdiv((long long)BH, 256)), dim3(256), 0, s, a);
    }
    {   // grouped GEMM 1: dpre2 -> [dh1_a | datt (| dvbar)] , dh2 carry (hh part);  dga -> dg_t
        GemmBuilder g;
        add_bwd1(g, d, o);
        g.finish(h);
        if (place(g, B, bwd1_slabs(d), {scratch}, pl, "bwd gemm 1")) return 1;
        if (g.launch(s, h, &h->prof)) return fail("bwd gemm 1 launch failed");
        BwdMidArgs a;
        a.nslab = pl.v[0].n; a.st0 = pl.v[0].stride; a.st1 = pl.v[1].stride; a.st2 = pl.v[2].stride;
        // datt; dg_t -> shift-gate backward (dq into dpre1[:, 5H:6H], dtc); dh1 so far (= dh1_a + carry, into dh_tot) and the
        // hh part of the new dh2 carry (the LSTM1-input part is added by the next k_bwd_head from GEMM 3's slabs)
        a.C0 = pl.v[0].base; a.C1 = pl.v[1].base; a.C2 = pl.v[2].base; a.M = B; a.H = H; a.D = D;
        a.datt = t.datt; a.dh1_c = t.dh1_c; a.dh_tot = t.dh_tot; a.dh2_c = t.dh2_c;
        a.gates1 = q.g1; a.c1 = q.c1n; a.dq = q.dpre1 + 5 * H; a.dtc = t.dtc; a.bm_dq = p.ptr(y + DY_dq);
        const int wmax = D > H ? D : H;
        hipLaunchKernelGGL(k_bwd_mid, dim3(cdiv((long long)B * wmax, 256), 3), dim3(256), 0, s, a);
    }
    {   // attention
        with_shared_rows(K, [&](auto SH, int k) {
            hipLaunchKernelGGL(k_dalpha<decltype(SH)::value>, dim3(cdiv((long long)B * R1, 4)), dim3(256), 0, s, t.datt, q.sent, c.regions, c.rmask, c.ridx, q.slot, B, c.L, c.R, D,
                               t.dalpha, k);
        });
        // two workgroups per row in launches of <= 128 rows (as k_attend): half the A columns each, its 512 threads = 256 columns x 2 row groups
        const int NTb = A >= 512 ? 512 : 256;
        const int np = attend_bwd_parts(h, B, NTb);
        const int RG = np > 1 ? NTb / (A / np) : 1;
        const size_t smem = (size_t)(R1 + 8 + (np > 1 ? (RG - 1) * (A / np) * 2 : 0)) * sizeof(float);
        // K > 1: rows of an image may name the same slot: each row writes its (R, A) block, the blocks are added onto dP in row order
        with_shared_rows(K, [&](auto SH, int) {
            constexpr bool sh = decltype(SH)::value;
            auto go = [&](auto NT) {
                constexpr int nt = decltype(NT)::value;
                hipLaunchKernelGGL((k_attend_bwd<nt, sh>), dim3(cdiv(B * np, 8) * 8), dim3(nt), smem, s, t.datt, t.dalpha, t.dzsum, q.alpha, q.hA, q.sa, q.sent, c.P, c.regions, c.rmask, c.ridx,
                                   q.slot, 0, B, c.L, c.R, A, D, w.att_a_weight, w.att_s_weight, q.dsent, q.dsa, q.dhA, sh ? t.dP_rows : t.dP, q.dwa, q.dws,
                                   p.ptr(y + DY_dhA), p.ptr(y + DY_dsent), p.ptr(y + DY_dsa), np, K);
            };
            if (A >= 512) go(std::integral_constant<int, 512>{}); else go(std::integral_constant<int, 256>{});
        });
        if (K > 1) hipLaunchKernelGGL(k_dP_rows_sum, dim3(cdiv((long long)Bi * c.R * (A / 4), 256)), dim3(256), 0, s, t.dP_rows, q.slot, c.rmask, Bi, K, c.L, c.R, A, t.dP);
    }
    {   // grouped GEMM 2: [dq | dhA] -> dh1_b ; [dsent | dsa] -> ds_t;  then the sentinel gate and LSTM1 pointwise backward
        GemmBuilder g;
        add_bwd2(g, d, o);
        g.finish(h);
        if (place(g, B, bwd2_slabs(d), {scratch}, pl, "bwd gemm 2")) return 1;
        if (g.launch(s, h, &h->prof)) return fail("bwd gemm 2 launch failed");
        hipLaunchKernelGGL(k_bwd_tail, dim3(cdiv((long long)BH, 256)), dim3(256), 0, s, pl.v[0].base, pl.v[1].base, pl.v[0].n, pl.v[0].stride, t.dh_tot, t.dtc, t.dc1_c[cb], q.g1, q.c1n,
                           tt > 0 ? q.c1o : (float*)nullptr, B, H, q.dpre1, t.dc1_c[cb ^ 1], p.ptr(y + DY_dpre1));
    }
    // grouped GEMM 3: dpre1 -> dh1 carry, dh2 carry (LSTM1 input part); its slabs stay in t.scratch for the next k_bwd_head
    if (bwd_gemm3(h, t, tt > 0 ? &o : nullptr, p, s)) return 1;
    LAUNCHCHK();
    return 0;
}
// sel: vsr_train_backward_selected - grad_logp_words is then the (rows, T) gradient of the targets' log-probs
// stats_call: vsr_train_backward_selected_stats - grad_mean / grad_ent (rows, T) are the gradients of the row statistics, either may be null
// (= zero); with both null the pass is vsr_train_backward_selected's, kernel instance included
static int train_backward_impl(vsr_handle* h, bool sel, const float* grad_logp_words, const float* grad_logp_gates, const vsr_weights* grads,
                               void* stream, bool stats_call = false, const float* grad_mean = nullptr, const float* grad_ent = nullptr) {
    const char* who = stats_call ? "vsr_train_backward_selected_stats" : sel ? "vsr_train_backward_selected" : "vsr_train_backward";
    if (check_ready(h, who)) return 1;
    TrainCtx& t = *h->tc;
    if (!t.valid) return fail("%s: no saved forward (call vsr_train_forward%s first)", who, sel ? "_selected" : "");
    if (sel && t.tape_max) return fail("vsr_train_backward_selected: the current forward is a tape (a manual step() loop keeps the dense head): call vsr_train_backward");
    if (t.tape_max && !t.sealed) return fail("vsr_train_backward: the current forward is a tape of %d steps that has not been sealed (vsr_train_tape_seal)", t.tape_steps);
    if (sel && !t.sparse) return fail("vsr_train_backward_selected: the current forward was taken by vsr_train_forward / vsr_train_forward_rows (dense head, a (B,T,V) "
                                      "log-prob tensor): call vsr_train_backward with the dense gradient");
    if (!sel && t.sparse) return fail("vsr_train_backward: the current forward was taken by vsr_train_forward_selected (sparse head: no (B,T,V) log-prob tensor "
                                      "exists): call vsr_train_backward_selected with the (rows, T) gradient");
    if (t.sparse && t.consumed) return fail("vsr_train_backward_selected: the forward of generation %lld has already been differentiated and is consumed - the "
                                            "backward of the sparse head turns the saved log-prob rows into their gradient in place, so a second backward "
                                            "needs a new vsr_train_forward_selected", (long long)t.generation);
    if ((grad_mean || grad_ent) && !t.ent) return fail("vsr_train_backward_selected_stats: a gradient of logp_mean / entropy was given, but the current forward was taken by "
                                                       "vsr_train_forward_selected (no row statistics were computed): take it with vsr_train_forward_selected_stats");
    if (!grad_logp_words || !grad_logp_gates || !grads) return fail("%s: null tensor", who);
    hipStream_t s = (hipStream_t)stream;
    const vsr_dims& d = h->d;
    Ctx& c = h->c;
    const int B = t.B, T = t.T, TB = t.TB, TBp = t.TBp;           // (B: decoder rows)
    const int K = t.rpi;                                          // rows per image of the saved forward
    const int H = d.rnn_size, A = d.att_size, D = d.det_feat_size, E = d.input_encoding_size, V = d.vocab_size;
    const int RL = c.B * c.L * c.R;
    const size_t BH = (size_t)B * H;
    float* const* G = reinterpret_cast<float* const*>(grads);     // same field order as vsr_weights
    for (int i = 0; i < N_GRADS; ++i)
        if (!G[i]) return fail("%s: gradient pointer %d is null", who, i);
    if (t.sparse) {                        // from here on the saved rows are (about to be) overwritten: in the handle's copy and in the filed one
        t.consumed = true;
        for (SavedForward& sf : h->saved->v)
            if (sf.t.generation == t.generation) sf.t.consumed = true;
    }

    // f16x2 flavour: the W operands of the backward GEMMs - transposed weights here, transposed activations in phase B - are written as
    // fp16-pair images by the transposing kernel itself; the A operands are gradients: their producers fold max |x| into the dynamic slots
    // of the exponent table (DY_* / DW_*)
    // (routes_f16x2(): THE condition GemmBuilder::finish(), gemm_route.h, routes a launch to the f16x2 kernels by: a backward pass that wrote only images
    // for launches that then fall through to the fp32-operand kernels would read unwritten buffers - finish() refuses such a launch too.  Not under
    // bf16(): there the transposes write the twins)
    const bool h2b = h->routes_f16x2() && !h->bf16() && t.h2img && T <= DYN_MAX_T;
    h->img.mark_train_image_only(h2b);
    BwdPass p;
    p.dlg = grad_logp_gates;
    p.dyn = h2b ? h->h2_exps + H2_DYN0 : nullptr;
    if (h2b) HIPCHK(hipMemsetAsync(p.dyn, 0, H2_NDYN * sizeof(int), s));
    if (bwd_gemm3(h, t, nullptr, p, s)) return 1;          // (nothing waits for the first step's k_bwd_head)
    const int NV = c.nvalid, NVp = (int)up4((size_t)NV);     // non-padding region rows: the only ones att_va saw
    // under a caller's row bound (vsr_set_valid_rows_bound) NV is the BOUND and the list's tail [n, NV) repeats its first entry: the two
    // gathers below read those rows as zeros (k_transpose_t's rlimit = the device-side count), so att_va's gradient sums over n rows
    const int* nv_dev = c.bounded ? c.nvalid_dev : nullptr;
    // (the K padding of the transposed operands - TBp, Bp, NVp columns - is zero-filled by the transposing kernel itself)
    TOperand ops[N_TOPS];              // (a sealed tape: with the T / TB / TBp of the steps taken)
    train_operands(h, t, ops);
    for (int i : {(int)TX_reg, (int)TY_dP}) { ops[i].R = NV; ops[i].ld_out = NVp; }       // the pair gathered through the list of the non-padding rows
    // entry i -> its buffer.  img: a W operand's registered image, or (self_slot >= 0) the buffer itself holds an image; tb: collected
    auto tr = [&](int i, bool img, int self_slot, TransBatch* tb, const int* list = nullptr, const int* rlimit = nullptr) {
        transpose(h, s, ops[i].src, ops[i].ld_in, ops[i].R, ops[i].C, t.*ops[i].buf, ops[i].ld_out, list, img, self_slot, rlimit, tb);
    };
    auto transpose_ops = [&](int lo, int hi) {          // W operands [lo, hi) of the table in one batched launch (TransBatch), in table order
        TransBatch tb;
        for (int i = lo; i < hi; ++i) tr(i, h2b, -1, &tb);
        tb.flush(s);
    };
    // ---- transposed weights (the optimizer may have changed them since the last call)
    const int Vp = (int)up4(V);        // K of the dh2_vocab GEMM must be a multiple of 8: zero-padded columns
    if (Vp != V) {
        HIPCHK(hipMemsetAsync(t.wT_out, 0, (size_t)H * Vp * sizeof(float), s));
        if (uint16_t* tw = h->bf16() ? const_cast<uint16_t*>(h->img.bf16_of(t.wT_out)) : nullptr) HIPCHK(hipMemsetAsync(tw, 0, (size_t)H * Vp * sizeof(uint16_t), s));
        if (const ImageRange* r2 = h2b ? h->img.h2_of(t.wT_out) : nullptr) HIPCHK(hipMemsetAsync(const_cast<float*>(r2->h2), 0, (size_t)H * Vp * sizeof(float), s));
    }
    transpose_ops(0, N_TW);
    {   // dP, the carries of the last step: one launch
        ZeroList zl;
        zl.add(t.dP, (size_t)RL * A * sizeof(float));
        zl.add(t.dh1_c, BH * sizeof(float)); zl.add(t.dh2_c, BH * sizeof(float)); zl.add(t.dc1_c[0], BH * sizeof(float)); zl.add(t.dc2_c[0], BH * sizeof(float));
        if (zl.launch(s)) return fail("vsr_train_backward: zero launch failed");
    }

    // ---- phase 0: dlogits (t,b) and the vocabulary part of dh2 for every step
    if (t.sparse && (grad_mean || grad_ent))
        hipLaunchKernelGGL(k_dlogits_sel<true>, dim3(TB), dim3(256), 0, s, grad_logp_words, t.tgt32, B, T, V, Vp, t.dlogits, p.ptr(DW_dlogits), grad_mean, grad_ent, t.ent);
    else if (t.sparse)
        hipLaunchKernelGGL(k_dlogits_sel<false>, dim3(TB), dim3(256), 0, s, grad_logp_words, t.tgt32, B, T, V, Vp, t.dlogits, p.ptr(DW_dlogits), nullptr, nullptr, nullptr);
    else hipLaunchKernelGGL(k_dlogits_tb, dim3(TB), dim3(256), 0, s, t.logp_w, grad_logp_words, B, T, V, Vp, t.dlogits, p.ptr(DW_dlogits));
    // the dense products outside the time loop (products.h): written in place where no tile is split, else summed out of the slab scratch
    const ProdRun run{h, &h->prof, s, t.scratch, t.scratch_floats, nullptr, 1.f, who};
    auto in_place = [](Prod q) { q.in_place = true; return q; };
    {
        Prod q = in_place(prod1(TB, H, Vp, t.dlogits, Vp, t.wT_out, Vp, t.dh2_voc, H));
        q.seg[0].a_cls = p.slot(DW_dlogits);
        if (run_product(run, q)) return 1;
    }
    LAUNCHCHK();

    // ---- phase A: reverse time (the cell-carry buffers alternate)
    for (int tt = T - 1; tt >= 0; --tt, p.cb ^= 1)
        if (train_backward_step(h, t, tt, p, s)) return 1;

    // ---- phase B: weight gradients, reduction over all T*B rows.  First the operands (train_operands) ...
    transpose_ops(N_TW, TX_reg);              // the activations, rows (t, b); TX_reg through the list of the non-padding rows:
    if (NV > 0) tr(TX_reg, h2b, -1, nullptr, c.vlist, nv_dev);
    if (h2b) hipLaunchKernelGGL(k_h2_dyn_fold, dim3(1), dim3(64), 0, s, p.dyn, T, T * K);
    // the transposed gradients are the A operands of the weight-gradient GEMMs: with the whole-pass bounds known (k_h2_dyn_fold) they are
    // written as fp16-pair images IN PLACE of the fp32 values and those GEMMs take the all-DMA kernel (a_img: the buffer holds an image)
    bool a_img[N_TOPS] = {};
    const bool tyi = h2b && h->gk.h2_aimg && TBp % 8 == 0 && (reinterpret_cast<uintptr_t>(t.tY_dpre1) & 255) == 0;     // (every buffer of the workspace shares that alignment)
    {
        TransBatch tby;
        for (int i = TY_dpre1; i < TY_dpre1sum; ++i) { a_img[i] = tyi; tr(i, tyi, p.slot(ops[i].slot), &tby); }
        tby.flush(s);
    }
    const TOperand& dP = ops[TY_dP];
    // index lists: several slot entries of an image name the same bank row; att_va's gradient runs over bank rows, so the
    // entry gradients are first summed per bank row, in ascending entry order (deterministic, like the embedding gradient)
    if (c.ridx) hipLaunchKernelGGL(k_dP_to_bank, dim3(c.n_img * c.Rb), dim3(128), 0, s, t.dP, c.ridx, c.L * c.R, c.Rb, A, t.dP_bank);
    if (h2b && NV > 0) {
        const long long ndp = (long long)(c.ridx ? (size_t)c.n_img * c.Rb : (size_t)RL) * A;
        hipLaunchKernelGGL(k_absmax, dim3((unsigned)std::min<long long>(1024, cdiv(ndp, 1024))), dim3(256), 0, s, dP.src, ndp, reinterpret_cast<unsigned*>(p.dyn + DW_dP));
    }
    a_img[TY_dP] = tyi && NVp % 8 == 0;
    if (NV > 0) tr(TY_dP, a_img[TY_dP], p.slot(dP.slot), nullptr, c.vlist, nv_dev);
    // the gradient of the hoisted v-bar projection: per IMAGE, the sum over its rows (ascending) and steps
    sum_over_t(s, t.dpre1, T, K, B, 6 * H, t.dpre1sum);
    tr(TY_dpre1sum, false, -1, nullptr);
    LAUNCHCHK();

    // ... then the table of the gradients, row by row.  Gradients are finished bucket by bucket, largest first, and a bucket's event is
    // recorded where the walk leaves it (vsr_train_bucket_map / vsr_train_wait_bucket): a data-parallel caller starts the all-reduce of a
    // finished bucket on a side stream while the remaining weight-gradient GEMMs run.  The last bucket is the smallest (14 MB).
    if (!h->bucket_ev[0])
        for (int i = 0; i < VSR_GRAD_BUCKETS; ++i) HIPCHK(hipEventCreateWithFlags(&h->bucket_ev[i], hipEventDisableTiming));
    const std::vector<GradRow> rows = train_grad_table(d);
    auto product = [&](const GradRow& r) {              // (the operands by entry: K = their padded rows)
        const TOperand &Y = ops[r.ty], &X = ops[r.tx];
        const int Kp = (int)Y.ld_out;
        Prod q = in_place(prod1(r.M, X.C, Kp, t.*Y.buf + (size_t)r.r0 * Kp, Kp, t.*X.buf, (int)X.ld_out, G[r.g] + r.col, r.ldd));
        q.seg[0].a_cls = p.slot(a_img[r.ty] || r.slot < 0 ? Y.slot : r.slot); q.seg[0].a_img = a_img[r.ty];
        return q;
    };
    int bucket = 0;
    for (size_t i = 0; i < rows.size();) {
        const GradRow& r = rows[i];
        if (r.bucket != bucket) {
            if (r.bucket != bucket + 1 || r.bucket >= VSR_GRAD_BUCKETS) return fail("%s: the gradient table's buckets are not 0 .. %d in order", who, VSR_GRAD_BUCKETS - 1);
            HIPCHK(hipEventRecord(h->bucket_ev[bucket++], s));
        }
        if (!r.on) { ++i; continue; }
        if (r.kind == GradRow::PROD && r.pre == GradRow::PRE_VA && NV == 0) {       // att_va saw no row
            HIPCHK(hipMemsetAsync(G[r.g], 0, (size_t)r.M * ops[r.tx].C * sizeof(float), s));
            ++i;
        } else if (r.kind == GradRow::PROD && r.launch == GradRow::ALONE) {
            if (r.pre == GradRow::PRE_DPRE2SUM) {       // the v-bar columns of lstm_cell_2.weight_ih: as dpre1sum above
                sum_over_t(s, t.dpre2, T, K, B, 4 * H, t.dpre2sum);
                tr(TY_dpre2sum, false, -1, nullptr);
            }
            if (run_product(run, product(r))) return 1;
            ++i;
        } else if (r.kind == GradRow::PROD) {           // the run of products that share this launch
            Prod P[GEMM_MAX_PROB];
            int n = 0;
            for (; i < rows.size() && rows[i].kind == GradRow::PROD && rows[i].launch == r.launch && rows[i].bucket == r.bucket; ++i) {
                if (!rows[i].on) continue;
                if (n == GEMM_MAX_PROB) return fail("%s: more than %d products in one launch of the gradient table", who, GEMM_MAX_PROB);
                P[n++] = product(rows[i]);
            }
            if (n && run_products(run, P, n)) return 1;
        } else if (r.kind == GradRow::COLSUM) {         // (through the idle slab scratch)
            const bool shared = i > 0 && rows[i - 1].kind == GradRow::COLSUM && rows[i - 1].src == r.src && rows[i - 1].bucket == r.bucket;
            if (!shared) colsum_partials(s, t.*r.src, r.ld, TB, r.C, t.scratch);
            colsum_finish(s, t.scratch, r.C, r.c0, r.n, G[r.g], r.g2 >= 0 ? G[r.g2] : nullptr);
            ++i;
        } else {   // EMBED: dx = dpre1 . [W_ih1 ; W_is ; W_ig][:, x columns], summed onto the rows that were looked up (ordered, no atomics)
            const int xoff = (d.h2_first_lstm ? H : 0) + D, sP1 = p.slot(DW_step + DY_dpre1), sQ = p.slot(DW_step + DY_dq);
            Prod q = in_place(prod1(TB, E, 4 * H, t.dpre1, 6 * H, t.wT_ih1 + (size_t)xoff * 4 * H, 4 * H, t.dx_all, E));
            q.seg[0].a_cls = sP1;
            q.seg[1] = ProdSeg{t.dpre1 + 4 * H, 6 * H, t.wT_is + (size_t)xoff * H, H, H, sP1};
            q.seg[2] = ProdSeg{t.dpre1 + 5 * H, 6 * H, t.wT_ig + (size_t)xoff * H, H, H, sQ};
            q.nseg = 3;
            if (run_product(run, q)) return 1;
            HIPCHK(hipMemsetAsync(G[r.g], 0, (size_t)V * E * sizeof(float), s));
            hipLaunchKernelGGL(k_embed_grad_rows, dim3(TB), dim3(256), 0, s, t.dx_all, t.word32, TB, E, G[r.g]);
            ++i;
        }
    }
    if (bucket != VSR_GRAD_BUCKETS - 1) return fail("%s: the gradient table ends in bucket %d of %d", who, bucket, VSR_GRAD_BUCKETS);
    HIPCHK(hipEventRecord(h->bucket_ev[bucket], s));
    h->buckets_recorded = true;
    LAUNCHCHK();
    return 0;
}
extern "C" int vsr_train_backward(vsr_handle* h, const float* grad_logp_words, const float* grad_logp_gates, const vsr_weights* grads,
                                  void* stream) {
    return train_backward_impl(h, false, grad_logp_words, grad_logp_gates, grads, stream);
}
extern "C" int vsr_train_backward_selected(vsr_handle* h, const float* grad_logp_sel, const float* grad_logp_gates, const vsr_weights* grads,
                                           void* stream) {
    return train_backward_impl(h, true, grad_logp_sel, grad_logp_gates, grads, stream);
}
extern "C" int vsr_train_backward_selected_stats(vsr_handle* h, const float* grad_logp_sel, const float* grad_logp_mean, const float* grad_entropy,
                                                 const float* grad_logp_gates, const vsr_weights* grads, void* stream) {
    return train_backward_impl(h, true, grad_logp_sel, grad_logp_gates, grads, stream, true, grad_logp_mean, grad_entropy);
}

// Completion order of the 28 gradients inside vsr_train_backward: bucket_of[i] (field order of vsr_weights) in
// [0, VSR_GRAD_BUCKETS); bucket b is complete when its event has fired.  Static (does not depend on the shapes).
extern "C" int vsr_train_bucket_map(int32_t* bucket_of, int32_t* n_buckets) {
    if (!bucket_of || !n_buckets) return fail("vsr_train_bucket_map: null argument");
    for (int i = 0; i < N_GRADS; ++i) bucket_of[i] = -1;
    for (const GradRow& r : train_grad_table(vsr_dims{}))        // (the rows of every configuration: sizes and flags do not move a bucket)
        for (int g : {r.g, r.g2}) {
            if (g < 0) continue;
            if (bucket_of[g] >= 0 && bucket_of[g] != r.bucket) return fail("vsr_train_bucket_map: gradient %d has rows in buckets %d and %d", g, bucket_of[g], r.bucket);
            bucket_of[g] = r.bucket;
        }
    for (int i = 0; i < N_GRADS; ++i)
        if (bucket_of[i] < 0) return fail("vsr_train_bucket_map: gradient %d has no bucket", i);
    *n_buckets = VSR_GRAD_BUCKETS;
    return 0;
}

// Make `stream` wait (on the device; the host does not block) until bucket `bucket` of the last vsr_train_backward is complete.
extern "C" int vsr_train_wait_bucket(vsr_handle* h, int32_t bucket, void* stream) {
    if (!h || !h->tc) return fail("vsr_train_wait_bucket: null handle");
    if (bucket < 0 || bucket >= VSR_GRAD_BUCKETS) return fail("vsr_train_wait_bucket: bucket %d not in [0, %d)", bucket, VSR_GRAD_BUCKETS);
    if (!h->buckets_recorded) return fail("vsr_train_wait_bucket: no backward pass has run on this handle");
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->bucket_ev[bucket], 0));
    return 0;
}

// ---------------------------------------------------------------------------------------------- test hook
// copies an internal training buffer (by name) into a caller tensor: lets the parity tests localise a gradient
// mismatch to one stage instead of only seeing the 28 end results.
extern "C" int vsr_debug_copy(vsr_handle* h, const char* name, float* dst, size_t n_floats, void* stream) {
    if (!h || !name || !dst) return fail("vsr_debug_copy: null argument");
    TrainCtx& t = *h->tc;
    struct Ent { const char* n; const float* p; };
    const Ent tab[] = {{"dh2_voc", t.dh2_voc}, {"dpre1", t.dpre1}, {"dpre2", t.dpre2}, {"gates1", t.gates1}, {"gates2", t.gates2},
                       {"c1s", t.c1s}, {"c2s", t.c2s}, {"h1s", t.h1s}, {"h2s", t.h2s}, {"dlogits", t.dlogits}, {"alphas", t.alphas},
                       {"dhA", t.dhA_all}, {"dsent", t.dsent_all}, {"dsa", t.dsa_all}, {"dga", t.dga_all}, {"dP", t.dP},
                       {"atts", t.atts}, {"sents", t.sents}, {"wT_out", t.wT_out}, {"dx_all", t.dx_all}};
    for (const Ent& e : tab)
        if (!strcmp(e.n, name)) {
            HIPCHK(hipMemcpyAsync(dst, e.p, n_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
            return 0;
        }
    return fail("vsr_debug_copy: unknown buffer '%s'", name);
}
