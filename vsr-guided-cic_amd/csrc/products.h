// The ONE dense-product path of the host code outside the timestep: the ordering models' inference and training passes (ssp.inc.h) and the
// decoder's training pass (train.inc.h) describe each product as a Prod and hand it to run_products.
//   out (M, N) = epilogue(sum over the k segments of A_i (M, K_i) . W_i (N, K_i)^T)
// The epilogue (k_prod_finish, kernels.h), every term optional, in THIS order:
//   + bias[n]
//   act         SSP_ACT_RELU: max(., 0), SSP_ACT_TANH
//   keep        (M N bytes, compact) dropout: keep ? . scale : 0 - the forward's site, or in the backward the site of the tensor whose
//               gradient this is
//   relu_y      backward through relu + dropout in one: the taped y = drop(relu(.)) is > 0 exactly where both let the gradient pass, and
//               the factor there is scale (1: a ReLU without dropout)
//   + residual  (may be out's buffer: accumulation)
// A product has keep or relu_y, never both.  Which terms a product has selects the instance of the finish kernel (prod_finish).
// ldo / ldy / ldr: the leading dimensions of out / relu_y / residual, 0 = N (compact).
// in_place: where no tile of the launch is split (one slab) and every product of the launch allows it, the GEMM writes `out` itself and no
// finish kernel runs.  Refused for a product with an epilogue term, and meant only where the results have always been produced that way: the
// finish kernel's sum of ONE slab is 0.f + v, which turns a -0 into +0, and the in-place write does not.
// Planning (plan_products) is host arithmetic on a GemmState and calls no HIP function: tools/products_host.hip drives it on the CPU.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "gemm_route.h"
#include "kernels.h"

static int fail(const char* fmt, ...);        // the includer's error sink (vsrcap.hip)

namespace vsr {

// a_cls: the bound class of A (H2Slot; H2A_NONE: the launch cannot take the f16x2 kernels).  a_img: A holds an fp16-pair image IN PLACE of
// the fp32 values (a transposed gradient of the decoder's backward pass): the launch must take the all-DMA kernel
struct ProdSeg { const float* A; int lda; const float* W; int ldw; int K; int a_cls = H2A_NONE; bool a_img = false; };
struct Prod {
    int M, N;
    ProdSeg seg[GEMM_MAX_SEG];
    int nseg;
    float* out; int ldo;
    const float* bias; int act; const uint8_t* keep; const float* relu_y; int ldy; const float* residual; int ldr;
    bool in_place;
};
// what a pass gives all its products.  prof: the profile its launches count in, or null.  scale = 1 / (1 - p): the forward gives it, the
// backward the tape's header (hdr) that carries it.
struct ProdRun { const GemmState* st; GemmProfile* prof; hipStream_t s; float* scratch; size_t scratch_floats; const int* hdr; float scale; const char* pass; };

inline Prod prod1(int M, int N, int K, const float* A, int lda, const float* W, int ldw, float* out, int ldo = 0) {
    Prod p{};
    p.M = M; p.N = N; p.seg[0] = ProdSeg{A, lda, W, ldw, K}; p.nseg = 1; p.out = out; p.ldo = ldo;
    return p;
}
// a layer of a forward pass: out = drop(act(A W^T + bias)) (+ residual), W (N, K) compact; keep: the dropout site's bytes, null = none
inline Prod lin(int M, int N, int K, const float* A, int lda, const float* W, const float* bias, float* out, int act = SSP_ACT_NONE,
                const float* residual = nullptr, const uint8_t* keep = nullptr) {
    Prod p = prod1(M, N, K, A, lda, W, K, out);
    p.bias = bias; p.act = act; p.residual = residual; p.keep = keep;
    return p;
}
// the instance of k_prod_finish a product takes: k_prod_finish<lin, gate>
struct ProdFinish { bool lin; int gate; };
inline ProdFinish prod_finish(const Prod& p) {
    const int gate = p.keep ? FIN_KEEP : (p.relu_y ? FIN_RELU_Y : FIN_NONE);
    return ProdFinish{gate != FIN_NONE || p.bias || p.act != SSP_ACT_NONE || p.residual, gate};
}

struct ProdPlan {
    GemmBuilder g;                        // the planned launch.  In place: C / ldc are the destinations; else C is still to be set to scratch + off[i]
    int ns = 0;                           // the launch's slab count
    bool in_place = false;
    size_t off[GEMM_MAX_PROB] = {};       // slab path: where product i's nslab_i slabs of M N floats begin in the scratch
    char err[200] = "";                   // why the launch was refused
    int refuse(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, sizeof(err), fmt, ap);
        va_end(ap);
        return 1;
    }
};
// Up to GEMM_MAX_PROB products in ONE launch, planned: validated, routed (GemmBuilder::finish), in place or through slabs, the slabs placed.
// Problems and segments go to the GEMM in the order given (it numbers the tiles and fixes the summation order, step_gemms.h).  Returns
// non-zero with pl.err set when the launch is refused.
inline int plan_products(const GemmState& st, const Prod* P, int n, size_t scratch_floats, ProdPlan& pl) {
    if (n < 1 || n > GEMM_MAX_PROB) return pl.refuse("%d products in one launch (1 to %d fit)", n, GEMM_MAX_PROB);
    GemmBuilder& g = pl.g = GemmBuilder();
    bool in_place = true, a_img = false;
    for (int i = 0; i < n; ++i) {
        if (P[i].nseg > GEMM_MAX_SEG) return pl.refuse("a product of %d k segments (%d fit)", P[i].nseg, GEMM_MAX_SEG);
        GemmProb& p = g.prob(P[i].M, P[i].N, nullptr, P[i].N);
        for (int k = 0; k < P[i].nseg; ++k) {
            const ProdSeg& sg = P[i].seg[k];
            if ((sg.K & 3) || (sg.lda & 3) || (sg.ldw & 3) || !aligned16(sg.A) || !aligned16(sg.W))
                return pl.refuse("operand not in whole 16-byte groups (K %d, lda %d, ldw %d)", sg.K, sg.lda, sg.ldw);
            GemmBuilder::seg(p, sg.A, sg.lda, nullptr, sg.W, sg.ldw, sg.K, sg.a_img ? reinterpret_cast<const uint16_t*>(sg.A) : nullptr, sg.a_cls);
            a_img = a_img || sg.a_img;
        }
        if (P[i].in_place && prod_finish(P[i]).lin) return pl.refuse("an in-place product cannot have an epilogue");
        if (P[i].keep && P[i].relu_y) return pl.refuse("a product has keep or relu_y, not both");
        in_place = in_place && P[i].in_place;
    }
    g.a_image_only = a_img && !st.bf16();
    pl.ns = g.finish(&st);
    if (g.a_image_only && g.route.kernel != GemmKernel::H2A)
        return pl.refuse("an A operand exists only as an fp16-pair image but the launch did not take the all-DMA kernel");
    pl.in_place = pl.ns == 1 && in_place;
    if (pl.in_place) {                    // every tile is produced by one workgroup: written in place
        for (int i = 0; i < n; ++i) { g.a.p[i].C = P[i].out; g.a.p[i].ldc = P[i].ldo ? P[i].ldo : P[i].N; g.a.p[i].slab_stride = 0; }
        return 0;
    }
    // Compact, in the order given, each product with its OWN slab count (gemm_tight_slabs: what its tiles can meet).  The slabs between that
    // and the launch's count would hold zeros, and the finish kernel's sum starts from +0: leaving them out changes no bit.
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        g.a.p[i].nslab = gemm_tight_slabs(g.a, i);
        g.a.p[i].slab_stride = (long long)P[i].M * P[i].N;
        pl.off[i] = off;
        off += (size_t)P[i].M * P[i].N * g.a.p[i].nslab;
    }
    if (off > scratch_floats) return pl.refuse("GEMM scratch too small (%zu floats of slabs, %zu fit)", off, scratch_floats);
    return 0;
}

// plans, launches, and gives every product that went through slabs its finish kernel
inline int run_products(const ProdRun& c, const Prod* P, int n) {
    ProdPlan pl;
    if (plan_products(*c.st, P, n, c.scratch_floats, pl)) return fail("%s: %s", c.pass, pl.err);
    GemmArgs& a = pl.g.a;
    if (!pl.in_place)
        for (int i = 0; i < n; ++i) a.p[i].C = c.scratch + pl.off[i];
    if (pl.g.launch(c.s, c.st, c.prof)) return fail("%s: gemm launch failed", c.pass);
    if (pl.in_place) return 0;
    for (int i = 0; i < n; ++i) {
        const Prod& p = P[i];
        const long long tot = (long long)p.M * p.N;
        auto ld = [&](int l) { return (long long)(l ? l : p.N); };
        const ProdFinish f = prod_finish(p);
        auto finish = f.gate == FIN_NONE ? (f.lin ? k_prod_finish<true, FIN_NONE> : k_prod_finish<false, FIN_NONE>)
                                         : (f.gate == FIN_KEEP ? k_prod_finish<true, FIN_KEEP> : k_prod_finish<true, FIN_RELU_Y>);
        hipLaunchKernelGGL(finish, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c.s, a.p[i].C, a.p[i].nslab, tot, p.M, p.N, p.bias, p.act, p.residual, ld(p.ldr),
                           p.out, ld(p.ldo), p.keep ? (const void*)p.keep : (const void*)p.relu_y, ld(p.ldy), c.hdr, c.scale);
    }
    return 0;
}
inline int run_product(const ProdRun& c, const Prod& p) { return run_products(c, &p, 1); }

}  // namespace vsr
