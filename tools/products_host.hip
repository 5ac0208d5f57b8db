// plan_products (csrc/products.h) on the CPU: reads launches from stdin, plans each on a GemmState of 256 CUs and prints the plan or the
// refusal.  No HIP call is made; driven by tests/test_products_logic.py (build: build.py, build_products_tool).
//   per launch:   x3_on h2_on scratch_floats n
//   per product:  M N nseg in_place has_bias has_keep has_relu_y ldo
//   per segment:  K lda ldw a_byte_offset a_img
// Output, one line per launch: "refused <message>" or "ok ns <ns> in_place <0|1>" followed by, per product,
//   " | c_is_out <0|1> ldc <ldc> stride <slab_stride> nslab <nslab> off <scratch offset> finish <none | k_prod_finish<LIN,GATE>>"
#include <cstdarg>
#include <cstdio>

static int fail(const char*, ...) { return 1; }        // (run_products' error sink; nothing here runs a product)
#include "../vsr-guided-cic_amd/csrc/products.h"

using namespace vsr;

int main() {
    // operands are never read: made-up addresses on 16-byte boundaries
    char* const A0 = reinterpret_cast<char*>(uintptr_t(0x10000000)), * const W0 = reinterpret_cast<char*>(uintptr_t(0x20000000));
    float* const some = reinterpret_cast<float*>(uintptr_t(0x30000000));
    auto out_of = [](int i) { return reinterpret_cast<float*>(uintptr_t(0x40000000) + uintptr_t(i) * 0x1000000); };
    int x3, h2, n;
    unsigned long long scratch;
    while (scanf("%d %d %llu %d", &x3, &h2, &scratch, &n) == 4) {
        if (n < 0 || n > 16) return 2;
        GemmState st;
        st.x3_on = x3 != 0; st.h2_on = h2 != 0;
        st.gk.set_cus(256);
        Prod P[16];
        for (int i = 0; i < n; ++i) {
            int M, N, nseg, inpl, bias, keep, relu_y, ldo;
            if (scanf("%d %d %d %d %d %d %d %d", &M, &N, &nseg, &inpl, &bias, &keep, &relu_y, &ldo) != 8 || nseg < 0 || nseg > GEMM_MAX_SEG) return 2;
            Prod p{};
            p.M = M; p.N = N; p.nseg = nseg; p.in_place = inpl != 0; p.out = out_of(i); p.ldo = ldo;
            if (bias) p.bias = some;
            if (keep) p.keep = reinterpret_cast<const uint8_t*>(some);
            if (relu_y) p.relu_y = some;
            for (int k = 0; k < nseg; ++k) {
                int K, lda, ldw, aoff, aimg;
                if (scanf("%d %d %d %d %d", &K, &lda, &ldw, &aoff, &aimg) != 5) return 2;
                p.seg[k] = ProdSeg{reinterpret_cast<const float*>(A0 + aoff), lda, reinterpret_cast<const float*>(W0), ldw, K, H2A_NONE, aimg != 0};
            }
            P[i] = p;
        }
        ProdPlan pl;
        if (plan_products(st, P, n, (size_t)scratch, pl)) { printf("refused %s\n", pl.err); continue; }
        printf("ok ns %d in_place %d", pl.ns, (int)pl.in_place);
        for (int i = 0; i < n; ++i) {
            const GemmProb& g = pl.g.a.p[i];
            const ProdFinish f = prod_finish(P[i]);
            printf(" | c_is_out %d ldc %d stride %lld nslab %d off %zu finish ", (int)(g.C == P[i].out), g.ldc, g.slab_stride, g.nslab, pl.off[i]);
            if (pl.in_place) printf("none");
            else printf("k_prod_finish<%s,%s>", f.lin ? "true" : "false", f.gate == FIN_NONE ? "FIN_NONE" : (f.gate == FIN_KEEP ? "FIN_KEEP" : "FIN_RELU_Y"));
        }
        printf("\n");
    }
    return 0;
}
