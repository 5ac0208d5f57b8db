// The flavour rule and the registry of operand images (csrc/gemm_route.h: GemmState, OperandImages) and what GemmBuilder::finish() makes of
// them, on the CPU: a script on stdin drives a bare GemmState of 256 CUs through the registry calls of the entry points (vsr_bind_weights,
// the two refreshes, register_train_images, the backward pass's image-only mark) and routes one-segment launches on it.  No HIP call is
// made and no operand is read: every address is made up.  Driven by tests/test_route_logic.py (build: build.py, build_route_tool).
// Script, one command per line (regions by name, offsets in floats):
//   reset | x3 <0|1> | tile <gemm_tile> | aimg <0|1> | bind | bf16 <0|1> | h2 <0|1> | only <0|1> | table
//   train <0|1|2>     (0: clear; 2: a stale workspace whose second operand has come to lie inside the weight w1)
//   look <region> <off>
//   launch <M> <W region> <off> <K> <ldw> <A region> <off> <lda> <a_cls> <A16: 0|1> <keep_fp32> <a_image_only>      (N = 4096)
// Output: "launch <switches and knobs> M : kernel tm tn mt mf a16 ns stale_w stale_h2 | W=<region+bytes> A=<region+bytes> exp=<exp_idx>",
// "look ..." with every lookup of the address, and for `table` one line per switch state x gemm_tile {0, 64} x h2_aimg {0, 1}.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../vsr-guided-cic_amd/csrc/gemm_route.h"

using namespace vsr;

// ---- the address space: fp32 buffers, then where their images live
struct Region { const char* name; uintptr_t base; size_t bytes; };
static const size_t NW = 4096;                    // rows of every W operand
static const Region REGIONS[] = {
    {"w0", 0x1000000000, NW * 1024 * 4}, {"w1", 0x1100000000, NW * 1024 * 4}, {"emb", 0x1200000000, NW * 1024 * 4},      // two GEMM matrices, the embedding table
    {"t0", 0x2000000000, NW * 1024 * 4}, {"t1", 0x2100000000, NW * 1020 * 4},                                            // a training workspace's W operands
    {"a", 0x3000000000, 512 * 1024 * 4}, {"a16", 0x3100000000, 512 * 1024 * 4},                                          // an fp32 A operand, the image its producer wrote
    {"b16w", 0x4000000000, 2 * NW * 1024 * 2}, {"h2w", 0x4100000000, 4096 + 3 * NW * 1024 * 4},                          // the refreshes' buffers
    {"tw", 0x4200000000, 2 * NW * 1024 * 2}, {"ti", 0x4300000000, 2 * NW * 1024 * 4}};                                   // the workspace's twins and images
static const Region& region(const char* name) {
    for (const Region& r : REGIONS)
        if (!strcmp(r.name, name)) return r;
    fprintf(stderr, "unknown region %s\n", name);
    exit(2);
}
static const float* at(const char* name, long long off) { return reinterpret_cast<const float*>(region(name).base) + off; }
static const char* where(const void* p, char (&buf)[64]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (!p) return "-";
    for (const Region& r : REGIONS)
        if (a >= r.base && a < r.base + r.bytes) { snprintf(buf, sizeof(buf), "%s+%zu", r.name, (size_t)(a - r.base)); return buf; }
    snprintf(buf, sizeof(buf), "?%zx", (size_t)a);
    return buf;
}
static size_t up8(size_t n) { return (n + 7) & ~size_t(7); }
struct Operand { const char* name; size_t n; int slot; };
static const Operand MATRICES[] = {{"w0", NW * 1024, 0}, {"w1", NW * 1024, 1}};
static const Operand EMBED = {"emb", NW * 1024, H2A_EMBED};
static const Operand TRAIN_OPS[] = {{"t0", NW * 1024, H2A_UNIT}, {"t1", NW * 1020, H2A_ATT}};
static const Operand STALE_OPS[] = {{"t0", NW * 1024, H2A_UNIT}, {"w1", NW * 1020, H2A_ATT}};

// ---- the registry calls of the entry points, in their order (vsrcap.hip, train.inc.h); the launches of a refresh left out
static void bind(GemmState& st) {
    if (st.bf16_on) { st.bf16_on = false; st.img.clear_weights_bf16(); }
    if (st.h2_on) { st.h2_on = false; st.img.clear_h2(); }
}
static void refresh_bf16(GemmState& st, bool on) {
    st.img.clear_weights_bf16();
    const uint16_t* out = reinterpret_cast<const uint16_t*>(region("b16w").base);
    if (on)
        for (const Operand& m : MATRICES) { st.img.add_weight_bf16(at(m.name, 0), m.n, out); out += up8(m.n); }
    st.bf16_on = on;
}
static void refresh_h2(GemmState& st, bool on) {
    if (!on) { st.h2_on = false; st.img.clear_h2(); return; }
    st.img.clear_weights_h2();
    const float* out = reinterpret_cast<const float*>(region("h2w").base + 4096);
    for (const Operand& m : MATRICES) { st.img.add_weight_h2(at(m.name, 0), m.n, out, m.slot); out += up8(m.n); }
    st.img.add_weight_h2(at(EMBED.name, 0), EMBED.n, out, EMBED.slot);
    st.h2_exps = reinterpret_cast<int*>(region("h2w").base);
    st.h2_on = true;
}
static void train(GemmState& st, int mode) {                // carve_train's list, then register_train_images
    if (!mode) { st.img.clear_train(); return; }
    std::vector<ImageRange> ops;
    const uint16_t* tw = reinterpret_cast<const uint16_t*>(region("tw").base);
    const float* ti = reinterpret_cast<const float*>(region("ti").base);
    for (const Operand& o : mode == 2 ? STALE_OPS : TRAIN_OPS) {
        ops.push_back(ImageRange{at(o.name, 0), at(o.name, 0) + o.n, ImageRange::TRAIN, tw, st.train_h2_images() ? ti : nullptr, o.slot});
        tw += o.n; ti += up8(o.n);
    }
    st.img.register_train(ops);
}
static void only(GemmState& st, bool on) { st.img.mark_train_image_only(on); }
static void look(const GemmState& st, const float* p) {
    char b[5][64];
    const ImageRange* r = st.img.h2_of(p);
    const ImageRange* rw = st.img.h2_of_weight(p);
    printf("look %s : bf16=%s h2=%s slot=%d h2_weight=%s slot=%d slot_of=%d only_bf16=%d only_h2=%d\n", where(p, b[0]), where(st.img.bf16_of(p), b[1]),
           where(r ? r->h2_at(p) : nullptr, b[2]), r ? r->slot : -1, where(rw ? rw->h2_at(p) : nullptr, b[3]), rw ? rw->slot : -1, st.img.h2_slot_of(p),
           (int)st.img.only_bf16(p), (int)st.img.only_h2(p));
}
static const char* flavour_name(Flavour f) { return f == Flavour::BF16 ? "bf16" : f == Flavour::F16X2 ? "f16x2" : f == Flavour::F32X3 ? "f32x3" : "f32"; }
static void table() {
    for (int s = 0; s < 8; ++s)
        for (int tile : {0, 64})
            for (int aimg : {0, 1}) {
                GemmState st;
                st.bf16_on = s & 4; st.h2_on = s & 2; st.x3_on = s & 1;
                st.gk.gemm_tile = tile; st.gk.h2_aimg = aimg != 0;
                printf("state bf16=%d h2=%d x3=%d tile=%d aimg=%d : flavour=%s bf16=%d f16x2=%d routes_f16x2=%d train_h2_images=%d writes_h2_a_images=%d "
                       "measures_h2_bounds=%d has_weight_images=%d\n", (int)st.bf16_on, (int)st.h2_on, (int)st.x3_on, tile, aimg, flavour_name(st.flavour()), (int)st.bf16(),
                       (int)st.f16x2(), (int)st.routes_f16x2(), (int)st.train_h2_images(), (int)st.writes_h2_a_images(), (int)st.measures_h2_bounds(), (int)st.has_weight_images());
            }
}
// ---- (end of what depends on the registry's interface)

static const char* kernel_name(GemmKernel k) {
    switch (k) {
        case GemmKernel::F32: return "F32"; case GemmKernel::F32_R16: return "F32_R16"; case GemmKernel::BF16W: return "BF16W";
        case GemmKernel::X3: return "X3"; case GemmKernel::X3S: return "X3S"; case GemmKernel::H2: return "H2";
        case GemmKernel::H2S: return "H2S"; case GemmKernel::H2A: return "H2A"; case GemmKernel::B16A: return "B16A";
    }
    return "?";
}

int main() {
    GemmState st;
    st.gk.set_cus(256);
    char cmd[32], wr[32], ar[32];
    while (scanf("%31s", cmd) == 1) {
        int v = 0;
        if (!strcmp(cmd, "reset")) { st = GemmState(); st.gk.set_cus(256); }
        else if (!strcmp(cmd, "bind")) bind(st);
        else if (!strcmp(cmd, "table")) table();
        else if (!strcmp(cmd, "look")) {
            long long off;
            if (scanf("%31s %lld", wr, &off) != 2) return 2;
            look(st, at(wr, off));
        } else if (!strcmp(cmd, "launch")) {
            int M, K, ldw, lda, cls, a16, keep, aonly;
            long long woff, aoff;
            if (scanf("%d %31s %lld %d %d %31s %lld %d %d %d %d %d", &M, wr, &woff, &K, &ldw, ar, &aoff, &lda, &cls, &a16, &keep, &aonly) != 12) return 2;
            GemmBuilder g;
            GemmProb& p = g.prob(M, (int)NW, nullptr, (int)NW);
            GemmBuilder::seg(p, at(ar, aoff), lda, nullptr, at(wr, woff), ldw, K, a16 ? reinterpret_cast<const uint16_t*>(at("a16", aoff)) : nullptr, cls);
            g.keep_fp32 = keep != 0; g.a_image_only = aonly != 0;
            const int ns = g.finish(&st);
            const GemmSeg& S = g.a.p[0].seg[0];
            char b[2][64];
            printf("launch bf16=%d h2=%d x3=%d tile=%d aimg=%d M=%d : kernel=%s tm=%d tn=%d mt=%d mf=%d a16=%d ns=%d stale_w=%d stale_h2=%d | W=%s A=%s exp=%d\n", (int)st.bf16_on,
                   (int)st.h2_on, (int)st.x3_on, st.gk.gemm_tile, (int)st.gk.h2_aimg, M, kernel_name(g.route.kernel), g.route.tm, g.route.tn, g.route.mt, g.route.mf,
                   (int)g.route.a16, ns, (int)g.stale_w, (int)g.stale_h2, where(S.W, b[0]), where(S.A, b[1]), S.exp_idx);
        } else {
            if (scanf("%d", &v) != 1) return 2;
            if (!strcmp(cmd, "x3")) st.x3_on = v != 0;
            else if (!strcmp(cmd, "tile")) st.gk.gemm_tile = v;
            else if (!strcmp(cmd, "aimg")) st.gk.h2_aimg = v != 0;
            else if (!strcmp(cmd, "bf16")) refresh_bf16(st, v != 0);
            else if (!strcmp(cmd, "h2")) refresh_h2(st, v != 0);
            else if (!strcmp(cmd, "train")) train(st, v);
            else if (!strcmp(cmd, "only")) only(st, v != 0);
            else { fprintf(stderr, "unknown command %s\n", cmd); return 2; }
        }
    }
    return 0;
}
