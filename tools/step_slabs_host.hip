// Slab placement of the step launches (csrc/step_gemms.h: the *_slabs layouts, place_slabs, plan_s56, slab_floats) on the CPU: plans and
// places every launch of DESIGN.md's layout table on a bare GemmState of 256 CUs and prints where everything landed.  No HIP call is
// made; driven by tests/test_step_slabs_logic.py (build: build.py, build_step_slabs_tool).
//   step_slabs_host H A D E V M h2_first_lstm img_second_lstm x3_on refuse
// Every area is given the capacity the workspace functions size it with: slab_floats(layout, M, area).  Output, per launch:
//   launch <name> nprob <n> ns <launch's slab count> replan <0|1>
//   prob <i> area <k> off <floats from the area's base> N <columns> ldc <ldc> stride <slab_stride> nslab <nslab> tight <gemm_tight_slabs>
//   view <group> area <k> off <..> n <slabs> stride <..>
//   area <k> used <floats the placed groups take> cap <capacity given>
// refuse = 1: after that, every area that holds slabs is given one float less than `used` and the launch is placed again:
//   refused <the message the library would fail with, "<name>: ..."> | accepted <name> area <k>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../vsr-guided-cic_amd/csrc/step_gemms.h"

using namespace vsr;

static float* fake(uintptr_t i) { return reinterpret_cast<float*>(uintptr_t(0x1000000000) * (i + 1)); }      // never read: made-up 16-byte aligned addresses
static const int NAREA = 3;

// places g's launch in areas of the given capacities and prints it; then (refuse) once more per area with one float too few
static void show(const char* name, GemmBuilder& g, int M, const SlabLayout& l, const size_t* cap, const size_t* skip, bool replan, bool refuse) {
    SlabArea areas[NAREA];
    for (int k = 0; k < NAREA; ++k) areas[k] = SlabArea{fake(k) + skip[k], cap[k]};
    SlabPlan pl;
    printf("launch %s nprob %d ns %d replan %d\n", name, g.a.nprob, g.a.nslab, (int)replan);
    if (place_slabs(g.a, M, l, areas, NAREA, pl)) { printf("refused %s: %s\n", name, pl.err); return; }
    int area_of[GEMM_MAX_PROB] = {};
    size_t used[NAREA] = {};
    for (int k = 0; k < l.ng; ++k) {
        for (int i = l.g[k].first; i < l.g[k].first + l.g[k].n; ++i) area_of[i] = l.g[k].area;
        used[l.g[k].area] += (size_t)pl.v[k].stride * pl.v[k].n;
    }
    for (int i = 0; i < g.a.nprob; ++i) {
        const GemmProb& p = g.a.p[i];
        printf("prob %d area %d off %lld N %d ldc %d stride %lld nslab %d tight %d\n", i, area_of[i], (long long)(p.C - fake(area_of[i])), p.N, p.ldc, p.slab_stride, p.nslab,
               gemm_tight_slabs(g.a, i));
    }
    for (int k = 0; k < l.ng; ++k)
        printf("view %d area %d off %lld n %d stride %lld\n", k, l.g[k].area, (long long)(pl.v[k].base - fake(l.g[k].area)), pl.v[k].n, pl.v[k].stride);
    for (int k = 0; k < NAREA; ++k)
        if (slab_row_floats(l, k)) printf("area %d used %zu cap %zu\n", k, used[k], cap[k]);
    if (!refuse) return;
    for (int k = 0; k < NAREA; ++k) {
        if (!used[k]) continue;
        SlabArea less[NAREA];
        for (int j = 0; j < NAREA; ++j) less[j] = areas[j];
        less[k].floats = used[k] - 1;
        GemmArgs a = g.a;
        if (place_slabs(a, M, l, less, NAREA, pl)) printf("refused %s: %s\n", name, pl.err);
        else printf("accepted %s area %d\n", name, k);
    }
}

int main(int argc, char** argv) {
    if (argc != 11) return 2;
    vsr_dims d;
    memset(&d, 0, sizeof(d));
    d.rnn_size = atoi(argv[1]); d.att_size = atoi(argv[2]); d.det_feat_size = atoi(argv[3]); d.input_encoding_size = atoi(argv[4]); d.vocab_size = atoi(argv[5]);
    const int M = atoi(argv[6]);
    d.h2_first_lstm = atoi(argv[7]); d.img_second_lstm = atoi(argv[8]);
    const bool refuse = atoi(argv[10]) != 0;
    GemmState st;
    st.x3_on = atoi(argv[9]) != 0;
    st.gk.set_cus(256);
    st.gk.read_env();                     // (the VSR_* routing knobs, as vsr_create: what a GPU test's environment does to the plans can be read here)
    vsr_weights w;
    float** wp = reinterpret_cast<float**>(&w);
    for (size_t i = 0; i < sizeof(w) / sizeof(float*); ++i) wp[i] = fake(8 + i);
    StepOperands o;
    o.M = M;
    o.h1_old = fake(40); o.h2_old = fake(41); o.h1_new = fake(42); o.h2_new = fake(43); o.s_t = fake(44); o.g_t = fake(45); o.att = fake(46);
    o.x = w.embed_weight;
    BwdStepOperands b;
    b.M = M;
    b.dpre1 = fake(50); b.dpre2 = fake(51); b.dhA = fake(52); b.dsent = fake(53); b.dsa = fake(54); b.dga = fake(55);
    b.wT_ih1 = fake(60); b.wT_is = fake(61); b.wT_ig = fake(62); b.wT_hh1 = fake(63); b.wT_hs = fake(64); b.wT_ih2 = fake(65); b.wT_hh2 = fake(66);
    b.wT_hg = fake(67); b.wT_ha = fake(68); b.wT_sfc = fake(69); b.wT_sa = fake(70); b.wT_ga = fake(71);
    const size_t none[NAREA] = {0, 0, 0};

    // one launch in area 0 at the capacity slab_floats gives its layout
    auto one = [&](const char* name, GemmBuilder& g, int m, const SlabLayout& l) {
        if (g.a.nprob > 0) g.finish(&st);
        const size_t cap[NAREA] = {slab_floats(l, (size_t)m), 0, 0};
        show(name, g, m, l, cap, none, false, refuse);
    };
    { GemmBuilder g; add_vproj(g, d, w, fake(47), M); one("vproj", g, M, lstm1_slabs(d)); }
    if (d.img_second_lstm) { GemmBuilder g; add_vproj2(g, d, w, fake(47), M); one("vproj2", g, M, vproj2_slabs(d)); }
    { GemmBuilder g; add_att_va(g, d, w, fake(48), nullptr, M); one("att_va", g, M, att_va_slabs(d)); }
    {   // the x projection: a decode-cache chunk (at most 512 rows of the embedding table) and the training forwards' rows
        StepOperands oc = o;
        oc.M = M < 512 ? M : 512;
        GemmBuilder g, gt;
        add_lstm1(g, d, w, oc, L1_X); one("cache_chunk", g, oc.M, lstm1_slabs(d));
        add_lstm1(gt, d, w, o, L1_X); one("train_xproj", gt, M, lstm1_slabs(d));
    }
    const struct { const char* name; int parts; } s1[] = {{"S1_none", 0}, {"S1_x", L1_X}, {"S1_rec", L1_H2 | L1_H1}, {"S1_all", L1_H2 | L1_X | L1_H1}};
    for (const auto& v : s1) { GemmBuilder g; add_lstm1(g, d, w, o, v.parts); one(v.name, g, M, lstm1_slabs(d, g.a.nprob)); }
    { GemmBuilder g; add_s2(g, d, w, o); one("S2", g, M, s2_slabs(d)); }
    for (int with_h2 = 0; with_h2 < 2; ++with_h2) {
        char name[32];
        GemmBuilder g;
        add_s5(g, d, w, o, with_h2 != 0);
        snprintf(name, sizeof(name), "train_S5_h2%d", with_h2);
        one(name, g, M, s5_slabs(d));
        // decode S5 / S6, planned together: no sums for the next step, all of them with the vocabulary, the h1 part split off into S5
        for (int mode = 0; mode < 3; ++mode) {
            Step56 p;
            plan_s56(&st, d, w, o, with_h2 != 0, mode > 0, mode == 2 && d.h2_first_lstm, p);
            const SlabLayout l5 = s5_decode_slabs(d, p.g5.a.nprob, p.ns_h1), l6 = s6_slabs(d, p.g6.a.nprob, p.ns_pre1);
            const size_t cap5[NAREA] = {slab_floats(l5, (size_t)M, 0), slab_floats(l5, (size_t)M, 1), slab_floats(l5, (size_t)M, 2)};
            snprintf(name, sizeof(name), "S5_h2%d_mode%d", with_h2, mode);
            show(name, p.g5, M, l5, cap5, none, p.replanned, refuse);
            // S6's second area: the rest of pre1 behind S5's ns_h1 slabs
            const size_t behind = (size_t)p.ns_h1 * M * 6 * d.rnn_size;
            const size_t cap6[NAREA] = {slab_floats(l6, (size_t)M, 0), cap5[2] - behind, 0}, skip6[NAREA] = {0, behind, 0};
            snprintf(name, sizeof(name), "S6_h2%d_mode%d", with_h2, mode);
            printf("pre1 ns_h1 %d ns_pre1 %d nblk6 %d\n", p.ns_h1, p.ns_pre1, p.nblk6);
            show(name, p.g6, M, l6, cap6, skip6, p.replanned, refuse);
        }
    }
    { GemmBuilder g; add_vocab(g, d, w, o); one("train_vocab", g, M, vocab_slabs(d)); }
    { GemmBuilder g; add_bwd1(g, d, b); one("bwd1", g, M, bwd1_slabs(d)); }
    { GemmBuilder g; add_bwd2(g, d, b); one("bwd2", g, M, bwd2_slabs(d)); }
    { GemmBuilder g; add_bwd3(g, d, b); one("bwd3", g, M, bwd3_slabs(d, g.a.nprob)); }
    { GemmBuilder g; one("bwd3_none", g, M, bwd3_slabs(d, 0)); }
    return 0;
}
