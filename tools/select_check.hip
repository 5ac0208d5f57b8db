// Standalone check of the kernels that turn logits into ids (vsr-guided-cic_amd/csrc/kernels.h): k_vocab, k_select_beam<K>, k_backtrack.
// No library, no handle, no torch: every kernel runs on inputs built here and is compared with a plain host reference in this file.
//   tools/select_check [vocab | beam | backtrack | all]
// One line per case, then the list of k_vocab crossings reached (vocab group), then "N of M cases failed".  The exit status is non-zero
// when a case failed or a HIP call returned an error (after which nothing more is launched).
//
// The inputs leave the reference no choice.  Every bias, slab entry, logit, gate logit and running score is a multiple of 1/8 of small
// magnitude ([-8, 8]; running scores [-64, 0]): every fp32 sum the kernels form is exact in any order, the host forms the same fp32 values,
// and the ties are exactly the ties a case designed.  No row is ever excluded from a comparison.
//   exact:  ids, parents, gates, slots, masks, the bad-verb counter, every sentinel around an output;
//           bit-equal floats: top_v of verb-forced rows, seq_out / hist_lpw / hist_lpg of the beam selection, all of k_backtrack's
//   2e-5:   log-probs x - lse against an fp64 lse (the project's bound for log-probs)
// (A row of up to 12 292 logits cannot hold distinct grid values: the "distinct" row has K + 1 distinct leaders over a random rest.)
//
// Which branch of k_vocab a row takes follows from the row alone (the kernel is not instrumented): element v belongs to thread
// (v / 4) % NT; the threshold is the K-th largest wave maximum (NT / 64 >= K) or the K-th best thread maximum; nc counts x >= threshold.
// row_regime() below evaluates that on the host and the tool refuses to pass when a required crossing was not reached.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../vsr-guided-cic_amd/csrc/kernels.h"

using namespace vsr;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error: %s: %s\n", #x, hipGetErrorString(e_)); fflush(stdout); exit(2); } } while (0)

constexpr double TOL = 2e-5;
static int g_cases = 0, g_failed = 0;
static double g_maxerr = 0.0;

struct Rng {
    uint32_t s;
    explicit Rng(uint32_t seed) : s(seed * 2654435761u + 12345u) {}
    uint32_t next() { s = s * 1664525u + 1013904223u; return s >> 8; }
    int range(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }      // inclusive
};

template <class T> static T* to_dev(const std::vector<T>& h) {
    T* d = nullptr;
    CK(hipMalloc(&d, std::max<size_t>(h.size(), 4) * sizeof(T)));
    if (!h.empty()) CK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

// an output array between two guard zones; everything starts as a sentinel, `want` holds what the kernel must leave behind
template <class T> struct OutBuf {
    static constexpr size_t G = 16;
    std::vector<T> want;
    std::vector<char> approx;
    std::vector<double> want64;
    T* d = nullptr;
    const char* name;
    OutBuf(const char* nm, size_t n, T sentinel) : want(n + 2 * G, sentinel), approx(n + 2 * G, 0), want64(n + 2 * G, 0.0), name(nm) { d = to_dev(want); }
    OutBuf(const OutBuf&) = delete;
    ~OutBuf() { (void)hipFree(d); }
    T* ptr() { return d + G; }
    void refill(T sentinel) { std::fill(want.begin(), want.end(), sentinel); std::fill(approx.begin(), approx.end(), 0); CK(hipMemcpy(d, want.data(), want.size() * sizeof(T), hipMemcpyHostToDevice)); }
    void set(size_t i, T v) { want[G + i] = v; approx[G + i] = 0; }
    void set_approx(size_t i, double v) { want64[G + i] = v; approx[G + i] = 1; }
    // number of wrong elements (the first one is printed)
    int check() {
        std::vector<T> got(want.size());
        CK(hipMemcpy(got.data(), d, got.size() * sizeof(T), hipMemcpyDeviceToHost));
        int bad = 0;
        for (size_t i = 0; i < got.size(); ++i) {
            bool ok;
            if (approx[i]) {
                const double e = std::fabs((double)got[i] - want64[i]);
                ok = e <= TOL;                                   // (a NaN fails)
                if (e > g_maxerr || e != e) g_maxerr = e == e ? e : 1e30;
            } else {
                ok = memcmp(&got[i], &want[i], sizeof(T)) == 0;
            }
            if (!ok && bad++ == 0) {
                if (approx[i]) printf("    %s[%lld]: got %.9g, want %.9g (fp64), |diff| %.3g > %.1g\n", name, (long long)i - (long long)G, (double)got[i], want64[i], std::fabs((double)got[i] - want64[i]), TOL);
                else printf("    %s[%lld]: got %.9g, want %.9g (exact%s)\n", name, (long long)i - (long long)G, (double)got[i], (double)want[i], (i < G || i >= want.size() - G) ? ", guard zone" : "");
            }
        }
        return bad;
    }
};

static void finish_case(const std::string& line, int bad) {
    ++g_cases;
    if (bad) ++g_failed;
    printf("%s %s\n", line.c_str(), bad ? "FAIL" : "ok");
}

// =============================================================================================== k_vocab
// n distinct ids of [0, V) not yet in `used`
static std::vector<int> pick_ids(int V, int n, Rng& rng, std::vector<char>& used) {
    std::vector<int> ids;
    while ((int)ids.size() < n) {
        const int v = rng.range(0, V - 1);
        if (!used[v]) { used[v] = 1; ids.push_back(v); }
    }
    return ids;
}

// The rows of one launch, as logits in eighths ([-48, 48]; the bias takes [-16, 16] of the budget of a single slab).
struct Rows {
    int V = 0, M = 0;
    std::vector<int> x8;
    std::vector<std::string> name;
    int* row(int r) { return x8.data() + (size_t)r * V; }
    int add(const std::string& nm) { x8.resize((size_t)(M + 1) * V, 0); name.push_back(nm); return M++; }
    void fill(int r, int lo, int hi, Rng& rng) { int* x = row(r); for (int v = 0; v < V; ++v) x[v] = rng.range(lo, hi); }
};

// a layer of c scattered ids at level 8 under the leaders: with the leaders in one thread / one wave every other wave's (thread's) maximum
// is this level, the threshold drops to it and the candidate list is K + c long
static void mid_layer(Rows& R, int r, Rng& rng, std::vector<char>& used) {
    const int c = std::min(100, (R.V - (int)std::count(used.begin(), used.end(), 1)) / 2);
    for (int v : pick_ids(R.V, c, rng, used)) R.row(r)[v] = 8;
}

static Rows build_rows(int V, int K, int NT, Rng& rng) {
    Rows R;
    R.V = V;
    {   // K + 1 distinct leaders over a random rest
        const int r = R.add("distinct");
        R.fill(r, -48, 20, rng);
        std::vector<char> used(V, 0);
        const std::vector<int> ids = pick_ids(V, K + 1, rng, used);
        for (int i = 0; i <= K; ++i) R.row(r)[ids[i]] = 48 - i;
    }
    {
        const int r = R.add("const");
        for (int v = 0; v < V; ++v) R.row(r)[v] = 8;
    }
    // m ids share the maximum: id 0, id V - 1, the rest scattered
    std::vector<int> ms = {K, K + 1, 64, 65, NT * K, NT * K + 1};
    std::sort(ms.begin(), ms.end());
    ms.erase(std::unique(ms.begin(), ms.end()), ms.end());
    for (int m : ms) {
        if (m > V) continue;
        const int r = R.add("tie" + std::to_string(m));
        R.fill(r, -48, 0, rng);
        std::vector<char> used(V, 0);
        std::vector<int> ids;
        used[0] = 1; ids.push_back(0);
        if (m >= 2) { used[V - 1] = 1; ids.push_back(V - 1); }
        for (int v : pick_ids(V, m - (int)ids.size(), rng, used)) ids.push_back(v);
        for (int v : ids) R.row(r)[v] = 24;
    }
    {   // K - 1 distinct leaders, then a tie group across the K-th place: its lowest id is in, the others are out
        const int r = R.add("straddle");
        R.fill(r, -48, 0, rng);
        std::vector<char> used(V, 0);
        const std::vector<int> lead = pick_ids(V, K - 1, rng, used);
        for (int i = 0; i < K - 1; ++i) R.row(r)[lead[i]] = 47 - i;
        for (int v : pick_ids(V, 5, rng, used)) R.row(r)[v] = 24;
    }
    {   // the K best owned by one thread: thread tid owns the ids 4 (tid + NT j) + e
        const int r = R.add("one-thread");
        R.fill(r, -48, 0, rng);
        std::vector<char> used(V, 0);
        const int nthr = std::min(NT, (V + 3) / 4), tid = rng.range(0, nthr - 1);
        std::vector<int> ids;
        for (int e = 0; e < 4 && (int)ids.size() < K; ++e)
            for (int j = 0; (int)ids.size() < K; ++j) {
                const int v = 4 * (tid + NT * j) + e;
                if (v >= V) break;
                ids.push_back(v); used[v] = 1;
            }
        for (int v : pick_ids(V, K - (int)ids.size(), rng, used)) ids.push_back(v);       // (a thread of a short row owns fewer than K ids)
        for (int i = 0; i < K; ++i) { const int a = rng.range(i, K - 1); std::swap(ids[i], ids[a]); }
        for (int i = 0; i < K; ++i) R.row(r)[ids[i]] = 48 - i;
        mid_layer(R, r, rng, used);
    }
    {   // the K best in K different threads of one wave
        const int r = R.add("one-wave");
        R.fill(r, -48, 0, rng);
        std::vector<char> used(V, 0);
        int w0 = rng.range(0, NT / 64 - 1);
        if (256 * w0 + 4 * K > V) w0 = 0;
        const int avail = std::min(64, (V - 256 * w0 + 3) / 4);           // threads of the wave that own an id
        std::vector<int> ids;
        for (int i = 0; i < K && i < avail; ++i) {
            const int thr = 64 * w0 + (i * 7) % avail;
            int v = 4 * thr + i % 4;
            if (v >= V) v = 4 * thr;
            const int jmax = (V - 1 - v) / (4 * NT);
            v += 4 * NT * rng.range(0, jmax);
            if (!used[v]) { used[v] = 1; ids.push_back(v); }
        }
        for (int v : pick_ids(V, K - (int)ids.size(), rng, used)) ids.push_back(v);
        for (int i = 0; i < K; ++i) R.row(r)[ids[i]] = 48 - i;
        mid_layer(R, r, rng, used);
    }
    {   // the K-th best is the row minimum: x >= threshold admits everything
        const int r = R.add("kth=min");
        for (int v = 0; v < V; ++v) R.row(r)[v] = -48;
        std::vector<char> used(V, 0);
        const std::vector<int> lead = pick_ids(V, K - 1, rng, used);
        for (int i = 0; i < K - 1; ++i) R.row(r)[lead[i]] = 47 - i;
    }
    return R;
}

// bias (shared by the rows) and nsplit slabs whose exact sum is the row; every entry a multiple of 1/8 in [-8, 8]
struct Operands {
    int ns; long long stride;
    std::vector<float> bias, slabs;
};
static Operands split_rows(const Rows& R, int ns, Rng& rng) {
    Operands o;
    const int V = R.V, M = R.M;
    o.ns = ns;
    o.stride = (long long)M * V + ((V & 3) ? 7 : 8);               // larger than M V (a multiple of 4 where the loads are 16 bytes wide)
    std::vector<int> b8(V);
    o.bias.resize(V);
    for (int v = 0; v < V; ++v) { b8[v] = rng.range(-16, 16); o.bias[v] = b8[v] / 8.f; }
    o.slabs.assign((size_t)ns * o.stride, 77.f);                  // (the gaps between the slabs hold a value no sum may pick up)
    for (int r = 0; r < M; ++r)
        for (int v = 0; v < V; ++v) {
            int need = R.x8[(size_t)r * V + v] - b8[v];           // in [-64, 64]
            for (int k = 0; k < ns; ++k) {
                const int rem = ns - 1 - k;
                const int lo = std::max(-64, need - 64 * rem), hi = std::min(64, need + 64 * rem);
                const int p = rng.range(lo, hi);
                o.slabs[(size_t)k * o.stride + (size_t)r * V + v] = p / 8.f;
                need -= p;
            }
        }
    return o;
}

struct VocabCase {
    int V, K, mode, gs = 0, gt = 0;
    Rows R;
    // verb forcing (verbs empty: none)
    int L = 3, rpi = 1, n_verbs = 0;
    std::vector<float> verbs;
    std::vector<int> slot, vt_ptr, vt_ids;
    std::vector<int> forced;
    std::string tag;
};

struct VArgs {
    const float* logits; int ns; long long stride; const float* bias; int M, V, mode; float* top_v; int* top_i; float* full; long long full_stride;
    const int* forced; const float* verbs; const int* slot; int rpi, L, gt; const int* vt_ptr; const int* vt_ids; int n_verbs; GateLogitArgs gate; int* bad; int gs;
};
template <int K, int NT> static void launch_vocab_inst(const VArgs& a, const VocabLaunch& vl) {
    hipLaunchKernelGGL((k_vocab<K, NT>), dim3(a.M), dim3(NT), vl.lds_bytes, 0, a.logits, a.ns, a.stride, a.bias, a.M, a.V, a.mode, a.top_v, a.top_i, a.full,
                       a.full_stride, a.forced, (uint64_t)0, (uint32_t)0, a.verbs, a.slot, a.rpi, a.L, a.gt, a.vt_ptr, a.vt_ids, a.n_verbs, vl.lds_row, a.gate, a.bad, a.gs);
}
template <int K> static void launch_vocab_k(const VArgs& a, const VocabLaunch& vl) {
    if (vl.nt == 512) launch_vocab_inst<K, 512>(a, vl); else launch_vocab_inst<K, 256>(a, vl);
}
static void launch_vocab_any(int K, const VArgs& a) {
    const VocabLaunch vl = vocab_launch_rule(a.V);                // the library's own rule (kernels.h)
    switch (K) {
        case 1: launch_vocab_k<1>(a, vl); break;   case 2: launch_vocab_k<2>(a, vl); break;
        case 3: launch_vocab_k<3>(a, vl); break;   case 4: launch_vocab_k<4>(a, vl); break;
        case 5: launch_vocab_k<5>(a, vl); break;   case 6: launch_vocab_k<6>(a, vl); break;
        case 7: launch_vocab_k<7>(a, vl); break;   default: launch_vocab_k<8>(a, vl); break;
    }
}

static std::map<std::string, int> g_cross;

// the candidate regime a TOPK row (K > 1) takes, from the row alone
static const char* row_regime(const int* x, int V, int K, int NT) {
    const int NW = NT / 64;
    std::vector<int> best;
    if (NW >= K) {
        best.assign(NW, INT32_MIN);
        for (int v = 0; v < V; ++v) { int& m = best[((v >> 2) % NT) / 64]; m = std::max(m, x[v]); }
    } else {
        best.assign(NT, INT32_MIN);
        for (int v = 0; v < V; ++v) { int& m = best[(v >> 2) % NT]; m = std::max(m, x[v]); }
    }
    std::sort(best.begin(), best.end(), [](int a, int b) { return a > b; });
    const int tau = best[K - 1];                                   // INT32_MIN: fewer owners than K, everything is a candidate
    long long nc = 0;
    for (int v = 0; v < V; ++v) nc += x[v] >= tau;
    return nc <= 64 ? "wave0" : (nc <= (long long)NT * K ? "middle" : "full-row");
}

static double lse64(const int* x, int V) {
    int mx = x[0];
    for (int v = 1; v < V; ++v) mx = std::max(mx, x[v]);
    double s = 0.0;
    for (int v = 0; v < V; ++v) s += std::exp((x[v] - mx) / 8.0);
    return mx / 8.0 + std::log(s);
}
// ids by (logit descending, id ascending): the first n
static std::vector<int> best_ids(const int* x, int V, int n) {
    std::vector<int> ids(V);
    for (int v = 0; v < V; ++v) ids[v] = v;
    std::partial_sort(ids.begin(), ids.begin() + n, ids.end(), [&](int a, int b) { return x[a] > x[b] || (x[a] == x[b] && a < b); });
    ids.resize(n);
    return ids;
}

static void run_vocab(VocabCase& c, int ns, uint32_t seed) {
    Rng rng(seed);
    Rows& R = c.R;
    const int V = c.V, K = c.K, M = R.M;
    const VocabLaunch vl = vocab_launch_rule(V);
    const int NT = vl.nt, KU = NT == 512 ? 2 : 4;
    const Operands op = split_rows(R, ns, rng);
    float* d_logits = to_dev(op.slabs);
    float* d_bias = to_dev(op.bias);
    const bool has_verbs = !c.verbs.empty();
    float* d_verbs = has_verbs ? to_dev(c.verbs) : nullptr;
    int* d_slot = has_verbs ? to_dev(c.slot) : nullptr;
    int* d_vt_ptr = c.vt_ptr.empty() ? nullptr : to_dev(c.vt_ptr);
    int* d_vt_ids = c.vt_ptr.empty() ? nullptr : to_dev(c.vt_ids);
    int* d_forced = c.forced.empty() ? nullptr : to_dev(c.forced);
    const long long full_stride = V + 5;

    // gate block: A columns, 2 slabs; w_g multiples of 1/8 in [-1, 1], the other operands on the [-8, 8] grid
    const int A = 70, gns = 2;
    const long long gstride = (long long)M * A + 3;
    std::vector<float> ga((size_t)gns * gstride), hA((size_t)M * A), w_g(A), zsum(M);
    for (float& x : ga) x = rng.range(-64, 64) / 8.f;
    for (float& x : hA) x = rng.range(-64, 64) / 8.f;
    for (float& x : w_g) x = rng.range(-8, 8) / 8.f;
    for (float& x : zsum) x = rng.range(-64, 64) / 8.f;
    float *d_ga = to_dev(ga), *d_hA = to_dev(hA), *d_wg = to_dev(w_g), *d_zsum = to_dev(zsum);

    const size_t ntop = c.mode == VM_TOPK && c.gs == 0 ? (size_t)M * K : (size_t)M;
    OutBuf<float> top_v("top_v", ntop, 12345.f), full("full_out", c.mode == VM_FULL ? (size_t)M * full_stride : 1, 12345.f), lg("lg", (size_t)M * 2, 12345.f);
    OutBuf<int> top_i("top_i", ntop, -777), bad("bad", 1, -777);

    // per-row verb and mode
    std::vector<int> verb(M, -1);
    if (has_verbs)
        for (int r = 0; r < M; ++r) {
            const float vf = c.verbs[(size_t)(r / c.rpi) * c.L + c.slot[r]];
            verb[r] = vf != -1.f ? (int)vf : -1;
        }

    std::vector<double> lse_row(M);
    for (int r = 0; r < M; ++r) lse_row[r] = lse64(R.row(r), V);

    for (int gate_on = 0; gate_on < 2; ++gate_on) {
        top_v.refill(12345.f); full.refill(12345.f); lg.refill(12345.f); top_i.refill(-777); bad.refill(-777);
        int nbad = 0;
        std::map<std::string, int> regimes;
        for (int r = 0; r < M; ++r) {
            const int* x = R.row(r);
            int mode = c.mode, srow = r;
            if (c.gs > 0) { if (r % c.gs == 0) mode = VM_TOPK; else srow = r - r / c.gs - 1; }
            if (verb[r] != -1) {
                // step_v as oracle/vsr_oracle.py states it (_force_verbs): one word at log-prob 0, the rest -1e6
                int pick = 0;
                if (c.gt) {
                    pick = verb[r];
                    if (pick < 0 || pick >= V) { ++nbad; pick = 0; }
                } else if (verb[r] >= 0 && verb[r] < c.n_verbs && c.vt_ptr[verb[r] + 1] > c.vt_ptr[verb[r]]) {
                    pick = -1;
                    for (int q = c.vt_ptr[verb[r]]; q < c.vt_ptr[verb[r] + 1]; ++q)
                        if (pick < 0 || x[c.vt_ids[q]] > x[pick]) pick = c.vt_ids[q];      // strict '>': the first maximum in list order wins
                }
                if (mode == VM_FULL) {
                    for (int v = 0; v < V; ++v) full.set((size_t)r * full_stride + v, v == pick ? 0.f : -1e6f);
                } else if (mode == VM_TOPK && c.gs == 0) {
                    for (int q = 0; q < K; ++q) {
                        top_v.set((size_t)r * K + q, q == 0 ? 0.f : -1e6f);
                        top_i.set((size_t)r * K + q, q == 0 ? pick : (q - 1 < pick ? q - 1 : q));
                    }
                } else {
                    const int id = mode == VM_FORCED ? c.forced[srow] : pick;
                    top_v.set(r, id == pick ? 0.f : -1e6f);
                    top_i.set(r, id);
                }
                regimes["verb"]++;
                continue;
            }
            const double lse = lse_row[r];
            if (mode == VM_FULL) {
                for (int v = 0; v < V; ++v) full.set_approx((size_t)r * full_stride + v, x[v] / 8.0 - lse);
            } else if (mode == VM_FORCED) {
                const int id = c.forced[srow];
                top_v.set_approx(r, x[id] / 8.0 - lse);
                top_i.set(r, id);
            } else {
                const int kk = c.gs > 0 ? 1 : K;                  // (a baseline row of a gs launch: the arg-max, K = 1)
                const std::vector<int> ids = best_ids(x, V, kk);
                for (int q = 0; q < kk; ++q) {
                    top_v.set_approx((size_t)r * kk + q, x[ids[q]] / 8.0 - lse);
                    top_i.set((size_t)r * kk + q, ids[q]);
                }
                if (kk > 1) regimes[row_regime(x, V, K, NT)]++;
            }
        }
        bad.set(0, nbad);
        // gate logits: log_softmax([w_g . tanh(ga + hA), zsum]) in fp64; verb rows [-1e3, 0]
        GateLogitArgs g{};
        if (gate_on) {
            g.ga = d_ga; g.nsplit = gns; g.stride = gstride; g.hA = d_hA; g.w_g = d_wg; g.zsum = d_zsum; g.verbs = d_verbs; g.slot = d_slot;
            g.rpi = c.rpi; g.L = c.L; g.M = M; g.A = A; g.lg = lg.ptr(); g.lg_stride = 2;
            for (int r = 0; r < M; ++r) {
                if (verb[r] != -1) { lg.set((size_t)r * 2, -1e3f); lg.set((size_t)r * 2 + 1, 0.f); continue; }
                double a = 0.0;
                for (int k = 0; k < A; ++k) a += (double)w_g[k] * std::tanh((double)ga[(size_t)r * A + k] + (double)ga[gstride + (size_t)r * A + k] + (double)hA[(size_t)r * A + k]);
                const double b = zsum[r], mx = std::max(a, b), l = mx + std::log(std::exp(a - mx) + std::exp(b - mx));
                lg.set_approx((size_t)r * 2, a - l);
                lg.set_approx((size_t)r * 2 + 1, b - l);
            }
        }
        VArgs a{d_logits, ns, op.stride, d_bias, M, V, c.mode, top_v.ptr(), top_i.ptr(), c.mode == VM_FULL ? full.ptr() : nullptr, full_stride, d_forced,
                d_verbs, d_slot, c.rpi, c.L, c.gt, d_vt_ptr, d_vt_ids, c.n_verbs, g, bad.ptr(), c.gs};
        const int zero = 0;
        CK(hipMemcpy(bad.ptr(), &zero, sizeof(int), hipMemcpyHostToDevice));
        launch_vocab_any(K, a);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());

        const double before = g_maxerr;
        g_maxerr = 0.0;
        const int nwrong = top_v.check() + top_i.check() + full.check() + lg.check() + bad.check();
        const double err = g_maxerr;
        g_maxerr = std::max(before, err);

        const char* tau = (c.mode == VM_TOPK && c.gs == 0 && K > 1) ? (NT / 64 >= K ? "wave-max" : "block-rounds") : "none";
        char head[256];
        snprintf(head, sizeof head, "NT=%d %s %s", NT, (V & 3) ? "scalar" : "vec", vl.lds_row ? "lds" : "global");
        std::string reg;
        for (auto& kv : regimes) {
            reg += (reg.empty() ? "" : ",") + kv.first + "x" + std::to_string(kv.second);
            if (kv.first != "verb") g_cross[std::string(head) + " tau=" + tau + " regime=" + kv.first] += kv.second;
        }
        g_cross[std::string(head) + " mode=" + c.tag] += 1;
        if (ns > KU) g_cross["NT=" + std::to_string(NT) + ((V & 3) ? " scalar" : " vec") + " slab tail (nsplit > " + std::to_string(KU) + ")"] += 1;
        char line[512];
        snprintf(line, sizeof line, "vocab %-14s V=%-5d K=%d nsplit=%d gate=%d M=%-2d %s tau=%s rows[%s] max|dlogp|=%.2e", c.tag.c_str(), V, K, ns, gate_on, M, head, tau,
                 reg.c_str(), err);
        finish_case(line, nwrong);
    }
    for (void* p : {(void*)d_logits, (void*)d_bias, (void*)d_verbs, (void*)d_slot, (void*)d_vt_ptr, (void*)d_vt_ids, (void*)d_forced, (void*)d_ga, (void*)d_hA,
                    (void*)d_wg, (void*)d_zsum})
        if (p) CK(hipFree(p));
}

// the verb launches: 10 rows of 5 images (rpi = 2), L = 3 slots
static VocabCase verb_case(int V, int K, int mode, int gt, Rng& rng) {
    VocabCase c;
    c.V = V; c.K = K; c.mode = mode; c.gt = gt; c.rpi = 2; c.L = 3;
    c.tag = std::string(mode == VM_TOPK ? "topk" : mode == VM_FULL ? "full" : "forced") + (gt ? "+verb-gt" : "+verb-tab");
    c.R.V = V;
    for (int r = 0; r < 10; ++r) { c.R.add("verb"); c.R.fill(r, -48, 20, rng); }
    c.verbs.assign(5 * 3, -1.f);
    c.slot.resize(10);
    // row r of image r / 2 reads slot r % 2 * 2 (slots 0 and L - 1), except the last image's rows (slot 1: no verb there)
    for (int r = 0; r < 10; ++r) c.slot[r] = r < 8 ? (r % 2) * 2 : 1;
    auto verb_of = [&](int r) -> float& { return c.verbs[(size_t)(r / 2) * 3 + c.slot[r]]; };
    if (gt) {
        verb_of(0) = (float)(V - 1);     // in range
        verb_of(1) = -2.f;               // < 0: counted, word 0
        verb_of(2) = (float)(V + 3);     // >= V: counted, word 0
        verb_of(3) = 0.f;
        verb_of(4) = (float)(V / 2);
        // rows 5 .. 9: entry -1, the normal path
    } else {
        // verb 0: one id; verb 1: several ids whose two best logits tie (the first in list order, which is the HIGHER id, wins); verb 2: empty
        c.n_verbs = 3;
        c.vt_ptr = {0, 1, 5, 5};
        c.vt_ids = {V - 1, 17, 30, 3, 5};
        verb_of(0) = 0.f;
        verb_of(1) = 1.f;
        int* x = c.R.row(1);
        x[17] = -8; x[30] = 16; x[3] = 16; x[5] = 0;
        verb_of(2) = 2.f;                // empty list: word 0
        verb_of(3) = 3.f;                // >= n_verbs: word 0
        verb_of(4) = 1.f;                // the list again on a random row (no tie designed)
        verb_of(5) = -2.f;               // negative and not -1: word 0, nothing counted without gt
    }
    if (mode == VM_FORCED) {
        c.forced.resize(10);
        for (int r = 0; r < 10; ++r) c.forced[r] = rng.range(0, V - 1);
        c.forced[0] = V - 1;                 // the forced id is the verb's word on row 0 (log-prob 0), another word elsewhere (-1e6)
    }
    return c;
}

static void group_vocab() {
    const int Vs[] = {37, 256, 1000, 4095, 4096, 4501, 12288, 12289, 12292};
    const int NSs[] = {1, 2, 3, 4, 5, 8};
    uint32_t seed = 1;
    for (int V : Vs) {
        const int NT = vocab_launch_rule(V).nt;
        for (int K = 1; K <= 8; ++K)
            for (int ns : NSs) {
                Rng rng(seed++);
                VocabCase c;
                c.V = V; c.K = K; c.mode = VM_TOPK; c.tag = "topk";
                c.R = build_rows(V, K, NT, rng);
                run_vocab(c, ns, seed++);
            }
        for (int ns : NSs) {                                       // VM_FULL: the whole row, rows built as for K = 5
            Rng rng(seed++);
            VocabCase c;
            c.V = V; c.K = 1; c.mode = VM_FULL; c.tag = "full";
            c.R = build_rows(V, 5, NT, rng);
            run_vocab(c, ns, seed++);
        }
        for (int ns : {1, 5}) {                                    // VM_FORCED: id 0, id V - 1, the arg-max, random ids
            Rng rng(seed++);
            VocabCase c;
            c.V = V; c.K = 1; c.mode = VM_FORCED; c.tag = "forced";
            c.R = build_rows(V, 5, NT, rng);
            c.forced.resize(c.R.M);
            for (int r = 0; r < c.R.M; ++r) c.forced[r] = rng.range(0, V - 1);
            c.forced[0] = 0; c.forced[1] = V - 1; c.forced[2] = best_ids(c.R.row(2), V, 1)[0];
            run_vocab(c, ns, seed++);
        }
        for (int ns : {2, 8}) {                                    // gs = 4: rows 0, 4, 8 are greedy baseline rows, the others read forced[sample_row]
            Rng rng(seed++);
            VocabCase c;
            c.V = V; c.K = 1; c.mode = VM_FORCED; c.gs = 4; c.rpi = 4; c.tag = "forced-gs4";
            c.R = build_rows(V, 5, NT, rng);
            while (c.R.M < 12) { const int r = c.R.add("random"); c.R.fill(r, -48, 48, rng); }
            c.R.M = 12; c.R.x8.resize((size_t)12 * V);
            { int* x = c.R.row(4); for (int v = 0; v < V; ++v) x[v] = std::min(x[v], 24); x[V - 1] = 24; x[V / 2] = 24; }   // a baseline row whose maximum ties
            c.forced.resize(9);
            for (int& f : c.forced) f = rng.range(0, V - 1);
            c.forced[0] = 0; c.forced[1] = V - 1;
            run_vocab(c, ns, seed++);
        }
        for (int gt = 0; gt < 2; ++gt) {
            const int modes[][2] = {{VM_TOPK, 1}, {VM_TOPK, 5}, {VM_TOPK, 8}, {VM_FULL, 1}, {VM_FORCED, 1}};
            for (auto& mk : modes) {
                Rng rng(seed++);
                VocabCase c = verb_case(V, mk[1], mk[0], gt, rng);
                run_vocab(c, 3, seed++);
            }
        }
    }
    printf("k_vocab crossings reached (rows per regime, launches per mode / slab tail):\n");
    for (auto& kv : g_cross) printf("  %-70s %d\n", kv.first.c_str(), kv.second);
    // what the inputs must have reached, by their construction
    auto reached = [&](std::initializer_list<const char*> words) {
        for (auto& kv : g_cross) {
            bool all = true;
            for (const char* w : words) all = all && kv.first.find(w) != std::string::npos;
            if (all && kv.second > 0) return true;
        }
        return false;
    };
    int missing = 0;
    missing += !reached({"regime=middle"});
    missing += !reached({"NT=512", "regime=middle"});
    missing += !reached({"NT=256", "tau=wave-max", "regime=middle"});
    missing += !reached({"NT=256", "tau=block-rounds", "regime=middle"});
    missing += !reached({"NT=256", "tau=block-rounds", "regime=wave0"});
    missing += !reached({"regime=full-row"});
    missing += !reached({"NT=256", "slab tail"});
    missing += !reached({"NT=512", "slab tail"});
    missing += !reached({"global", "scalar", "regime="});
    missing += !reached({"global", "vec", "regime="});
    for (const char* nt : {"NT=256", "NT=512"})
        for (const char* ld : {"scalar", "vec"})
            missing += !reached({nt, ld, "lds", "regime="});
    char line[128];
    snprintf(line, sizeof line, "vocab crossings: %d required crossings missing", missing);
    finish_case(line, missing);
}

// =============================================================================================== k_select_beam<K>
template <int K> static void launch_beam_k(const SelBeamArgs& a) { hipLaunchKernelGGL(k_select_beam<K>, dim3(a.B), dim3(64), 0, 0, a); }
static void launch_beam(int K, const SelBeamArgs& a) {
    switch (K) {
        case 1: launch_beam_k<1>(a); break;   case 2: launch_beam_k<2>(a); break;   case 3: launch_beam_k<3>(a); break;   case 4: launch_beam_k<4>(a); break;
        case 5: launch_beam_k<5>(a); break;   case 6: launch_beam_k<6>(a); break;   case 7: launch_beam_k<7>(a); break;   default: launch_beam_k<8>(a); break;
    }
}

enum BeamStructure { BS_RANDOM, BS_IDENTICAL, BS_BOUNDARY_TIE, BS_FROZEN_MASK, BS_FROZEN_EOS, BS_SLOT_EDGES, BS_COUNT };
static const char* const BS_NAME[] = {"random", "identical-beams", "boundary-tie", "frozen-by-mask", "frozen-by-eos", "slot-edges"};

struct BeamIn {
    std::vector<float> top_v, lg, seq_in, mask_in;
    std::vector<int> top_i, slot, word_prev, gate_prev;
};
struct BeamCand { float val; long long flat; int j, w, g, k; float mw, mg, lw, lgv; };

// the candidates of image b in flat order, then a stable sort by value: (value descending, flat (beam, word, gate) index ascending)
static std::vector<BeamCand> beam_reference(const BeamIn& in, int b, int K, int t, int cb, int beam, int L, int eos_w, int eos_g) {
    std::vector<BeamCand> c;
    for (int j = 0; j < cb; ++j)
        for (int i = 0; i < K; ++i)
            for (int g = 0; g < 2; ++g) {
                const int row = b * cb + j;
                float mw = 1.f, mg = 1.f;
                if (t > 0) {
                    mw = in.mask_in[(b * beam + j) * 2] * (in.word_prev[row] != eos_w ? 1.f : 0.f);
                    mg = in.mask_in[(b * beam + j) * 2 + 1] * (in.gate_prev[row] != eos_g ? 1.f : 0.f);
                }
                const float seq = t > 0 ? in.seq_in[b * beam + j] : 0.f;
                const bool alive = mw + mg > 0.f;
                const float lw = in.top_v[(size_t)row * K + i], lgv = in.lg[row * 2 + g];
                BeamCand x;
                x.j = j; x.g = g; x.mw = mw; x.mg = mg; x.lgv = lgv;
                if (alive) { x.w = in.top_i[(size_t)row * K + i]; x.val = seq + (lw + lgv); x.lw = lw; }
                else { x.w = i; x.val = i == 0 ? seq : -999.f; x.lw = 0.f; }       // frozen: word 0 keeps the score, the others get -999
                x.k = std::min(std::max(in.slot[row] + g, 0), L - 1);
                x.flat = ((long long)j * 0x40000000LL + x.w) * 2 + g;
                c.push_back(x);
            }
    std::stable_sort(c.begin(), c.end(), [](const BeamCand& a, const BeamCand& b) { return a.val > b.val || (a.val == b.val && a.flat < b.flat); });
    return c;
}

static void run_beam(int K, int t, int st, uint32_t seed0) {
    const int B = 3, beam = K, cb = t > 0 ? beam : 1, L = 4, T = 4, rows = B * cb, eos_w = 7, eos_g = 2;
    BeamIn in;
    bool tie_ok = st != BS_BOUNDARY_TIE;
    for (int attempt = 0; attempt < 200; ++attempt) {              // (host only: BS_BOUNDARY_TIE draws until every image has the tie it is about)
        Rng rng(seed0 * 1000u + attempt);
        in = BeamIn{};
        in.top_v.resize((size_t)rows * K); in.top_i.resize((size_t)rows * K); in.lg.resize(rows * 2); in.slot.resize(rows);
        in.word_prev.resize(rows); in.gate_prev.resize(rows); in.seq_in.resize(B * beam); in.mask_in.assign(B * beam * 2, 1.f);
        const bool coarse = st == BS_BOUNDARY_TIE;
        for (int r = 0; r < rows; ++r) {
            std::vector<char> used(1000, 0);
            const std::vector<int> ids = pick_ids(1000, K, rng, used);     // distinct within a row; the word eos_w may be among them
            for (int i = 0; i < K; ++i) {
                in.top_i[(size_t)r * K + i] = ids[i];
                in.top_v[(size_t)r * K + i] = coarse ? -(float)rng.range(1, 3) : rng.range(-64, 0) / 8.f;
            }
            in.lg[r * 2] = coarse ? -(float)rng.range(1, 2) : rng.range(-64, 0) / 8.f;
            in.lg[r * 2 + 1] = coarse ? -(float)rng.range(1, 2) : rng.range(-64, 0) / 8.f;
            in.slot[r] = st == BS_SLOT_EDGES ? (r % 2 ? L - 1 : 0) : rng.range(0, L - 1);
            in.word_prev[r] = rng.range(8, 999);
            in.gate_prev[r] = rng.range(0, 1);
        }
        for (int i = 0; i < B * beam; ++i) in.seq_in[i] = coarse ? -(float)rng.range(4, 5) : rng.range(-512, 0) / 8.f;
        if (st == BS_IDENTICAL)                                    // every beam of an image carries beam 0's numbers: every candidate ties across beams
            for (int b = 0; b < B; ++b)
                for (int j = 1; j < cb; ++j) {
                    const int r0 = b * cb, r = b * cb + j;
                    for (int i = 0; i < K; ++i) { in.top_v[(size_t)r * K + i] = in.top_v[(size_t)r0 * K + i]; in.top_i[(size_t)r * K + i] = in.top_i[(size_t)r0 * K + i]; }
                    in.lg[r * 2] = in.lg[r0 * 2]; in.lg[r * 2 + 1] = in.lg[r0 * 2 + 1];
                    in.seq_in[b * beam + j] = in.seq_in[b * beam];
                }
        if (st == BS_FROZEN_MASK || st == BS_FROZEN_EOS)           // beam j: j % 4 = 0 alive, 1 word stream frozen, 2 gate stream frozen, 3 both (a frozen hypothesis)
            for (int b = 0; b < B; ++b)
                for (int j = 0; j < cb; ++j) {
                    const int f = (j + b) % 4, r = b * cb + j;
                    // image 2 mixes the two ways of freezing a stream
                    const bool by_mask = st == BS_FROZEN_MASK ? b != 2 : b == 2;
                    if (f & 1) { if (by_mask) in.mask_in[(b * beam + j) * 2] = 0.f; else in.word_prev[r] = eos_w; }
                    if (f & 2) { if (by_mask) in.mask_in[(b * beam + j) * 2 + 1] = 0.f; else in.gate_prev[r] = eos_g; }
                    // a frozen hypothesis carries the best score there is: its word 0 survives (both gates tie), its -999 siblings must not
                    if (f == 3) in.seq_in[b * beam + j] = 0.f;
                }
        if (tie_ok) break;
        tie_ok = true;
        for (int b = 0; b < B; ++b) {
            const std::vector<BeamCand> c = beam_reference(in, b, K, t, cb, beam, L, eos_w, eos_g);
            tie_ok = tie_ok && (int)c.size() > beam && c[beam - 1].val == c[beam].val;
        }
        if (tie_ok) break;
    }

    float *d_top_v = to_dev(in.top_v), *d_lg = to_dev(in.lg), *d_seq_in = to_dev(in.seq_in), *d_mask_in = to_dev(in.mask_in);
    int *d_top_i = to_dev(in.top_i), *d_slot = to_dev(in.slot), *d_wp = to_dev(in.word_prev), *d_gp = to_dev(in.gate_prev);
    const size_t nb = (size_t)B * beam, nh = (size_t)T * B * beam;
    OutBuf<float> seq_out("seq_out", nb, 12345.f), mask_out("mask_out", nb * 2, 12345.f), hist_lpw("hist_lpw", nh, 12345.f), hist_lpg("hist_lpg", nh, 12345.f);
    OutBuf<int> word_next("word_next", nb, -777), gate_next("gate_next", nb, -777), slot_next("slot_next", nb, -777), parent_row("parent_row", nb, -777),
        hist_parent("hist_parent", nh, -777), hist_word("hist_word", nh, -777), hist_gate("hist_gate", nh, -777);
    for (int b = 0; b < B; ++b) {
        const std::vector<BeamCand> c = beam_reference(in, b, K, t, cb, beam, L, eos_w, eos_g);
        for (int q = 0; q < beam; ++q) {
            const BeamCand& x = c[q];
            const size_t o = (size_t)b * beam + q, h = (size_t)t * B * beam + o;
            seq_out.set(o, x.val); word_next.set(o, x.w); gate_next.set(o, x.g); parent_row.set(o, b * cb + x.j); slot_next.set(o, x.k);
            mask_out.set(o * 2, x.mw); mask_out.set(o * 2 + 1, x.mg);
            hist_parent.set(h, x.j); hist_word.set(h, x.w); hist_gate.set(h, x.g);
            hist_lpw.set(h, x.lw * x.mw); hist_lpg.set(h, x.lgv * x.mg);      // zeroed once the stream saw EOS
        }
    }
    SelBeamArgs a{};
    a.t = t; a.cb = cb; a.beam = beam; a.L = L; a.eos_w = eos_w; a.eos_g = eos_g;
    a.top_v = d_top_v; a.top_i = d_top_i; a.lg = d_lg; a.slot = d_slot; a.word_prev = d_wp; a.gate_prev = d_gp;
    a.seq_in = d_seq_in; a.seq_out = seq_out.ptr(); a.mask_in = d_mask_in; a.mask_out = mask_out.ptr();
    a.word_next = word_next.ptr(); a.gate_next = gate_next.ptr(); a.slot_next = slot_next.ptr(); a.parent_row = parent_row.ptr();
    a.hist_parent = hist_parent.ptr(); a.hist_word = hist_word.ptr(); a.hist_gate = hist_gate.ptr(); a.hist_lpw = hist_lpw.ptr(); a.hist_lpg = hist_lpg.ptr(); a.B = B;
    launch_beam(K, a);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    int nwrong = seq_out.check() + mask_out.check() + hist_lpw.check() + hist_lpg.check() + word_next.check() + gate_next.check() + slot_next.check() +
                 parent_row.check() + hist_parent.check() + hist_word.check() + hist_gate.check();
    if (!tie_ok) { printf("    no draw gave every image a tie between the last survivor and the first loser\n"); ++nwrong; }
    char line[256];
    snprintf(line, sizeof line, "beam K=%d t=%d cb=%d B=%d %-16s", K, t, cb, B, BS_NAME[st]);
    finish_case(line, nwrong);
    for (void* p : {(void*)d_top_v, (void*)d_lg, (void*)d_seq_in, (void*)d_mask_in, (void*)d_top_i, (void*)d_slot, (void*)d_wp, (void*)d_gp}) CK(hipFree(p));
}

static void group_beam() {
    uint32_t seed = 5000;
    for (int K = 1; K <= 8; ++K)
        for (int t : {0, 2})
            for (int st = 0; st < BS_COUNT; ++st) {
                if (t == 0 && (st == BS_FROZEN_MASK || st == BS_FROZEN_EOS || st == BS_IDENTICAL)) continue;      // (nothing is frozen and there is one beam at t = 0)
                run_beam(K, t, st, seed++);
            }
}

// =============================================================================================== k_backtrack
static void run_backtrack(int T, int beam, int out_size, bool ties, bool with_lp, uint32_t seed) {
    Rng rng(seed);
    const int B = 3;
    const size_t nh = (size_t)T * B * beam;
    std::vector<float> seq(B * beam), lpw(nh), lpg(nh);
    std::vector<int> par(nh), wrd(nh), gat(nh);
    for (size_t i = 0; i < nh; ++i) {
        par[i] = rng.range(0, beam - 1); wrd[i] = rng.range(0, 9999); gat[i] = rng.range(0, 1);
        lpw[i] = rng.range(-64, 0) / 8.f; lpg[i] = rng.range(-64, 0) / 8.f;
    }
    for (int b = 0; b < B; ++b) {
        std::vector<char> used(513, 0);
        if (ties) for (int q = 0; q < beam; ++q) seq[b * beam + q] = -(float)rng.range(0, 2);           // three levels: ties at beam >= 4, likely below
        else { const std::vector<int> v = pick_ids(513, beam, rng, used); for (int q = 0; q < beam; ++q) seq[b * beam + q] = -v[q] / 8.f; }
    }
    if (ties && beam > 1) seq[1] = seq[0];                                                             // (image 0 always has one)
    float *d_seq = to_dev(seq), *d_lpw = to_dev(lpw), *d_lpg = to_dev(lpg);
    int *d_par = to_dev(par), *d_wrd = to_dev(wrd), *d_gat = to_dev(gat);
    const size_t no = (size_t)B * out_size * T;
    OutBuf<int64_t> words("words", no, -777), gates("gates", no, -777);
    OutBuf<float> lp_w("lp_w", no, 12345.f), lp_g("lp_g", no, 12345.f), scores("scores", (size_t)B * out_size, 12345.f);
    for (int b = 0; b < B; ++b) {
        std::vector<int> order(beam);
        for (int q = 0; q < beam; ++q) order[q] = q;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return seq[b * beam + x] > seq[b * beam + y]; });      // on ties the lower slot first
        for (int o = 0; o < out_size; ++o) {
            int q = order[o];
            const size_t dst = ((size_t)b * out_size + o) * T;
            if (with_lp) {
                scores.set((size_t)b * out_size + o, seq[b * beam + q]);
                for (int t = 0; t < T; ++t) {       // the per-slot log-probs follow the final slot, not the ancestry
                    const size_t h = (size_t)t * B * beam + b * beam + order[o];
                    lp_w.set(dst + t, lpw[h]); lp_g.set(dst + t, lpg[h]);
                }
            }
            for (int t = T - 1; t >= 0; --t) {
                const size_t h = (size_t)t * B * beam + b * beam + q;
                words.set(dst + t, wrd[h]); gates.set(dst + t, gat[h]);
                q = par[h];
            }
        }
    }
    hipLaunchKernelGGL(k_backtrack, dim3(B), dim3(64), (size_t)3 * T * beam * sizeof(int), 0, T, B, beam, out_size, d_seq, d_par, d_wrd, d_gat, d_lpw, d_lpg,
                       words.ptr(), gates.ptr(), with_lp ? lp_w.ptr() : nullptr, with_lp ? lp_g.ptr() : nullptr, with_lp ? scores.ptr() : nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    const int nwrong = words.check() + gates.check() + lp_w.check() + lp_g.check() + scores.check();
    char line[256];
    snprintf(line, sizeof line, "backtrack T=%-2d beam=%d out_size=%d seq=%-8s lp/scores=%s", T, beam, out_size, ties ? "ties" : "distinct", with_lp ? "written" : "null");
    finish_case(line, nwrong);
    for (void* p : {(void*)d_seq, (void*)d_lpw, (void*)d_lpg, (void*)d_par, (void*)d_wrd, (void*)d_gat}) CK(hipFree(p));
}

static void group_backtrack() {
    uint32_t seed = 9000;
    for (int T : {1, 5, 20})
        for (int beam : {1, 5, 8})
            for (int out_size = 1; out_size <= beam; out_size += std::max(beam - 1, 1))      // 1 and beam
                for (int ties = 0; ties < 2; ++ties)
                    for (int with_lp = 0; with_lp < 2; ++with_lp) run_backtrack(T, beam, out_size, ties != 0, with_lp != 0, seed++);
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    if (what != "vocab" && what != "beam" && what != "backtrack" && what != "all") {
        printf("usage: select_check [vocab | beam | backtrack | all]\n");
        return 2;
    }
    int ndev = 0;
    CK(hipGetDeviceCount(&ndev));
    if (what == "vocab" || what == "all") group_vocab();
    if (what == "beam" || what == "all") group_beam();
    if (what == "backtrack" || what == "all") group_backtrack();
    printf("largest |log-prob - fp64 reference| of the run: %.3e (bound %.1e)\n", g_maxerr, TOL);
    printf("%d of %d cases failed\n", g_failed, g_cases);
    return g_failed ? 1 : 0;
}
