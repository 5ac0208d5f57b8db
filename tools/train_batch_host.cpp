// The training-batch logic of csrc/train_batch_logic.h on the CPU, as the kernels of csrc/train_batch_kernels.h run it: the scans per job
// slot, the exclusive scan of the row and item counts in slot order, the compacted tables.  Reads cases from stdin, prints one line per
// case (tests/test_train_batch_logic.py compares them with the numpy yardsticks of vsrcap/trainbatch.py).
// Build: python vsr-guided-cic_amd/build.py --tool
//
//   input   n_cases, then per case:  N L Lg MV MS N_sink n_verbs max_items has_gt has_idx
//           control_verb (N MV)  det_seqs_v (N L MV)  det_seqs_sr (N L MS)  [gt_seqs_v (N Lg MV)  gt_seqs_sr (N Lg MS)]  [idx_list (N L)]
//   output  verbs (N MV)  det_roles (N MV, 10)  gt_roles (N MV, 10)  item_gather (Q, N_sink)  tr_locs (Q, N_sink)  gt_locs (Q, N_sink)
//           item_key (Q, 3)  counts (4)  status (N)      with Q = max_items, or N MV 10 when max_items is 0
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../vsr-guided-cic_amd/csrc/train_batch_logic.h"

using namespace vsr_rank;

static bool read_ints(std::vector<int32_t>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i) {
        long long x;
        if (scanf("%lld", &x) != 1) return false;
        v[i] = (int32_t)x;
    }
    return true;
}

int main() {
    int n_cases = 0;
    if (scanf("%d", &n_cases) != 1) return 2;
    for (int c = 0; c < n_cases; ++c) {
        int N, L, Lg, MV, MS, N_sink, max_items, has_gt, has_idx;
        long long n_verbs;
        if (scanf("%d %d %d %d %d %d %lld %d %d %d", &N, &L, &Lg, &MV, &MS, &N_sink, &n_verbs, &max_items, &has_gt, &has_idx) != 10) return 2;
        if (N <= 0 || max_items < 0 || !tb_limits_ok(L, has_gt ? Lg : 1, MV, MS, N_sink)) {
            fprintf(stderr, "case %d: outside the limits\n", c);
            return 3;
        }
        const int S = N * MV, Qcap = max_items > 0 ? max_items : S * RANK_L;
        std::vector<int32_t> cv, dv, dsr, gv, gsr, idx;
        if (!read_ints(cv, (size_t)S) || !read_ints(dv, (size_t)N * L * MV) || !read_ints(dsr, (size_t)N * L * MS)) return 2;
        if (has_gt && (!read_ints(gv, (size_t)N * Lg * MV) || !read_ints(gsr, (size_t)N * Lg * MS))) return 2;
        if (has_idx && !read_ints(idx, (size_t)N * L)) return 2;
        std::vector<TbJob> jobs(S);
        for (int s = 0; s < S; ++s) {
            const int n = s / MV, v = s % MV;
            tb_scan_job(&cv[(size_t)n * MV], &dv[(size_t)n * L * MV], &dsr[(size_t)n * L * MS], has_gt ? &gv[(size_t)n * Lg * MV] : nullptr,
                        has_gt ? &gsr[(size_t)n * Lg * MS] : nullptr, has_idx ? &idx[(size_t)n * L] : nullptr, v, L, Lg, MV, MS, N_sink, n_verbs, &jobs[s]);
        }
        std::vector<long long> verbs(S, 0);
        std::vector<int32_t> det((size_t)S * RANK_L, 0), gt((size_t)S * RANK_L, 0), gather((size_t)Qcap * N_sink, -1), key((size_t)Qcap * 3, 0), status(N);
        std::vector<float> tr((size_t)Qcap * N_sink, 0.f), gl((size_t)Qcap * N_sink, 0.f);
        int n_rows = 0, n_found = 0, st_or = 0;
        for (int n = 0; n < N; ++n) {
            status[n] = tb_caption_status(&jobs[(size_t)n * MV], MV);
            st_or |= status[n];
        }
        for (int s = 0; s < S; ++s) {
            const TbJob& job = jobs[s];
            const int n = s / MV;
            if (!job.verb || (status[n] & TB_DROP_CAPTION)) continue;
            verbs[n_rows] = job.verb;
            for (int i = 0; i < RANK_L; ++i) { det[(size_t)n_rows * RANK_L + i] = job.scan.role[i]; gt[(size_t)n_rows * RANK_L + i] = job.gt_roles[i]; }
            ++n_rows;
            for (int i = 0; i < job.n_items; ++i, ++n_found) {
                if (n_found >= Qcap) continue;
                const size_t q = (size_t)n_found;
                tb_item(&job.scan, i, n, L, N_sink, &idx[(size_t)n * L], &gather[q * N_sink], &tr[q * N_sink], &gl[q * N_sink]);
                key[q * 3] = n; key[q * 3 + 1] = s % MV; key[q * 3 + 2] = job.scan.role[job.scan.item_role[i]];
            }
        }
        const int n_items = n_found < Qcap ? n_found : Qcap;
        for (int s = 0; s < S; ++s) printf("%lld ", verbs[s]);
        for (int32_t x : det) printf("%d ", x);
        for (int32_t x : gt) printf("%d ", x);
        for (int32_t x : gather) printf("%d ", x);
        for (float x : tr) printf("%.9g ", x);
        for (float x : gl) printf("%.9g ", x);
        for (int32_t x : key) printf("%d ", x);
        printf("%d %d %d %d ", n_rows, n_items, st_or, n_found - n_items);
        for (int32_t st : status) printf("%d ", st);
        printf("\n");
    }
    return 0;
}
