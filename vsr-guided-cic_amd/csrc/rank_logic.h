// Integer bookkeeping of the eval loop's caption ranking (coco_scripts/eval_coco.py:141-221, utils/tools.py:35-71), stated ONCE for the
// host and the device: plain C++, no HIP types.  rank_kernels.h runs these functions one job / one caption per thread;
// tools/rank_logic_host.cpp runs them on the CPU, where tests/test_rank_logic.py holds them to the Python of vsrcap/evalbatch.py
// (rank_captions, verb_rank_merge).
//
//   job      one (caption n, verb column v).  Active iff control_verb[n, 0..v] are all non-zero (the reference breaks at the first 0) and
//            the scan below finds a match.
//   scan     j < L, k < MV in that order; on det_seqs_v[n,j,k] == verb && find_sr < 10 read sr = det_seqs_sr[n,j,k]: the first sight of
//            sr appends it to the role list, later sights mark it repeated; either way j joins sr's slot list.  The gate guards both
//            branches, so the 10th distinct role ends the scan for good.
//   items    per active job one Sinkhorn item per repeated role, in ascending role id; rows = the first N_sink slots of the role.
//   finish   per active job, in verb order, walk pred until 0: a role with one slot gives that slot, a repeated role its (truncated)
//            slots ordered by the argsort of assign[item][0:len] (a permutation: rank = number of smaller entries); the jobs' lists
//            are folded left to right with rank_merge (verb_rank_merge, quirks kept); the first L entries are the rank row.
// Every list holds slot positions, i.e. values in [0, L) with L == 10: sets of values are bit masks, maps from values are small arrays.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RANK_HD __host__ __device__
#else
#define RANK_HD
#endif

namespace vsr_rank {

constexpr int RANK_L = 10;                                   // S-SSP's sequence length: slots per caption, roles per job
constexpr int RANK_MAX_MV = 8, RANK_MIN_SINK = 2, RANK_MAX_SINK = 16;
constexpr int RANK_VERB_CAP = RANK_L * RANK_MAX_MV;          // matches of one job = entries of one verb's list
constexpr int RANK_MERGED_CAP = RANK_MAX_MV * RANK_VERB_CAP; // a merge adds at most the right list's length
constexpr int RANK_ROLE_IDS = 26;                            // the role embedding's rows (sort_model.py: sr ids in [0, 26))

enum : int32_t {
    RANK_NO_JOB = 1,        // the caption has no active job (the reference indexes verb_ranks[0] and raises)
    RANK_ITEM_OVERFLOW = 2, // one of the caption's Sinkhorn items lies beyond max_items and was not evaluated
    RANK_BAD_ROLE = 4,      // a matched role id outside [0, 26) (the reference's embedding raises)
    RANK_BAD_VERB = 8,      // verb < 0, or verb % 10000 outside [0, n_verbs) (the reference's embedding raises)
    RANK_BAD_PLAN = 16      // the plan was not written for this call's (N, MV, N_sink)
};

struct RankJob {
    int32_t n_roles;                    // distinct roles found; 0 = inactive
    int32_t n_match;                    // matches taken = entries of m_role / m_slot
    int32_t n_items;                    // repeated roles
    int32_t flags;                      // RANK_BAD_ROLE | RANK_BAD_VERB
    int32_t role[RANK_L];               // in order of first sight (what S-SSP is given)
    int32_t count[RANK_L];              // full length of each role's slot list
    int32_t item_role[RANK_L];          // indices into role[] of the repeated roles, ascending role id
    uint8_t m_role[RANK_VERB_CAP];      // the matches in scan order: index into role[] ...
    uint8_t m_slot[RANK_VERB_CAP];      // ... and slot j
};

RANK_HD inline bool rank_limits_ok(int L, int MV, int MS, int N_sink) {
    return L == RANK_L && MV >= 1 && MV <= RANK_MAX_MV && MS >= MV && N_sink >= RANK_MIN_SINK && N_sink <= RANK_MAX_SINK;
}

// The scan of job (n, v).  cv: control_verb[n] (MV), dv: det_seqs_v[n] (L, MV), dsr: det_seqs_sr[n] (L, MS).  Returns the verb (0 when
// the job is inactive, with job->n_roles == 0).
RANK_HD inline int32_t rank_scan_job(const int32_t* cv, const int32_t* dv, const int32_t* dsr, int v, int L, int MV, int MS, int64_t n_verbs,
                                     RankJob* job) {
    job->n_roles = job->n_match = job->n_items = job->flags = 0;
    for (int i = 0; i < RANK_L; ++i) job->role[i] = job->count[i] = job->item_role[i] = 0;
    for (int i = 0; i <= v; ++i)
        if (cv[i] == 0) return 0;
    const int32_t verb = cv[v];
    int find_sr = 0, n_match = 0, flags = 0;
    for (int j = 0; j < L; ++j)
        for (int k = 0; k < MV; ++k)
            if (dv[j * MV + k] == verb && find_sr < RANK_L) {
                const int32_t sr = dsr[j * MS + k];
                int r = 0;
                while (r < find_sr && job->role[r] != sr) ++r;
                if (r == find_sr) {
                    job->role[find_sr++] = sr;
                    if (sr < 0 || sr >= RANK_ROLE_IDS) flags |= RANK_BAD_ROLE;
                }
                job->count[r] += 1;
                job->m_role[n_match] = (uint8_t)r;
                job->m_slot[n_match] = (uint8_t)j;
                ++n_match;
            }
    if (!find_sr) return 0;
    const int32_t vm = verb % 10000;                   // C remainder, as k_ssp_embed takes it: a NEGATIVE verb id is invalid and flagged here
    if (vm < 0 || vm >= n_verbs) flags |= RANK_BAD_VERB;
    int n_items = 0;
    for (int r = 0; r < find_sr; ++r)
        if (job->count[r] > 1) {                       // insertion into the ascending-id order
            int at = n_items++;
            while (at > 0 && job->role[job->item_role[at - 1]] > job->role[r]) { job->item_role[at] = job->item_role[at - 1]; --at; }
            job->item_role[at] = r;
        }
    job->n_roles = find_sr;
    job->n_match = n_match;
    job->n_items = n_items;
    job->flags = flags;
    return verb;
}

// slots of role index r, in scan order, at most `cap` of them -> out; returns how many
RANK_HD inline int rank_role_slots(const RankJob* job, int r, int cap, uint8_t* out) {
    int n = 0;
    for (int m = 0; m < job->n_match && n < cap; ++m)
        if (job->m_role[m] == r) out[n++] = job->m_slot[m];
    return n;
}

// row of item_gather for item i of a job of caption n: n * L + slot for the first N_sink slots of the role, -1 beyond
RANK_HD inline void rank_item_gather(const RankJob* job, int i, int n, int L, int N_sink, int32_t* row) {
    uint8_t slots[RANK_MAX_SINK];
    const int len = rank_role_slots(job, job->item_role[i], N_sink, slots);
    for (int c = 0; c < N_sink; ++c) row[c] = c < len ? n * L + slots[c] : -1;
}

// verb_rank_merge(la, lb) of vsrcap/evalbatch.py (utils/tools.py:35-71) -> out (capacity cap); returns its length.  lb is overwritten
// (the reference rewrites it too); shared / pos: scratch of na entries each.
RANK_HD inline int rank_merge(const uint8_t* la, int na, uint8_t* lb, int nb, uint8_t* out, int cap, uint8_t* shared, uint8_t* pos) {
    int ns = 0;
    uint32_t in_shared = 0;
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j)
            if (lb[j] == la[i]) {                      // the first position in lb
                shared[ns] = la[i];
                pos[ns] = (uint8_t)j;
                ++ns;
                in_shared |= 1u << la[i];
                break;
            }
    bool ordered = true;
    for (int i = 1; i < ns; ++i) ordered = ordered && pos[i - 1] <= pos[i];
    if (!ordered) {                                    // lb[sorted(pos)[j]] = shared[j]: counting sort over the positions of lb
        int j = 0;
        for (int p = 0; p < nb; ++p)
            for (int i = 0; i < ns; ++i)
                if (pos[i] == p) lb[p] = shared[j++];
    }
    int right = -1, right_of[16];
    for (int i = 0; i < 16; ++i) right_of[i] = -1;
    for (int idx = nb - 1; idx >= 0; --idx) {          // a value met twice keeps the neighbour of its FIRST occurrence (a dict, written last)
        const int b = lb[idx];
        if (in_shared >> b & 1u) right = b;
        else right_of[b] = right;
    }
    int n = 0;
    for (; n < na && n < cap; ++n) out[n] = la[n];
    for (int idx = 0; idx < nb; ++idx) {
        const int b = lb[idx];
        if (in_shared >> b & 1u) continue;
        if (n >= cap) break;
        int at = n;                                    // append when there is no right neighbour
        if (right_of[b] >= 0)
            for (at = 0; at < n && out[at] != right_of[b]; ++at) {}      // in front of its first occurrence
        for (int i = n; i > at; --i) out[i] = out[i - 1];
        out[at] = (uint8_t)b;
        ++n;
    }
    return n;
}

struct RankScratch {
    uint8_t a[RANK_MERGED_CAP], b[RANK_MERGED_CAP], shared[RANK_MERGED_CAP], pos[RANK_MERGED_CAP], verb[RANK_VERB_CAP];
};

// The rank row of caption n.  jobs / item_off: the caption's MV job slots; pred: (MV, 10) of those slots; assign: (Qcap, N_sink) of ALL
// items.  Returns the status; a non-zero status leaves rank_row all -1.
RANK_HD inline int32_t rank_finish_caption(const RankJob* jobs, const int32_t* item_off, const int32_t* pred, const int32_t* assign, int MV, int L,
                                           int N_sink, int Qcap, RankScratch* sc, int32_t* rank_row) {
    for (int j = 0; j < L; ++j) rank_row[j] = -1;
    int32_t status = 0;
    int active = 0;
    for (int v = 0; v < MV; ++v) {
        if (!jobs[v].n_roles) continue;
        ++active;
        status |= jobs[v].flags;
        if (jobs[v].n_items && item_off[v] + jobs[v].n_items > Qcap) status |= RANK_ITEM_OVERFLOW;
    }
    if (!active) status |= RANK_NO_JOB;
    if (status) return status;
    uint8_t *cur = sc->a, *nxt = sc->b;
    int n_cur = 0, seen = 0;
    for (int v = 0; v < MV; ++v) {
        const RankJob* job = &jobs[v];
        if (!job->n_roles) continue;
        int nv = 0;
        for (int t = 0; t < RANK_L; ++t) {
            const int32_t sr = pred[v * RANK_L + t];
            if (sr == 0) break;
            int r = 0;
            while (r < job->n_roles && job->role[r] != sr) ++r;
            if (r == job->n_roles) continue;           // not a role of this job: S-SSP picks among the job's roles only
            if (job->count[r] == 1) {
                if (nv < RANK_VERB_CAP) nv += rank_role_slots(job, r, 1, sc->verb + nv);
                continue;
            }
            int i = 0;
            while (i < job->n_items && job->item_role[i] != r) ++i;
            if (i == job->n_items) continue;           // (cannot happen on a plan the scan wrote)
            const int32_t* a = assign + (long long)(item_off[v] + i) * N_sink;
            uint8_t slots[RANK_MAX_SINK];
            const int len = rank_role_slots(job, r, N_sink, slots);
            if (nv + len > RANK_VERB_CAP) continue;
            for (int x = 0; x < len; ++x) {             // argsort of a permutation's prefix: no ties
                int smaller = 0;
                for (int y = 0; y < len; ++y) smaller += a[y] < a[x];
                sc->verb[nv + smaller] = slots[x];
            }
            nv += len;
        }
        if (!seen++) {
            for (int i = 0; i < nv; ++i) cur[i] = sc->verb[i];
            n_cur = nv;
        } else {
            n_cur = rank_merge(cur, n_cur, sc->verb, nv, nxt, RANK_MERGED_CAP, sc->shared, sc->pos);
            uint8_t* t = cur; cur = nxt; nxt = t;
        }
    }
    for (int j = 0; j < L && j < n_cur; ++j) rank_row[j] = cur[j];
    return 0;
}

}  // namespace vsr_rank
