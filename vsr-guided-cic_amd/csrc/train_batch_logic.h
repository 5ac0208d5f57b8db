// Integer bookkeeping of the ordering models' TRAINING batches (coco_scripts/train_region_sort.py:133-179, coco_scripts/train_sinkhorn.py:
// 144-205 and their Flickr twins), stated ONCE for the host and the device: plain C++, no HIP types.  The training twin of rank_logic.h,
// whose scan (rank_scan_job, the find_sr < 10 gate on both branches) it calls unchanged.  train_batch_kernels.h runs these functions one
// job per thread; tools/train_batch_host.cpp runs them on the CPU, where tests/test_train_batch_logic.py holds them to the numpy
// transcription of the reference's loops in vsrcap/trainbatch.py (ssp_train_batch, sinkhorn_train_items).
//
//   job      one (caption n, verb column v) at slot s = n MV + v, active under exactly rank_scan_job's rule: control_verb[n, 0..v] all
//            non-zero and at least one match in the det scan.  A verb with no match is skipped and later columns still count (the
//            reference's `continue`).
//   row      the S-SSP sequence of an active job: the raw verb id (S_SSP.forward takes it % 10000), det_roles = RankJob::role (first
//            sights in scan order, zero padded), gt_roles = the same first-sight scan over gt_seqs_v (Lg, MV) / gt_seqs_sr (Lg, MS) with
//            its own find_gt_sr < 10 gate.  gt_roles may be all zero: the row is emitted all the same, as in the reference.
//   items    one per repeated role of an active job.  ORDER: ascending role id, the order rank_logic.h uses.  The reference iterates a
//            Python set; its loss is a sum over the items, so only the rounding of that sum depends on the order - ascending id is THIS
//            PROJECT'S DEFINITION.
//            slots  = the first N_sink entries of the role's slot list in scan order (train_sinkhorn_flickr.py skips j >= sinkhorn_len,
//                     train_sinkhorn.py would raise IndexError); a cut list sets TB_TRUNCATED
//            gather = n L + slots[c], -1 beyond len        tr_locs = slots[c], the literal 10.0 beyond len (train_sinkhorn.py:191, not N_sink)
//            g      = idx_list[n, slots[c]], 10 beyond len; a used value outside [0, 10) sets TB_BAD_IDX (it may tie with the padding)
//            change = the STABLE argsort of g over all N_sink entries, ties to the lower index.  torch.argsort without stable=True
//                     promises no tie order, so the stable rule is THIS PROJECT'S DEFINITION; without TB_BAD_IDX and with distinct
//                     idx_list values there is no tie among the entries that are read.
//            gt_locs = change[c] for c < len, 10.0 beyond (the reference's gt_locs_).  Its `matrix` is never used by the loss: not built.
//   status   per caption, the OR of its active jobs' flags.  A caption with RANK_BAD_ROLE or RANK_BAD_VERB emits no rows and no items
//            (the reference's embeddings would raise on it).
#pragma once
#include "rank_logic.h"

namespace vsr_rank {

constexpr int TB_PAD_LOC = 10;      // the padding value of tr_locs / gt_locs / g: the literal of train_sinkhorn.py:191-193

enum : int32_t {
    TB_TRUNCATED = 32,              // a Sinkhorn item's slot list was cut to N_sink entries
    TB_BAD_IDX = 64                 // an idx_list value outside [0, 10) at a used slot
};
constexpr int32_t TB_DROP_CAPTION = RANK_BAD_ROLE | RANK_BAD_VERB;

struct TbJob {
    RankJob scan;                   // the det scan: role[] = det_roles, item_role[] / m_role / m_slot = the item descriptors
    int32_t verb;                   // raw id; 0 = inactive
    int32_t n_items;                // 0 without idx_list
    int32_t flags;                  // RANK_BAD_ROLE | RANK_BAD_VERB | TB_TRUNCATED | TB_BAD_IDX
    int32_t gt_roles[RANK_L];
};

RANK_HD inline bool tb_limits_ok(int L, int Lg, int MV, int MS, int N_sink) { return rank_limits_ok(L, MV, MS, N_sink) && Lg >= 1; }

// Tables of item i of job `job` of caption n.  idx: idx_list[n] (L).  gather / tr_locs / gt_locs: N_sink entries each, or all three null
// (flags only).  Returns TB_TRUNCATED | TB_BAD_IDX.
RANK_HD inline int32_t tb_item(const RankJob* job, int i, int n, int L, int N_sink, const int32_t* idx, int32_t* gather, float* tr_locs, float* gt_locs) {
    uint8_t slots[RANK_MAX_SINK];
    int32_t g[RANK_MAX_SINK];
    const int r = job->item_role[i];
    const int len = rank_role_slots(job, r, N_sink, slots);
    int32_t flags = job->count[r] > N_sink ? TB_TRUNCATED : 0;
    for (int c = 0; c < N_sink; ++c) {
        g[c] = c < len ? idx[slots[c]] : TB_PAD_LOC;
        if (c < len && (g[c] < 0 || g[c] >= RANK_L)) flags |= TB_BAD_IDX;
    }
    if (!gather) return flags;
    for (int c = 0; c < N_sink; ++c) {
        gather[c] = c < len ? n * L + slots[c] : -1;
        tr_locs[c] = c < len ? (float)slots[c] : (float)TB_PAD_LOC;
        gt_locs[c] = (float)TB_PAD_LOC;
    }
    for (int x = 0; x < N_sink; ++x) {                 // change[before] = x, before = entries sorted in front of x under the stable rule
        int before = 0;
        for (int y = 0; y < N_sink; ++y) before += g[y] < g[x] || (g[y] == g[x] && y < x);
        if (before < len) gt_locs[before] = (float)x;
    }
    return flags;
}

// Job (n, v).  cv / dv / dsr as in rank_scan_job; gv: gt_seqs_v[n] (Lg, MV) and gsr: gt_seqs_sr[n] (Lg, MS), or both null (gt_roles
// stay zero); idx: idx_list[n] (L) or null (no items).
RANK_HD inline void tb_scan_job(const int32_t* cv, const int32_t* dv, const int32_t* dsr, const int32_t* gv, const int32_t* gsr, const int32_t* idx, int v,
                                int L, int Lg, int MV, int MS, int N_sink, int64_t n_verbs, TbJob* out) {
    out->verb = rank_scan_job(cv, dv, dsr, v, L, MV, MS, n_verbs, &out->scan);
    out->n_items = 0;
    out->flags = out->scan.flags;
    for (int i = 0; i < RANK_L; ++i) out->gt_roles[i] = 0;
    if (!out->scan.n_roles) { out->verb = 0; return; }
    if (gv) {
        int find_gt_sr = 0;
        for (int j = 0; j < Lg; ++j)
            for (int k = 0; k < MV; ++k)
                if (gv[j * MV + k] == out->verb && find_gt_sr < RANK_L) {
                    const int32_t sr = gsr[j * MS + k];
                    int r = 0;
                    while (r < find_gt_sr && out->gt_roles[r] != sr) ++r;
                    if (r < find_gt_sr) continue;
                    out->gt_roles[find_gt_sr++] = sr;
                    if (sr < 0 || sr >= RANK_ROLE_IDS) out->flags |= RANK_BAD_ROLE;
                }
    }
    if (idx) {
        out->n_items = out->scan.n_items;
        for (int i = 0; i < out->n_items; ++i) out->flags |= tb_item(&out->scan, i, 0, L, N_sink, idx, nullptr, nullptr, nullptr);
    }
}

// status of a caption = OR of the flags of its MV job slots (inactive slots carry none)
RANK_HD inline int32_t tb_caption_status(const TbJob* jobs, int MV) {
    int32_t st = 0;
    for (int v = 0; v < MV; ++v) st |= jobs[v].flags;
    return st;
}

}  // namespace vsr_rank
