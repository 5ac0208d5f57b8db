// Kernels that build the ordering models' training batches on the device: from the loader's integer annotations to the
// tensors S_SSP.forward and SinkhornNet.loc_loss take.  The integer logic is train_batch_logic.h (shared with the host tool); here it
// is mapped to threads:
//   k_tb_jobs      one thread per (caption, verb column) job slot: the det scan, the gt scan, the items' flags -> the slot's TbJob in the plan
//   k_tb_compact   one block: exclusive scan of the slots' row and item counts in slot order (fixed order, no atomics, as k_rank_items
//                  does it), then the compacted S-SSP rows, the compacted item tables, counts and the per-caption status
//   k_tb_gather    out[r] = rows[gather[r]] or zeros for any row length that is a multiple of 4; rows of 2352 floats go through
//                  k_rank_gather (rank_kernels.h), called unmodified
// Plain loads and stores only: two runs write the same bits, padding included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_batch_logic.h"

namespace vsr {

using namespace vsr_rank;

struct TbPlan { int32_t* row_off; int32_t* item_off; TbJob* jobs; };
struct TbOut {
    int64_t* verbs; int32_t* det_roles; int32_t* gt_roles;                   // (S), (S, 10), (S, 10); gt_roles may be null
    int32_t* item_gather; float* tr_locs; float* gt_locs; int32_t* item_key;  // (Qcap, N_sink) x 3, (Qcap, 3); all four may be null
    int32_t* counts; int32_t* status;                                         // (4), (N)
};

__global__ __launch_bounds__(64) void k_tb_jobs(const int32_t* __restrict__ control_verb, const int32_t* __restrict__ det_v, const int32_t* __restrict__ det_sr,
                                                const int32_t* __restrict__ gt_v, const int32_t* __restrict__ gt_sr, const int32_t* __restrict__ idx_list, int N, int L,
                                                int Lg, int MV, int MS, int N_sink, long long n_verbs, TbPlan plan) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N * MV) return;
    const int n = s / MV, v = s - n * MV;
    tb_scan_job(control_verb + (long long)n * MV, det_v + (long long)n * L * MV, det_sr + (long long)n * L * MS, gt_v ? gt_v + (long long)n * Lg * MV : nullptr,
                gt_v ? gt_sr + (long long)n * Lg * MS : nullptr, idx_list ? idx_list + (long long)n * L : nullptr, v, L, Lg, MV, MS, N_sink, n_verbs, plan.jobs + s);
}

__global__ __launch_bounds__(256) void k_tb_compact(TbPlan plan, const int32_t* __restrict__ idx_list, int N, int L, int MV, int N_sink, int Qcap, TbOut o) {
    __shared__ int sh_r[256], sh_i[256], sh_or[256];
    __shared__ int carry_r, carry_i;
    const int tid = threadIdx.x, S = N * MV;
    if (tid == 0) carry_r = carry_i = 0;
    __syncthreads();
    for (int base = 0; base < S; base += 256) {
        const int s = base + tid;
        int cr = 0, ci = 0;
        if (s < S && plan.jobs[s].verb != 0 && !(tb_caption_status(plan.jobs + (s / MV) * MV, MV) & TB_DROP_CAPTION)) {
            cr = 1;
            ci = plan.jobs[s].n_items;
        }
        sh_r[tid] = cr;
        sh_i[tid] = ci;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {                       // inclusive scan of the chunk, both counts
            const int ar = tid >= d ? sh_r[tid - d] : 0, ai = tid >= d ? sh_i[tid - d] : 0;
            __syncthreads();
            sh_r[tid] += ar;
            sh_i[tid] += ai;
            __syncthreads();
        }
        if (s < S) {                                              // -1: the slot emits nothing
            plan.row_off[s] = cr ? carry_r + sh_r[tid] - cr : -1;
            plan.item_off[s] = carry_i + sh_i[tid] - ci;
        }
        __syncthreads();
        if (tid == 255) { carry_r += sh_r[255]; carry_i += sh_i[255]; }
        __syncthreads();
    }
    const int n_rows = carry_r, n_found = carry_i, n_items = n_found < Qcap ? n_found : Qcap;
    int st_or = 0;
    for (int n = tid; n < N; n += 256) {
        const int32_t st = tb_caption_status(plan.jobs + (long long)n * MV, MV);
        o.status[n] = st;
        st_or |= st;
    }
    sh_or[tid] = st_or;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 256; ++i) st_or |= sh_or[i];
        o.counts[0] = n_rows; o.counts[1] = n_items; o.counts[2] = st_or; o.counts[3] = n_found - n_items;
    }
    // padding: rows beyond n_rows and items beyond n_items are zeros, -1 in item_gather
    for (int i = n_rows + tid; i < S; i += 256) o.verbs[i] = 0;
    for (int i = n_rows * RANK_L + tid; i < S * RANK_L; i += 256) {
        o.det_roles[i] = 0;
        if (o.gt_roles) o.gt_roles[i] = 0;
    }
    if (o.item_gather) {
        for (long long i = (long long)n_items * N_sink + tid; i < (long long)Qcap * N_sink; i += 256) {
            o.item_gather[i] = -1;
            o.tr_locs[i] = 0.f;
            o.gt_locs[i] = 0.f;
        }
        for (long long i = (long long)n_items * 3 + tid; i < (long long)Qcap * 3; i += 256) o.item_key[i] = 0;
    }
    for (int s = tid; s < S; s += 256) {                          // (this thread wrote row_off[s] / item_off[s] above)
        const TbJob* job = plan.jobs + s;
        const int row = plan.row_off[s];
        if (row < 0) continue;
        const int n = s / MV;
        o.verbs[row] = job->verb;
        for (int i = 0; i < RANK_L; ++i) {
            o.det_roles[row * RANK_L + i] = job->scan.role[i];
            if (o.gt_roles) o.gt_roles[row * RANK_L + i] = job->gt_roles[i];
        }
        if (!o.item_gather) continue;
        const int off = plan.item_off[s];
        for (int i = 0; i < job->n_items; ++i) {
            const long long q = off + i;
            if (q >= Qcap) break;
            tb_item(&job->scan, i, n, L, N_sink, idx_list + (long long)n * L, o.item_gather + q * N_sink, o.tr_locs + q * N_sink, o.gt_locs + q * N_sink);
            o.item_key[q * 3 + 0] = n;
            o.item_key[q * 3 + 1] = s - n * MV;
            o.item_key[q * 3 + 2] = job->scan.role[job->scan.item_role[i]];
        }
    }
}

// out[r] = rows[gather[r]] or zeros, D4 float4 per row: one wave per row, four rows per block, grid-strided (k_rank_gather's mapping for
// a row length known only at run time)
__global__ __launch_bounds__(256) void k_tb_gather(const float* __restrict__ rows, const int32_t* __restrict__ gather, long long n_rows, long long n_src, int D4,
                                                   float* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long r = (long long)blockIdx.x * 4 + wave; r < n_rows; r += (long long)gridDim.x * 4) {
        const int g = gather[r];
        float4* dst = reinterpret_cast<float4*>(out) + r * D4;
        if (g >= 0 && g < n_src) {
            const float4* src = reinterpret_cast<const float4*>(rows) + (long long)g * D4;
            for (int c = lane; c < D4; c += 64) dst[c] = src[c];
        } else {
            for (int c = lane; c < D4; c += 64) dst[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

}  // namespace vsr
