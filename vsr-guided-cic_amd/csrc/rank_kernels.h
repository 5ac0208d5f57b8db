// Kernels of the eval loop's caption ranking on the device: the glue between the ordering models and the beam.
// The integer logic is rank_logic.h (shared with the host tool); here it is mapped to threads:
//   k_rank_jobs    one thread per (caption, verb column) job slot: the scan, S-SSP's inputs, the job's tables in the plan
//   k_rank_items   one block: exclusive scan of the jobs' item counts (fixed order, no atomics), the Sinkhorn items' gather rows
//   k_rank_gather  the items' feature rows, the only kernel here that moves real bytes (N_sink x 2352 fp32 = 94 KB per item at 10)
//   k_rank_finish  one block of one wave per caption; ONLY lane 0 works (a serial walk over lists kept in LDS, the other 63 lanes
//                  return at once): integer bookkeeping, not a throughput kernel, and nothing in it is parallel
// Plain loads and stores only: two runs write the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rank_logic.h"

namespace vsr {

using namespace vsr_rank;

constexpr int RANK_HDR_INTS = 8;          // [0] N, [1] MV, [2] N_sink, [3] Qcap, [4] items found (may exceed Qcap), [5..7] unused
constexpr int SH_ROW = 2352, SH_ROW4 = SH_ROW / 4;

struct RankPlan { int32_t* hdr; int32_t* item_cnt; int32_t* item_off; RankJob* jobs; };

__global__ __launch_bounds__(64) void k_rank_jobs(const int32_t* __restrict__ control_verb, const int32_t* __restrict__ det_v,
                                                  const int32_t* __restrict__ det_sr, int N, int L, int MV, int MS, int N_sink, int Qcap,
                                                  long long n_verbs, RankPlan plan, int64_t* __restrict__ job_verbs, int32_t* __restrict__ job_roles) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0) {
        plan.hdr[0] = N; plan.hdr[1] = MV; plan.hdr[2] = N_sink; plan.hdr[3] = Qcap;
        plan.hdr[5] = plan.hdr[6] = plan.hdr[7] = 0;
    }
    if (s >= N * MV) return;
    const int n = s / MV, v = s - n * MV;
    RankJob* job = plan.jobs + s;
    const int32_t verb = rank_scan_job(control_verb + (long long)n * MV, det_v + (long long)n * L * MV, det_sr + (long long)n * L * MS, v, L, MV, MS,
                                       n_verbs, job);
    job_verbs[s] = verb;
    for (int i = 0; i < RANK_L; ++i) job_roles[s * RANK_L + i] = job->role[i];       // zeros beyond n_roles and when inactive
    plan.item_cnt[s] = job->n_items;
}

__global__ __launch_bounds__(256) void k_rank_items(RankPlan plan, int S, int L, int MV, int N_sink, int Qcap, int Qfill, int32_t* __restrict__ item_gather) {
    __shared__ int sh[256];
    __shared__ int carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < S; base += 256) {
        const int s = base + tid;
        const int c = s < S ? plan.item_cnt[s] : 0;
        sh[tid] = c;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {                       // inclusive scan of the chunk
            const int add = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        if (s < S) plan.item_off[s] = carry + sh[tid] - c;
        __syncthreads();
        if (tid == 255) carry += sh[255];
        __syncthreads();
    }
    const int total = carry;
    if (tid == 0) plan.hdr[4] = total;
    for (long long i = tid; i < (long long)Qfill * N_sink; i += 256)
        if (i / N_sink >= total || i / N_sink >= Qcap) item_gather[i] = -1;      // every row of every unused item (Qfill >= Qcap rows exist)
    for (int s = tid; s < S; s += 256) {                          // (this thread wrote item_off[s] above)
        const RankJob* job = plan.jobs + s;
        const int off = plan.item_off[s];
        for (int i = 0; i < job->n_items; ++i)
            if (off + i < Qcap) rank_item_gather(job, i, s / MV, L, N_sink, item_gather + (long long)(off + i) * N_sink);
    }
}

// seq[r] = rows[item_gather[r]] or zeros: one wave per row of 588 float4, four rows per block, grid-strided
__global__ __launch_bounds__(256) void k_rank_gather(const float* __restrict__ rows, const int32_t* __restrict__ item_gather, long long n_rows,
                                                     long long n_src, float* __restrict__ seq) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long r = (long long)blockIdx.x * 4 + wave; r < n_rows; r += (long long)gridDim.x * 4) {
        const int g = item_gather[r];
        float4* dst = reinterpret_cast<float4*>(seq + r * SH_ROW);
        if (g >= 0 && g < n_src) {
            const float4* src = reinterpret_cast<const float4*>(rows + (long long)g * SH_ROW);
            for (int c = lane; c < SH_ROW4; c += 64) dst[c] = src[c];
        } else {
            for (int c = lane; c < SH_ROW4; c += 64) dst[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

__global__ __launch_bounds__(64) void k_rank_finish(RankPlan plan, const int32_t* __restrict__ pred, const int32_t* __restrict__ assign, int N, int L,
                                                    int MV, int N_sink, int32_t* __restrict__ rank, int32_t* __restrict__ status) {
    __shared__ RankScratch sc;
    const int n = blockIdx.x;
    if (threadIdx.x != 0) return;
    int32_t row[RANK_L];
    int32_t st;
    if (plan.hdr[0] != N || plan.hdr[1] != MV || plan.hdr[2] != N_sink) {
        st = RANK_BAD_PLAN;
        for (int j = 0; j < RANK_L; ++j) row[j] = -1;
    } else {
        st = rank_finish_caption(plan.jobs + (long long)n * MV, plan.item_off + (long long)n * MV, pred + (long long)n * MV * RANK_L, assign, MV, L, N_sink,
                                 plan.hdr[3], &sc, row);
    }
    for (int j = 0; j < L; ++j) rank[(long long)n * L + j] = row[j];
    status[n] = st;
}

}  // namespace vsr
