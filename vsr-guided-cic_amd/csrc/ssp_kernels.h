// Kernels of the two ordering models that run before the decoder in the eval loop:
//   S-SSP  /root/reference/models/sort_model.py:105-183 (generate, mode 'not-normal'), sort_modules.py:25-135,
//          transformer_modules.py:18-147 (attention), :182-215 (embedding x sqrt(512)), :302-345 (feed-forward, encoder layer)
//   R-SSP  /root/reference/models/sinkhorn_network.py:30-51 (MLP, 20 Sinkhorn iterations) and the assignment of
//          coco_scripts/eval_coco.py:185-189 (munkres on max - value of the transposed matrix)
// All sequences / items of a loader batch are processed together: the matrix products run on the stream-K fp32-MFMA GEMM
// (rows = sequences x positions), everything here is the pointwise / tiny-attention / selection part.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace vsr {

constexpr int SSP_H = 512, SSP_HEADS = 8, SSP_HD = 64, SSP_FF = 2048, SSP_LEN = 10, SSP_ROLES = 26;

// x[s, j, :] = sqrt(512) * (table[tok[s * ld_tok + j]] (+ vtable[verb[s] % 10000]))     (transformer_modules.py:193-203,
// sort_modules.py:52: v_embed(verb) + sr_embed(roles); sort_modules.py:125: embed_layer(tokens))
__global__ __launch_bounds__(128) void k_ssp_embed(const int* __restrict__ tok, int ld_tok, int len, const float* __restrict__ table,
                                                   const int64_t* __restrict__ verbs, const float* __restrict__ vtable, int n_verbs,
                                                   int S, float* __restrict__ out) {
    const int row = blockIdx.x;                       // s * len + j
    const int s = row / len, j = row - s * len;
    int t = tok[s * ld_tok + j];
    if (t < 0 || t >= SSP_ROLES) t = 0;
    const float sc = 22.627416997969522f;             // sqrt(512)
    const float4 a = *reinterpret_cast<const float4*>(table + (long long)t * SSP_H + threadIdx.x * 4);
    float4 o = make_float4(a.x * sc, a.y * sc, a.z * sc, a.w * sc);
    if (verbs) {
        long long v = verbs[s] % 10000;                // sort_model.py:108
        if (v < 0 || v >= n_verbs) v = 0;
        const float4 b = *reinterpret_cast<const float4*>(vtable + v * SSP_H + threadIdx.x * 4);
        o = make_float4(b.x * sc + a.x * sc, b.y * sc + a.y * sc, b.z * sc + a.z * sc, b.w * sc + a.w * sc);
    }
    *reinterpret_cast<float4*>(out + (long long)row * SSP_H + threadIdx.x * 4) = o;
}

// nn.LayerNorm(512), eps 1e-5, biased variance: one wave per row.  TRAIN: the same arithmetic, and the normalised row x^ and 1 / std
// go to the training tape (k_layernorm512_bwd reads them)
template <bool TRAIN>
__device__ __forceinline__ void layernorm512_row(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, int rows,
                                                 float* __restrict__ out, float* __restrict__ xhat, float* __restrict__ rstd_out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* xr = x + (long long)row * SSP_H;
    float4 v[2];
    v[0] = *reinterpret_cast<const float4*>(xr + lane * 4);
    v[1] = *reinterpret_cast<const float4*>(xr + 256 + lane * 4);
    float s = (v[0].x + v[0].y) + (v[0].z + v[0].w) + (v[1].x + v[1].y) + (v[1].z + v[1].w);
    const float mean = wave_sum(s) * (1.0f / SSP_H);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
        q += dx * dx + dy * dy + dz * dz + dw * dw;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / SSP_H) + 1e-5f);
    if (TRAIN && lane == 0) rstd_out[row] = rstd;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = i * 256 + lane * 4;
        const float4 ww = *reinterpret_cast<const float4*>(w + c), bb = *reinterpret_cast<const float4*>(b + c);
        float4 o;
        o.x = (v[i].x - mean) * rstd * ww.x + bb.x; o.y = (v[i].y - mean) * rstd * ww.y + bb.y;
        o.z = (v[i].z - mean) * rstd * ww.z + bb.z; o.w = (v[i].w - mean) * rstd * ww.w + bb.w;
        *reinterpret_cast<float4*>(out + (long long)row * SSP_H + c) = o;
        if (TRAIN)
            *reinterpret_cast<float4*>(xhat + (long long)row * SSP_H + c) =
                make_float4((v[i].x - mean) * rstd, (v[i].y - mean) * rstd, (v[i].z - mean) * rstd, (v[i].w - mean) * rstd);
    }
}
__global__ __launch_bounds__(256) void k_layernorm512(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                      int rows, float* __restrict__ out) {
    layernorm512_row<false>(x, w, b, rows, out, nullptr, nullptr);
}

// multi-head attention over short sequences: one wave per (sequence, head), lane = channel of the 64-wide head.
//   logits[i][j] = q_i . k_j / 8, masked entries -1e3 (transformer_modules.py:36-53), softmax over ALL Tk keys, ctx = weights . v
// mask_tok (optional): decoder self-attention, key j visible to query i iff j <= i and tok[s][j] != 0 (sort_modules.py:121-128);
// a query with no visible key gets the uniform softmax of Tk equal logits, as in the reference.
// TRAIN (k_ssp_mha_train): the softmax weights go to the tape (P (S, 8, Tq, Tk), before dropout) and the optional keep bytes of the
// site (same shape, 1 = keep) scale them by 1 / (1 - p) or zero them - dropout on the softmax OUTPUT, no renormalisation.
template <bool TRAIN>
__device__ __forceinline__ void ssp_mha_wave(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int Tq, int Tk,
                                             const int* __restrict__ mask_tok, int ld_tok, float* __restrict__ ctx, float* __restrict__ P,
                                             const uint8_t* __restrict__ keep, float scale) {
    const int s = blockIdx.x, hd = blockIdx.y, lane = threadIdx.x;
    const long long col = (long long)hd * SSP_HD + lane;
    float kk[SSP_LEN + 1], vv[SSP_LEN + 1];
#pragma unroll
    for (int j = 0; j < SSP_LEN + 1; ++j) {
        kk[j] = j < Tk ? k[((long long)s * Tk + j) * SSP_H + col] : 0.f;
        vv[j] = j < Tk ? v[((long long)s * Tk + j) * SSP_H + col] : 0.f;
    }
    for (int i = 0; i < Tq; ++i) {
        const float qi = q[((long long)s * Tq + i) * SSP_H + col];
        float lg[SSP_LEN + 1];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < SSP_LEN + 1; ++j) {
            if (j < Tk) {
                float d = wave_sum(qi * kk[j]) * 0.125f;
                if (mask_tok && !(j <= i && mask_tok[s * ld_tok + j] != 0)) d = -1e3f;
                lg[j] = d;
                mx = fmaxf(mx, d);
            }
        }
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < SSP_LEN + 1; ++j)
            if (j < Tk) { lg[j] = expf(lg[j] - mx); se += lg[j]; }
        float o = 0.f;
        const long long pw = (((long long)s * SSP_HEADS + hd) * Tq + i) * Tk;
#pragma unroll
        for (int j = 0; j < SSP_LEN + 1; ++j)
            if (j < Tk) {
                float pj = lg[j] / se;
                if (TRAIN) {
                    if (lane == j) P[pw + j] = pj;
                    if (keep) pj = keep[pw + j] ? pj * scale : 0.f;
                }
                o += pj * vv[j];
            }
        ctx[((long long)s * Tq + i) * SSP_H + col] = o;
    }
}
__global__ __launch_bounds__(64) void k_ssp_mha(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int Tq, int Tk,
                                                const int* __restrict__ mask_tok, int ld_tok, float* __restrict__ ctx) {
    ssp_mha_wave<false>(q, k, v, Tq, Tk, mask_tok, ld_tok, ctx, nullptr, nullptr, 1.f);
}

// one step of the greedy "pick from the remaining roles" decode (sort_model.py:146-175): one wave per sequence.
//   logits (S, 26) = expander(state of the last position); among the roles still remaining (in their input order) the one
//   with the largest log-prob (first maximum) is emitted, removed, and becomes the next input token.
__global__ __launch_bounds__(64) void k_ssp_select(const float* __restrict__ logits, const int* __restrict__ roles, int* __restrict__ remain,
                                                   int t, int S, int* __restrict__ tokens /* (S, 11) */, int* __restrict__ pred, float* __restrict__ logp) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const float x = lane < SSP_ROLES ? logits[s * SSP_ROLES + lane] : -INFINITY;
    const float mx = wave_max(x);
    const float se = wave_sum(lane < SSP_ROLES ? expf(x - mx) : 0.f);
    const float lse = mx + logf(se);
    float best = -INFINITY;
    int at = -1;
    if (lane == 0) {
        for (int j = 0; j < SSP_LEN; ++j)
            if (remain[s * SSP_LEN + j]) {
                const float lp = logits[s * SSP_ROLES + roles[s * SSP_LEN + j]] - lse;
                if (lp > best) { best = lp; at = j; }              // strict: first maximum
            }
        int tok = 0;
        if (at >= 0) {
            tok = roles[s * SSP_LEN + at];
            remain[s * SSP_LEN + at] = 0;
            pred[s * SSP_LEN + t] = tok;
            logp[s * SSP_LEN + t] = best;
        }
        tokens[s * (SSP_LEN + 1) + t + 1] = tok;
    }
}

// A role id outside [0, SSP_ROLES) is not "remaining" (k_ssp_select indexes the 26 logits with it); the reference raises IndexError in
// its embedding for such an id (sort_model.py:108), the host wrapper does the same before the call.
__global__ void k_ssp_init(const int* __restrict__ roles, int S, int* __restrict__ remain, int* __restrict__ tokens, int* __restrict__ pred,
                           float* __restrict__ logp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S * SSP_LEN) {
        const int r = roles[i];
        const bool ok = r >= 0 && r < SSP_ROLES;
        remain[i] = ok && r != 0;
        pred[i] = 0;
        logp[i] = 0.f;
    }
    if (i < S * (SSP_LEN + 1)) tokens[i] = 0;
}

// gather the last position's rows: out[s] = x[s * T + T - 1]
__global__ __launch_bounds__(128) void k_ssp_last(const float* __restrict__ x, int T, float* __restrict__ out) {
    const int s = blockIdx.x;
    *reinterpret_cast<float4*>(out + (long long)s * SSP_H + threadIdx.x * 4) =
        *reinterpret_cast<const float4*>(x + ((long long)s * T + T - 1) * SSP_H + threadIdx.x * 4);
}

// ---------------------------------------------------------------------------------------------- Sinkhorn + assignment
// cat[r] = [t1 (128) | v2 (128) | pos (4)] from the two MLP branches and the raw position columns of the input row
__global__ void k_sh_cat(const float* __restrict__ t1, const float* __restrict__ v2, const float* __restrict__ seq, int rows, float* __restrict__ cat) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)rows * 260) return;
    const int r = (int)(i / 260), c = (int)(i % 260);
    cat[i] = c < 128 ? t1[(long long)r * 128 + c] : c < 256 ? v2[(long long)r * 128 + c - 128] : seq[(long long)r * 2352 + 2348 + c - 256];
}

// n_iters x (column-normalise, row-normalise) of the N x N matrix of one wave (N <= 16) with the reference's eps 10e-8
// (sinkhorn_network.py:30-37).  div (optional, (2 n_iters, N)): the divisors, in the order they are applied - the tape of the
// training forward (k_sinkhorn_train_fwd); the arithmetic does not depend on it, so both callers produce the same bits.
__device__ __forceinline__ void sinkhorn_normalise(float (*x)[17], int N, int n_iters, int lane, float* __restrict__ div) {
    for (int it = 0; it < n_iters; ++it) {
        if (lane < N) {                                  // x / (eps + sum over rows): lane = column
            float s = 0.f;
            for (int r = 0; r < N; ++r) s += x[r][lane];
            s += 10e-8f;
            if (div) div[(2 * it) * N + lane] = s;
            for (int r = 0; r < N; ++r) x[r][lane] = x[r][lane] / s;
        }
        __syncthreads();
        if (lane < N) {                                  // x / (eps + sum over columns): lane = row
            float s = 0.f;
            for (int c = 0; c < N; ++c) s += x[lane][c];
            s += 10e-8f;
            if (div) div[(2 * it + 1) * N + lane] = s;
            for (int c = 0; c < N; ++c) x[lane][c] = x[lane][c] / s;
        }
        __syncthreads();
    }
}

// One wave per item: x = exp(tanh(fc) / tau) (N x N, N <= 16), n_iters x (column-normalise, row-normalise) with the reference's
// eps 10e-8 (sinkhorn_network.py:30-37), then the assignment of eval_coco.py:185-189 on mx = x^T: columns chosen so that
// sum(max(mx) - mx[row][col]) is minimal (Kuhn-Munkres with potentials, O(N^3), fp64, lane 0).  assign[row] = column.
__global__ __launch_bounds__(64) void k_sinkhorn_assign(const float* __restrict__ fc /* (Q, N, N): tanh already applied */, int N, int n_iters,
                                                        float tau, float* __restrict__ tr, int* __restrict__ assign) {
    __shared__ float x[16][17];
    __shared__ double cost[16][16];
    const int qi = blockIdx.x, lane = threadIdx.x;
    const float* f = fc + (long long)qi * N * N;
    for (int i = lane; i < N * N; i += 64) x[i / N][i % N] = expf(f[i] / tau);
    __syncthreads();
    sinkhorn_normalise(x, N, n_iters, lane, nullptr);
    if (tr)
        for (int i = lane; i < N * N; i += 64) tr[(long long)qi * N * N + i] = x[i / N][i % N];
    if (lane == 0) {
        double mxv = -1e300;
        for (int r = 0; r < N; ++r)
            for (int c = 0; c < N; ++c) mxv = fmax(mxv, (double)x[r][c]);
        for (int r = 0; r < N; ++r)
            for (int c = 0; c < N; ++c) cost[r][c] = mxv - (double)x[c][r];      // mx = x^T
        // Hungarian algorithm (potentials u, v; p[j] = row matched to column j), 1-based as in the classic formulation
        double u[17], v[17], minv[17];
        int p[17], way[17];
        bool used[17];
        for (int i = 0; i <= N; ++i) { u[i] = 0; v[i] = 0; p[i] = 0; way[i] = 0; }
        for (int i = 1; i <= N; ++i) {
            p[0] = i;
            int j0 = 0;
            for (int j = 0; j <= N; ++j) { minv[j] = 1e300; used[j] = false; }
            do {
                used[j0] = true;
                const int i0 = p[j0];
                double delta = 1e300;
                int j1 = 0;
                for (int j = 1; j <= N; ++j)
                    if (!used[j]) {
                        const double cur = cost[i0 - 1][j - 1] - u[i0] - v[j];
                        if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
                        if (minv[j] < delta) { delta = minv[j]; j1 = j; }
                    }
                for (int j = 0; j <= N; ++j)
                    if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
                    else minv[j] -= delta;
                j0 = j1;
            } while (p[j0] != 0);
            do {
                const int j1 = way[j0];
                p[j0] = p[j1];
                j0 = j1;
            } while (j0);
        }
        for (int j = 1; j <= N; ++j) assign[(long long)qi * N + p[j] - 1] = j - 1;
    }
}

// ---------------------------------------------------------------------------------------------- SinkhornNet training
// TAPE of the Sinkhorn part (chosen: the DIVISORS, 2 n_iters N floats per item, not the O(n_iters N^2) intermediate matrices).
// With y = x / d, d = eps + sum of x along the normalised axis, the backward of one normalisation is
//     dx = (dy - sum(dy . y)) / d        (sum along the same axis)
// and x = y d rebuilds the step's input from its output, so the walk back needs tr, the divisors and nothing else.  The rebuilt
// x differs from the forward's by one rounding per step; the first matrix exp(tanh / tau) is recomputed from the taped tanh.

// The tape's header: what the forward ran with, written by the forward and read by the backward.
constexpr int SH_TAPE_HDR_INTS = 4;      // [0] n_iters, [1] the bits of tau, [2] N, [3] unused

// the training forward's Sinkhorn: k_sinkhorn_assign's arithmetic (same helper, same order => the same bits in tr) without the
// assignment; div (Q, 2 n_iters, N) receives the divisors, hdr the n_iters and tau they belong to.  One wave per item.
__global__ __launch_bounds__(64) void k_sinkhorn_train_fwd(const float* __restrict__ th /* (Q, N, N): tanh output */, int N, int n_iters, float tau,
                                                           float* __restrict__ tr, float* __restrict__ tr_tape, float* __restrict__ div, int* __restrict__ hdr) {
    __shared__ float x[16][17];
    const int qi = blockIdx.x, lane = threadIdx.x;
    if (qi == 0 && lane < SH_TAPE_HDR_INTS) hdr[lane] = lane == 0 ? n_iters : lane == 1 ? __float_as_int(tau) : lane == 2 ? N : 0;
    const float* f = th + (long long)qi * N * N;
    for (int i = lane; i < N * N; i += 64) x[i / N][i % N] = expf(f[i] / tau);
    __syncthreads();
    sinkhorn_normalise(x, N, n_iters, lane, div + (long long)qi * 2 * n_iters * N);
    for (int i = lane; i < N * N; i += 64) {
        const float v = x[i / N][i % N];
        tr[(long long)qi * N * N + i] = v;
        tr_tape[(long long)qi * N * N + i] = v;
    }
}

// Backward of the Sinkhorn part, one wave per item (N <= 16): d_tr -> the 2 n_iters normalisations walked backwards -> exp(. / tau)
// -> tanh -> d_pre (Q N, ld) = the gradient of W_fc's pre-activation; columns N .. ld - 1 (the k padding of the GEMMs that read it)
// receive zeros.  Every sum is a sequential loop of one lane: no atomics, the same bits on every run.  n_iters and tau are the
// FORWARD's, from the tape's header (n_iters clamped to the max_iters pairs of divisor rows an item's slot holds).
__global__ __launch_bounds__(64) void k_sinkhorn_bwd(const int* __restrict__ hdr, int max_iters, const float* __restrict__ tr, const float* __restrict__ div,
                                                     const float* __restrict__ th, const float* __restrict__ d_tr, int N, float* __restrict__ d_pre, int ld) {
    __shared__ float y[16][17], g[16][17];
    const int qi = blockIdx.x, lane = threadIdx.x;
    const int n_iters = min(max(hdr[0], 0), max_iters);
    const float tau = __int_as_float(hdr[1]);
    const long long base = (long long)qi * N * N;
    for (int i = lane; i < N * N; i += 64) { y[i / N][i % N] = tr[base + i]; g[i / N][i % N] = d_tr[base + i]; }
    __syncthreads();
    const float* dv = div + (long long)qi * 2 * n_iters * N;
    for (int it = n_iters - 1; it >= 0; --it) {
        if (lane < N) {                                  // the row normalisation: lane = row
            const float d = dv[(2 * it + 1) * N + lane];
            float s = 0.f;
            for (int c = 0; c < N; ++c) s += g[lane][c] * y[lane][c];
            for (int c = 0; c < N; ++c) { g[lane][c] = (g[lane][c] - s) / d; y[lane][c] = y[lane][c] * d; }
        }
        __syncthreads();
        if (lane < N) {                                  // the column normalisation: lane = column
            const float d = dv[(2 * it) * N + lane];
            float s = 0.f;
            for (int r = 0; r < N; ++r) s += g[r][lane] * y[r][lane];
            for (int r = 0; r < N; ++r) { g[r][lane] = (g[r][lane] - s) / d; y[r][lane] = y[r][lane] * d; }
        }
        __syncthreads();
    }
    for (int i = lane; i < N * ld; i += 64) {
        const int r = i / ld, c = i % ld;
        float o = 0.f;
        if (c < N) {
            const float t = th[base + r * N + c];
            o = g[r][c] * (expf(t / tau) / tau) * (1.f - t * t);
        }
        d_pre[((long long)qi * N + r) * ld + c] = o;
    }
}

// The location loss of train_sinkhorn.py:207-209 for Q items, one wave per item (lane = column j of tr):
//   resort_j = sum_i tr_locs[q][i] tr[q][i][j];   loss_items[q] = mean_j (resort_j - gt_locs[q][j])^2
//   d_tr[q][i][j] = scale (2 / N) (resort_j - gt_j) tr_locs[q][i]          (the gradient of scale x sum_q loss_items[q])
// The N squares are added by lane 0 in column order.
__global__ __launch_bounds__(64) void k_sinkhorn_loc_loss(const float* __restrict__ tr, const float* __restrict__ tr_locs, const float* __restrict__ gt_locs,
                                                          int N, float scale, float* __restrict__ loss_items, float* __restrict__ d_tr) {
    __shared__ float diff[16];
    const int qi = blockIdx.x, lane = threadIdx.x;
    const float* t = tr + (long long)qi * N * N;
    const float* a = tr_locs + (long long)qi * N;
    if (lane < N) {
        float s = 0.f;
        for (int i = 0; i < N; ++i) s += a[i] * t[i * N + lane];
        diff[lane] = s - gt_locs[(long long)qi * N + lane];
    }
    __syncthreads();
    if (lane == 0) {
        float s = 0.f;
        for (int j = 0; j < N; ++j) s += diff[j] * diff[j];
        loss_items[qi] = s / (float)N;
    }
    if (d_tr) {
        const float k = scale * 2.f / (float)N;
        for (int i = lane; i < N * N; i += 64) d_tr[(long long)qi * N * N + i] = k * diff[i % N] * a[i / N];
    }
}

// ---------------------------------------------------------------------------------------------- S-SSP training
// S_SSP.forward (sort_model.py:80-103): the encoder on (verb, roles), the decoder teacher-forced in ONE pass over [bos, gt_0 .. gt_9],
// the label-smoothed KL loss.  Rows: encoder r = s * 10 + j, decoder r = s * 11 + t.  Dropout masks are DATA: a byte per element
// (1 = keep) of each of the 33 tensors nn.Dropout sees, in the reference's call order (ssp.inc.h: ssp_sites); a kernel that already
// touches an element applies keep / (1 - p).  No float atomics: every sum below has a fixed order.
constexpr int SSP_TD = SSP_LEN + 1;
constexpr int SSP_SITES = 33;
constexpr uint32_t SSP_DROPOUT_STREAM = 0x53535044u;       // "SSPD": the Philox counter word that keeps this use apart from the samplers'
constexpr float SSP_CONFIDENCE = 0.9f;                     // LabelSmoothingKLDivLoss(0.1, 26): 1 - label_smoothing at the target
// The tape's header, written by the forward, read by the backward's kernels:
//   [0] S   [1] bits of the p the forward applied (0.0 when it ran without masks)   [2] 1 = it ran with masks   [3] bits of sum(m)
//   [4 .. 29] bits of the 26 off-target values of the forward's label_smooth.one_hot buffer
constexpr int SSP_TAPE_HDR_INTS = 32;

struct SspSites { long long off[SSP_SITES + 1]; long long n[SSP_SITES]; };      // byte offset (16-aligned) and element count per site

// keep iff u01 >= p; element e of a site draws word e % 4 of Philox(key = seed, counter = (e / 4, site, 0, SSP_DROPOUT_STREAM)).
// One thread per 4 bytes of the buffer (sites start on 16-byte boundaries: a group never straddles two); alignment gaps get 0.
__global__ __launch_bounds__(256) void k_ssp_dropout_masks(const SspSites st, uint64_t seed, float p, uint8_t* __restrict__ masks) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g * 4 >= st.off[SSP_SITES]) return;
    int site = 0;
    for (int i = 1; i < SSP_SITES; ++i)
        if (g * 4 >= st.off[i]) site = i;
    const long long e = g * 4 - st.off[site];
    uint32_t r[4];
    Philox::gen(seed, (uint32_t)(e >> 2), (uint32_t)site, 0u, SSP_DROPOUT_STREAM, r);
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (e + i < st.n[site] && Philox::u01(r[i]) >= p) w |= 1u << (8 * i);
    reinterpret_cast<uint32_t*>(masks)[g] = w;
}

// the factors of four consecutive elements: keep ? scale : 0 (all 1 without masks); idx a multiple of 4
__device__ __forceinline__ float4 ssp_keep4(const uint8_t* __restrict__ keep, long long idx, float scale) {
    if (!keep) return make_float4(1.f, 1.f, 1.f, 1.f);
    const uint32_t w = *reinterpret_cast<const uint32_t*>(keep + idx);
    return make_float4((w & 0xffu) ? scale : 0.f, (w & 0xff00u) ? scale : 0.f, (w & 0xff0000u) ? scale : 0.f, (w & 0xff000000u) ? scale : 0.f);
}

// ids as the kernels want them: verbs % 10000 (sort_model.py:81) as int32, roles and gt with ids outside [0, 26) read as 0 (the host
// wrapper raises for those before it calls), tok (S, 11) = [0, gt_0 .. gt_9]
__global__ void k_ssp_train_prep(const int64_t* __restrict__ verbs, const int* __restrict__ roles, const int* __restrict__ gt, int S, int n_verbs,
                                 int* __restrict__ verbs32, int* __restrict__ roles_c, int* __restrict__ gt_c, int* __restrict__ tok) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    auto clean = [](int r) { return (r < 0 || r >= SSP_ROLES) ? 0 : r; };
    if (i < S * SSP_TD) {
        const int s = i / SSP_TD, t = i - s * SSP_TD;
        tok[i] = t == 0 ? 0 : clean(gt[s * SSP_LEN + t - 1]);
    }
    if (i < S * SSP_LEN) { roles_c[i] = clean(roles[i]); gt_c[i] = clean(gt[i]); }
    if (i < S) {
        const long long v = verbs[i] % 10000;
        verbs32[i] = (v < 0 || v >= n_verbs) ? 0 : (int)v;
    }
}

// x[s, j, :] = drop(sqrt(512) table[tok[s, j]]) (+ drop(sqrt(512) vtable[verb[s]]), one mask row per sequence: site 0 is (S, 1, 512))
__global__ __launch_bounds__(128) void k_ssp_embed_train(const int* __restrict__ tok, int len, const float* __restrict__ table, const int* __restrict__ verbs32,
                                                         const float* __restrict__ vtable, const uint8_t* __restrict__ keep_tok,
                                                         const uint8_t* __restrict__ keep_verb, float scale, float* __restrict__ out) {
    const int row = blockIdx.x, s = row / len, c = threadIdx.x * 4;
    const float sc = 22.627416997969522f;             // sqrt(512)
    const float4 a = *reinterpret_cast<const float4*>(table + (long long)tok[row] * SSP_H + c);
    const float4 ka = ssp_keep4(keep_tok, (long long)row * SSP_H + c, scale);
    float4 o = make_float4(a.x * sc * ka.x, a.y * sc * ka.y, a.z * sc * ka.z, a.w * sc * ka.w);
    if (verbs32) {
        const float4 b = *reinterpret_cast<const float4*>(vtable + (long long)verbs32[s] * SSP_H + c);
        const float4 kb = ssp_keep4(keep_verb, (long long)s * SSP_H + c, scale);
        o = make_float4(b.x * sc * kb.x + o.x, b.y * sc * kb.y + o.y, b.z * sc * kb.z + o.z, b.w * sc * kb.w + o.w);
    }
    *reinterpret_cast<float4*>(out + (long long)row * SSP_H + c) = o;
}

__global__ __launch_bounds__(256) void k_layernorm512_train(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, int rows,
                                                            float* __restrict__ out, float* __restrict__ xhat, float* __restrict__ rstd) {
    layernorm512_row<true>(x, w, b, rows, out, xhat, rstd);
}

// Backward of the layer norm, one wave per row as the forward: with g = dy gamma,
//     dx = rstd (g - mean(g) - x^ mean(g x^))   (+ add: the gradient that reaches x through the residual connection)
// and gx = dy x^ beside dy: d gamma and d beta are the ordered column sums (k_colsum) of gx and dy.  dx may be add's buffer.
__global__ __launch_bounds__(256) void k_layernorm512_bwd(const float* __restrict__ dy, const float* __restrict__ gamma, const float* __restrict__ xhat,
                                                          const float* __restrict__ rstd, const float* add, int rows, float* dx, float* __restrict__ gx) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const long long base = (long long)row * SSP_H;
    float4 g[2], xh[2];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = i * 256 + lane * 4;
        const float4 d = *reinterpret_cast<const float4*>(dy + base + c), w = *reinterpret_cast<const float4*>(gamma + c);
        xh[i] = *reinterpret_cast<const float4*>(xhat + base + c);
        g[i] = make_float4(d.x * w.x, d.y * w.y, d.z * w.z, d.w * w.w);
        *reinterpret_cast<float4*>(gx + base + c) = make_float4(d.x * xh[i].x, d.y * xh[i].y, d.z * xh[i].z, d.w * xh[i].w);
        s1 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
        s2 += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
    }
    const float m1 = wave_sum(s1) * (1.0f / SSP_H), m2 = wave_sum(s2) * (1.0f / SSP_H), r = rstd[row];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = i * 256 + lane * 4;
        float4 o = make_float4(r * (g[i].x - m1 - xh[i].x * m2), r * (g[i].y - m1 - xh[i].y * m2), r * (g[i].z - m1 - xh[i].z * m2), r * (g[i].w - m1 - xh[i].w * m2));
        if (add) {
            const float4 a = *reinterpret_cast<const float4*>(add + base + c);
            o = make_float4(o.x + a.x, o.y + a.y, o.z + a.z, o.w + a.w);
        }
        *reinterpret_cast<float4*>(dx + base + c) = o;
    }
}

__global__ __launch_bounds__(64) void k_ssp_mha_train(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int Tq, int Tk,
                                                      const int* __restrict__ mask_tok, int ld_tok, float* __restrict__ ctx, float* __restrict__ P,
                                                      const uint8_t* __restrict__ keep, float scale) {
    ssp_mha_wave<true>(q, k, v, Tq, Tk, mask_tok, ld_tok, ctx, P, keep, scale);
}

// Backward of k_ssp_mha_train, its mirror: one wave per (sequence, head), lane = channel.  With Pd = P keep / (1 - p) the dropped weights,
//     dv_j += Pd_ij dctx_i      dPd_ij = dctx_i . v_j      dP = dPd keep / (1 - p)      dlogit_ij = P_ij (dP_ij - sum_j' P_ij' dP_ij' / sum_j' P_ij')
//     dq_i += dlogit_ij k_j / 8      dk_j += dlogit_ij q_i / 8      for the VISIBLE (i, j) only: a masked logit is the constant -1e3
// (query 0 of the decoder sees no key: uniform weights over all keys, full gradient into v, none into q and k).
// The softmax part runs in fp64 and divides by the taped weights' own sum, so that a row's dlogits add up to zero as they do on paper: the
// gradient of linear_K's BIAS is exactly that sum weighted by q (a constant added to every key's logit changes nothing), i.e. zero, and
// the column sums of an fp32 dk would leave 1e-9 .. 1e-8 of rounding noise there where fp64 autograd leaves 1e-17.  dbk (S, 512) receives
// this wave's sum_j dk_j from the fp64 accumulators; d bias = its ordered column sum over the sequences.
__global__ __launch_bounds__(64) void k_ssp_mha_bwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                    const float* __restrict__ P, const uint8_t* __restrict__ keep, const int* __restrict__ hdr,
                                                    const float* __restrict__ dctx, int Tq, int Tk, const int* __restrict__ mask_tok, int ld_tok,
                                                    float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ dv, float* __restrict__ dbk) {
    const int s = blockIdx.x, hd = blockIdx.y, lane = threadIdx.x;
    const long long col = (long long)hd * SSP_HD + lane;
    const float scale = ssp_keep_scale(hdr);
    float kk[SSP_TD], vv[SSP_TD], dvv[SSP_TD];
    double dkk[SSP_TD];
#pragma unroll
    for (int j = 0; j < SSP_TD; ++j) {
        kk[j] = j < Tk ? k[((long long)s * Tk + j) * SSP_H + col] : 0.f;
        vv[j] = j < Tk ? v[((long long)s * Tk + j) * SSP_H + col] : 0.f;
        dkk[j] = 0.0; dvv[j] = 0.f;
    }
    for (int i = 0; i < Tq; ++i) {
        const long long row = ((long long)s * Tq + i) * SSP_H + col;
        const float qi = q[row], di = dctx[row];
        const long long pw = (((long long)s * SSP_HEADS + hd) * Tq + i) * Tk;
        double pp[SSP_TD], dp[SSP_TD];
        double dot = 0.0, sp = 0.0;
#pragma unroll
        for (int j = 0; j < SSP_TD; ++j)
            if (j < Tk) {
                const float f = keep ? (keep[pw + j] ? scale : 0.f) : 1.f;
                const float pj = P[pw + j];
                dvv[j] += pj * f * di;
                pp[j] = (double)pj;
                dp[j] = (double)(wave_sum(di * vv[j]) * f);
                dot += pp[j] * dp[j];
                sp += pp[j];
            }
        dot /= sp;
        double dqi = 0.0;
#pragma unroll
        for (int j = 0; j < SSP_TD; ++j)
            if (j < Tk) {
                const bool masked = mask_tok && !(j <= i && mask_tok[s * ld_tok + j] != 0);
                const double dl = masked ? 0.0 : pp[j] * (dp[j] - dot) * 0.125;
                dqi += dl * (double)kk[j];
                dkk[j] += dl * (double)qi;
            }
        dq[row] = (float)dqi;
    }
    double bs = 0.0;
#pragma unroll
    for (int j = 0; j < SSP_TD; ++j)
        if (j < Tk) {
            dk[((long long)s * Tk + j) * SSP_H + col] = (float)dkk[j];
            dv[((long long)s * Tk + j) * SSP_H + col] = dvv[j];
            bs += dkk[j];
        }
    dbk[(long long)s * SSP_H + col] = (float)bs;
}

// the gradient of x where y = drop(x): out = keep ? in scale : 0; n a multiple of 4
__global__ void k_ssp_drop_bwd(const float* __restrict__ in, const uint8_t* __restrict__ keep, const int* __restrict__ hdr, long long n, float* __restrict__ out) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float4 f = ssp_keep4(keep, i, ssp_keep_scale(hdr)), v = *reinterpret_cast<const float4*>(in + i);
    *reinterpret_cast<float4*>(out + i) = make_float4(v.x * f.x, v.y * f.y, v.z * f.z, v.w * f.w);
}

// The label-smoothed KL term of one row (compute_loss, sort_model.py:66-78; LabelSmoothingKLDivLoss), one wave per row (lane = class):
//   logp = log_softmax(logits) -> the tape;   target [gt_0 .. gt_9, 0][t];   q = one_hot[c] (the module's buffer), 0.9 at the target
//   row_loss = m sum_c q_c (log q_c - logp_c),   m = [1, gt_0 != 0, .., gt_9 != 0][t]  (11 entries: decoder_mask[:, :-1])
__global__ __launch_bounds__(256) void k_ssp_kl_loss(const float* __restrict__ logits, const int* __restrict__ gt, const float* __restrict__ one_hot, int R,
                                                     float* __restrict__ logp, float* __restrict__ row_loss) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const int s = row / SSP_TD, t = row - s * SSP_TD;
    const bool live = lane < SSP_ROLES;
    const float x = live ? logits[(long long)row * SSP_ROLES + lane] : -INFINITY;
    const float mx = wave_max(x);
    const float se = wave_sum(live ? expf(x - mx) : 0.f);
    const float lp = x - mx - logf(se);
    const int tgt = t < SSP_LEN ? gt[s * SSP_LEN + t] : 0;
    const bool m = t == 0 || gt[s * SSP_LEN + t - 1] != 0;
    float term = 0.f;
    if (live) {
        const float qc = lane == tgt ? SSP_CONFIDENCE : one_hot[lane];
        term = qc * (logf(qc) - lp);
        logp[(long long)row * SSP_ROLES + lane] = lp;
    }
    term = wave_sum(term);
    if (lane == 0) row_loss[row] = m ? term : 0.f;
}

// loss = sum of the row terms / sum(m), both added in a fixed order by ONE block (the row terms in fp64); sum(m) >= S: never zero.
// Writes the tape's header.
__global__ __launch_bounds__(256) void k_ssp_loss_finish(const float* __restrict__ row_loss, const int* __restrict__ gt, const float* __restrict__ one_hot, int S,
                                                         float p_applied, int with_masks, float* __restrict__ loss, int* __restrict__ hdr) {
    __shared__ double acc[256];
    __shared__ int cnt[256];
    double a = 0.0;
    int n = 0;
    for (int r = threadIdx.x; r < S * SSP_TD; r += 256) {
        const int s = r / SSP_TD, t = r - s * SSP_TD;
        a += (double)row_loss[r];
        n += (t == 0 || gt[s * SSP_LEN + t - 1] != 0) ? 1 : 0;
    }
    acc[threadIdx.x] = a; cnt[threadIdx.x] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { acc[threadIdx.x] += acc[threadIdx.x + o]; cnt[threadIdx.x] += cnt[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)(acc[0] / (double)cnt[0]);
        hdr[0] = S; hdr[1] = __float_as_int(p_applied); hdr[2] = with_masks; hdr[3] = __float_as_int((float)cnt[0]);
        hdr[30] = 0; hdr[31] = 0;
    }
    if (threadIdx.x < SSP_ROLES) hdr[4 + threadIdx.x] = __float_as_int(one_hot[threadIdx.x]);
}

// d logits (R, ld) = d_loss (m / sum(m)) (softmax sum(q) - q), sum(q) = 0.9 + 25 off-target values (not 1); columns 26 .. ld - 1 (the
// k padding of the products that read it) receive zeros; q's off-target values are the forward's, from the header.  A tape whose header does not carry this call's S and mask mode was not
// written by the forward this backward belongs to: every gradient then comes out NaN.
__global__ void k_ssp_kl_bwd(const float* __restrict__ logp, const int* __restrict__ gt, const int* __restrict__ hdr, int S, int with_masks, const float* __restrict__ d_loss, int R, int ld, float* __restrict__ dlog) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)R * ld) return;
    const int row = (int)(i / ld), c = (int)(i % ld);
    float o = 0.f;
    if (c < SSP_ROLES) {
        const int s = row / SSP_TD, t = row - s * SSP_TD;
        const int tgt = t < SSP_LEN ? gt[s * SSP_LEN + t] : 0;
        const bool m = t == 0 || gt[s * SSP_LEN + t - 1] != 0;
        float sq = 0.f;
        for (int k = 0; k < SSP_ROLES; ++k) sq += k == tgt ? SSP_CONFIDENCE : __int_as_float(hdr[4 + k]);
        const float qc = c == tgt ? SSP_CONFIDENCE : __int_as_float(hdr[4 + c]);
        if (m) o = (d_loss[0] / __int_as_float(hdr[3])) * (expf(logp[(long long)row * SSP_ROLES + c]) * sq - qc);
        if (hdr[0] != S || hdr[2] != with_masks) o = __int_as_float(0x7fc00000);
    }
    dlog[i] = o;
}

// d sr_embed_layer.weight (26, 512): the index inverted.  One block per (table row, 64-column chunk) scans the Re encoder ids, then the
// Rd decoder ids, in four interleaved phases that are added in a fixed order; the dropout bytes of sites 1 and 14 and sqrt(512) applied here.
__global__ __launch_bounds__(256) void k_ssp_sr_embed_bwd(const int* __restrict__ roles, const float* __restrict__ d_enc, const uint8_t* __restrict__ keep_enc, int Re,
                                                          const int* __restrict__ tok, const float* __restrict__ d_dec, const uint8_t* __restrict__ keep_dec, int Rd,
                                                          const int* __restrict__ hdr, float* __restrict__ out) {
    __shared__ float red[4][64];
    const int id = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    const float scale = ssp_keep_scale(hdr);
    float acc = 0.f;
    for (int r = ph; r < Re; r += 4)
        if (roles[r] == id) {
            const long long at = (long long)r * SSP_H + c;
            acc += keep_enc ? (keep_enc[at] ? d_enc[at] * scale : 0.f) : d_enc[at];
        }
    for (int r = ph; r < Rd; r += 4)
        if (tok[r] == id) {
            const long long at = (long long)r * SSP_H + c;
            acc += keep_dec ? (keep_dec[at] ? d_dec[at] * scale : 0.f) : d_dec[at];
        }
    red[ph][threadIdx.x & 63] = acc;
    __syncthreads();
    if (ph == 0) out[(long long)id * SSP_H + c] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x])) * 22.627416997969522f;
}

// d v_embed_layer.weight (n_verbs, 512), dense as nn.Embedding gives it: one block per table row scans the S verbs in order; a sequence
// contributes the sum over its 10 positions (the verb embedding is broadcast over them) under its ONE mask row of site 0.  Unused rows: 0.
__global__ __launch_bounds__(128) void k_ssp_v_embed_bwd(const int* __restrict__ verbs32, const float* __restrict__ d_enc, const uint8_t* __restrict__ keep,
                                                         const int* __restrict__ hdr, int S, float* __restrict__ out) {
    const int id = blockIdx.x, c = threadIdx.x * 4;
    const float scale = ssp_keep_scale(hdr);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s)
        if (verbs32[s] == id) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = 0; j < SSP_LEN; ++j) {
                const float4 d = *reinterpret_cast<const float4*>(d_enc + ((long long)s * SSP_LEN + j) * SSP_H + c);
                t = make_float4(t.x + d.x, t.y + d.y, t.z + d.z, t.w + d.w);
            }
            const float4 f = ssp_keep4(keep, (long long)s * SSP_H + c, scale);
            acc = make_float4(acc.x + t.x * f.x, acc.y + t.y * f.y, acc.z + t.z * f.z, acc.w + t.w * f.w);
        }
    const float sc = 22.627416997969522f;
    *reinterpret_cast<float4*>(out + (long long)id * SSP_H + c) = make_float4(acc.x * sc, acc.y * sc, acc.z * sc, acc.w * sc);
}

}  // namespace vsr
