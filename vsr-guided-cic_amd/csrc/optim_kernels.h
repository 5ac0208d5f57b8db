// The optimizer step of the library's own (vsr_adam_step): Adam over all 28 parameter tensors in ONE launch, which in the same pass leaves
// what the handle derives from the new weights - the max |p| of the tensors the f16x2 flavour scales (gemm_h2.h), or the bf16 copies of the
// 14 matrices (gemm_bf16.h).  torch.optim.Adam(fused=True) writes the weights in four launches and the refresh that has to follow reads
// them twice more; here a parameter is read once and written once per step.
//
// Per element, torch's fused kernel expression for expression (ATen/native/cuda/fused_adam_utils.cuh, ADAM_MODE::ORIGINAL, no amsgrad, no
// maximize): the hyper-parameters are doubles there, so the two moment updates and the `+ eps` are formed in double and rounded to fp32
// once; the step size, the square root and the quotient are fp32.
//     g   += p wd                                   (wd != 0; L2, not AdamW)
//     m    = beta1 m + (1 - beta1) g
//     v    = beta2 v + (1 - beta2) g g
//     p   -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)          bc1, sqrt(bc2): formed on the host in double, fp32 here
// Block -> tensor through the compare chain over static indices of gemm_h2.h's H2Multi (a run-time index into a by-value argument struct
// goes to scratch).  A tensor takes the 16-byte path only when all of its pointers are 16-byte aligned (gradients may be views of one
// flat buffer at arbitrary 4-byte offsets); the last n % 4 elements, and misaligned tensors as a whole, go element by element.  Nothing
// is read or written at or beyond n.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_bf16.h"

namespace vsr {

constexpr int ADAM_NT = 28;             // the tensors of vsr_weights
constexpr int ADAM_MAX_BLOCKS = 2048;   // 256 CUs x 8 workgroups of 256 threads: the cap of the memory-bound grid (the host takes the workgroups resident at once, if fewer); the rest is grid-stride
struct AdamMulti {
    float* p[ADAM_NT];
    const float* g[ADAM_NT];            // null: no gradient - the tensor and its moments stay, it is still measured / converted
    float* m[ADAM_NT];
    float* v[ADAM_NT];
    uint16_t* b16[ADAM_NT];             // bf16 copy to write, or null
    long long n[ADAM_NT];
    int blk[ADAM_NT + 1];               // first block of tensor i; blk[ADAM_NT] = grid size
    int slot[ADAM_NT];                  // slot of the bound table max |p_new| is folded into, or -1
};
static_assert(sizeof(AdamMulti) <= 2048, "the table travels by value: well inside the kernel-argument limit");
struct AdamHyper {
    double beta1, beta2, eps, wd;
    float step_size, bc2_sqrt;          // lr / bc1 and sqrt(bc2) of this step
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamHyper& hy) {
    if (hy.wd != 0) g = (float)((double)g + (double)p * hy.wd);
    m = (float)(hy.beta1 * (double)m + (1 - hy.beta1) * (double)g);
    v = (float)(hy.beta2 * (double)v + (1 - hy.beta2) * (double)g * (double)g);
    const float denom = (float)((double)(sqrtf(v) / hy.bc2_sqrt) + hy.eps);
    p -= hy.step_size * m / denom;
}
__device__ __forceinline__ void adam_elem4(float4& p, const float4& g, float4& m, float4& v, const AdamHyper& hy) {
    adam_elem(p.x, g.x, m.x, v.x, hy); adam_elem(p.y, g.y, m.y, v.y, hy);
    adam_elem(p.z, g.z, m.z, v.z, hy); adam_elem(p.w, g.w, m.w, v.w, hy);
}
__device__ __forceinline__ float absmax4(float mx, const float4& a) {
    return fmaxf(mx, fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))));
}
// a NaN must reach the bound as +inf (fmaxf drops it)
__device__ __forceinline__ bool nan4(const float4& a) { return !(a.x == a.x) || !(a.y == a.y) || !(a.z == a.z) || !(a.w == a.w); }
__device__ __forceinline__ void store_bf16x4(uint16_t* dst, const float4& a) {
    uint2 o;
    o.x = pack_bf16(a.x, a.y); o.y = pack_bf16(a.z, a.w);
    *reinterpret_cast<uint2*>(dst) = o;
}

__global__ __launch_bounds__(256) void k_adam_multi(const AdamMulti t, const AdamHyper hy, unsigned* __restrict__ bounds) {
    float* p = t.p[0];
    const float* g = t.g[0];
    float* m = t.m[0];
    float* v = t.v[0];
    uint16_t* b16 = t.b16[0];
    long long n = t.n[0];
    int b0 = 0, b1 = t.blk[1], slot = t.slot[0];
#pragma unroll
    for (int i = 1; i < ADAM_NT; ++i)
        if ((int)blockIdx.x >= t.blk[i]) { p = t.p[i]; g = t.g[i]; m = t.m[i]; v = t.v[i]; b16 = t.b16[i]; n = t.n[i]; b0 = t.blk[i]; b1 = t.blk[i + 1]; slot = t.slot[i]; }
    const bool upd = g != nullptr;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(b16) & 7) == 0;
    const long long nthr = (long long)(b1 - b0) * 256, tid = (long long)(blockIdx.x - b0) * 256 + threadIdx.x;
    float mx = 0.f;
    bool nan = false;
    long long tail0 = 0;                 // first element of the part taken one by one
    if (vec) {
        const long long n4 = n & ~3LL, stride = nthr * 4;
        tail0 = n4;
        long long i = tid * 4;
        if (upd) {
            // two independent rounds: eight 16-byte loads in flight per thread before the first use
            for (; i + stride < n4; i += 2 * stride) {
                float4 pa = *reinterpret_cast<const float4*>(p + i), pb = *reinterpret_cast<const float4*>(p + i + stride);
                const float4 ga = *reinterpret_cast<const float4*>(g + i), gb = *reinterpret_cast<const float4*>(g + i + stride);
                float4 ma = *reinterpret_cast<const float4*>(m + i), mb = *reinterpret_cast<const float4*>(m + i + stride);
                float4 va = *reinterpret_cast<const float4*>(v + i), vb = *reinterpret_cast<const float4*>(v + i + stride);
                adam_elem4(pa, ga, ma, va, hy);
                adam_elem4(pb, gb, mb, vb, hy);
                *reinterpret_cast<float4*>(p + i) = pa; *reinterpret_cast<float4*>(p + i + stride) = pb;
                *reinterpret_cast<float4*>(m + i) = ma; *reinterpret_cast<float4*>(m + i + stride) = mb;
                *reinterpret_cast<float4*>(v + i) = va; *reinterpret_cast<float4*>(v + i + stride) = vb;
                if (b16) { store_bf16x4(b16 + i, pa); store_bf16x4(b16 + i + stride, pb); }
                mx = absmax4(absmax4(mx, pa), pb);
                nan = nan || nan4(pa) || nan4(pb);
            }
            for (; i < n4; i += stride) {
                float4 pa = *reinterpret_cast<const float4*>(p + i);
                const float4 ga = *reinterpret_cast<const float4*>(g + i);
                float4 ma = *reinterpret_cast<const float4*>(m + i), va = *reinterpret_cast<const float4*>(v + i);
                adam_elem4(pa, ga, ma, va, hy);
                *reinterpret_cast<float4*>(p + i) = pa;
                *reinterpret_cast<float4*>(m + i) = ma;
                *reinterpret_cast<float4*>(v + i) = va;
                if (b16) store_bf16x4(b16 + i, pa);
                mx = absmax4(mx, pa);
                nan = nan || nan4(pa);
            }
        } else if (b16 || slot >= 0) {
            for (; i < n4; i += stride) {
                const float4 pa = *reinterpret_cast<const float4*>(p + i);
                if (b16) store_bf16x4(b16 + i, pa);
                mx = absmax4(mx, pa);
                nan = nan || nan4(pa);
            }
        }
    }
    if (upd || b16 || slot >= 0)
        for (long long j = tail0 + tid; j < n; j += nthr) {
            float pj = p[j];
            if (upd) {
                float mj = m[j], vj = v[j];
                adam_elem(pj, g[j], mj, vj, hy);
                p[j] = pj; m[j] = mj; v[j] = vj;
            }
            if (b16) b16[j] = (uint16_t)(pack_bf16(pj, 0.f) & 0xffffu);
            mx = fmaxf(mx, fabsf(pj));
            nan = nan || !(pj == pj);
        }
    if (slot < 0) return;                // (uniform over the block)
    if (nan) mx = __int_as_float(0x7f800000);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
        if (__float_as_uint(mx) > __atomic_load_n(bounds + slot, __ATOMIC_RELAXED)) atomicMax(bounds + slot, __float_as_uint(mx));      // (the slot only grows: skip the same-address atomic when there is nothing to add)
    }
}

}  // namespace vsr
