// GEMM routing result -> kernel launch.  The ONE switch from a GemmRoute to a template instance: the library (GemmBuilder::launch)
// and tools/gemm_bench both launch every shipped instantiation through gemm_dispatch().
#pragma once
#include <type_traits>

#include "gemm_f32.h"
#include "gemm_bf16.h"
#include "gemm_x3.h"
#include "gemm_x3s.h"
#include "gemm_h2.h"
#include "gemm_h2a.h"
#include "gemm_b16a.h"

namespace vsr {

enum class GemmKernel {
    F32,       // exact fp32 MFMA (32x32x2), 64 / 128-row tiles                                 gemm_f32.h
    F32_R16,   // ... rows-16 kernel (16x16x4) for short problems
    BF16W,     // bf16 mode, register-staged (bf16 images of W, optionally of A)                gemm_bf16.h
    X3,        // f32x3: fp32 products through three bf16 terms per operand                     gemm_x3.h
    X3S,       // ... weight-streaming kernel for launches of one m-tile                        gemm_x3s.h
    H2,        // f16x2: fp16-pair images of W, fp32 A split in the kernel                      gemm_h2.h
    H2S,       // ... weight-streaming kernel
    H2A,       // ... all-DMA kernel: images of both operands                                   gemm_h2a.h
    B16A       // bf16 mode, all-DMA kernel: bf16 images of both operands                       gemm_b16a.h
};

// What GemmBuilder::finish() decides besides the plan in GemmArgs.  The workgroup tile is (tm ? 64 tm : 16 mt) rows x 64 tn columns
// for every kernel.
struct GemmRoute {
    GemmKernel kernel = GemmKernel::F32;
    int tm = 1, tn = 1;   // tile in units of 64 rows / 64 columns (tm = 0: the rows come in 16-row tiles, mt)
    int mt = 0;           // F32_R16, X3S, H2S: 16-row tiles of A per workgroup, 1..8
    int mf = 16;          // H2A: MFMA shape of the multipliers, 16 (16x16x32) or 32 (32x32x16)
    bool a16 = false;     // BF16W: every segment's A operand has a bf16 image (GemmSeg::A16)
};

inline int gemm_threads(GemmKernel k) {
    switch (k) {
        case GemmKernel::BF16W: case GemmKernel::B16A: return B16_THREADS;
        case GemmKernel::X3: case GemmKernel::H2: case GemmKernel::H2A: return X3_THREADS;      // (= H2_THREADS)
        case GemmKernel::F32_R16: return 512;
        default: return 256;                                                                      // (F32; X3S_THREADS = H2S_THREADS)
    }
}

// runtime 1..8 -> compile-time constant: f(std::integral_constant<int, v>); anything else runs as 8
template <class F> inline void with_const_1to8(int v, F&& f) {
    switch (v) {
        case 1: f(std::integral_constant<int, 1>{}); break;     case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;     case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;     case 6: f(std::integral_constant<int, 6>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;     default: f(std::integral_constant<int, 8>{}); break;
    }
}

inline void gemm_dispatch(const GemmRoute& r, const GemmArgs& a, hipStream_t s) {
    const dim3 grid(gemm_grid(a)), block(gemm_threads(r.kernel));
    const bool wide = r.tn == 4;            // the 128-row MFMA kernels: 128 x 256 tile (their TN = 2) or 128 x 128 (TN = 1)
#define GEMM_GO(...) hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, s, a)
    switch (r.kernel) {
        case GemmKernel::F32:
            if (r.tm == 2 && r.tn == 2) GEMM_GO(gemm_nt_f32_kernel<2, 2>);
            else if (r.tm == 2) GEMM_GO(gemm_nt_f32_kernel<2, 1>);
            else GEMM_GO(gemm_nt_f32_kernel<1, 1>);
            break;
        case GemmKernel::F32_R16:
            with_const_1to8(r.mt, [&](auto MT) { GEMM_GO(gemm_nt_f32_r16_kernel<decltype(MT)::value, 2>); });
            break;
        case GemmKernel::BF16W:
            if (r.a16) { if (wide) GEMM_GO(gemm_nt_bf16w_kernel<true, 2>); else GEMM_GO(gemm_nt_bf16w_kernel<true, 1>); }
            else { if (wide) GEMM_GO(gemm_nt_bf16w_kernel<false, 2>); else GEMM_GO(gemm_nt_bf16w_kernel<false, 1>); }
            break;
        case GemmKernel::X3:
            if (wide) GEMM_GO(gemm_nt_x3_kernel<2, 2>); else GEMM_GO(gemm_nt_x3_kernel<2, 1>); break;
        case GemmKernel::X3S:
            with_const_1to8(r.mt, [&](auto MT) { GEMM_GO(gemm_nt_x3s_kernel<decltype(MT)::value, 1>); });
            break;
        case GemmKernel::H2:
            if (wide) GEMM_GO(gemm_nt_h2_kernel<2, 2>); else GEMM_GO(gemm_nt_h2_kernel<2, 1>); break;
        case GemmKernel::H2S:
            with_const_1to8(r.mt, [&](auto MT) {
                if (r.tn == 2) GEMM_GO(gemm_nt_h2s_kernel<decltype(MT)::value, 2>); else GEMM_GO(gemm_nt_h2s_kernel<decltype(MT)::value, 1>);
            });
            break;
        case GemmKernel::H2A:   // (a ring of four stages fits the 128 x 128 tile and changes nothing: tools/gemm_bench H2_NW=4, profiles/r05_e_*)
            if (r.mf == 32) { if (wide) GEMM_GO(gemm_nt_h2a_kernel<2, 2, 3, 32>); else GEMM_GO(gemm_nt_h2a_kernel<2, 1, 3, 32>); }
            else { if (wide) GEMM_GO(gemm_nt_h2a_kernel<2, 2>); else GEMM_GO(gemm_nt_h2a_kernel<2, 1>); }
            break;
        case GemmKernel::B16A:
            if (wide) GEMM_GO(gemm_nt_b16a_kernel<2, 2>); else GEMM_GO(gemm_nt_b16a_kernel<2, 1>); break;
    }
#undef GEMM_GO
}

}  // namespace vsr
