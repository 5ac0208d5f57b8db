// What every grouped "NT" GEMM kernel (gemm_f32.h, gemm_bf16.h, gemm_b16a.h, gemm_x3*.h, gemm_h2*.h) and their planners share:
//   * the launch description (GemmSeg / GemmProb / GemmArgs), the workgroup numbering and a workgroup's k-tile range
//   * the flavour-independent device pieces of the tile kernels: which piece of which tile a k-tile belongs to (GemmPiece), where that
//     piece goes (GemmOut), the store of four staged floats of one output row with the zero-fill of the unused slabs (gemm_store4) and
//     the k-cursor of the LDS-DMA movers (GemmKCursor)
//   * the host planners (gemm_plan: stream-K ranges; gemm_plan_aligned: k-aligned pieces) and the launch's flop / byte counts
// Deliberately NOT here: how a kernel loads its operands (the register-staged movers' open_segment / open_tile / advance, the DMA issue
// paths), its k loop, and how it stages its accumulator layout for the row stores - those are the kernels' flavours.  The streaming
// kernels (gemm_x3s.h, gemm_nt_h2s_kernel) take one k-aligned piece per workgroup and store from registers: they use none of the pieces.
// gemm_f32.h's header comment explains the stream-K decomposition and the slabs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vsr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// The limits of one grouped launch.  The planners cut no tile into more than GEMM_MAX_SLABS pieces; every consumer of slabs (slab_sum*,
// k_attend's fused sums) holds that many loads in flight, and every slab workspace is sized by it.
constexpr int GEMM_MAX_SLABS = 8;
constexpr int GEMM_MAX_PROB = 4;     // problems per launch
constexpr int GEMM_MAX_SEG = 3;      // K segments per problem

struct GemmSeg {
    const float* A;      // (rows, lda) activations
    const int* a_idx;    // optional row gather: row m reads A + a_idx[m] * lda
    const float* W;      // (N, ldw) weight window start (already offset to the segment's first column)
    int lda;
    int ldw;
    int K;               // multiple of 4
    int exp_idx;         // f16x2 kernels only (gemm_h2.h): slots of GemmArgs::exps with the power-of-two scale exponents of W's image (low 16 bits) and of A's bound (high 16 bits)
    const uint16_t* A16; // bf16 kernel only, optional: a bf16 image of A (same rows, same lda) written by A's producer
};

struct GemmProb {
    GemmSeg seg[GEMM_MAX_SEG];
    float* C;            // (nslab, M, ldc)
    long long slab_stride;
    int nseg;
    int M;
    int N;
    int ldc;
    int tiles_m;
    int tiles_n;
    int ktiles;          // 32-wide k-tiles over all segments
    int it_begin;        // first global iteration of this problem
    int g_begin;         // aligned plan only: first workgroup of this problem ...
    int split;           // ... and the number of equal k pieces every one of its tiles is cut into
    int nslab;           // slabs THIS problem's tiles write (<= GemmArgs::nslab): its consumers add exactly these
};

struct GemmArgs {
    GemmProb p[GEMM_MAX_PROB];
    int nprob;
    int total_iters;
    int G;               // workgroups with a non-empty range (1 <= G <= total_iters); grid = 8 * ceil(G / 8)
    int nslab;           // slabs per tile (S)
    int aligned;         // 0: stream-K ranges (gemm_plan); 1: one k-aligned piece of one tile per workgroup (gemm_plan_aligned)
    const int* exps;     // f16x2 kernels only: device table of scale exponents (GemmSeg::w_exp / a_exp index it)
    int xcd_chunk;       // 0: ceil(G / 8) workgroups per XCD.  > 0 (aligned plan, gemm_plan_aligned): the workgroups are dealt in whole GROUPS of
    int xcd_unit;        // xcd_unit (= tiles_m) consecutive numbers, xcd_lo groups per XCD and one more on the first xcd_extra XCDs;
    int xcd_lo, xcd_extra;   // xcd_chunk = the largest per-XCD count = xcd_unit (xcd_lo + (xcd_extra > 0))
};

// Workgroup number of this block.  Blocks are dispatched round-robin over the 8 XCDs (block b runs on XCD b & 7); XCD x takes the
// CONTIGUOUS workgroup numbers [x chunk, (x + 1) chunk): neighbouring tiles share their operand windows in that XCD's L2.
// Returns G (= "no work") for the padding blocks of the grid.
__device__ __forceinline__ int gemm_wg_of_block(const GemmArgs& a) {
    const int i = blockIdx.x >> 3, x = blockIdx.x & 7;
    if (a.xcd_chunk == 0) {
        const int ch = (a.G + 7) >> 3;
        return x * ch + i;                     // (>= G for the padding blocks)
    }
    const int mine = a.xcd_unit * (a.xcd_lo + (x < a.xcd_extra ? 1 : 0));
    const int first = a.xcd_unit * (x * a.xcd_lo + (x < a.xcd_extra ? x : a.xcd_extra));
    return i < mine ? first + i : a.G;
}
inline int gemm_grid(const GemmArgs& a) { return 8 * (a.xcd_chunk ? a.xcd_chunk : (a.G + 7) / 8); }

// tile index -> tile origin: m fastest (the m-tiles of a weight n-tile are neighbours)
__device__ __forceinline__ void gemm_tile_origin(const GemmProb& P, int tile, int BM, int BN, int& m0, int& n0) {
    m0 = (tile % P.tiles_m) * BM; n0 = (tile / P.tiles_m) * BN;
}

constexpr int GEMM_BK = 32;
constexpr int GEMM_LDS = GEMM_BK + 4;

__device__ __host__ inline int gemm_range_begin(int g, int total, int G) { return (int)(((long long)g * total) / G); }

// the k-tile range [it0, it1) of workgroup g (both plans) and, for the aligned plan, its problem / tile / piece
struct GemmRange { int it0, it1, prob, tile, piece, split; };
__device__ __forceinline__ GemmRange gemm_range(const GemmArgs& args, int g) {
    GemmRange r;
    if (!args.aligned) {
        r.it0 = gemm_range_begin(g, args.total_iters, args.G);
        r.it1 = gemm_range_begin(g + 1, args.total_iters, args.G);
        r.prob = r.tile = r.piece = r.split = 0;
        return r;
    }
    int p = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (i < args.nprob && g >= args.p[i].g_begin) p = i;
    const GemmProb& P = args.p[p];
    const int local = g - P.g_begin, tiles = P.tiles_m * P.tiles_n;
    r.prob = p;
    r.piece = local / tiles;
    r.tile = local - r.piece * tiles;
    r.split = P.split;
    const int base = P.it_begin + r.tile * P.ktiles;
    r.it0 = base + (int)(((long long)r.piece * P.ktiles) / P.split);
    r.it1 = base + (int)(((long long)(r.piece + 1) * P.ktiles) / P.split);
    return r;
}

// ---- the tile kernels' flavour-independent device pieces ------------------------------------------------------------------------
// The piece of a tile a workgroup is multiplying: problem, tile, k-tiles left before the piece is flushed, the slab it goes to, and
// whether it completes the tile (the workgroup that finishes a tile zero-fills the slabs the tile did not use).
struct GemmPiece { int prob, tile, left, piece; bool last; };

// Stream-K ranges: global k-tile `it` of workgroup g's range [.., it1) -> its piece; returns the k-tile's index inside its tile.
// (The problem is found by a compare chain over static indices and every later index is that chain's result: a run-time index hipcc
// cannot trace back to one makes it copy the whole argument struct to scratch.)
__device__ __forceinline__ int gemm_piece_streamk(const GemmArgs& args, int g, int it, int it1, GemmPiece& c) {
    int p = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (i < args.nprob && it >= args.p[i].it_begin) p = i;
    const GemmProb& P = args.p[p];
    const int local = it - P.it_begin;
    c.prob = p;
    c.tile = local / P.ktiles;
    const int kt = local - c.tile * P.ktiles;
    const int tile_base = it - kt;
    // first workgroup whose range contains the tile's first iteration
    const int g_first = (int)((((long long)tile_base + 1) * args.G - 1) / args.total_iters);
    c.piece = g - g_first;
    const int rem = P.ktiles - kt;
    c.left = rem < it1 - it ? rem : it1 - it;
    c.last = (c.left == rem);
    return kt;
}
// Either plan (the kernels that are given k-aligned plans too): an aligned workgroup has one piece of one tile, nothing to search.
__device__ __forceinline__ int gemm_piece_at(const GemmArgs& args, const GemmRange& rg, int g, int it, int it1, GemmPiece& c) {
    if (args.aligned) {
        c.prob = rg.prob; c.tile = rg.tile; c.piece = rg.piece;
        c.left = it1 - it;
        c.last = rg.piece == rg.split - 1;
        return it - (args.p[rg.prob].it_begin + rg.tile * args.p[rg.prob].ktiles);
    }
    return gemm_piece_streamk(args, g, it, it1, c);
}

// Where a piece goes: the tile's origin, the piece's slab, the number of unused slabs behind it that get zeros (a finished tile's), and
// whether rows can leave as 16-byte stores (an aligned window).  slab_stride rides along for gemm_store4.
struct GemmOut { int m0, n0; float* C; int extra; bool vec_ok; long long slab_stride; };
__device__ __forceinline__ GemmOut gemm_out_of(const GemmProb& P, const GemmPiece& c, int BM, int BN) {
    GemmOut o;
    gemm_tile_origin(P, c.tile, BM, BN, o.m0, o.n0);
    o.C = P.C + (long long)c.piece * P.slab_stride;
    o.extra = c.last ? P.nslab - 1 - c.piece : 0;
    o.vec_ok = ((P.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(P.C) & 15) == 0) && ((P.slab_stride & 3) == 0);
    o.slab_stride = P.slab_stride;
    return o;
}

// Four staged floats v of one output row -> dst = &C[m][n] (n < N) of the piece's slab, zeros to the same place of the `extra` unused
// slabs: one 16-byte store each, or element by element at an N tail or in an unaligned window.  This decides what a slab consumer reads.
__device__ __forceinline__ void gemm_store4(float* dst, const float4 v, int n, int N, const GemmOut& o) {
    if (o.vec_ok && n + 3 < N) {
        *reinterpret_cast<float4*>(dst) = v;
        for (int x = 1; x <= o.extra; ++x)
            *reinterpret_cast<float4*>(dst + (long long)x * o.slab_stride) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        const float vv[4] = {v.x, v.y, v.z, v.w};
        for (int q = 0; q < 4; ++q)
            if (n + q < N) {
                dst[q] = vv[q];
                for (int x = 1; x <= o.extra; ++x) dst[(long long)x * o.slab_stride + q] = 0.f;
            }
    }
}

// k-cursor of the LDS-DMA movers (gemm_h2.h, gemm_h2a.h, gemm_b16a.h): walks the BK-wide k-tiles of a workgroup's range across segment,
// tile and problem boundaries.  Scalars only; `fresh` tells the mover to recompute the pointers it derives from (prob, tile, seg), and the
// mover clears it.
template <int BK>
struct GemmKCursor {
    int prob, tile, tile_left, seg, seg_left, k, K;
    bool fresh;
    __device__ __forceinline__ void open(const GemmArgs& a, int prob_, int tile_, int kt) {
        prob = prob_; tile = tile_;
        const GemmProb& P = a.p[prob_];
        tile_left = P.ktiles - kt;
        int sg = 0;
        while (sg < P.nseg - 1 && kt >= (P.seg[sg].K + BK - 1) / BK) { kt -= (P.seg[sg].K + BK - 1) / BK; ++sg; }
        seg = sg; K = P.seg[sg].K; k = kt * BK; seg_left = (K + BK - 1) / BK - kt; fresh = true;
    }
    __device__ __forceinline__ void settle(const GemmArgs& a) {      // stand on a k-tile: cross segment / tile / problem boundaries
        if (tile_left == 0) {
            if (tile + 1 < a.p[prob].tiles_m * a.p[prob].tiles_n) open(a, prob, tile + 1, 0);
            else open(a, prob + 1, 0, 0);
        } else if (seg_left == 0) {
            ++seg; K = a.p[prob].seg[seg].K; k = 0; seg_left = (K + BK - 1) / BK; fresh = true;
        }
    }
    __device__ __forceinline__ void next() { k += BK; --seg_left; --tile_left; }
};


// Host side: fill tiles / iteration offsets, pick the number of workgroups and the slab count.
//   slots      resident workgroups the launch should fill (CUs x 4 for this 36.9 KB-LDS kernel)
//   min_iters  smallest range worth a workgroup (prologue + flush amortisation)
// Returns nslab; the caller then sets every problem's C / slab_stride (slabs are nslab deep).
inline int gemm_plan(GemmArgs& a, int slots, int min_iters = 8, int BM = 64, int BN = 64, int BK = GEMM_BK) {
    int total = 0, kt_max = 1;
    for (int i = 0; i < a.nprob; ++i) {
        GemmProb& p = a.p[i];
        p.tiles_m = (p.M + BM - 1) / BM;
        p.tiles_n = (p.N + BN - 1) / BN;
        p.ktiles = 0;
        for (int s = 0; s < p.nseg; ++s) p.ktiles += (p.seg[s].K + BK - 1) / BK;
        p.it_begin = total;
        total += p.tiles_m * p.tiles_n * p.ktiles;
        if (p.ktiles > kt_max) kt_max = p.ktiles;
    }
    a.total_iters = total;
    int G = total / min_iters;
    if (G > slots) G = slots;
    const int L_min = (kt_max + GEMM_MAX_SLABS - 2) / (GEMM_MAX_SLABS - 1);            // keep pieces per tile <= GEMM_MAX_SLABS
    if (G > total / L_min) G = total / L_min;
    if (G < 1) G = 1;
    a.G = G;
    const int L = total / G;                       // shortest range
    a.nslab = G == 1 ? 1 : (kt_max + L - 1) / L + 1;
    if (a.nslab > GEMM_MAX_SLABS) a.nslab = GEMM_MAX_SLABS;
    for (int i = 0; i < a.nprob; ++i) a.p[i].nslab = a.nslab;      // (gemm_tight_slabs: fewer for a short-K problem of a merged launch)
    a.aligned = 0;
    a.xcd_chunk = 0;
    return a.nslab;
}

// K-ALIGNED plan (the 128 x 256 kernels of gemm_bf16.h / gemm_f32x3.h): every tile of problem p is cut into split_p equal k
// pieces and every workgroup takes exactly ONE piece of ONE tile; workgroups are numbered piece-major, tiles m-fastest, so the
// 32 workgroups of an XCD (contiguous numbers) are neighbouring tiles AT THE SAME k: they walk the same weight / activation
// k-windows at the same time and share them in L2, where the stream-K ranges (k offsets shifted from tile to tile) send almost
// every tile load to the Infinity Cache.  The slab count is exact (max split) and a tile writes exactly
// split_p slabs.  Chooses the smallest critical path T = max_p ceil(ktiles_p / split_p) with sum_p tiles_p split_p <= slots,
// pieces of at least min_iters k-tiles, split <= GEMM_MAX_SLABS.  Returns 0 (and leaves the plan untouched) when the tiles alone exceed the
// slots: the caller then uses gemm_plan.
inline int gemm_plan_aligned(GemmArgs& a, int slots, int min_iters, int BM, int BN, int BK) {
    int tiles[GEMM_MAX_PROB], kt[GEMM_MAX_PROB], kt_max = 1, sum_tiles = 0;
    for (int i = 0; i < a.nprob; ++i) {
        const GemmProb& p = a.p[i];
        tiles[i] = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
        kt[i] = 0;
        for (int s = 0; s < p.nseg; ++s) kt[i] += (p.seg[s].K + BK - 1) / BK;
        if (kt[i] > kt_max) kt_max = kt[i];
        sum_tiles += tiles[i];
    }
    if (sum_tiles > slots || sum_tiles == 0) return 0;
    int best_T = kt_max;
    for (int T = kt_max; T >= 1; --T) {
        int wgs = 0;
        bool ok = true;
        for (int i = 0; i < a.nprob && ok; ++i) {
            const int s = (kt[i] + T - 1) / T;
            ok = s <= GEMM_MAX_SLABS && (s == 1 || kt[i] / s >= min_iters);
            wgs += tiles[i] * s;
        }
        if (!ok || wgs > slots) break;
        best_T = T;
    }
    int total = 0, g = 0, nslab = 1;
    for (int i = 0; i < a.nprob; ++i) {
        GemmProb& p = a.p[i];
        p.tiles_m = (p.M + BM - 1) / BM;
        p.tiles_n = (p.N + BN - 1) / BN;
        p.ktiles = kt[i];
        p.it_begin = total;
        total += tiles[i] * kt[i];
        p.split = (kt[i] + best_T - 1) / best_T;
        p.g_begin = g;
        g += tiles[i] * p.split;
        if (p.split > nslab) nslab = p.split;
    }
    a.total_iters = total;
    a.G = g;
    a.nslab = nslab;
    for (int i = 0; i < a.nprob; ++i) a.p[i].nslab = nslab;       // every problem writes / zero-fills the launch's slab count (gemm_tight_slabs: its own split)
    a.aligned = 1;
    // XCD dealing in whole m-groups (round 6): workgroups are numbered m-fastest, so tiles_m consecutive numbers are the m-tiles of ONE
    // weight n-tile at ONE k window.  With ceil(G / 8) numbers per XCD a group straddles two XCDs whenever that is not a multiple of
    // tiles_m (G = 200, tiles_m = 4: 25 per XCD, every fourth group split) and its weight window is fetched by two L2s.  Deal whole
    // groups instead - when every problem has the same tiles_m and the larger chunk still fits the XCD's share of the slots.
    a.xcd_chunk = 0;
    int u = a.p[0].tiles_m;
    for (int i = 1; i < a.nprob; ++i) if (a.p[i].tiles_m != u) u = 1;
    if (u > 1 && g % u == 0) {
        const int groups = g / u, lo = groups / 8, extra = groups % 8, ch = u * (lo + (extra ? 1 : 0));
        if (ch <= (slots + 7) / 8) { a.xcd_chunk = ch; a.xcd_unit = u; a.xcd_lo = lo; a.xcd_extra = extra; }
    }
    return nslab;
}

// Slabs problem i of a planned launch really needs: a tile of k k-tiles meets at most ceil(k / L) + 1 stream-K ranges of at least L
// iterations (k-aligned plan: exactly its split).  A caller whose consumer reads problem i on its own may lower GemmProb::nslab to
// this (the kernel then writes / zero-fills that many slabs for the problem, the consumer adds that many): the vocabulary GEMM that
// shares a launch with the LSTM1 sums of the next step, att_ga next to LSTM2.
inline int gemm_tight_slabs(const GemmArgs& a, int i) {
    if (a.aligned) return a.p[i].split;
    if (a.G <= 1) return 1;
    const int L = a.total_iters / a.G;
    const int ns = (a.p[i].ktiles + L - 1) / L + 1;
    return ns < a.nslab ? ns : a.nslab;
}

inline double gemm_flops(const GemmArgs& a) {
    double f = 0;
    for (int i = 0; i < a.nprob; ++i)
        for (int s = 0; s < a.p[i].nseg; ++s) f += 2.0 * a.p[i].M * a.p[i].N * a.p[i].seg[s].K;
    return f;
}

// ALGORITHMIC bytes of a launch: every operand element and every output element once (w_bytes = bytes per weight element:
// 4, or 2 when the W operands are bf16 copies); gathered A rows count once per output row.
inline double gemm_bytes(const GemmArgs& a, int w_bytes) {
    double b = 0;
    for (int i = 0; i < a.nprob; ++i) {
        b += 4.0 * a.p[i].M * a.p[i].N;
        for (int s = 0; s < a.p[i].nseg; ++s) b += 4.0 * a.p[i].M * a.p[i].seg[s].K + (double)w_bytes * a.p[i].N * a.p[i].seg[s].K;
    }
    return b;
}

}  // namespace vsr
