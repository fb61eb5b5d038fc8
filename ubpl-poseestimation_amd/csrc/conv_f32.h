// Shared by the exact-f32 convolution files (conv_f32_fwd.hip, conv1x1_dma.hip,
// conv_f32_wgrad.hip): the tile constants, the split-K cost model and the forward plan.
//
// Convolutions of the stacked hourglass as implicit GEMMs on the CDNA4 matrix
// cores: the Conv wrapper (models/base/layers.py:31-50) in its three shapes —
// 1x1 stride 1 (Residual conv1/conv3/skip, features, heads, merges), 3x3
// stride 1 pad 1 (Residual conv2) and the 7x7 stride 2 pad 3 stem
// (models/pose/hourglass.py:22).
//
// GEMM view, NCHW, n = b*P + p (P = Ho*Wo, contiguous in memory):
//   forward  Y[b,m,p] = sum_k W~[m,k] * X~[b,k,p] + bias[m] (+ R[b,m,p])
//            GROUPED TAP-MAJOR k = (ci/16)*16T + tap*16 + ci%16 (tap = kh*KS+kw,
//            T = KS*KS), W~ = the weights re-laid out [Cout][Cin/16][T][16]
//            (ubpl_conv_weight_tapmajor), so a K tile of BK = 16 channels
//            shares one tap (input coordinates once per tile, not per element)
//            and the T taps of one 16-channel group follow each other: the
//            re-reads of an input row stay inside the L2 working set.  X~ = im2col of
//            relu(x*scale + shift): the pre-activation BN+ReLU of Residual is
//            applied while the operand is staged (bn(x) never touches HBM;
//            scale/shift sit in LDS for the whole workgroup);
//   dgrad    = forward with the weights flipped/transposed (stride 1 only);
//   wgrad    dW[m,n] = sum_k dY[m,k] * X~[k,n] over k = (b, p), n tap-major,
//            split along k over workgroups into a slab and reduced
//            deterministically (the reduce writes the reference layout);
//            the n-tile-0 workgroups also sum dY rows = the bias gradient.
// Small grids (deep hourglass levels: 32x32 .. 4x4 planes, K = 1152) split K
// over workgroups too (slab + reduce-epilogue), so every level fills the chip.
//
// Matrix core: v_mfma_f32_32x32x2_f32 (exact f32 fmaf chains).  Lane maps
// (cdna_hip_programming.md §3): A[i=l&31][k=l>>5], B[k=l>>5][j=l&31],
// C/D col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5).  4 waves in a 2x2 grid;
// operands staged k-major in LDS (As[k][m], Bs[k][n]) so a fragment read is
// 32 consecutive floats per half-wave; register-staged double buffer with one
// barrier per K step.
#pragma once
#include "common.h"
using ubpl::among;
using ubpl::conv_kgroup;
using ubpl::cu_count;
using ubpl::launch_split_reduce;
using ubpl::pick;
using ubpl::Plan;
using ubpl::xcd_remap;

namespace {

constexpr int NT = 256;
constexpr int BK = 16;
constexpr int MAXC = 256;  // largest Cin with a fused BN prologue

// component-wise select (a float4 ternary can be lowered to a pointer select through scratch)
__device__ __forceinline__ float4 sel4(bool ok, float4 v) {
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

// The supported (KS, stride): (1, 1), (3, 1) and the stem's (7, 2).
constexpr int conv_stride(int KS) { return KS == 7 ? 2 : 1; }
inline bool conv_shape_ok(int KS, int stride) { return (KS == 1 || KS == 3 || KS == 7) && stride == conv_stride(KS); }

// Resident workgroups per CU of a kernel for the cost model (dflt where the query fails): each
// file asks for its own kernels, once.
inline int query_occ(const void* f, int dflt) {
    int o = 0;
    const bool ok = hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, f, NT, 0) == hipSuccess && o > 0;
    (void)hipGetLastError();
    return ok ? o : dflt;
}

// ---- grid planning: a cost model over whole CU rounds.
// Blocks spread evenly over the CUs; a CU with c blocks (r = min(c, occ)
// resident) runs them in c * (steps + 2) K steps at a rate that needs ~3
// resident blocks to hide latency.  Split-K adds the slab written by the
// main kernel and re-read by the reduce, plus one launch.
double split_cost(int64_t tiles, int s, int64_t nsteps, int occ, int ncu, double step_flops, double slab_bytes_per_split) {
    const int64_t blocks = tiles * s;
    const int64_t per_cu = (blocks + ncu - 1) / ncu;
    const int64_t r = per_cu < occ ? per_cu : occ;
    const double eff = r >= 3 ? 1.0 : (r + 1) / 4.0;
    const int64_t steps = (nsteps + s - 1) / s;
    const double rate = 0.6e12 * 0.8;             // f32 MFMA flop/s per CU, sustained
    double t = (double)per_cu * (double)(steps + 2) * step_flops / (rate * eff);
    if (s > 1) t += 2.0 * s * slab_bytes_per_split / 5e12 + 4e-6;
    return t;
}

int best_split(int64_t tiles, int64_t nsteps, int maxs, int occ, int ncu, double step_flops,
               double slab_bytes_per_split) {
    int best = 1;
    double bc = split_cost(tiles, 1, nsteps, occ, ncu, step_flops, slab_bytes_per_split);
    for (int s = 2; s <= maxs; ++s) {
        const double c = split_cost(tiles, s, nsteps, occ, ncu, step_flops, slab_bytes_per_split);
        if (c < bc * 0.97) {      // a split must pay for itself clearly
            bc = c;
            best = s;
        }
    }
    return best;
}

// Tile height + split-K for the forward (BN = 128, BK = 16); occ128 / occ64: the occupancy of
// the kernel's 128- and 64-row forms.  force_bm (64 | 128, else 0): a tuning hook that pins the
// tile height (the 1x1 DMA kernel's UBPL_DMA_BM).
Plan fwd_plan(int Cout, int64_t N, int Ktot, int occ128, int occ64, int force_bm = 0) {
    constexpr int bn = 128;
    const int ncu = cu_count();
    const int nkt = (Ktot + BK - 1) / BK;
    const int maxs = nkt / 2 > 0 ? nkt / 2 : 1;            // >= 2 K steps per split
    Plan best{64, 1, 0};
    double bc = 1e30;
    for (int bm : {128, 64}) {
        if (bm == 128 && Cout <= 64) continue;
        if (force_bm && bm != force_bm && !(force_bm == 128 && Cout <= 64)) continue;
        const int64_t tiles = ((Cout + bm - 1) / bm) * ((N + bn - 1) / bn);
        const int occ = bm == 128 ? occ128 : occ64;
        const double sf = 2.0 * bm * bn * BK;
        const int s = best_split(tiles, nkt, maxs, occ, ncu, sf, 4.0 * Cout * N);
        // 64-row tiles re-read the B operand twice as often: ~15% slower per flop (measured)
        const double c = split_cost(tiles, s, nkt, occ, ncu, sf, 4.0 * Cout * N) / (bm == 128 ? 1.0 : 0.85);
        if (c < bc) {
            bc = c;
            best.bm = bm;
            best.splits = s;
        }
    }
    const int steps = (nkt + best.splits - 1) / best.splits;
    best.kchunk = steps * BK;
    best.splits = (nkt + steps - 1) / steps;
    return best;
}

}  // namespace
