// The exact-f32 1x1 convolution fed by LDS-DMA: conv1x1_dma_kernel and
// ubpl_conv1x1_forward_kmajor.  (MFMA lane maps: conv_f32.h.)
//
// 1x1 stride-1 conv as Y[m, n] = sum_k Wk[k][m] * X[b, k, p] (n = b*P + p)
// with the weights k-major ([Cin][Cout]: the data-gradient re-layout of a 1x1
// conv, or the reference layout itself for a data gradient).  Both operand
// tiles are k-rows of contiguous floats — BN (128) pixels of one input channel
// (NCHW as it lies) and BM output channels — so they go global -> LDS by
// LDS-DMA (global_load_lds_dwordx4, 1 KB per wave instruction), no staging
// registers.  The fused pre-activation relu(x*scale + shift) is applied to the
// B fragment after its LDS read (2 VALU per 2 MFMAs).  3-stage ring with
// counted vmcnt and a raw s_barrier, as conv_psa.hip's conv_psa_kernel.
// Fragment reads are ds_read_b32 of 32 consecutive floats per half-wave
// (conflict-free, no swizzle).
#include <cstdlib>

#include "conv_f32.h"

namespace {

template <int BM, bool PRO>
__global__ void __launch_bounds__(NT, 2) conv1x1_dma_kernel(const float* __restrict__ x, const float* __restrict__ wk,
                                                          const float* __restrict__ bias,
                                                          const float* __restrict__ pscale,
                                                          const float* __restrict__ pshift, const float* res,
                                                          float* y, int B, int K, int P, int M, int kchunk,
                                                          float* __restrict__ slab, float* __restrict__ stat_part) {
    constexpr int BN1 = 128;
    constexpr int TM = BM / 64, TN = BN1 / 64;
    constexpr int NS = 3;
    constexpr int AB = BK * BM * 4, BB = BK * BN1 * 4;       // bytes per stage
    constexpr int A_INS = AB / 1024, B_INS = BB / 1024;     // DMA instructions per stage
    constexpr int A_PW = A_INS / 4, B_PW = B_INS / 4;       // per wave
    constexpr int A_RPI = 1024 / (BM * 4);                  // rows per A instruction
    __shared__ __attribute__((aligned(16))) char lds[NS * (AB + BB)];

    const int64_t N = (int64_t)B * P;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: SGPR)
    const int wm = (wid >> 1) * (BM / 2), wn = (wid & 1) * (BN1 / 2);
    const int lam = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                              gridDim.x * gridDim.y * gridDim.z);
    const int by = lam % gridDim.y, bx = (lam / gridDim.y) % gridDim.x, bz = lam / (gridDim.y * gridDim.x);
    const int m0 = by * BM;
    const int64_t n0 = (int64_t)bx * BN1;
    const int k_begin = bz * kchunk;
    const int k_end = min(K, k_begin + kchunk);

    // DMA sources (per lane, k-independent part).  A instruction q (of A_INS)
    // covers k rows q*A_RPI .. +A_RPI-1; lane L: row q*A_RPI + L / (BM/4),
    // columns 4*(L % (BM/4)) .. +3.  B instruction q: rows 2q, 2q+1; lane L:
    // row 2q + (L >> 5), pixels 4*(L & 31) .. +3 of the tile.
    const int a_row = lane / (BM / 4);
    const int a_col = min(m0 + 4 * (lane % (BM / 4)), M - 4);
    const int b_row = lane >> 5;
    // per-lane 32-bit byte offsets over wave-uniform bases (scalar + vector
    // addressing).  K % 16 == 0 (checked by the entry point): every DMA row is
    // a real k row.
    const uint32_t a_lane = (uint32_t)((a_row * M + a_col) * 4);
    uint32_t b_lane;
    {
        int64_t n = n0 + 4 * (lane & 31);
        n = n < N ? n : N - 4;
        const int64_t b = n / P;
        b_lane = (uint32_t)((b * K * P + (n - b * P) + (int64_t)b_row * P) * 4);
    }
    auto stage = [&](int buf, int kt) {
        char* base = lds + buf * (AB + BB);
#pragma unroll
        for (int i = 0; i < A_PW; ++i) {
            const int q = wid * A_PW + i;
            const int k0 = min(kt + q * A_RPI, K - A_RPI);
            const char* ab = reinterpret_cast<const char*>(wk + (int64_t)k0 * M);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(ab + a_lane), (lds_ptr_t)(base + q * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < B_PW; ++i) {
            const int q = wid * B_PW + i;
            const int k0 = min(kt + 2 * q, K - 2);
            const char* bb = reinterpret_cast<const char*>(x + (int64_t)k0 * P);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(bb + b_lane), (lds_ptr_t)(base + AB + q * 1024), 16, 0, 0);
        }
    };

    // accumulators start at bias (+ residual), as conv_fwd_kernel
    const int li = lane & 31, lk = lane >> 5;
    int64_t obase[TN];
    bool nok[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int64_t n = n0 + wn + 32 * j + li;
        nok[j] = n < N;
        const int64_t nc = nok[j] ? n : N - 1;
        const int b = (int)(nc / P);
        const int p = (int)(nc - (int64_t)b * P);
        obase[j] = (int64_t)b * M * P + p;
    }
    floatx16 acc[TM][TN];
    const bool direct = slab == nullptr;
    ubpl::seed_acc<TM, TN>(acc, direct ? bias : nullptr, direct ? res : nullptr, obase, m0 + wm, M, P);

    const int nkt = (k_end - k_begin + BK - 1) / BK;
    if (nkt > 0) stage(0, k_begin);
    if (nkt > 1) stage(1, k_begin + BK);
    for (int t = 0; t < nkt; ++t) {
        if (t + 1 < nkt) vm_wait<A_PW + B_PW>();
        else vm_wait<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + 2 < nkt) stage((t + 2) % NS, k_begin + (t + 2) * BK);
        const int kt = k_begin + t * BK;
        const float* As = reinterpret_cast<const float*>(lds + (t % NS) * (AB + BB));
        const float* Bs = reinterpret_cast<const float*>(lds + (t % NS) * (AB + BB) + AB);
        // the K step's 16 (scale, shift) pairs by scalar loads (kt is uniform;
        // an LDS table would alias the DMA images and cost a vmcnt(0) per step)
        float scs[BK], shs[BK];
        if (PRO) {
            const int kb = __builtin_amdgcn_readfirstlane(min(kt, K - BK));
#pragma unroll
            for (int q = 0; q < BK; ++q) {
                scs[q] = pscale[kb + q];
                shs[q] = pshift[kb + q];
            }
        }
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            const int kr = 2 * s + lk;
            const bool kok = kt + kr < k_end;        // K tail: zero the B fragment
            float af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = As[kr * BM + wm + 32 * i + li];
            float sc = 1.f, sh = 0.f;
            if (PRO) {
                sc = lk ? scs[2 * s + 1] : scs[2 * s];
                sh = lk ? shs[2 * s + 1] : shs[2 * s];
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                float v = Bs[kr * BN1 + wn + 32 * j + li];
                if (PRO) v = fmaxf(fmaf(v, sc, sh), 0.f);
                bf[j] = kok ? v : 0.f;
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    if (slab != nullptr) {
        float* sl = slab + (int64_t)bz * M * N;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t n = n0 + wn + 32 * j + li;
            if (n >= N) continue;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                    if (m < M) sl[(int64_t)m * N + n] = acc[i][j][r];
                }
        }
        return;
    }
    if (stat_part) ubpl::tile_bn_partials<TM, TN>(acc, nok, m0 + wm, M, n0 + wn, N, stat_part);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        if (!nok[j]) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m < M) y[obase[j] + (int64_t)m * P] = acc[i][j][r];
            }
    }
}

// ------------------------------------------------------------------ host side
Plan plan_of(int Cout, int64_t N, int Cin) {
    static const int occ128 = query_occ((const void*)conv1x1_dma_kernel<128, true>, 2);
    static const int occ64 = query_occ((const void*)conv1x1_dma_kernel<64, true>, 2);
    // tuning hook: UBPL_DMA_BM=64|128 pins the tile height
    static const int force_bm = [] {
        const char* e = getenv("UBPL_DMA_BM");
        return e ? atoi(e) : 0;
    }();
    return fwd_plan(Cout, N, Cin, occ128, occ64, force_bm);
}

// What every launch of ubpl_conv1x1_forward_kmajor shares
struct DmaArgs {
    const float *x, *wk, *bias, *pscale, *pshift, *res;
    float* y;
    int B, K, P, M;
    Plan pl;
    float *slab, *stat_part;
    hipStream_t st;
};

template <int BM, bool PRO>
int launch_1x1_dma(const DmaArgs& a) {
    const Plan& pl = a.pl;
    const int64_t N = (int64_t)a.B * a.P;
    dim3 grid((unsigned)((N + 127) / 128), (unsigned)((a.M + BM - 1) / BM), (unsigned)pl.splits);
    const bool split = pl.splits > 1;
    hipLaunchKernelGGL((conv1x1_dma_kernel<BM, PRO>), grid, dim3(NT), 0, a.st, a.x, a.wk, a.bias, a.pscale, a.pshift,
                       split ? nullptr : a.res, a.y, a.B, a.K, a.P, a.M, pl.kchunk, split ? a.slab : nullptr,
                       split ? nullptr : a.stat_part);
    UBPL_LAUNCH_CHECK();
    if (split) {
        launch_split_reduce(a.slab, pl.splits, a.M, a.P, N, a.bias, a.res, a.y, a.st);
        UBPL_LAUNCH_CHECK();
        if (a.stat_part) return ubpl_bn_partials(a.y, a.B, a.M, a.P, a.stat_part, a.st);
    }
    return 0;
}

}  // namespace

UBPL_API int64_t ubpl_conv1x1_kmajor_workspace(int B, int Cin, int Cout, int P) {
    const Plan pl = plan_of(Cout, (int64_t)B * P, Cin);
    return pl.splits > 1 ? (int64_t)pl.splits * Cout * B * P : 0;
}

// 1x1 stride-1 conv with k-major weights wk [Cin][Cout] (the data-gradient
// re-layout of a 1x1 conv; for a data gradient, the reference weights
// themselves): y[B,Cout,P] = conv(relu(x*pscale + pshift) or x) + bias (+ res,
// may alias y).  Needs Cin % 16 == 0, Cout % 4 == 0, P % 4 == 0, Cin <= 256 with a prologue,
// 16-B aligned x / wk.  slab: ubpl_conv1x1_kmajor_workspace floats (nullable at 0).
// stat_part (nullable): BatchNorm partials of y (ubpl_bn_partials layout).
UBPL_API int ubpl_conv1x1_forward_kmajor(const float* x, int B, int Cin, int P, const float* wk, const float* bias,
                                         int Cout, const float* pscale, const float* pshift, const float* res,
                                         float* y, float* slab, float* stat_part, void* stream) {
    const bool pro = pscale != nullptr;
    if ((pro && Cin > MAXC) || Cin % BK != 0 || Cout % 4 != 0 || P % 4 != 0 || (((uintptr_t)x) & 15) ||
        (((uintptr_t)wk) & 15))
        return (int)hipErrorInvalidValue;
    const DmaArgs a{x, wk, bias, pscale, pshift, res, y, B, Cin, P, Cout, plan_of(Cout, (int64_t)B * P, Cin),
                    slab, stat_part, (hipStream_t)stream};
    if (a.pl.splits > 1 && slab == nullptr) return (int)hipErrorInvalidValue;
    return pick([&](auto BM, auto PRO) { return launch_1x1_dma<BM, PRO>(a); }, among<128, 64>{a.pl.bm},
                among<0, 1>{pro});
}
