// The exact-f32 weight (and bias) gradient: conv_wgrad2_kernel (k-contiguous float4
// staging), conv_wgrad_kernel (any plane) and ubpl_conv2d_wgrad.  Both write a split-k slab that
// conv_reduce.hip's wgrad_reduce_kernel sums.  GEMM view and lane maps: conv_f32.h.
#include "conv_f32.h"

namespace {

// ------------------------------------------------------------------ wgrad
// n tap-major: n = tap*Cin + ci; TAPN: a BN-wide n tile lies in one tap.
template <int BM, int BN, int KS, int ST, bool PRO, bool TAPN>
__global__ void __launch_bounds__(NT) conv_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                       const float* __restrict__ pscale,
                                                       const float* __restrict__ pshift, int B, int Cin, int H,
                                                       int W, int Cout, int Ho, int Wo, int kchunk,
                                                       float* __restrict__ slab, int with_bias) {
    constexpr int PADK = (KS - 1) / 2;
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int WBK = 32;
    constexpr int ALD = BM + 1, BLD = BN + 1;
    constexpr int RSTEP = NT / WBK;
    constexpr int A_PER = BM / RSTEP, B_PER = BN / RSTEP;
    __shared__ float As[2][WBK][ALD];
    __shared__ float Bs[2][WBK][BLD];
    __shared__ float s_sc[PRO ? MAXC : 1], s_sh[PRO ? MAXC : 1];

    const int P = Ho * Wo, HWin = H * W;
    const int64_t Kall = (int64_t)B * P;
    const int Ntot = Cin * KS * KS;
    const int Nt = Ntot + 1;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: SGPR)
    const int wm = (wid >> 1) * (BM / 2), wn = (wid & 1) * (BN / 2);
    const int m0 = blockIdx.y * BM;
    const int nb0 = blockIdx.x * BN;
    const int64_t k_begin = (int64_t)blockIdx.z * kchunk;
    const int64_t k_end = min(Kall, k_begin + kchunk);
    const int lk_ld = tid % WBK;
    const int lr_ld = tid / WBK;
    const bool bias_blk = with_bias && blockIdx.x == 0;
    // tap of this workgroup's n tile (TAPN)
    const int tap_blk = nb0 / Cin, ci_blk = nb0 - tap_blk * Cin;
    const int kh_blk = tap_blk / KS, kw_blk = tap_blk - kh_blk * KS;

    if (PRO) {
        for (int c = tid; c < Cin; c += NT) {
            s_sc[c] = pscale[c];
            s_sh[c] = pshift[c];
        }
        __syncthreads();
    }

    float ra[A_PER], rb[B_PER];
    auto load = [&](int64_t kt) {
        const int64_t k = kt + lk_ld;
        const bool kv = k < k_end;
        const int64_t kc = kv ? k : k_begin;        // clamped, always valid
        const int b = (int)(kc / P);
        const int p = (int)(kc - (int64_t)b * P);
        const int oh = p / Wo, ow = p - oh * Wo;
        const float* dyb = dy + (int64_t)b * Cout * P + p;
#pragma unroll
        for (int j = 0; j < A_PER; ++j) {
            const int m = m0 + lr_ld + j * RSTEP;
            const float v = dyb[(int64_t)min(m, Cout - 1) * P];
            ra[j] = (kv && m < Cout) ? v : 0.f;
        }
        const float* xb = x + (int64_t)b * Cin * HWin;
        if constexpr (TAPN) {
            const int ih = oh * ST - PADK + kh_blk, iw = ow * ST - PADK + kw_blk;
            const bool inb = kv && ih >= 0 && ih < H && iw >= 0 && iw < W;
            const float* src = xb + (inb ? ih * W + iw : 0);
#pragma unroll
            for (int j = 0; j < B_PER; ++j) {
                const int r = lr_ld + j * RSTEP;
                const bool ok = inb && nb0 + r < Ntot;
                const int ci = min(ci_blk + r, Cin - 1);
                float v = src[(int64_t)ci * HWin];
                if (PRO) v = fmaxf(fmaf(v, s_sc[ci], s_sh[ci]), 0.f);
                rb[j] = ok ? v : 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < B_PER; ++j) {
                const int n = nb0 + lr_ld + j * RSTEP;
                float v = 0.f;
                if (kv && n < Ntot) {
                    const int tap = n / Cin, ci = n - tap * Cin;
                    const int kh = tap / KS, kw = tap - kh * KS;
                    const int ih = oh * ST - PADK + kh, iw = ow * ST - PADK + kw;
                    if (ih >= 0 && ih < H && iw >= 0 && iw < W) {
                        v = xb[(int64_t)ci * HWin + ih * W + iw];
                        if (PRO) v = fmaxf(fmaf(v, s_sc[ci], s_sh[ci]), 0.f);
                    }
                }
                rb[j] = v;
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < A_PER; ++j) As[buf][lk_ld][lr_ld + j * RSTEP] = ra[j];
#pragma unroll
        for (int j = 0; j < B_PER; ++j) Bs[buf][lk_ld][lr_ld + j * RSTEP] = rb[j];
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float bsum = 0.f;

    const int nkt = (int)((k_end - k_begin + WBK - 1) / WBK);
    if (nkt > 0) {
        load(k_begin);
        store(0);
    }
    __syncthreads();
    const int li = lane & 31, lk = lane >> 5;
    for (int t = 0; t < nkt; ++t) {
        const int cur = t & 1;
        if (t + 1 < nkt) load(k_begin + (int64_t)(t + 1) * WBK);
        if (bias_blk && tid < BM) {
#pragma unroll 8
            for (int kk = 0; kk < WBK; ++kk) bsum += As[cur][kk][tid];
        }
#pragma unroll
        for (int s = 0; s < WBK / 2; ++s) {
            float af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = As[cur][2 * s + lk][wm + 32 * i + li];
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = Bs[cur][2 * s + lk][wn + 32 * j + li];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < nkt) {
            store(cur ^ 1);
            __syncthreads();
        }
    }

    float* sl = slab + (int64_t)blockIdx.z * Cout * Nt;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = nb0 + wn + 32 * j + li;
        if (n >= Ntot) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m < Cout) sl[(int64_t)m * Nt + n] = acc[i][j][r];
            }
    }
    if (bias_blk && tid < BM && m0 + tid < Cout) sl[(int64_t)(m0 + tid) * Nt + Ntot] = bsum;
}

// ------------------------------------------------------------------ wgrad v2
// Both operands run along k = b*P + p in memory (dY[b][m][p], x[b][ci][p']),
// so they are staged k-contiguous: float4 global loads, As[m][16] / Bs[n][16]
// (64-B rows of four 16-B slots, slot XOR-swizzled by (row>>2)&3: conflict-free
// ds_write_b128 and ds_read_b128, no padding, 32 KB double-buffered).  Inside
// a 16-k step the reduction order is permuted: lane half h = l>>5 takes
// k = 8h + 4q + e at MFMA (q, e), so one ds_read_b128 carries the operands of
// four MFMAs.  n is tap-major (n = tap*Cin + ci) with the tap decoded per
// staged row once, so any Cin (64, the stem's 3) works; the n-tile-0
// workgroups sum their dY rows from registers (bias gradient).
template <int BM, int BN, int KS, int ST, bool PRO, bool VEC1>
__global__ void __launch_bounds__(NT, 4) conv_wgrad2_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ pscale,
                                                           const float* __restrict__ pshift, int B, int Cin, int H,
                                                           int W, int Cout, int Ho, int Wo, int kchunk,
                                                           float* __restrict__ slab, int with_bias) {
    constexpr int PADK = (KS - 1) / 2;
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int AR = BM / 64, BR = BN / 64;   // staged rows per thread
    __shared__ float4 As[2][BM * 4];
    __shared__ float4 Bs[2][BN * 4];
    __shared__ float s_sc[PRO ? MAXC : 1], s_sh[PRO ? MAXC : 1];

    const int P = Ho * Wo, HWin = H * W;
    const int Kall = B * P;
    const int Ntot = Cin * KS * KS, Nt = Ntot + 1;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: SGPR)
    const int wm = (wid >> 1) * (BM / 2), wn = (wid & 1) * (BN / 2);
    // XCD-aware tile order: the n tiles (taps) and m tiles of one k split read
    // the same dy / x rows and share an L2.
    const int lam = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                              gridDim.x * gridDim.y * gridDim.z);
    const int bx = lam % gridDim.x, by = (lam / gridDim.x) % gridDim.y, bz = lam / (gridDim.x * gridDim.y);
    const int m0 = by * BM, nb0 = bx * BN;
    const int k_begin = bz * kchunk;
    const int k_end = min(Kall, k_begin + kchunk);
    const int q = tid & 3, r0 = tid >> 2;
    const bool bias_blk = with_bias && bx == 0;

    if (PRO) {
        for (int c = tid; c < Cin; c += NT) {
            s_sc[c] = pscale[c];
            s_sh[c] = pshift[c];
        }
        __syncthreads();
    }
    int am[AR];
    bool aok[AR];
#pragma unroll
    for (int j = 0; j < AR; ++j) {
        const int m = m0 + r0 + 64 * j;
        aok[j] = m < Cout;
        am[j] = min(m, Cout - 1);
    }
    int bci[BR], bdh[BR], bdw[BR];
    bool bok[BR];
#pragma unroll
    for (int j = 0; j < BR; ++j) {
        const int n = nb0 + r0 + 64 * j;
        bok[j] = n < Ntot;
        const int nn = min(n, Ntot - 1);
        const int tap = nn / Cin, ci = nn - tap * Cin;
        const int kh = tap / KS, kw = tap - kh * KS;
        bci[j] = ci;
        bdh[j] = kh - PADK;
        bdw[j] = kw - PADK;
    }

    // raw loads stay in registers across the MFMAs; masks / prologue at store
    float4 ra[AR], rb[BR];
    float bsum[AR];
    bool kv_st = false;
    unsigned bmask = 0;          // generic B path: 4 in-bounds bits per staged row
#pragma unroll
    for (int j = 0; j < AR; ++j) bsum[j] = 0.f;
    auto load = [&](int kt) {
        const int k = kt + 4 * q;
        kv_st = k < k_end;                          // k_end % 4 == 0: all four or none
        const int kc = kv_st ? k : k_begin;
        const int b = kc / P, p = kc - b * P;
#pragma unroll
        for (int j = 0; j < AR; ++j)
            ra[j] = *reinterpret_cast<const float4*>(dy + ((int64_t)b * Cout + am[j]) * P + p);
        if constexpr (VEC1) {
#pragma unroll
            for (int j = 0; j < BR; ++j)
                rb[j] = *reinterpret_cast<const float4*>(x + ((int64_t)b * Cin + bci[j]) * HWin + p);
        } else {
            const int oh = p / Wo, ow = p - oh * Wo;   // Wo % 4 == 0: one output row
            bmask = 0;
#pragma unroll
            for (int j = 0; j < BR; ++j) {
                const int ih = oh * ST + bdh[j];
                const bool rok = bok[j] && ih >= 0 && ih < H;
                const float* src = x + ((int64_t)b * Cin + bci[j]) * HWin + (rok ? ih * W : 0);
                float e4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int iw = (ow + e) * ST + bdw[j];
                    const bool ok = rok && iw >= 0 && iw < W;
                    e4[e] = src[ok ? iw : 0];
                    bmask |= (ok ? 1u : 0u) << (4 * j + e);
                }
                rb[j] = make_float4(e4[0], e4[1], e4[2], e4[3]);
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < AR; ++j) {
            const int row = r0 + 64 * j;
            const float4 v = sel4(kv_st && aok[j], ra[j]);
            As[buf][row * 4 + (q ^ ((row >> 2) & 3))] = v;
            if (bias_blk) bsum[j] += (v.x + v.y) + (v.z + v.w);
        }
#pragma unroll
        for (int j = 0; j < BR; ++j) {
            const int row = r0 + 64 * j;
            float4 v = rb[j];
            if (PRO) {
                const float sc = s_sc[bci[j]], sh = s_sh[bci[j]];
                v.x = fmaxf(fmaf(v.x, sc, sh), 0.f);
                v.y = fmaxf(fmaf(v.y, sc, sh), 0.f);
                v.z = fmaxf(fmaf(v.z, sc, sh), 0.f);
                v.w = fmaxf(fmaf(v.w, sc, sh), 0.f);
            }
            if constexpr (VEC1) {
                v = sel4(kv_st && bok[j], v);
            } else {
                const unsigned mj = kv_st ? (bmask >> (4 * j)) : 0u;
                v = make_float4((mj & 1) ? v.x : 0.f, (mj & 2) ? v.y : 0.f, (mj & 4) ? v.z : 0.f,
                                (mj & 8) ? v.w : 0.f);
            }
            Bs[buf][row * 4 + (q ^ ((row >> 2) & 3))] = v;
        }
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nkt = (k_end - k_begin + 15) / 16;
    // T14 order, as in conv_fwd_kernel
    if (nkt > 0) {
        load(k_begin);
        store(0);
    }
    if (nkt > 1) load(k_begin + 16);
    const int li = lane & 31, h = lane >> 5;
    for (int t = 0; t < nkt; ++t) {
        const int cur = t & 1;
        __syncthreads();
        if (t + 1 < nkt) {
            store(cur ^ 1);
            if (t + 2 < nkt) load(k_begin + (t + 2) * 16);
        }
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
            const int sl = 2 * h + q2;
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm + 32 * i + li;
                af[i] = As[cur][row * 4 + (sl ^ ((row >> 2) & 3))];
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wn + 32 * j + li;
                bf[j] = Bs[cur][row * 4 + (sl ^ ((row >> 2) & 3))];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
    }

    float* sl = slab + (int64_t)bz * Cout * Nt;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = nb0 + wn + 32 * j + li;
        if (n >= Ntot) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < Cout) sl[(int64_t)m * Nt + n] = acc[i][j][r];
            }
    }
    if (bias_blk) {
#pragma unroll
        for (int j = 0; j < AR; ++j) {
            float v = bsum[j];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            if (q == 0 && aok[j]) sl[(int64_t)(m0 + r0 + 64 * j) * Nt + Ntot] = v;
        }
    }
}

// k-contiguous float4 staging (conv_wgrad2_kernel) needs P % 4 == 0 and, for a
// spatial kernel, whole float4 groups inside one output row.
bool wgrad_v2_shape(int KS, int Ho, int Wo) { return (Ho * Wo) % 4 == 0 && (KS == 1 || Wo % 4 == 0); }

struct WPlan {
    int splits, kchunk, bm, bn;
};

// Split of the k = b*P + p reduction over workgroups for the weight gradient.
// v2: BM x BN tiles in {64,128}^2, 16-k steps, chosen by the cost model with a
// per-flop efficiency for the smaller tiles; v1: 64x64, 32-k steps.
WPlan wgrad_plan(int B, int Cin, int Cout, int KS, int Ho, int Wo, bool v2) {
    // resident workgroups per CU: conv_wgrad_kernel, and conv_wgrad2_kernel [bm == 128][bn == 128]
    static const int occ_v1 = query_occ((const void*)conv_wgrad_kernel<64, 64, 3, 1, true, true>, 4);
    static const int occ_v2[2][2] = {{query_occ((const void*)conv_wgrad2_kernel<64, 64, 3, 1, true, false>, 8),
                                      query_occ((const void*)conv_wgrad2_kernel<64, 128, 3, 1, true, false>, 5)},
                                     {query_occ((const void*)conv_wgrad2_kernel<128, 64, 3, 1, true, false>, 5),
                                      query_occ((const void*)conv_wgrad2_kernel<128, 128, 3, 1, true, false>, 4)}};
    const int ncu = cu_count();
    const int64_t K = (int64_t)B * Ho * Wo;
    const int64_t Ntot = (int64_t)Cin * KS * KS;
    // keep the slab (splits * Cout * (Ntot+1) floats, written + re-read) no larger
    // than the operands it is computed from (dy and x: K * (Cout + Cin) floats)
    // (slabs up to 8 MB are allowed regardless: small levels need the splits)
    int64_t cap = (K * (Cout + Cin)) / ((int64_t)Cout * (Ntot + 1));
    const int64_t cap_small = (int64_t)(8 << 20) / (4 * (int64_t)Cout * (Ntot + 1));
    if (cap < cap_small) cap = cap_small;
    WPlan best{1, 0, 64, 64};
    double bc = 1e30;
    for (int bm : {128, 64})
        for (int bn : {128, 64}) {
            if (!v2 && (bm != 64 || bn != 64)) continue;
            if (bm == 128 && Cout <= 64) continue;
            if (bn == 128 && Ntot <= 64) continue;
            const int kb = v2 ? 16 : 32;
            const int64_t tiles = ((Ntot + bn - 1) / bn) * ((Cout + bm - 1) / bm);
            const int64_t nsteps = (K + kb - 1) / kb;
            int64_t maxs = (K + 4 * kb - 1) / (4 * kb);     // every split >= 4 k steps
            if (maxs > cap) maxs = cap;
            if (maxs > 512) maxs = 512;
            if (maxs < 1) maxs = 1;
            const int occ = v2 ? occ_v2[bm == 128][bn == 128] : occ_v1;
            const double sf = 2.0 * bm * bn * kb, sb = 4.0 * Cout * (Ntot + 1);
            const int s = best_split(tiles, nsteps, (int)maxs, occ, ncu, sf, sb);
            const double eff = (bm * bn == 16384) ? 1.0 : (bm * bn == 8192 ? 0.85 : 0.7);
            const double c = split_cost(tiles, s, nsteps, occ, ncu, sf, sb) / eff;
            if (c < bc) {
                bc = c;
                int64_t chunk = (K + s - 1) / s;
                chunk = (chunk + kb - 1) / kb * kb;
                best.kchunk = (int)chunk;
                best.splits = (int)((K + chunk - 1) / chunk);
                best.bm = bm;
                best.bn = bn;
            }
        }
    return best;
}

// What every launch of ubpl_conv2d_wgrad shares
struct WgradArgs {
    const float *dy, *x, *pscale, *pshift;
    int B, Cin, H, W, Cout, KS, Ho, Wo;
    WPlan pl;
    float* slab;
    int with_bias;
    hipStream_t st;
};

// The instantiations that are built.  conv_wgrad2_kernel<BM, BN, KS, ST, PRO, VEC1>: every tile,
// VEC1 (float4 rows of x) on 1x1 only; conv_wgrad_kernel<64, 64, KS, ST, PRO, TAPN>: TAPN (an n
// tile inside one tap) always on 1x1, never on the stem.
constexpr bool wgrad_built(bool V2, int BM, int BN, int KS, bool FLAG) {
    if (V2) return KS == 1 || !FLAG;
    return BM == 64 && BN == 64 && (KS == 3 || FLAG == (KS == 1));
}

// (the two kernels take the same arguments)
template <int BM, int BN, class Kernel>
int launch_wgrad(Kernel kernel, const WgradArgs& a) {
    const int Ntot = a.Cin * a.KS * a.KS;
    dim3 grid((unsigned)((Ntot + BN - 1) / BN), (unsigned)((a.Cout + BM - 1) / BM), (unsigned)a.pl.splits);
    hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, a.st, a.dy, a.x, a.pscale, a.pshift, a.B, a.Cin, a.H, a.W, a.Cout,
                       a.Ho, a.Wo, a.pl.kchunk, a.slab, a.with_bias);
    UBPL_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// Floats of slab workspace ubpl_conv2d_wgrad needs.
UBPL_API int64_t ubpl_conv2d_wgrad_workspace(int B, int Cin, int Cout, int KS, int Ho, int Wo) {
    int64_t s = wgrad_plan(B, Cin, Cout, KS, Ho, Wo, false).splits;
    if (wgrad_v2_shape(KS, Ho, Wo)) {
        const int64_t s2 = wgrad_plan(B, Cin, Cout, KS, Ho, Wo, true).splits;
        if (s2 > s) s = s2;
    }
    return s * Cout * (Cin * KS * KS + 1);
}

// dw[Cout,Cin,KS,KS] (+)= sum over (b,p) dy * im2col(relu(x*pscale+pshift) or x);
// db[Cout] (+)= sum over (b,p) dy (db nullable).  slab: workspace floats.
UBPL_API int ubpl_conv2d_wgrad(const float* dy, const float* x, int B, int Cin, int H, int W, int Cout, int KS,
                               int stride, const float* pscale, const float* pshift, int Ho, int Wo, float* slab,
                               float* dw, float* db, int accumulate, void* stream) {
    const bool pro = pscale != nullptr;
    if (pro && Cin > MAXC) return (int)hipErrorInvalidValue;
    if (!conv_shape_ok(KS, stride)) return (int)hipErrorInvalidValue;
    const bool v2 = wgrad_v2_shape(KS, Ho, Wo) && (((uintptr_t)dy & 15) == 0);
    // v2: VEC1, float4 rows of x (1x1); v1: TAPN, an n tile inside one tap (1x1, or Cin % 64 == 0 on 3x3)
    const bool flag = v2 ? KS == 1 && (((uintptr_t)x & 15) == 0) && ((H * W) % 4 == 0)
                         : KS == 1 || (KS == 3 && Cin % 64 == 0);
    const WgradArgs a{dy, x, pscale, pshift, B, Cin, H, W, Cout, KS, Ho, Wo, wgrad_plan(B, Cin, Cout, KS, Ho, Wo, v2),
                      slab, db != nullptr, (hipStream_t)stream};
    const int rc = pick(
        [&](auto V2, auto KS_, auto PRO, auto FLAG, auto BM, auto BN) {
            constexpr int ST = conv_stride(KS_);
            if constexpr (!wgrad_built(V2, BM, BN, KS_, FLAG)) return (int)hipErrorInvalidValue;
            else if constexpr (V2) return launch_wgrad<BM, BN>(conv_wgrad2_kernel<BM, BN, KS_, ST, PRO, FLAG>, a);
            else return launch_wgrad<BM, BN>(conv_wgrad_kernel<BM, BN, KS_, ST, PRO, FLAG>, a);
        },
        among<0, 1>{v2}, among<1, 3, 7>{KS}, among<0, 1>{pro}, among<0, 1>{flag}, among<128, 64>{a.pl.bm},
        among<128, 64>{a.pl.bn});
    if (rc) return rc;
    return ubpl_wgrad_slab_reduce(slab, a.pl.splits, Cout, Cin, KS * KS, a.with_bias, dw, db, accumulate, stream);
}
