// The exact-f32 forward convolution (and, with flipped weights, the stride-1 data gradient):
// conv_fwd_kernel and ubpl_conv2d_forward.  GEMM view and lane maps: conv_f32.h.
#include "conv_f32.h"

namespace {

// ------------------------------------------------------------------ forward
// TAPK: k tiles never straddle a tap (Cin % BK == 0 or KS == 1).
// AVEC: Ktot % 4 == 0 and 16-B aligned weights: float4 weight loads only.
template <int BM, int BN, int KS, int ST, bool PRO, bool VECB, bool TAPK, bool AVEC>
__global__ void __launch_bounds__(NT, 4) conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias,
                                                     const float* __restrict__ pscale,
                                                     const float* __restrict__ pshift, const float* res, float* y,
                                                     int B, int Cin, int H, int W, int Cout, int Ho, int Wo,
                                                     int kchunk, float* __restrict__ slab) {
    constexpr int PADK = (KS - 1) / 2;
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int ALD = BM + 2, BLD = BN + 4;
    constexpr int A_PER = BM * BK / NT;          // 8 (BM=128) or 4 (BM=64)
    constexpr int B_PER = BK * BN / NT;          // 8
    constexpr int VROWS = NT / (BN / 4);         // vector loader rows per pass
    __shared__ float As[2][BK][ALD];
    __shared__ float Bs[2][BK][BLD];
    __shared__ float2 s_ss[PRO ? MAXC : 1];   // (scale, shift) per input channel

    const int P = Ho * Wo, HWin = H * W;
    const int64_t N = (int64_t)B * P;
    const int Ktot = Cin * KS * KS;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: SGPR)
    const int wm = (wid >> 1) * (BM / 2), wn = (wid & 1) * (BN / 2);
    // XCD-aware tile order: the m tiles of one n tile, then neighbouring n
    // tiles (shared halo rows), share an L2; split-K slowest.
    const int lam = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                              gridDim.x * gridDim.y * gridDim.z);
    const int by = lam % gridDim.y, bx = (lam / gridDim.y) % gridDim.x, bz = lam / (gridDim.y * gridDim.x);
    const int m0 = by * BM;
    const int64_t n0 = (int64_t)bx * BN;
    const int k_begin = bz * kchunk;
    const int k_end = min(Ktot, k_begin + kchunk);
    constexpr int T = KS * KS;
    const int G = conv_kgroup(Cin);

    if (PRO) {
        for (int c = tid; c < Cin; c += NT) s_ss[c] = make_float2(pscale[c], pshift[c]);
    }

    // A loader: row am, k chunk ak0 .. ak0 + A_PER - 1 (vectorised when aligned)
    const int am = tid % BM;
    const int ak0 = (tid / BM) * A_PER;
    // B loader column(s)
    const int bnl = VECB ? 4 * (tid % (BN / 4)) : tid % BN;
    const int bk0 = VECB ? tid / (BN / 4) : tid / BN;
    int cb = 0, coh = 0, cow = 0;
    const int64_t ncol = n0 + bnl;
    const bool cvalid = ncol < N;
    if (cvalid) {
        cb = (int)(ncol / P);
        const int p = (int)(ncol - (int64_t)cb * P);
        coh = p / Wo;
        cow = p - coh * Wo;
    }
    const float* xb = x + (int64_t)cb * Cin * HWin;

    float ra[A_PER];
    float rb[B_PER];
    bool b_inb = false;

    // Loads are unconditional at a clamped (always valid) address and stay raw
    // in registers while the K step's MFMAs run; masks and the BN prologue are
    // applied when the values are stored to LDS.  (A load under a per-element
    // branch, or a select right after it, makes hipcc wait vmcnt(0) on the spot:
    // cdna_hip_programming.md §5 'Three .s-level traps' (c).)
    const int am_c = min(m0 + am, Cout - 1);
    const bool am_ok = m0 + am < Cout;
    const float* wrow = w + (int64_t)am_c * Ktot;
    auto load_a = [&](int kt) {
        const int k = kt + ak0;
        if constexpr (AVEC) {
            // clamped to the last aligned 4-vector; the tail is masked at store time
            const float4* src = reinterpret_cast<const float4*>(wrow);
#pragma unroll
            for (int j = 0; j < A_PER / 4; ++j) {
                const float4 v = src[min(k + 4 * j, Ktot - 4) >> 2];
                ra[4 * j] = v.x;
                ra[4 * j + 1] = v.y;
                ra[4 * j + 2] = v.z;
                ra[4 * j + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < A_PER; ++j) ra[j] = wrow[min(k + j, Ktot - 1)];
        }
    };
    auto load_b = [&](int kt) {
        if constexpr (VECB) {
            // 1x1 stride 1: X~[ci][n..n+3] = x[b, ci, p..p+3] (P % 4 == 0)
            const int p = coh * Wo + cow;
#pragma unroll
            for (int j = 0; j < BK / VROWS; ++j) {
                const int kc = min(kt + bk0 + j * VROWS, Cin - 1);
                const float4 v = *reinterpret_cast<const float4*>(xb + (int64_t)kc * P + p);
                rb[4 * j] = v.x;
                rb[4 * j + 1] = v.y;
                rb[4 * j + 2] = v.z;
                rb[4 * j + 3] = v.w;
            }
        } else if constexpr (TAPK) {
            // one (channel group, tap) per K tile (G == BK): input coordinates once per tile
            const int kg = kt / BK;
            const int tap = kg % T, ci0 = (kg / T) * BK;
            const int kh = tap / KS, kw = tap - kh * KS;
            const int ih = coh * ST - PADK + kh, iw = cow * ST - PADK + kw;
            b_inb = cvalid && ih >= 0 && ih < H && iw >= 0 && iw < W;
            const float* src = xb + (b_inb ? ih * W + iw : 0);
#pragma unroll
            for (int j = 0; j < B_PER; ++j) rb[j] = src[(int64_t)min(ci0 + bk0 + j * (NT / BN), Cin - 1) * HWin];
        } else {
            // generic (stem, Cin = 3): tap and channel per element
#pragma unroll
            for (int j = 0; j < B_PER; ++j) {
                const int k = kt + bk0 + j * (NT / BN);
                float v = 0.f;
                if (cvalid && k < k_end) {
                    const int cb = k / (G * T), rem = k - cb * G * T;
                    const int tap = rem / G, ci = cb * G + (rem - (rem / G) * G);
                    const int kh = tap / KS, kw = tap - kh * KS;
                    const int ih = coh * ST - PADK + kh, iw = cow * ST - PADK + kw;
                    if (ih >= 0 && ih < H && iw >= 0 && iw < W) {
                        v = xb[(int64_t)ci * HWin + ih * W + iw];
                        if (PRO) v = fmaxf(fmaf(v, s_ss[ci].x, s_ss[ci].y), 0.f);
                    }
                }
                rb[j] = v;
            }
        }
    };
    // prologue evaluated unconditionally, then selected (a conditional LDS read
    // becomes an exec-mask branch with its own lgkmcnt wait)
    auto store_ab = [&](int buf, int kt) {
        {
            const int k = kt + ak0;
#pragma unroll
            for (int j = 0; j < A_PER; ++j) As[buf][ak0 + j][am] = (am_ok && k + j < k_end) ? ra[j] : 0.f;
        }
        if constexpr (VECB) {
#pragma unroll
            for (int j = 0; j < BK / VROWS; ++j) {
                const int k = kt + bk0 + j * VROWS;
                const bool ok = cvalid && k < k_end;
                float4 v = make_float4(rb[4 * j], rb[4 * j + 1], rb[4 * j + 2], rb[4 * j + 3]);
                if (PRO) {
                    const float2 ss = s_ss[min(k, Cin - 1)];
                    v.x = fmaxf(fmaf(v.x, ss.x, ss.y), 0.f);
                    v.y = fmaxf(fmaf(v.y, ss.x, ss.y), 0.f);
                    v.z = fmaxf(fmaf(v.z, ss.x, ss.y), 0.f);
                    v.w = fmaxf(fmaf(v.w, ss.x, ss.y), 0.f);
                }
                *reinterpret_cast<float4*>(&Bs[buf][bk0 + j * VROWS][bnl]) = sel4(ok, v);
            }
        } else if constexpr (TAPK) {
            const int ci0 = ((kt / BK) / T) * BK;
#pragma unroll
            for (int j = 0; j < B_PER; ++j) {
                const int r = bk0 + j * (NT / BN);
                const bool ok = b_inb && kt + r < k_end;
                float v = rb[j];
                if (PRO) {
                    const float2 ss = s_ss[min(ci0 + r, Cin - 1)];
                    v = fmaxf(fmaf(v, ss.x, ss.y), 0.f);
                }
                Bs[buf][r][bnl] = ok ? v : 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < B_PER; ++j) Bs[buf][bk0 + j * (NT / BN)][bnl] = rb[j];
        }
    };

    // Accumulators start at bias (+ residual): those loads overlap the operand
    // prologue instead of trailing the main loop, and the epilogue only stores.
    // An element is read and written by the same thread, so res may alias y.
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
        obase[j] = (int64_t)b * Cout * P + p;
    }
    floatx16 acc[TM][TN];
    const bool direct = slab == nullptr;
    ubpl::seed_acc<TM, TN>(acc, direct ? bias : nullptr, direct ? res : nullptr, obase, m0 + wm, Cout, P);

    if (PRO) __syncthreads();  // s_sc / s_sh ready
    const int nkt = (k_end - k_begin + BK - 1) / BK;
    // T14 order (cdna_hip_programming.md §5 'glds vs register staging'): tile
    // t+1 is written to LDS right AFTER the barrier that ends tile t-1's reads,
    // and tile t+2's loads are issued at once, so every load has a whole K step
    // of MFMAs to land in.
    if (nkt > 0) {
        load_a(k_begin);
        load_b(k_begin);
        store_ab(0, k_begin);
    }
    if (nkt > 1) {
        load_a(k_begin + BK);
        load_b(k_begin + BK);
    }
    for (int t = 0; t < nkt; ++t) {
        const int cur = t & 1;
        __syncthreads();   // tile t visible; tile t-1's reads of buffer cur^1 done
        if (t + 1 < nkt) {
            store_ab(cur ^ 1, k_begin + (t + 1) * BK);
            if (t + 2 < nkt) {
                load_a(k_begin + (t + 2) * BK);
                load_b(k_begin + (t + 2) * BK);
            }
        }
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
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
    }

    if (slab != nullptr) {
        // split-K partial tile: slab[z][m][n]
        float* sl = slab + (int64_t)bz * Cout * N;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t n = n0 + wn + 32 * j + li;
            if (n >= N) continue;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                    if (m < Cout) sl[(int64_t)m * N + n] = acc[i][j][r];
                }
        }
        return;
    }
    // ---- epilogue: stores, coalesced along n (bias / residual are in acc)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        if (!nok[j]) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m < Cout) y[obase[j] + (int64_t)m * P] = acc[i][j][r];
            }
    }
}

// ------------------------------------------------------------------ host side
Plan plan_of(int Cout, int64_t N, int Ktot) {
    static const int occ128 = query_occ((const void*)conv_fwd_kernel<128, 128, 3, 1, true, false, true, true>, 4);
    static const int occ64 = query_occ((const void*)conv_fwd_kernel<64, 128, 3, 1, true, false, true, true>, 5);
    return fwd_plan(Cout, N, Ktot, occ128, occ64);
}

// What every launch of ubpl_conv2d_forward shares
struct FwdArgs {
    const float *x, *w, *bias, *pscale, *pshift, *res;
    float* y;
    int B, Cin, H, W, Cout, Ho, Wo;
    Plan pl;
    float* slab;
    hipStream_t st;
};

// The conv_fwd_kernel instantiations that are built: vector activation loads on 1x1 only;
// float4 weight rows always on 3x3 (Cin % 16 == 0), never on the stem (Cin = 3).
constexpr bool fwd_built(int KS, bool VECB, bool AVEC) { return (KS == 1 || !VECB) && (KS == 3 ? AVEC : KS == 1 || !AVEC); }

template <int BM, int KS, bool PRO, bool VECB, bool AVEC>
int launch_fwd(const FwdArgs& a) {
    constexpr int BN = 128;
    constexpr bool TAPK = KS != 7;   // (the stem's 3 channels: a K tile straddles taps)
    const Plan& pl = a.pl;
    const int64_t N = (int64_t)a.B * a.Ho * a.Wo;
    dim3 grid((unsigned)((N + BN - 1) / BN), (unsigned)((a.Cout + BM - 1) / BM), (unsigned)pl.splits);
    const bool split = pl.splits > 1;
    hipLaunchKernelGGL((conv_fwd_kernel<BM, BN, KS, conv_stride(KS), PRO, VECB, TAPK, AVEC>), grid, dim3(NT), 0, a.st,
                       a.x, a.w, a.bias, a.pscale, a.pshift, split ? nullptr : a.res, a.y, a.B, a.Cin, a.H, a.W,
                       a.Cout, a.Ho, a.Wo, pl.kchunk, split ? a.slab : nullptr);
    UBPL_LAUNCH_CHECK();
    if (split) {
        launch_split_reduce(a.slab, pl.splits, a.Cout, a.Ho * a.Wo, N, a.bias, a.res, a.y, a.st);
        UBPL_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

// Floats of workspace ubpl_conv2d_forward needs (split-K slab); 0 = none.
// w must be in the layout of ubpl_conv_weight_tapmajor for KS > 1.
UBPL_API int64_t ubpl_conv2d_forward_workspace(int B, int Cin, int Cout, int KS, int Ho, int Wo) {
    const int64_t N = (int64_t)B * Ho * Wo;
    const Plan pl = plan_of(Cout, N, Cin * KS * KS);
    return pl.splits > 1 ? (int64_t)pl.splits * Cout * N : 0;
}

// y[B,Cout,Ho,Wo] = conv(relu(x*pscale + pshift) or x, w~, pad=(KS-1)/2) + bias (+ res).
// w~: [Cout][Cin] for KS == 1, tap-major [Cout][KS*KS][Cin] otherwise.
// Supported (KS, stride): (1,1), (3,1), (7,2).  res may alias y.  slab: the
// workspace of ubpl_conv2d_forward_workspace (nullable when that is 0).
UBPL_API int ubpl_conv2d_forward(const float* x, int B, int Cin, int H, int W, const float* w, const float* bias,
                                 int Cout, int KS, int stride, const float* pscale, const float* pshift,
                                 const float* res, float* y, int Ho, int Wo, float* slab, void* stream) {
    const bool pro = pscale != nullptr;
    if (pro && Cin > MAXC) return (int)hipErrorInvalidValue;
    const FwdArgs a{x, w, bias, pscale, pshift, res, y, B, Cin, H, W, Cout, Ho, Wo,
                    plan_of(Cout, (int64_t)B * Ho * Wo, Cin * KS * KS), slab, (hipStream_t)stream};
    if (a.pl.splits > 1 && slab == nullptr) return (int)hipErrorInvalidValue;
    if (!conv_shape_ok(KS, stride) || (KS == 3 && Cin % BK != 0)) return (int)hipErrorInvalidValue;
    // VECB: float4 activation loads (1x1: a K row is a pixel row of one channel);
    // AVEC: float4 weight rows (Ktot % 4 == 0 and w 16-B aligned; the stem's form takes any w)
    const bool vecb = KS == 1 && (Ho * Wo) % 4 == 0 && ((uintptr_t)x & 15) == 0;
    const bool avec = KS != 7 && (Cin * KS * KS) % 4 == 0 && ((uintptr_t)w & 15) == 0;
    return pick(
        [&](auto KS_, auto PRO, auto VECB, auto AVEC, auto BM) {
            if constexpr (fwd_built(KS_, VECB, AVEC)) return launch_fwd<BM, KS_, PRO, VECB, AVEC>(a);
            return (int)hipErrorInvalidValue;
        },
        among<1, 3, 7>{KS}, among<0, 1>{pro}, among<0, 1>{vecb}, among<0, 1>{avec}, among<128, 64>{a.pl.bm});
}
