// The register-staged split forward convolution (6xbf16): activations read as f32, split
// in registers after the fused BN+ReLU prologue, stored to LDS.  The model runs on the
// pre-split-activation and split-on-load kernels (conv_psa.hip, conv_psah.hip,
// conv1x1_sol.hip); this path stays for the tests and tools/conv_split_bench.py.
#include "split_common.h"

namespace {

// ------------------------------------------------------------------ forward
// x NCHW f32; wp: NP planes (stride wplane elements) of the grouped tap-major
// weights [Cout][Ktot] as bf16; Cin % 16 == 0.  Epilogue / split-K slab as
// conv_f32_fwd.hip's conv_fwd_kernel.
template <int BM, int KS, int ST, bool PRO, int NP>
__global__ void __launch_bounds__(NT, 2) conv_fwd_split_kernel(
    const float* __restrict__ x, const uint16_t* __restrict__ wp, int64_t wplane, const float* __restrict__ bias,
    const float* __restrict__ pscale, const float* __restrict__ pshift, const float* res, float* y, int B, int Cin,
    int H, int W, int Cout, int Ho, int Wo, int kchunk, float* __restrict__ slab) {
    constexpr int PADK = (KS - 1) / 2;
    constexpr int T = KS * KS;
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int ACH = BM == 128 ? 2 : 1;   // 16-B weight chunks per thread per piece
    __shared__ uint4 lds[2 * NP * (BM + BN) * 4];
    uint4* As = lds;
    uint4* Bs = lds + 2 * NP * BM * 4;

    const int P = Ho * Wo, HWin = H * W;
    const int64_t N = (int64_t)B * P;
    const int Ktot = Cin * T;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: SGPR)
    const int wm = (wid >> 1) * (BM / 2), wn = (wid & 1) * (BN / 2);
    const int lam = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                              gridDim.x * gridDim.y * gridDim.z);
    const int by = lam % gridDim.y, bx = (lam / gridDim.y) % gridDim.x, bz = lam / (gridDim.y * gridDim.x);
    const int m0 = by * BM;
    const int64_t n0 = (int64_t)bx * BN;
    const int k_begin = bz * kchunk;
    const int k_end = min(Ktot, k_begin + kchunk);

    // ---- A (weights) loader: row am, chunks ac0 .. ac0 + ACH - 1
    const int am = tid % BM;
    const int ac0 = (tid / BM) * ACH;
    const bool am_ok = m0 + am < Cout;
    const uint16_t* wrow = wp + (int64_t)min(m0 + am, Cout - 1) * Ktot;
    // ---- B (activations) loader: column bn, k half g (16 k = one (group, tap))
    const int bnl = tid & (BN - 1);
    const int g = __builtin_amdgcn_readfirstlane(tid >> 7);
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

    uint4 ra[NP][ACH];
    float rb[16];
    bool b_inb = false;

    auto load = [&](int kt) {
        {
            const int k = min(kt + 8 * ac0, Ktot - 8 * ACH);
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int c = 0; c < ACH; ++c)
                    ra[p][c] = *reinterpret_cast<const uint4*>(wrow + (int64_t)p * wplane + k + 8 * c);
        }
        const int kk = kt + 16 * g;
        const int kg = kk >> 4;
        const int tap = kg % T;
        const int ci0 = min((kg / T) * 16, Cin - 16);
        const int kh = tap / KS, kw = tap - kh * KS;
        const int ih = coh * ST - PADK + kh, iw = cow * ST - PADK + kw;
        b_inb = cvalid && kk < k_end && ih >= 0 && ih < H && iw >= 0 && iw < W;
        const float* src = xb + (int64_t)ci0 * HWin + (b_inb ? ih * W + iw : 0);
#pragma unroll
        for (int j = 0; j < 16; ++j) rb[j] = src[(int64_t)j * HWin];
    };
    auto store = [&](int buf, int kt) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int c = 0; c < ACH; ++c) {
                const int ch = ac0 + c;
                const bool ok = am_ok && kt + 8 * ch < k_end;
                As[((buf * NP + p) * BM + am) * 4 + swz(am, ch)] = ok ? ra[p][c] : make_uint4(0, 0, 0, 0);
            }
        // prologue on every element (unconditional scalar loads of the 16
        // channels' coefficients), then a select: a load or an LDS read under
        // the in-bounds condition becomes a branch with its own vmcnt(0)
        float v[16];
        if (PRO) {
            const int kg = (kt + 16 * g) >> 4;
            const int ci0 = __builtin_amdgcn_readfirstlane(min((kg / T) * 16, Cin - 16));
            float sc[16], sh[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                sc[j] = pscale[ci0 + j];
                sh[j] = pshift[ci0 + j];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = fmaxf(fmaf(rb[j], sc[j], sh[j]), 0.f);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = rb[j];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = b_inb ? v[j] : 0.f;
        uint32_t pk[NP][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t o[NP];
            split2<NP>(v[2 * i], v[2 * i + 1], o);
#pragma unroll
            for (int p = 0; p < NP; ++p) pk[p][i] = o[p];
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            uint4* rowp = Bs + ((buf * NP + p) * BN + bnl) * 4;
            rowp[swz(bnl, 2 * g)] = make_uint4(pk[p][0], pk[p][1], pk[p][2], pk[p][3]);
            rowp[swz(bnl, 2 * g + 1)] = make_uint4(pk[p][4], pk[p][5], pk[p][6], pk[p][7]);
        }
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nkt = (k_end - k_begin + BK - 1) / BK;
    if (nkt > 0) {
        load(k_begin);
        store(0, k_begin);
    }
    if (nkt > 1) load(k_begin + BK);
    const int li = lane & 31, h = lane >> 5;
    for (int t = 0; t < nkt; ++t) {
        const int cur = t & 1;
        __syncthreads();
        if (t + 1 < nkt) {
            store(cur ^ 1, k_begin + (t + 1) * BK);
            if (t + 2 < nkt) load(k_begin + (t + 2) * BK);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int c = 2 * s + h;
            bf16x8 af[TM][NP], bfr[TN][NP];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm + 32 * i + li;
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    af[i][p] = __builtin_bit_cast(bf16x8, As[((cur * NP + p) * BM + row) * 4 + swz(row, c)]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wn + 32 * j + li;
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    bfr[j][p] = __builtin_bit_cast(bf16x8, Bs[((cur * NP + p) * BN + row) * 4 + swz(row, c)]);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (NP == 3) {
                        // the bf16 MFMA aligns its 17 addends to the largest and
                        // truncates below ~2^-26 of it (tools/experiments/mfma_numerics):
                        // against a large running sum that bias grows with K.  Each
                        // 16-k chunk starts from 0 and is added with a rounded f32 add.
                        floatx16 tmp;
#pragma unroll
                        for (int r = 0; r < 16; ++r) tmp[r] = 0.f;
                        mfma_split<NP>(tmp, af[i], bfr[j]);
                        drain(acc[i][j], tmp);
                    } else {
                        mfma_split<NP>(acc[i][j], af[i], bfr[j]);
                    }
                }
        }
    }

    if (slab != nullptr) {
        float* sl = slab + (int64_t)bz * Cout * N;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t n = n0 + wn + 32 * j + li;
            if (n >= N) continue;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < Cout) sl[(int64_t)m * N + n] = acc[i][j][r];
                }
        }
        return;
    }
    // epilogue: + bias (+ residual; res may alias y: all loads before any store)
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
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = min(m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h, Cout - 1);
                if (bias) acc[i][j][r] += bias[m];
                if (res) acc[i][j][r] += res[obase[j] + (int64_t)m * P];
            }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        if (!nok[j]) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < Cout) y[obase[j] + (int64_t)m * P] = acc[i][j][r];
            }
    }
}

using namespace ubpl;

// occupancy of conv_fwd_split_kernel for the plan's cost model
const TileOcc& fwd_occ() {
    static const TileOcc d = query_tile_occ({{2, 1}, {3, 2}}, (const void*)conv_fwd_split_kernel<128, 3, 1, true, 2>,
                                            (const void*)conv_fwd_split_kernel<128, 3, 1, true, 3>,
                                            (const void*)conv_fwd_split_kernel<64, 3, 1, true, 2>,
                                            (const void*)conv_fwd_split_kernel<64, 3, 1, true, 3>, NT);
    return d;
}

struct FwdArgs {
    const float* x;
    const uint16_t* wp;
    int64_t plane;
    const float *bias, *ps, *sh, *res;
    float* y;
    int B, Cin, H, W, Cout, Ho, Wo;
    Plan pl;
    float* slab;
    hipStream_t st;
};

template <int BM, int KS, int ST, bool PRO, int NP>
int launch_fwd(const FwdArgs& a) {
    const int64_t N = (int64_t)a.B * a.Ho * a.Wo;
    dim3 grid((unsigned)((N + BN - 1) / BN), (unsigned)((a.Cout + BM - 1) / BM), (unsigned)a.pl.splits);
    const bool split = a.pl.splits > 1;
    hipLaunchKernelGGL((conv_fwd_split_kernel<BM, KS, ST, PRO, NP>), grid, dim3(NT), 0, a.st, a.x, a.wp, a.plane,
                       a.bias, a.ps, a.sh, split ? nullptr : a.res, a.y, a.B, a.Cin, a.H, a.W, a.Cout, a.Ho, a.Wo,
                       a.pl.kchunk, split ? a.slab : nullptr);
    UBPL_LAUNCH_CHECK();
    if (split) {
        launch_split_reduce(a.slab, a.pl.splits, a.Cout, a.Ho * a.Wo, N, a.bias, a.res, a.y, a.st);
        UBPL_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

// Floats of split-K workspace ubpl_conv2d_forward_split needs; 0 = none.
UBPL_API int64_t ubpl_conv2d_forward_split_workspace(int B, int Cin, int Cout, int KS, int Ho, int Wo, int npieces) {
    const int64_t N = (int64_t)B * Ho * Wo;
    const Plan pl = fwd_plan(Cout, N, Cin * KS * KS, npieces, BK, fwd_occ());
    return pl.splits > 1 ? (int64_t)pl.splits * Cout * N : 0;
}

// y = conv(relu(x*pscale + pshift) or x, w, pad (KS-1)/2) + bias (+ res) on the
// split-bf16 MFMA path.  wsplit: npieces (3) bf16 planes, `plane`
// elements apart, of the weights in ubpl_conv_weights_split's layout.
// (KS, stride) in {(1,1), (3,1)}; Cin % 16 == 0; res may alias y.
UBPL_API int ubpl_conv2d_forward_split(const float* x, int B, int Cin, int H, int W, const uint16_t* wsplit,
                                       int64_t plane, const float* bias, int Cout, int KS, int stride,
                                       const float* pscale, const float* pshift, const float* res, float* y, int Ho,
                                       int Wo, float* slab, int npieces, void* stream) {
    if (Cin % 16 != 0 || stride != 1 || npieces != 3) return (int)hipErrorInvalidValue;
    if ((((uintptr_t)wsplit) & 15) != 0 || (plane % 8) != 0) return (int)hipErrorInvalidValue;
    const int64_t N = (int64_t)B * Ho * Wo;
    const Plan pl = fwd_plan(Cout, N, Cin * KS * KS, npieces, BK, fwd_occ());
    if (pl.splits > 1 && slab == nullptr) return (int)hipErrorInvalidValue;
    const FwdArgs a{x, wsplit, plane, bias, pscale, pshift, res, y, B, Cin, H, W, Cout, Ho, Wo, pl, slab,
                    (hipStream_t)stream};
    return pick([&](auto KS_, auto BM, auto PRO) { return launch_fwd<BM, KS_, 1, PRO != 0, 3>(a); },
                among<1, 3>{KS}, among<128, 64>{pl.bm}, among<0, 1>{pscale != nullptr});
}
