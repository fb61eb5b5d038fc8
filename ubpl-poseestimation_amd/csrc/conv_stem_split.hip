// The 7x7 stride-2 stem on the split paths by space-to-depth: the phase image and the 4x4
// weights for ubpl_conv2d_forward_psa(KS = 4) (conv_psa.hip), and the stem's weight gradient.
// Shared pieces: split_common.h.
#include "split_common.h"

namespace {

// ------------------------------------------------------------------ the stem on the split path
// Space-to-depth: the 7x7 stride-2 pad-3 stem conv (models/pose/hourglass.py
// pre.0, models/base/layers.py:31-50) = a stride-1 4x4 conv over the 4 phase
// images x'[c*4 + 2ph + pw][i][j] = x[c][2i + ph][2j + pw] with taps
// (a, b) in 0..3 at offsets (a - 2, b - 2) and the kernel
// w'[o][c*4 + 2ph + pw][a][b] = w[o][c][2(a - 2) + ph + 3][2(b - 2) + pw + 3]
// (zero outside the 7x7 window): K = 16 channels x 16 taps on the split path
// instead of 147 on the exact-f32 kernel.  The phase image goes straight to the
// PSA layout (C*4 <= 16 channels, the rest zero) with a `pad` border.
template <int NP>
__global__ void __launch_bounds__(256) stem_s2d_split_kernel(const float* __restrict__ x, int C, int H, int W,
                                                            int pad, uint16_t* __restrict__ dst, int64_t plane) {
    const int Ho = H / 2, Wo = W / 2;
    const int Hp = Ho + 2 * pad, Wp = Wo + 2 * pad;
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= Hp * Wp) return;
    const int hp = pix / Wp, wq = pix - hp * Wp;
    const int i = hp - pad, j = wq - pad;
    const bool in = i >= 0 && i < Ho && j >= 0 && j < Wo;
    float v[16];
#pragma unroll
    for (int ch = 0; ch < 16; ++ch) {
        const int c = ch >> 2, ph = (ch >> 1) & 1, pw = ch & 1;
        const bool ok = in && c < C;
        const int64_t off = (((int64_t)b * C + (ok ? c : 0)) * H + (ok ? 2 * i + ph : 0)) * W + (ok ? 2 * j + pw : 0);
        const float t = x[off];
        v[ch] = ok ? t : 0.f;
    }
    ubpl::store_psa_row<NP>(v, dst + (((int64_t)b * Hp + hp) * Wp + wq) * 16, plane);
}

// w [Cout][C][KS][KS] (KS odd, stride 2, pad KS/2) -> the split, grouped
// tap-major weights of the s2d conv: [piece][Cout][KT*KT taps][16 channels]
// (KT = 4 for KS = 7): tap (a, b) of phase (ph, pw) is w[.][.][2(a - KT/2) +
// ph + KS/2][2(b - KT/2) + pw + KS/2], zero outside the KSxKS window.
template <int NP>
__global__ void __launch_bounds__(256) stem_weight_s2d_split_kernel(const float* __restrict__ w, int Cout, int C,
                                                                   int KS, int KT, uint16_t* __restrict__ dst,
                                                                   int64_t plane) {
    const int64_t total = (int64_t)Cout * KT * KT * 16;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % 16);
    const int tap = (int)((idx / 16) % (KT * KT));
    const int o = (int)(idx / (16 * KT * KT));
    const int a = tap / KT, bb = tap - a * KT;
    const int c = ch >> 2, ph = (ch >> 1) & 1, pw = ch & 1;
    const int kh = 2 * (a - KT / 2) + ph + KS / 2, kw = 2 * (bb - KT / 2) + pw + KS / 2;
    const bool ok = c < C && kh >= 0 && kh < KS && kw >= 0 && kw < KS;
    float v = ok ? w[(((int64_t)o * C + c) * KS + kh) * KS + kw] : 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const __bf16 hv = (__bf16)v;
        dst[(int64_t)p * plane + idx] = __builtin_bit_cast(uint16_t, hv);
        v -= (float)hv;
    }
}

// ------------------------------------------------------------------ the stem's weight gradient (space-to-depth)
// The 7x7 stride-2 stem's weight gradient as the weight gradient of its
// space-to-depth form (stem_s2d_split_kernel / stem_weight_s2d_split_kernel): a
// stride-1 4x4 conv of the 16-channel phase image, so
//   dW'[co][tap (a, b)][ci] = sum over (n, oh, ow) of dy[n, co, oh, ow] * x'[n, ci, oh + a - 2, ow + b - 2]
// on the split path, both operands PSA images: dys = split(dy) with a 1-pixel
// border (the BN backward emits it), xs = the forward's phase image with its
// 2-pixel border (kept for the backward).  GEMM: M = Cout (64-row blocks), N =
// 16 taps x 16 channels (all of it per workgroup), K = pixels, K step = 16
// consecutive pixels of one output row; split over workgroups into a slab
// [z][Cout][257] reduced by wgrad_reduce_kernel (T = 16, Cin = 16; last column:
// the bias gradient, from wave 0's A fragments).  Wave w takes kernel row a = w
// (4 taps x 16 channels = 64 columns) x the 64 rows: wave tile 64 x 64.
// Stage: A [piece][4 channel groups][16 px][32 B] (odd groups' pixel rows 0-3
// <-> 4-7 swapped, as wgrad3_psa_kernel), B the 4-row x 19-pixel halo of the
// step's receptive field [piece][4 rows][19 px][32 B] (a tap is a pixel offset);
// fragments by ds_read_b64_tr_b16.  3-stage ring.
template <int NP>
__global__ void __launch_bounds__(NT, 2) wgrad_stem_psa_kernel(const uint16_t* __restrict__ dys, int64_t dplane,
                                                              const uint16_t* __restrict__ xs, int64_t xplane,
                                                              int B, int Cout, int H, int W, int steps_per_split,
                                                              float* __restrict__ slab) {
    constexpr int NS = 3, HXP = 19, BROWS = 4 * HXP;       // halo: 4 rows x 19 pixels
    constexpr int API = 4 * 16 * 32;                       // A piece image: 4 groups x 16 px x 32 B
    constexpr int BPI = BROWS * 32;                        // B piece image
    constexpr int AB = NP * API, SUB = AB + NP * BPI;
    constexpr int AI = NP * 2, BI = NP * 3, NI = AI + BI;  // DMA instructions per stage (1 KB each)
    constexpr int NPW = (NI + 3) / 4;                      // per wave
    __shared__ __attribute__((aligned(16))) char lds[NS * SUB];
    typedef short v4i16 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) v4i16* tr_ptr_t;

    const int Hp = H + 2, Wp = W + 2, Hx = H + 4, Wx = W + 4;
    const int Go = Cout >> 4;
    constexpr int Ntot = 256, Nt = Ntot + 1;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid (Cout / 64, splits): the row blocks of one split side by side (same L2)
    const int lam = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int by = lam % gridDim.x, bz = lam / gridDim.x;
    const int m0 = by * 64;
    const int wsteps = W >> 4;
    const int total_steps = B * H * wsteps;
    const int s_begin = bz * steps_per_split;
    const int s_end = min(total_steps, s_begin + steps_per_split);
    const int nkt = max(0, s_end - s_begin);

    // per-instruction lane offsets (bytes, relative to the step's base): instruction i
    // of a stage, i = u * 4 + wid: A piece i / 2 (groups 2 (i % 2), +1), B piece
    // (i - AI) / 3, 32-pixel chunk (i - AI) % 3 (the last one overlapping: starts at 76 - 32)
    uint32_t loff[NPW];
    int lpiece[NPW];
    bool lisa[NPW], lon[NPW];
    const int lrow = lane >> 1, lhalf = lane & 1;
#pragma unroll
    for (int u = 0; u < NPW; ++u) {
        const int i = u * 4 + wid;
        lon[u] = i < NI;
        lisa[u] = i < AI;
        if (i < AI) {
            const int gl = 2 * (i % 2) + (lrow >> 4);
            const int rphys = lrow & 15, rlog = rphys ^ (4 * (gl & 1));
            lpiece[u] = i / 2;
            loff[u] = (uint32_t)((((int64_t)gl * Hp * Wp) + rlog) * 16 + 8 * lhalf) * 2;
        } else {
            const int j = i - AI, c = j % 3;
            const int q = min(c * 32, BROWS - 32) + lrow;
            const int a = q / HXP, px = q - a * HXP;
            lpiece[u] = j / 3;
            loff[u] = (uint32_t)(((int64_t)a * Wx + px) * 16 + 8 * lhalf) * 2;
        }
    }
    const char* dys_m = reinterpret_cast<const char*>(dys + (int64_t)(m0 >> 4) * Hp * Wp * 16);
    auto stage = [&](int buf, int s) {
        if (s >= s_end) return;
        const int b = s / (H * wsteps);
        const int rem = s - b * (H * wsteps);
        const int oh = rem / wsteps, ow0 = (rem - oh * wsteps) * 16;
        const int64_t aoff = ((int64_t)b * Go * Hp * Wp + (int64_t)(oh + 1) * Wp + ow0 + 1) * 16;
        const int64_t boff = (((int64_t)b * Hx + oh) * Wx + ow0) * 16;
        char* base = lds + buf * SUB;
#pragma unroll
        for (int u = 0; u < NPW; ++u) {
            if (!lon[u]) continue;
            const int i = u * 4 + wid;
            if (lisa[u]) {
                const char* src = dys_m + 2 * (lpiece[u] * dplane + aoff);
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + loff[u]),
                                                 (lds_ptr_t)(base + lpiece[u] * API + (i % 2) * 1024), 16, 0, 0);
            } else {
                const int j = i - AI, c = j % 3;
                const char* src = reinterpret_cast<const char*>(xs) + 2 * (lpiece[u] * xplane + boff);
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + loff[u]),
                                                 (lds_ptr_t)(base + AB + lpiece[u] * BPI + min(c * 32, BROWS - 32) * 32),
                                                 16, 0, 0);
            }
        }
    };
    // this wave's DMA instructions per stage (the counted waits below)
    const int mine = (NI - wid + 3) / 4;

    // transposed reads: 16-lane group g16 = lane >> 4; lane i16 = (qrow, pcol)
    const int g16 = lane >> 4, i16 = lane & 15;
    const int qrow = i16 >> 2, pcol = i16 & 3;
    int aoffs[2][2], boffs[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int grp = 2 * i + (g16 & 1);
            const int row = (8 * (g16 >> 1) + 4 * t + qrow) ^ (4 * (grp & 1));
            aoffs[i][t] = grp * 512 + row * 32 + 8 * pcol;
        }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int px = 8 * (g16 >> 1) + 4 * t + qrow + 2 * j + (g16 & 1);   // tap b = 2j + (g16 & 1)
            boffs[j][t] = (wid * HXP + px) * 32 + 8 * pcol;
        }

    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const bool bias_wave = wid == 0;
    float bsum[2] = {0.f, 0.f};

    stage(0, s_begin);
    stage(1, s_begin + 1);
    for (int t = 0; t < nkt; ++t) {
        // stage t landed (this wave's stage t+1 DMA may stay in flight)
        if (t + 1 < nkt) {
            // NP = 3: 15 instructions per stage (4 / 4 / 4 / 3 per wave); NP = 1: 5 (2 / 1 / 1 / 1)
            if (mine == 4) vm_wait<4>();
            else if (mine == 3) vm_wait<3>();
            else if (mine == 2) vm_wait<2>();
            else vm_wait<1>();
        } else {
            vm_wait<0>();
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + 2 < nkt) stage((t + 2) % NS, s_begin + t + 2);
        char* base = lds + (t % NS) * SUB;
        bf16x8 af[2][NP], bfr[2][NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + p * API + aoffs[i][0]));
                const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + p * API + aoffs[i][1]));
                const short8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                af[i][p] = __builtin_bit_cast(bf16x8, v);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + AB + p * BPI + boffs[j][0]));
                const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + AB + p * BPI + boffs[j][1]));
                const short8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                bfr[j][p] = __builtin_bit_cast(bf16x8, v);
            }
        }
        if (bias_wave) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int p = 0; p < NP; ++p)
#pragma unroll
                    for (int e = 0; e < 8; ++e) bsum[i] += (float)af[i][p][e];
        }
        floatx16 tmp[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) tmp[i][j] = mfma_split0<NP>(af[i], bfr[j]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) drain(acc[i][j], tmp[i][j]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    float* sl = slab + (int64_t)bz * Cout * Nt;
    const int li = lane & 31, h = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = 64 * wid + 32 * j + li;                   // tap 4 wid + 2 j + li / 16, channel li % 16
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                sl[(int64_t)m * Nt + n] = acc[i][j][r];
            }
    }
    if (bias_wave) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // lane (r, h) summed channel 32i + r over pixels 8h..8h+7 of each step
            const float v = bsum[i] + __shfl_xor(bsum[i], 32, 64);
            if (h == 0) sl[(int64_t)(m0 + 32 * i + li) * Nt + Ntot] = v;
        }
    }
}

// the space-to-depth weight gradient dws [Cout][16 ci][16 taps] + its bias column dbs
// [Cout] (wgrad_reduce_kernel's layout for Cin = 16, T = 16) -> the 7x7 gradient dw
// [Cout][C][7][7] (+)= and db (+)=: tap (a, b), channel c*4 + 2 ph + pw of the phase
// image holds w[.][c][2 (a - 2) + ph + 3][2 (b - 2) + pw + 3], i.e. kh -> (ph, a) =
// ((kh + 1) & 1, (kh + 1 - ph) / 2)
__global__ void __launch_bounds__(256) stem_wgrad_map_kernel(const float* __restrict__ dws,
                                                             const float* __restrict__ dbs, int Cout, int C,
                                                             float* __restrict__ dw, float* __restrict__ db,
                                                             int accumulate) {
    constexpr int KS = 7;
    const int64_t total = (int64_t)Cout * C * KS * KS;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (db != nullptr && idx < Cout) db[idx] = accumulate ? db[idx] + dbs[idx] : dbs[idx];
    if (idx >= total) return;
    const int kw = (int)(idx % KS), kh = (int)((idx / KS) % KS);
    const int c = (int)((idx / (KS * KS)) % C), o = (int)(idx / (KS * KS * C));
    const int ph = (kh + 1) & 1, a = (kh + 1 - ph) / 2;
    const int pw = (kw + 1) & 1, bb = (kw + 1 - pw) / 2;
    const float v = dws[(int64_t)o * 256 + (c * 4 + 2 * ph + pw) * 16 + a * 4 + bb];
    dw[idx] = accumulate ? dw[idx] + v : v;
}

using namespace ubpl;

int wgrad_stem_splits(int B, int Cout, int H, int W) {
    const int steps = B * H * (W / 16);
    int s = 512 / (Cout / 64);                          // one round of 2 workgroups per CU
    if (s < 1) s = 1;
    if (s > steps / 8) s = steps / 8 > 0 ? steps / 8 : 1;
    const int per = (steps + s - 1) / s;
    return (steps + per - 1) / per;
}

}  // namespace

// ---- the stem on the split path (space-to-depth, see stem_s2d_split_kernel)
// x [B][C][H][W] (C <= 4, H, W even) -> PSA planes [B][1][H/2 + 2pad][W/2 + 2pad][16]
// of the 4 phase images per channel; pad >= 2 for the 7x7 stem.
UBPL_API int ubpl_stem_s2d_split(const float* x, int B, int C, int H, int W, int pad, int npieces, uint16_t* dst,
                                 int64_t plane, void* stream) {
    if (C < 1 || C > 4 || (H & 1) || (W & 1) || (npieces != 3 && npieces != 1) || pad < 0 || (plane % 8) != 0)
        return (int)hipErrorInvalidValue;
    const int Hp = H / 2 + 2 * pad, Wp = W / 2 + 2 * pad;
    dim3 grid((unsigned)((Hp * Wp + 255) / 256), (unsigned)B);
    return pick([&](auto np) {
        hipLaunchKernelGGL(stem_s2d_split_kernel<np>, grid, dim3(256), 0, (hipStream_t)stream, x, C, H, W, pad, dst,
                           plane);
        UBPL_LAUNCH_CHECK();
        return 0;
    }, among<1, 3>{npieces});
}

// w [Cout][C][KS][KS] (KS odd, C <= 4) -> split weights of the s2d conv for
// ubpl_conv2d_forward_psa (Cin = 16, KS' = (KS + 1) / 2 rounded up to even = 4
// for the 7x7 stem): npieces planes of Cout * KS'^2 * 16 bf16.
UBPL_API int ubpl_stem_weight_s2d_split(const float* w, int Cout, int C, int KS, int npieces, uint16_t* dst,
                                        int64_t plane, void* stream) {
    const int KT = ((KS + 1) / 2 + 1) & ~1;
    if (C < 1 || C > 4 || !(KS & 1) || (npieces != 3 && npieces != 1) || KT != 4 || (plane % 8) != 0)
        return (int)hipErrorInvalidValue;
    const int64_t total = (int64_t)Cout * KT * KT * 16;
    return pick([&](auto np) {
        hipLaunchKernelGGL(stem_weight_s2d_split_kernel<np>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, w, Cout, C, KS, KT, dst, plane);
        UBPL_LAUNCH_CHECK();
        return 0;
    }, among<1, 3>{npieces});
}

// ---- the stem's weight gradient on the split path (space-to-depth)
UBPL_API int64_t ubpl_wgrad_stem_psa_workspace(int B, int Cout, int H, int W) {
    if (B < 1 || Cout % 64 || W % 16 || H < 1) return 0;
    return (int64_t)wgrad_stem_splits(B, Cout, H, W) * Cout * 257 + (int64_t)Cout * 257;
}

UBPL_API int ubpl_wgrad_stem_psa(const uint16_t* dys, int64_t dplane, const uint16_t* xs, int64_t xplane, int B,
                                 int C, int Cout, int H, int W, int KS, float* slab, float* dw, float* db,
                                 int accumulate, int npieces, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if ((npieces != 3 && npieces != 1) || KS != 7 || C < 1 || C > 4 || Cout % 64 || W % 16 || H < 1 || B < 1 ||
        slab == nullptr)
        return (int)hipErrorInvalidValue;
    if ((((uintptr_t)dys) & 15) || (((uintptr_t)xs) & 15) || (dplane % 8) || (xplane % 8))
        return (int)hipErrorInvalidValue;
    const int splits = wgrad_stem_splits(B, Cout, H, W);
    const int steps = B * H * (W / 16);
    const int per = (steps + splits - 1) / splits;
    int e = pick([&](auto np) {
        hipLaunchKernelGGL((wgrad_stem_psa_kernel<np>), dim3((unsigned)(Cout / 64), (unsigned)splits), dim3(NT), 0,
                           st, dys, dplane, xs, xplane, B, Cout, H, W, per, slab);
        UBPL_LAUNCH_CHECK();
        return 0;
    }, among<1, 3>{npieces});
    if (e) return e;
    float* dws = slab + (int64_t)splits * Cout * 257;
    e = ubpl_wgrad_slab_reduce(slab, splits, Cout, 16, 16, 1, dws, dws + (int64_t)Cout * 256, 0, stream);
    if (e) return e;
    const int64_t total = (int64_t)Cout * C * KS * KS;
    hipLaunchKernelGGL(stem_wgrad_map_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dws,
                       dws + (int64_t)Cout * 256, Cout, C, dw, db, accumulate);
    UBPL_LAUNCH_CHECK();
    return 0;
}
