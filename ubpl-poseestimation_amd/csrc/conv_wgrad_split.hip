// Weight gradients on the split paths: the 3x3 from pre-split operands (wgrad3_psa_kernel,
// wgrad3_psa64_kernel) and the 1x1 with both operands split on load (wgrad1_sol_kernel).
// Shared pieces: split_common.h.
#include "split_common.h"

namespace {

// ------------------------------------------------------------------ 3x3 weight gradient
// dW[co][tap][ci] = sum over (b, oh, ow) of dy[b,co,oh,ow] * x[b,ci,oh+kh-1,ow+kw-1]
// on the split path, both operands in the PSA layout with a 1-pixel border
// (dy: the data gradient's own pre-split operand; x: the forward's pre-split
// conv input = relu(bn(t1)), kept for the backward).  GEMM: M = co, N = (tap,
// ci) tap-major (n-tile = one tap x 128 channels), K = pixels, K step = 16
// consecutive pixels of one output row (W % 16 == 0), split over workgroups
// into a slab [z][Cout][9*Cin + 1] reduced by conv_reduce.hip's wgrad_reduce_kernel
// (last column: the bias gradient, summed by the tap-0 workgroups).
// The MFMA wants 8 consecutive pixels of one channel per lane, the PSA image
// holds 16 channels per pixel: fragments come from LDS by
// ds_read_b64_tr_b16 (a 16-lane group reads a 4-pixel x 16-channel block,
// lane i gets channel i's 4 pixels), two per 8-bf16 fragment.  LDS stage
// image [piece][16-channel group][16 pixel rows][32 B]; odd groups store
// pixel rows 0-3 <-> 4-7 swapped (pre-permuted DMA source) so the two groups a
// 32-lane half reads sit in opposite 128-B bank halves.
template <int NP, int CB = 128>
__global__ void __launch_bounds__(NT, 2) wgrad3_psa_kernel(const uint16_t* __restrict__ dys, int64_t dplane,
                                                          const uint16_t* __restrict__ xs, int64_t xplane, int B,
                                                          int Cin, int Cout, int H, int W, int steps_per_split,
                                                          float* __restrict__ slab, const float* __restrict__ dscale) {
    // NP = 2 (2xfp16): dys are the fp16 pieces of dy * (*dscale) (bn_bwd.hip fp16_scale_for), xs of
    // x * FP16_ACT_SCALE (the forward's image): the slab gets the products unscaled exactly.
    // CB = channel block of both tile sides (128, or 64 for the 64-channel convs:
    // wave tile 32 x 32, waves 0-1 move the operands)
    constexpr int BM = CB, TM = CB / 64, TN = CB / 64, NS = 3;
    constexpr int GR = CB / 16;                            // channel groups per operand tile
    constexpr int PI = GR * 512;                           // piece image: GR groups x 16 px x 32 B
    constexpr int AB = NP * PI, BB = NP * PI;              // bytes per 16-pixel step
    // 64-channel tiles carry two 16-pixel steps per stage (one barrier per 12 MFMA
    // chains instead of 6)
    constexpr int KS2 = CB == 64 ? 2 : 1;
    constexpr int SUB = AB + BB;
    __shared__ __attribute__((aligned(16))) char lds[NS * KS2 * SUB];
    typedef short v4i16 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) v4i16* tr_ptr_t;

    const int Hp = H + 2, Wp = W + 2;
    const int Gci = Cin >> 4, Gco = Cout >> 4;
    const int Ntot = 9 * Cin, Nt = Ntot + 1;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: SGPR)
    const int wm = (wid >> 1) * (CB / 2), wn = (wid & 1) * (CB / 2);
    // tile order: n tiles (tap, ci) fastest so the 9 taps of one K split share an L2
    const int lam = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                              gridDim.x * gridDim.y * gridDim.z);
    const int bx = lam % gridDim.x, by = (lam / gridDim.x) % gridDim.y, bz = lam / (gridDim.x * gridDim.y);
    const int m0 = by * BM;
    const int ntile_per_tap = Cin / CB;
    const int tap = bx / ntile_per_tap, ci0 = (bx - tap * ntile_per_tap) * CB;
    const int kh = tap / 3, kw = tap - 3 * (tap / 3);
    const int wsteps = W >> 4;
    const int total_steps = B * H * wsteps;
    const int s_begin = bz * steps_per_split;
    const int s_end = min(total_steps, s_begin + steps_per_split);
    const int nkt = max(0, s_end - s_begin);

    // DMA lane geometry: wave w < GR/2 moves channel groups 2w, 2w+1 of both operands
    const bool d_issue = wid < GR / 2;
    const int gl = 2 * wid + (lane >> 5);
    const int rphys = (lane & 31) >> 1;
    const int rlog = rphys ^ (4 * (gl & 1));
    const int64_t HWp = (int64_t)Hp * Wp;
    // per-lane 32-bit byte offsets; the rest of each DMA address is wave-uniform
    // (scalar base + vector offset addressing, no 64-bit VALU per instruction)
    const uint32_t a_lane = (uint32_t)(((gl * HWp + rlog) * 16 + 8 * (lane & 1)) * 2);
    const uint32_t b_lane = a_lane;
    const char* dys_m = reinterpret_cast<const char*>(dys + (int64_t)(m0 >> 4) * HWp * 16);
    const char* xs_c = reinterpret_cast<const char*>(xs + (int64_t)(ci0 >> 4) * HWp * 16);
    auto stage1 = [&](char* base, int s) {
        const int b = s / (H * wsteps);
        const int rem = s - b * (H * wsteps);
        const int oh = rem / wsteps, ow0 = (rem - oh * wsteps) * 16;
        const int64_t aoff = (int64_t)b * Gco * HWp * 16 + ((int64_t)(oh + 1) * Wp + ow0 + 1) * 16;
        const int64_t boff = (int64_t)b * Gci * HWp * 16 + ((int64_t)(oh + kh) * Wp + ow0 + kw) * 16;
        if (!d_issue) return;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const char* ab = dys_m + 2 * (p * dplane + aoff);
            const char* bb = xs_c + 2 * (p * xplane + boff);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(ab + a_lane), (lds_ptr_t)(base + p * PI + wid * 1024), 16,
                                             0, 0);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(bb + b_lane), (lds_ptr_t)(base + AB + p * PI + wid * 1024),
                                             16, 0, 0);
        }
    };
    auto stage = [&](int buf, int s) {   // steps s .. s + KS2 - 1 (those before s_end)
#pragma unroll
        for (int u = 0; u < KS2; ++u)
            if (s + u < s_end) stage1(lds + (buf * KS2 + u) * SUB, s + u);
    };

    // transposed-read geometry: 16-lane group g reads channel group (tile base
    // + (g & 1)), pixel rows 8*(g >> 1) + 4t + q (q = i16 >> 2), columns 4*(i16 & 3)
    const int g16 = lane >> 4, i16 = lane & 15;
    const int qrow = i16 >> 2, pcol = i16 & 3;
    auto tr_off = [&](int grp, int t) {   // byte offset inside a piece image
        const int row = (8 * (g16 >> 1) + 4 * t + qrow) ^ (4 * (grp & 1));
        return grp * 512 + row * 32 + 8 * pcol;
    };
    int aoffs[TM][2], boffs[TN][2];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t) aoffs[i][t] = tr_off((wm + 32 * i) / 16 + (g16 & 1), t);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t) boffs[j][t] = tr_off((wn + 32 * j) / 16 + (g16 & 1), t);

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // the bias gradient of split z is summed by the tap (z % 9) workgroups (their
    // first 128 input channels), spreading that VALU work over the taps
    const bool bias_wave = tap == bz % 9 && ci0 == 0 && wn == 0;
    float bsum[TM] = {};

    const int iters = (nkt + KS2 - 1) / KS2;
    if (iters > 0) stage(0, s_begin);
    if (iters > 1) stage(1, s_begin + KS2);
    for (int t = 0; t < iters; ++t) {
        // counted wait only when the newer stage in flight is a full one
        if (t + 1 < iters && s_begin + (t + 2) * KS2 <= s_end) vm_wait<2 * NP * KS2>();
        else vm_wait<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + 2 < iters) stage((t + 2) % NS, s_begin + (t + 2) * KS2);
#pragma unroll
        for (int u = 0; u < KS2; ++u) {
            if (s_begin + t * KS2 + u >= s_end) break;
            char* base = lds + ((t % NS) * KS2 + u) * SUB;
            bf16x8 af[TM][NP], bfr[TN][NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const v4i16 lo =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + p * PI + aoffs[i][0]));
                    const v4i16 hi =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + p * PI + aoffs[i][1]));
                    const short8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    af[i][p] = __builtin_bit_cast(bf16x8, v);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const v4i16 lo =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + AB + p * PI + boffs[j][0]));
                    const v4i16 hi =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + AB + p * PI + boffs[j][1]));
                    const short8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    bfr[j][p] = __builtin_bit_cast(bf16x8, v);
                }
            }
            if (bias_wave) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int e = 0; e < 8; ++e) bsum[i] += piece_elem<NP>(af[i][p], e);
            }
            floatx16 tmp[TM][TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) tmp[i][j] = mfma_split0<NP>(af[i], bfr[j]);
            __builtin_amdgcn_sched_barrier(0);   // chains first, adds after (see conv_psa_kernel)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) drain(acc[i][j], tmp[i][j]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    float* sl = slab + (int64_t)bz * Cout * Nt;
    const int li = lane & 31, h = lane >> 5;
    float inv = 1.f, binv = 1.f;
    if constexpr (NP == 2) {
        binv = 1.f / *dscale;
        inv = binv / ubpl::FP16_ACT_SCALE;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = tap * Cin + ci0 + wn + 32 * j + li;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                sl[(int64_t)m * Nt + n] = acc[i][j][r] * inv;
            }
    }
    if (bias_wave) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            // lane (r, h) summed channel wm + 32i + r over pixels 8h..8h+7 of each step
            const float v = bsum[i] + __shfl_xor(bsum[i], 32, 64);
            if (h == 0) sl[(int64_t)(m0 + wm + 32 * i + li) * Nt + Ntot] = v * binv;
        }
    }
}

// 64-channel 3x3 weight gradient (wgrad3_psa_kernel's operands and slab): an
// n-tile is one kernel ROW — the 3 taps (kh, 0..2) x 64 input channels — so a
// wave's tile is 32 output channels x 96 (3 taps x 32 channels): 18 MFMA
// chains per barrier instead of 6 with 64 x 64 one-tap tiles.  Stage image: A
// [piece][4 groups][16 px][32 B], then B per tap kw [piece][4 groups][16 px][32 B]
// (the three taps' shifted pixel windows DMA'd separately); wave 0 moves A,
// wave 1 + kw moves tap kw of B (6 DMA instructions each per stage).
template <int NP>
__global__ void __launch_bounds__(NT, 2) wgrad3_psa64_kernel(const uint16_t* __restrict__ dys, int64_t dplane,
                                                            const uint16_t* __restrict__ xs, int64_t xplane, int B,
                                                            int Cin, int Cout, int H, int W, int steps_per_split,
                                                            float* __restrict__ slab, const float* __restrict__ dscale) {
    // NP = 2: the scales of wgrad3_psa_kernel
    constexpr int TN = 3, NS = 3;
    constexpr int PI = 4 * 512;               // piece image: 4 groups x 16 px x 32 B
    constexpr int OB = NP * PI;               // one operand image (A, or one tap of B)
    constexpr int SB = 4 * OB;                // stage: A + 3 taps of B
    __shared__ __attribute__((aligned(16))) char lds[NS * SB];
    typedef short v4i16 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) v4i16* tr_ptr_t;

    const int Hp = H + 2, Wp = W + 2;
    const int Gci = Cin >> 4, Gco = Cout >> 4;
    const int Ntot = 9 * Cin, Nt = Ntot + 1;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: SGPR)
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 96;
    const int lam = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                              gridDim.x * gridDim.y * gridDim.z);
    const int bx = lam % gridDim.x, by = (lam / gridDim.x) % gridDim.y, bz = lam / (gridDim.x * gridDim.y);
    const int m0 = by * 64;
    const int nci = Cin / 64;
    const int kh = bx / nci, ci0 = (bx - kh * nci) * 64;
    const int wsteps = W >> 4;
    const int total_steps = B * H * wsteps;
    const int s_begin = bz * steps_per_split;
    const int s_end = min(total_steps, s_begin + steps_per_split);
    const int nkt = max(0, s_end - s_begin);

    // DMA: group pair gp (2 groups, one per half-wave), the swizzled pixel row
    const int64_t HWp = (int64_t)Hp * Wp;
    const int rphys = (lane & 31) >> 1;
    uint32_t lane_off[2];
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
        const int gl = 2 * gp + (lane >> 5);
        const int rlog = rphys ^ (4 * (gl & 1));
        lane_off[gp] = (uint32_t)(((gl * HWp + rlog) * 16 + 8 * (lane & 1)) * 2);
    }
    const char* dys_m = reinterpret_cast<const char*>(dys + (int64_t)(m0 >> 4) * HWp * 16);
    const char* xs_c = reinterpret_cast<const char*>(xs + (int64_t)(ci0 >> 4) * HWp * 16);
    const int kw_w = wid - 1;   // the B tap this wave moves (waves 1..3)
    auto stage = [&](int buf, int s) {
        const int b = s / (H * wsteps);
        const int rem = s - b * (H * wsteps);
        const int oh = rem / wsteps, ow0 = (rem - oh * wsteps) * 16;
        char* base = lds + buf * SB;
        const char* src;
        int64_t plane;
        if (wid == 0) {
            src = dys_m + 2 * ((int64_t)b * Gco * HWp * 16 + ((int64_t)(oh + 1) * Wp + ow0 + 1) * 16);
            plane = dplane;
        } else {
            src = xs_c + 2 * ((int64_t)b * Gci * HWp * 16 + ((int64_t)(oh + kh) * Wp + ow0 + kw_w) * 16);
            plane = xplane;
            base += OB * (1 + kw_w);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int gp = 0; gp < 2; ++gp)
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + 2 * p * plane + lane_off[gp]),
                                                 (lds_ptr_t)(base + p * PI + gp * 1024), 16, 0, 0);
    };

    // transposed-read geometry (as wgrad3_psa_kernel)
    const int g16 = lane >> 4, i16 = lane & 15;
    const int qrow = i16 >> 2, pcol = i16 & 3;
    auto tr_off = [&](int grp, int t) {
        const int row = (8 * (g16 >> 1) + 4 * t + qrow) ^ (4 * (grp & 1));
        return grp * 512 + row * 32 + 8 * pcol;
    };
    int aoffs[2], boffs[TN][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) aoffs[t] = tr_off(wm / 16 + (g16 & 1), t);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nb = wn / 32 + j;   // 32-column block: tap nb/2, channels 32*(nb&1) ..
#pragma unroll
        for (int t = 0; t < 2; ++t) boffs[j][t] = OB * (1 + (nb >> 1)) + tr_off(2 * (nb & 1) + (g16 & 1), t);
    }

    floatx16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const bool bias_wave = kh == bz % 3 && ci0 == 0 && wn == 0;
    float bsum = 0.f;

    if (nkt > 0) stage(0, s_begin);
    if (nkt > 1) stage(1, s_begin + 1);
    for (int t = 0; t < nkt; ++t) {
        if (t + 1 < nkt) vm_wait<2 * NP>();
        else vm_wait<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + 2 < nkt) stage((t + 2) % NS, s_begin + t + 2);
        const char* base = lds + (t % NS) * SB;
        bf16x8 af[NP], bfr[TN][NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            {
                const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + p * PI + aoffs[0]));
                const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + p * PI + aoffs[1]));
                const short8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                af[p] = __builtin_bit_cast(bf16x8, v);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + p * PI + boffs[j][0]));
                const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + p * PI + boffs[j][1]));
                const short8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                bfr[j][p] = __builtin_bit_cast(bf16x8, v);
            }
        }
        if (bias_wave) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int e = 0; e < 8; ++e) bsum += piece_elem<NP>(af[p], e);
        }
        floatx16 tmp[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) tmp[j] = mfma_split0<NP>(af, bfr[j]);
        __builtin_amdgcn_sched_barrier(0);   // chains first, adds after (see conv_psa_kernel)
#pragma unroll
        for (int j = 0; j < TN; ++j) drain(acc[j], tmp[j]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    float* sl = slab + (int64_t)bz * Cout * Nt;
    const int li = lane & 31, h = lane >> 5;
    float inv = 1.f, binv = 1.f;
    if constexpr (NP == 2) {
        binv = 1.f / *dscale;
        inv = binv / ubpl::FP16_ACT_SCALE;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nb = wn / 32 + j;
        const int n = (kh * 3 + (nb >> 1)) * Cin + ci0 + 32 * (nb & 1) + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
            sl[(int64_t)m * Nt + n] = acc[j][r] * inv;
        }
    }
    if (bias_wave) {
        const float v = bsum + __shfl_xor(bsum, 32, 64);
        if (h == 0) sl[(int64_t)(m0 + wm + li) * Nt + Ntot] = v * binv;
    }
}

// ------------------------------------------------------------------ 1x1 weight gradient, split on load
// dW[m][k] = sum over pixels n of dy[m][n] * v[k][n], v = relu(x*pscale + pshift)
// (PRO) or x; db[m] = sum dy[m][n].  GEMM: M = Cout, N = Cin, K = pixels, both
// operands pixel-contiguous in NCHW (no transposes).  K step = 16 pixels of one
// image (P % 16 == 0), split over workgroups into a slab [z][Cout][Cin + 1] (last
// column: the bias gradient, from the Cin-tile-0 workgroups) reduced by
// conv_reduce.hip's wgrad_reduce_kernel.  The f32 operands come global -> registers
// (two steps ahead), each element is split ONCE per workgroup by the thread
// that loaded it (thread t: row t/2 of both operands, pixels 8(t&1)..+7), and
// the pieces go to a double-buffered LDS image [operand][piece][128 rows][32 B]
// (chunk swizzle c ^ ((row >> 3) & 1), conflict-free ds_read_b128 fragments,
// conv_psa_kernel's layout).  Tile CM x CN (128 or 64 channels of dy / of x:
// the 64-channel convs of the first residual at 128x128), wave tile CM/2 x CN/2.
// With 64 rows an operand row is loaded by 4 threads (4 pixels each).
template <bool PRO, int NP = 3, int CM = 128, int CN = 128>
__global__ void __launch_bounds__(NT, 2) wgrad1_sol_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ pscale,
                                                          const float* __restrict__ pshift, int B, int Cin, int Cout,
                                                          int P, int steps_per_split, float* __restrict__ slab) {
    // NP = 3: 6xbf16; NP = 1: bf16 operands, f32 accumulation (the "bf16" precision)
    constexpr int TM = CM / 64, TN = CN / 64;
    constexpr int PIA = CM * 32, PIB = CN * 32;   // one piece image: rows x 16 pixels x 2 B
    constexpr int OA = NP * PIA;                  // dy pieces, then x pieces
    constexpr int SB = OA + NP * PIB;             // one stage
    constexpr int TPA = NT / CM, TPB = NT / CN;   // loader threads per row
    constexpr int PPA = 16 / TPA, PPB = 16 / TPB; // pixels per loader thread (8 or 4)
    constexpr int FA = PPA / 4, FB = PPB / 4;     // float4s per loader thread
    __shared__ __attribute__((aligned(16))) char lds[2 * SB];

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: SGPR)
    const int wm = (wid >> 1) * (CM / 2), wn = (wid & 1) * (CN / 2);
    const int lam = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                              gridDim.x * gridDim.y * gridDim.z);
    const int bx = lam % gridDim.x, by = (lam / gridDim.x) % gridDim.y, bz = lam / (gridDim.x * gridDim.y);
    const int m0 = by * CM, c0 = bx * CN;
    const int psteps = P >> 4;
    const int total = B * psteps;
    const int s_begin = bz * steps_per_split;
    const int s_end = min(total, s_begin + steps_per_split);
    const int nkt = max(0, s_end - s_begin);

    // loader / splitter: dy row ra, pixels PPA*qa .. +PPA-1 of the step; x row rb likewise
    const int ra = tid / TPA, qa = tid % TPA, rb = tid / TPB, qb = tid % TPB;
    const float* arow = dy + (int64_t)(m0 + ra) * P + PPA * qa;
    const float* brow = x + (int64_t)(c0 + rb) * P + PPB * qb;
    float sc = 1.f, sh = 0.f;
    if (PRO) {
        sc = pscale[c0 + rb];
        sh = pshift[c0 + rb];
    }
    // 16-B chunk (pixels 8c .. 8c+7) swizzled by row, then the 8-B half for 4-pixel loaders
    const int wofa = ra * 32 + 16 * (((PPA * qa) >> 3) ^ ((ra >> 3) & 1)) + 2 * ((PPA * qa) & 7);
    const int wofb = rb * 32 + 16 * (((PPB * qb) >> 3) ^ ((rb >> 3) & 1)) + 2 * ((PPB * qb) & 7);
    auto gload = [&](float4 (&a)[FA], float4 (&b)[FB], int s) {
        const int bb = s / psteps;
        const int p0 = (s - bb * psteps) * 16;
        const float4* a4 = reinterpret_cast<const float4*>(arow + (int64_t)bb * Cout * P + p0);
        const float4* b4 = reinterpret_cast<const float4*>(brow + (int64_t)bb * Cin * P + p0);
#pragma unroll
        for (int f = 0; f < FA; ++f) a[f] = a4[f];
#pragma unroll
        for (int f = 0; f < FB; ++f) b[f] = b4[f];
    };
    float bsum = 0.f;
    auto split_store = [&](int buf, const float4 (&a)[FA], const float4 (&b)[FB]) {
        float va[PPA], vb[PPB];
#pragma unroll
        for (int f = 0; f < FA; ++f) {
            va[4 * f] = a[f].x, va[4 * f + 1] = a[f].y, va[4 * f + 2] = a[f].z, va[4 * f + 3] = a[f].w;
        }
#pragma unroll
        for (int f = 0; f < FB; ++f) {
            vb[4 * f] = b[f].x, vb[4 * f + 1] = b[f].y, vb[4 * f + 2] = b[f].z, vb[4 * f + 3] = b[f].w;
        }
        if constexpr (PPA == 8)
            bsum += ((va[0] + va[1]) + (va[2] + va[3])) + ((va[4] + va[5]) + (va[6] + va[7]));
        else
            bsum += (va[0] + va[1]) + (va[2] + va[3]);
        if (PRO) {
#pragma unroll
            for (int e = 0; e < PPB; ++e) vb[e] = fmaxf(fmaf(vb[e], sc, sh), 0.f);
        }
        uint32_t pa[NP][PPA / 2], pb[NP][PPB / 2];
#pragma unroll
        for (int e = 0; e < PPA / 2; ++e) {
            uint32_t o[NP];
            split2<NP>(va[2 * e], va[2 * e + 1], o);
#pragma unroll
            for (int p = 0; p < NP; ++p) pa[p][e] = o[p];
        }
#pragma unroll
        for (int e = 0; e < PPB / 2; ++e) {
            uint32_t o[NP];
            split2<NP>(vb[2 * e], vb[2 * e + 1], o);
#pragma unroll
            for (int p = 0; p < NP; ++p) pb[p][e] = o[p];
        }
        char* base = lds + buf * SB;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if constexpr (PPA == 8)
                *reinterpret_cast<uint4*>(base + p * PIA + wofa) = make_uint4(pa[p][0], pa[p][1], pa[p][2], pa[p][3]);
            else
                *reinterpret_cast<uint2*>(base + p * PIA + wofa) = make_uint2(pa[p][0], pa[p][1]);
            if constexpr (PPB == 8)
                *reinterpret_cast<uint4*>(base + OA + p * PIB + wofb) =
                    make_uint4(pb[p][0], pb[p][1], pb[p][2], pb[p][3]);
            else
                *reinterpret_cast<uint2*>(base + OA + p * PIB + wofb) = make_uint2(pb[p][0], pb[p][1]);
        }
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    const int li = lane & 31, h = lane >> 5;

    float4 cA[FA], cB[FB], nA[FA], nB[FB];
    if (nkt > 0) gload(cA, cB, s_begin);
    if (nkt > 1) gload(nA, nB, s_begin + 1);
    for (int t = 0; t < nkt; ++t) {
        // buffer t&1 was last read in step t-2, before every wave's step t-1 barrier
        split_store(t & 1, cA, cB);
#pragma unroll
        for (int f = 0; f < FA; ++f) cA[f] = nA[f];
#pragma unroll
        for (int f = 0; f < FB; ++f) cB[f] = nB[f];
        if (t + 2 < nkt) gload(nA, nB, s_begin + t + 2);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const char* base = lds + (t & 1) * SB;
        bf16x8 af[TM][NP], bfr[TN][NP];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = wm + 32 * i + li;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                af[i][p] = *reinterpret_cast<const bf16x8*>(base + p * PIA + row * 32 + 16 * (h ^ ((row >> 3) & 1)));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int row = wn + 32 * j + li;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                bfr[j][p] =
                    *reinterpret_cast<const bf16x8*>(base + OA + p * PIB + row * 32 + 16 * (h ^ ((row >> 3) & 1)));
        }
        if constexpr (NP == 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) mfma_split<NP>(acc[i][j], af[i], bfr[j]);
        } else {
            floatx16 tmp[TM][TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    tmp[i][j] = mfma_split0<NP>(af[i], bfr[j]);
                }
            __builtin_amdgcn_sched_barrier(0);   // chains first, adds after (see conv_psa_kernel)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) drain(acc[i][j], tmp[i][j]);
        }
    }

    const int Nt = Cin + 1;
    float* sl = slab + (int64_t)bz * Cout * Nt;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = c0 + wn + 32 * j + li;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = m0 + wm + 32 * i + (q & 3) + 8 * (q >> 2) + 4 * h;
                sl[(int64_t)m * Nt + n] = acc[i][j][q];
            }
    }
    // bias gradient: the TPA threads of a row (adjacent lanes) hold its pixel chunks
    float bt = bsum + __shfl_xor(bsum, 1, 64);
    if constexpr (TPA == 4) bt += __shfl_xor(bt, 2, 64);
    if (bx == 0 && qa == 0) sl[(int64_t)(m0 + ra) * Nt + Cin] = bt;
}

using namespace ubpl;

// split-K of a weight gradient: `wgs` workgroups over `tiles` output tiles (whole rounds of
// the CUs, not one over), >= 8 K steps per split
int wgrad_splits(int wgs, int tiles, int steps) {
    int s = wgs / tiles;
    if (s < 1) s = 1;
    if (s > steps / 8) s = steps / 8 > 0 ? steps / 8 : 1;
    const int per = (steps + s - 1) / s;
    return (steps + per - 1) / per;
}

// ---- 3x3
int wgrad3_cb(int Cin, int Cout) { return (Cin % 128 == 0 && Cout % 128 == 0) ? 128 : 64; }

int wgrad3_splits(int B, int Cin, int Cout, int H, int W) {
    const int cb = wgrad3_cb(Cin, Cout);
    // 128: one tap x 128 channels per n-tile; 64: one kernel row (3 taps) x 64 channels
    const int tiles = cb == 128 ? 9 * (Cin / cb) * (Cout / cb) : 3 * (Cin / 64) * (Cout / 64);
    return wgrad_splits(knobs().wgrad3_wgs, tiles, B * H * (W / 16));
}

// ---- 1x1
int wgrad1_cb(int C) { return C % 128 == 0 ? 128 : 64; }

bool wgrad1_sol_supported(int B, int Cin, int Cout, int P) {
    return B > 0 && Cin % 64 == 0 && Cout % 64 == 0 && P % 16 == 0 && P > 0 &&
           (int64_t)B * Cin * P < (1LL << 31) && (int64_t)B * Cout * P < (1LL << 31);
}

int wgrad1_sol_splits(int B, int Cin, int Cout, int P) {
    const int tiles = (Cin / wgrad1_cb(Cin)) * (Cout / wgrad1_cb(Cout));
    return wgrad_splits(knobs().wgrad1_wgs, tiles, B * (P / 16));
}

}  // namespace

UBPL_API int64_t ubpl_wgrad3_psa_workspace(int B, int Cin, int Cout, int H, int W) {
    if (Cin % 64 || Cout % 64 || W % 16) return 0;
    return (int64_t)wgrad3_splits(B, Cin, Cout, H, W) * Cout * (9 * Cin + 1);
}

// dw[Cout,Cin,3,3] (+)= 3x3 weight gradient, db[Cout] (+)= sum dy (nullable), from
// PSA operands with a 1-pixel border: dys = split(dy) [B][Cout/16][H+2][W+2][16],
// xs = split(conv input) [B][Cin/16][H+2][W+2][16], npieces = 3.  Needs
// Cin % 64 == 0, Cout % 64 == 0 (128-channel tiles when both are multiples of 128), W % 16 == 0.
// slab: ubpl_wgrad3_psa_workspace floats.
UBPL_API int ubpl_wgrad3_psa(const uint16_t* dys, int64_t dplane, const uint16_t* xs, int64_t xplane, int B, int Cin,
                             int Cout, int H, int W, float* slab, float* dw, float* db, int accumulate, int npieces,
                             const float* dscale, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (Cin % 64 || Cout % 64 || W % 16 || npieces < 1 || npieces > 3 || slab == nullptr ||
        (npieces == 2) != (dscale != nullptr))
        return (int)hipErrorInvalidValue;
    if ((((uintptr_t)dys) & 15) || (((uintptr_t)xs) & 15) || (dplane % 8) || (xplane % 8)) return (int)hipErrorInvalidValue;
    const int splits = wgrad3_splits(B, Cin, Cout, H, W);
    const int steps = B * H * (W / 16);
    const int per = (steps + splits - 1) / splits;
    const int cb = wgrad3_cb(Cin, Cout);
    const int e = pick([&](auto np) {
        if (cb == 128)
            hipLaunchKernelGGL((wgrad3_psa_kernel<np, 128>),
                               dim3((unsigned)(9 * (Cin / 128)), (unsigned)(Cout / 128), (unsigned)splits), dim3(NT),
                               0, st, dys, dplane, xs, xplane, B, Cin, Cout, H, W, per, slab, dscale);
        else
            hipLaunchKernelGGL((wgrad3_psa64_kernel<np>),
                               dim3((unsigned)(3 * (Cin / 64)), (unsigned)(Cout / 64), (unsigned)splits), dim3(NT), 0,
                               st, dys, dplane, xs, xplane, B, Cin, Cout, H, W, per, slab, dscale);
        UBPL_LAUNCH_CHECK();
        return 0;
    }, among<1, 2, 3>{npieces});
    if (e) return e;
    return ubpl_wgrad_slab_reduce(slab, splits, Cout, Cin, 9, db != nullptr, dw, db, accumulate, stream);
}

// Floats of slab ubpl_wgrad1x1_split_load needs; 0 = shape not supported
// (Cin % 64, Cout % 64, P % 16): use ubpl_conv2d_wgrad.
UBPL_API int64_t ubpl_wgrad1x1_split_load_workspace(int B, int Cin, int Cout, int P) {
    if (!wgrad1_sol_supported(B, Cin, Cout, P)) return 0;
    return (int64_t)wgrad1_sol_splits(B, Cin, Cout, P) * Cout * (Cin + 1);
}

// dw[Cout,Cin,1,1] (+)= 1x1 weight gradient, db[Cout] (+)= sum dy (nullable),
// on the 6xbf16 path with both f32 operands split while they are staged
// (wgrad1_sol_kernel): dy [B,Cout,P], x [B,Cin,P], v = relu(x*pscale + pshift)
// when pscale != nullptr.  16-B aligned dy / x.
UBPL_API int ubpl_wgrad1x1_split_load(const float* dy, const float* x, int B, int Cin, int Cout, int P,
                                      const float* pscale, const float* pshift, float* slab, float* dw, float* db,
                                      int accumulate, int npieces, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!wgrad1_sol_supported(B, Cin, Cout, P) || slab == nullptr || (((uintptr_t)dy) & 15) ||
        (((uintptr_t)x) & 15) || (npieces != 1 && npieces != 3))
        return (int)hipErrorInvalidValue;
    const int splits = wgrad1_sol_splits(B, Cin, Cout, P);
    const int steps = B * (P / 16);
    const int per = (steps + splits - 1) / splits;
    // wgrad1_sol_kernel<PRO, NP, CM, CN>: 128-channel tiles along each side that 128 divides
    const int cm = wgrad1_cb(Cout), cn = wgrad1_cb(Cin);
    dim3 grid((unsigned)(Cin / cn), (unsigned)(Cout / cm), (unsigned)splits);
    const int e = pick(
        [&](auto PRO, auto NP, auto CM, auto CN) {
            hipLaunchKernelGGL((wgrad1_sol_kernel<PRO != 0, NP, CM, CN>), grid, dim3(NT), 0, st, dy, x, pscale, pshift,
                               B, Cin, Cout, P, per, slab);
            UBPL_LAUNCH_CHECK();
            return 0;
        },
        among<0, 1>{pscale != nullptr}, among<1, 3>{npieces}, among<128, 64>{cm}, among<128, 64>{cn});
    if (e) return e;
    return ubpl_wgrad_slab_reduce(slab, splits, Cout, Cin, 1, db != nullptr, dw, db, accumulate, stream);
}
