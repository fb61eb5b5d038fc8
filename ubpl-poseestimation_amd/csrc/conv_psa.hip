// Convolutions over pre-split activations ("PSA") on the split paths (2xfp16, 6xbf16, bf16):
// the activation split (split_act_kernel), the LDS-DMA forward / data-gradient kernel
// (conv_psa_kernel), its split-K reduce, and ubpl_conv2d_forward_psa, which also chooses
// the 3x3 input-halo kernel of conv_psah.hip.  Shared pieces: split_common.h.
#include "split_common.h"

namespace {

// ------------------------------------------------------------------ pre-split activations
// PSA layout: NP bf16 planes (`plane` elements apart) of [B][C/16][Hp][Wp][16],
// Hp = H + 2*pad, Wp = W + 2*pad, the border zero: a pixel's 16 channels of one
// group are 32 contiguous bytes = the two 16-B chunks of one B-operand row of
// a K step, and a 3x3 tap is a constant offset (no bounds checks in the conv).
// v = relu(x*scale + shift) (PRO) or x, then split; the border stays 0 (the
// reference pads the BN+ReLU output: models/base/layers.py:45-50).
// NP = 2 (2xfp16): the pieces of v * asc.  DUAL: also the 3-piece 6xbf16 image of v into dst3
// (the 2xfp16 forward's conv input, kept for the 6xbf16 weight gradient: one read, two images).
template <int NP, bool PRO, bool DUAL = false>
__global__ void __launch_bounds__(256) split_act_kernel(const float* __restrict__ x, int C, int H, int W,
                                                       const float* __restrict__ pscale,
                                                       const float* __restrict__ pshift, int pad,
                                                       uint16_t* __restrict__ dst, int64_t plane, float asc,
                                                       uint16_t* __restrict__ dst3, int64_t plane3) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad, G = C >> 4;
    const int b = blockIdx.z, g = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= Hp * Wp) return;
    const int hp = pix / Wp, wq = pix - hp * Wp;
    const int h = hp - pad, w = wq - pad;
    const bool in = h >= 0 && h < H && w >= 0 && w < W;
    const int64_t HW = (int64_t)H * W;
    const float* src = x + ((int64_t)b * C + 16 * g) * HW + (in ? h * W + w : 0);
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = src[j * HW];
    if (PRO) {
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = fmaxf(fmaf(v[j], pscale[16 * g + j], pshift[16 * g + j]), 0.f);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = in ? v[j] : 0.f;
    const int64_t o = (((int64_t)(b * G + g) * Hp + hp) * Wp + wq) * 16;
    ubpl::store_psa_row<NP>(v, dst + o, plane, NP == 2 ? asc : 1.f);
    if constexpr (DUAL) ubpl::store_psa_row<3>(v, dst3 + o, plane3);
}

// Forward conv (stride 1) over PSA activations and split weights, both staged
// global -> LDS by LDS-DMA (global_load_lds_dwordx4: no staging registers, no
// VALU), BK = 16 = one (channel group, tap) per K step.  LDS stage image:
// [piece][row][2 x 16 B] for A (BM rows) then B (128 rows); a DMA instruction
// fills 32 rows lane-linearly (lane L: row L>>1, slot L&1), so the chunk
// swizzle c ^ ((row >> 3) & 1) (conflict-free ds_read_b128 of a 32-row
// fragment) is applied on the SOURCE address and again on the read.  Wave w
// moves rows 32w..32w+31 of both operands.  3-stage ring: stage t+2 is issued
// right after the barrier that retires stage t (each wave's counted vmcnt
// leaves stage t+1's DMA in flight; raw s_barrier, never __syncthreads, whose
// fence would drain it: cdna_hip_programming.md §5 'Pipelining across barriers').
// EPI: the opt-in BatchNorm-partials epilogues (UBPL_FWD_EPI / UBPL_BWD_EPI)
// are compiled in; without them the kernel needs no scratch (the epilogue's
// register pressure spilled ~190 VGPRs to scratch in every launch).
// KSUB: 16-k steps per stage and barrier (1; 2-4 on the one-piece bf16 path,
// whose single MFMA per tile per 16-k step left the loop bound by the ring's
// barriers and waits: KSUB steps of MFMAs between two barriers)
template <int BM, int KS, int NP, int BNT = 128, int WGM = 2, bool EPI = false, int KSUB = 1>
__global__ void __launch_bounds__(NT, 2) conv_psa_kernel(const uint16_t* __restrict__ xs, int64_t xplane,
                                                        const uint16_t* __restrict__ wp, int64_t wplane,
                                                        const float* __restrict__ bias, const float* res, float* y,
                                                        int B, int Cin, int H, int W, int pad, int Cout, int kchunk,
                                                        float* __restrict__ slab, float* __restrict__ stat_part,
                                                        ubpl::BnBwdEpi bwd, float osc,
                                                        const float* __restrict__ ascp) {
    // osc: the accumulators' scale (2xfp16: weight scale x activation scale, the latter
    // read from *ascp when the image's scale lives on the device — a data gradient's,
    // bn_bwd.hip fp16_scale_for; 1 on the other paths)
    if (ascp != nullptr) osc *= *ascp;
    constexpr int PADK = KS / 2;   // odd KS: centred; even KS (the stem, 4x4): taps -KS/2 .. KS/2 - 1
    constexpr int T = KS * KS;
    // waves: WGM along the output channels x 4/WGM along the pixels (64-row
    // tiles on 256 pixels: 1 x 4, wave tile 64 x 64)
    constexpr int WGN = 4 / WGM;
    constexpr int TM = BM / WGM / 32, TN = BNT / WGN / 32;
    constexpr int AB = NP * BM * 32, BB = NP * BNT * 32;   // bytes per stage
    // 128-pixel tiles: 3-stage ring; 256-pixel tiles (wave tile 64 x 128, twice
    // the MFMAs per barrier and per fragment byte): 2 stages, 2 workgroups per CU
    constexpr int NS = BNT == 256 ? 2 : 3;
    constexpr int BQ = BNT / 128;                          // B DMA instructions per wave per piece
    constexpr int SB = AB + BB;                            // one 16-k step's image
    __shared__ __attribute__((aligned(16))) char lds[NS * KSUB * SB];

    const int P = H * W, Hp = H + 2 * pad, Wp = W + 2 * pad, G = Cin >> 4;
    const int64_t N = (int64_t)B * P;
    const int Ktot = Cin * T;
    // (wid wave-uniform in an SGPR: the DMA index math stays scalar)
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int dw = wid;                                    // the wave's share of the DMA pieces
    const int wm = (wid / WGN) * (BM / WGM), wn = (wid % WGN) * (BNT / WGN);
    const int lam = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                              gridDim.x * gridDim.y * gridDim.z);
    const int by = lam % gridDim.y, bx = (lam / gridDim.y) % gridDim.x, bz = lam / (gridDim.y * gridDim.x);
    const int m0 = by * BM;
    const int64_t n0 = (int64_t)bx * BNT;
    const int k_begin = bz * kchunk;
    const int k_end = min(Ktot, k_begin + kchunk);

    // DMA lane geometry
    const int lr = lane >> 1;
    const int lchunk = (lane & 1) ^ ((lr >> 3) & 1);
    const bool a_issue = BM / 32 >= NT / 64 || dw < BM / 32;   // every wave when BM >= 128
    // per-lane 32-bit byte offsets over wave-uniform bases (scalar + vector
    // addressing: no 64-bit VALU per DMA instruction)
    const uint32_t a_lane = (uint32_t)(((int64_t)min(m0 + 32 * dw + lr, Cout - 1) * Ktot + 8 * lchunk) * 2);
    uint32_t b_lane[BQ];   // wave w moves pixel rows 32*(BQ*w + q) .. +31
#pragma unroll
    for (int q = 0; q < BQ; ++q) {
        int64_t n = n0 + 32 * (BQ * dw + q) + lr;
        n = n < N ? n : N - 1;
        const int b = (int)(n / P);
        const int p = (int)(n - (int64_t)b * P);
        const int oh = p / W, ow = p - oh * W;
        b_lane[q] =
            (uint32_t)(((((int64_t)b * G * Hp + oh + pad - PADK) * Wp + ow + pad - PADK) * 16 + 8 * lchunk) * 2);
    }
    // DMA piece d (0 .. NP*(1+BQ)-1) of stage (buf, kt): d = p*(1+BQ) + 0 -> A piece p,
    // d = p*(1+BQ) + 1 + q -> B piece p, row block q
    constexpr int NDMA = NP * (1 + BQ);
    // buf: the 16-k step's image slot (stage * KSUB + sub-step)
    auto stage_piece = [&](int buf, int kt, int d) {
        const int kg = kt >> 4;
        const int tap = kg % T, cg = kg / T;
        const int kh = tap / KS, kw = tap - kh * KS;
        const int64_t boff = ((int64_t)cg * Hp + kh) * Wp * 16 + kw * 16;
        char* base = lds + buf * SB;
        const int p = d / (1 + BQ), r = d % (1 + BQ);
        if (r == 0) {
            const char* ab = reinterpret_cast<const char*>(wp + p * wplane + kt);
            if (a_issue)
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)(ab + a_lane),
                                                 (lds_ptr_t)(base + p * BM * 32 + dw * 1024), 16, 0, 0);
        } else {
            const int q = r - 1;
            const char* bb = reinterpret_cast<const char*>(xs + p * xplane + boff);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(bb + b_lane[q]),
                                             (lds_ptr_t)(base + AB + p * BNT * 32 + (BQ * dw + q) * 1024), 16, 0,
                                             0);
        }
    };
    // stage sb: its KSUB 16-k steps (those before k_end)
    auto stage = [&](int buf, int sb) {
#pragma unroll
        for (int u = 0; u < KSUB; ++u) {
            const int kt = k_begin + (sb * KSUB + u) * 16;
            if (KSUB == 1 || kt < k_end) {
#pragma unroll
                for (int d = 0; d < NDMA; ++d) stage_piece(buf * KSUB + u, kt, d);
            }
        }
    };

    const int nk16 = (k_end - k_begin) >> 4;               // 16-k steps
    const int nkt = (nk16 + KSUB - 1) / KSUB;              // stages

    // accumulators start at bias (+ residual): see conv_f32_fwd.hip conv_fwd_kernel
    const int li = lane & 31, h = lane >> 5;
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
    ubpl::seed_acc<TM, TN, true>(acc, direct ? bias : nullptr, direct ? res : nullptr, obase, m0 + wm, Cout, P, osc);
    const float inv = 1.f / osc;

    if (nkt > 0) stage(0, 0);
    if (NS == 3 && nkt > 1) stage(1, 1);
    for (int t = 0; t < nkt; ++t) {
        // retire stage t (this wave's DMA), then the barrier: every wave's
        // stage t has landed and every wave is done reading stage t-1
        if (NS == 3 && t + 1 < nkt && (KSUB == 1 || (t + 2) * KSUB <= nk16)) {
            if (a_issue) vm_wait<KSUB * (NP + BQ * NP)>();
            else vm_wait<KSUB * BQ * NP>();
        } else {
            vm_wait<0>();
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + NS - 1 < nkt) stage((t + NS - 1) % NS, t + NS - 1);
#pragma unroll
        for (int u = 0; u < KSUB; ++u) {
        if (KSUB > 1 && (t * KSUB + u) >= nk16) break;
        const int cur = t % NS;
        const char* base = lds + (cur * KSUB + u) * SB;
        bf16x8 af[TM][NP], bfr[TN][NP];
        auto read_b = [&](int j) {
            const int row = wn + 32 * j + li;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                bfr[j][p] = *reinterpret_cast<const bf16x8*>(base + AB + p * BNT * 32 + row * 32 +
                                                            16 * (h ^ ((row >> 3) & 1)));
            }
        };
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = wm + 32 * i + li;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                af[i][p] = *reinterpret_cast<const bf16x8*>(base + p * BM * 32 + row * 32 + 16 * (h ^ ((row >> 3) & 1)));
            }
        }
        if constexpr (NP >= 2 && TN > 2) {
            // ping-pong chunks: tile q's 6-MFMA chain is issued with tile q-1's
            // 16 drain adds between its MFMAs (3 VALU slots per MFMA gap), so the
            // adds hide in the matrix pipe's gaps instead of trailing each chain
#pragma unroll
            for (int j = 0; j < TN / 2; ++j) read_b(j);
            __builtin_amdgcn_sched_barrier(0);
            floatx16 prev = mfma_split0<NP>(af[0], bfr[0]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = TN / 2; j < TN; ++j) read_b(j);
#pragma unroll
            for (int q = 1; q < TM * TN; ++q) {
                const int j = q / TM, i = q % TM, pj = (q - 1) / TM, pi = (q - 1) % TM;
                const floatx16 cur = mfma_split0<NP>(af[i], bfr[j]);
                drain(acc[pi][pj], prev);
                pp_schedule<NP>();
                prev = cur;
            }
            drain(acc[TM - 1][TN - 1], prev);
        } else if constexpr (NP >= 2) {
#pragma unroll
            for (int j = 0; j < TN; ++j) read_b(j);
            // every tile's chunk chain first, the f32 adds after them (behind a
            // scheduling barrier): an add right behind its own chain waits out
            // the MFMA latency (s_nop) with the other tiles' chains not issued
            floatx16 tmp[TM][TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    tmp[i][j] = mfma_split0<NP>(af[i], bfr[j]);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) drain(acc[i][j], tmp[i][j]);
        } else {
#pragma unroll
            for (int j = 0; j < TN; ++j) read_b(j);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) mfma_split<NP>(acc[i][j], af[i], bfr[j]);
        }
        }   // sub-steps
        // fragments consumed (the MFMAs waited on them) before the next barrier
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
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
                    if (m < Cout) sl[(int64_t)m * N + n] = acc[i][j][r] * inv;
                }
        }
        return;
    }
    if (EPI && stat_part) ubpl::tile_bn_partials<TM, TN>(acc, nok, m0 + wm, Cout, n0 + wn, N, stat_part);
    if (EPI && bwd.part) ubpl::tile_bn_bwd_partials<TM, TN>(acc, nok, obase, m0 + wm, Cout, P, n0 + wn, N, bwd);
    store_tile<TM, TN>(acc, nok, obase, m0 + wm, Cout, P, y, m0 + BM <= Cout && n0 + BNT <= N, inv);
}

using namespace ubpl;

// occupancy of conv_psa_kernel for the plan's cost model
const TileOcc& psa_occ() {
    static const TileOcc d = query_tile_occ({{2, 2}, {3, 2}}, (const void*)conv_psa_kernel<128, 3, 2>,
                                            (const void*)conv_psa_kernel<128, 3, 3>,
                                            (const void*)conv_psa_kernel<64, 3, 2>,
                                            (const void*)conv_psa_kernel<64, 3, 3>, NT);
    return d;
}

Plan psa_plan(int B, int Cin, int Cout, int KS, int H, int W, int npieces) {
    return fwd_plan(Cout, (int64_t)B * H * W, Cin * KS * KS, npieces, 16, psa_occ());
}

// The conv_psa_kernel instantiations that are built: KSUB > 1 on the one-piece 256-pixel
// tiles only; the 4x4 stem on 64 x 256 tiles, never 2xfp16; no 1x1 on 64 x 256 split pieces.
constexpr bool psa_built(int BM, int KS, int NP, int BNT, int KSUB) {
    if (KSUB != 1 && !(NP == 1 && BNT == 256 && KS != 4)) return false;
    if (KS == 4) return BM == 64 && BNT == 256 && NP != 2;
    if (BM == 64 && BNT == 256 && KS == 1) return NP == 1;
    return true;
}

template <int BM, int KS, int NP, int BNT, int KSUB>
int launch_psa(const PsaChoice& c, const PsaArgs& a) {
    constexpr int WGM = BM == 64 && BNT == 256 ? 1 : 2;   // 64 x 256: 1 x 4 waves, wave tile 64 x 64
    const int P = a.H * a.W;
    const int64_t N = (int64_t)a.B * P;
    const Plan& pl = a.pl;
    const bool split = pl.splits > 1;
    const BnBwdEpi off{nullptr, nullptr, 0, nullptr};
    if constexpr (NP != 2) {   // (epilogue partials: not on the scaled 2xfp16 accumulators)
        if (!split && (a.stat_part || a.bwd.part)) {
            hipLaunchKernelGGL((conv_psa_kernel<BM, KS, NP, BNT, WGM, true, KSUB>), c.grid, dim3(NT), 0, a.st, a.xs,
                               a.xplane, a.wp, a.wplane, a.bias, a.res, a.y, a.B, a.Cin, a.H, a.W, a.pad, a.Cout,
                               pl.kchunk, nullptr, a.stat_part, a.bwd, a.osc, a.act_scale);
            UBPL_LAUNCH_CHECK();
            return 0;
        }
    }
    hipLaunchKernelGGL((conv_psa_kernel<BM, KS, NP, BNT, WGM, false, KSUB>), c.grid, dim3(NT), 0, a.st, a.xs,
                       a.xplane, a.wp, a.wplane, a.bias, split ? nullptr : a.res, a.y, a.B, a.Cin, a.H, a.W, a.pad,
                       a.Cout, pl.kchunk, split ? a.slab : nullptr, nullptr, off, a.osc, a.act_scale);
    UBPL_LAUNCH_CHECK();
    if (split) {
        launch_split_reduce(a.slab, pl.splits, a.Cout, P, N, a.bias, a.res, a.y, a.st);
        UBPL_LAUNCH_CHECK();
        if (a.stat_part) {
            const int e = ubpl_bn_partials(a.y, a.B, a.Cout, P, a.stat_part, a.st);
            if (e) return e;
        }
        if (a.bwd.part)
            return ubpl_bn_backward_partials(a.y, a.bwd.x, a.B, a.Cout, P, a.bwd.coef, a.bwd.coef + a.Cout,
                                             a.bwd.coef + 2 * a.Cout, a.bwd.relu, a.bwd.part, a.st);
    }
    return 0;
}

// Which kernel runs a launch, from (shape, npieces, plan, knobs, epilogue partials).
// Returns 0, or the error of a launch no kernel takes.
int psa_choose(const PsaArgs& a, PsaChoice& c) {
    Knobs& k = knobs();
    const Plan& pl = a.pl;
    const int KS = a.KS, npieces = a.npieces, H = a.H, W = a.W, Cout = a.Cout;
    const int64_t N = (int64_t)a.B * H * W;
    const int mt = (Cout + pl.bm - 1) / pl.bm;
    const bool partials = a.stat_part || a.bwd.part;
    c = PsaChoice{false, W, pl.bm, 1, 2, 128, 1, dim3()};
    auto psa_grid = [&] { return dim3((unsigned)((N + c.BNT - 1) / c.BNT), (unsigned)mt, (unsigned)pl.splits); };
    if (KS == 4) {   // the space-to-depth stem (ubpl_stem_s2d_split): 64-row tiles on 256 pixels
        if (pl.bm != 64 || pl.splits != 1 || (npieces != 3 && npieces != 1) || N % 256 != 0)
            return (int)hipErrorInvalidValue;
        c.BNT = 256;
        c.grid = psa_grid();
        return 0;
    }
    // 3x3 stride-1 pad-1 on the split / bf16 paths, 128- or 64-row tiles, whole-row 256-pixel
    // tiles: the input halo staged once per channel group (conv_psah_kernel).  Default
    // (measured, tools/psa_bench.py, profiles/r04_psa_diag.txt): the split paths (6xbf16, 2xfp16)
    // on the one-halo-buffer, two-workgroups-per-CU variant (6xbf16: 212 vs 221 us at 128 ch
    // 64x64, 750 vs 786 at 256 ch, 250 vs 295 at 64 ch 128x128, 69 vs 75 at 128 ch 32x32); the
    // bf16 path at W <= 64 (54.6 vs 59.4 us at 128 ch 64x64, 184 vs 206 at 256 ch, 22.0 vs 27.0
    // at 128 ch 32x32; 104 vs 87 at 128x128: not there).
    // halo dispatch (Knobs::psa_dispatch()): -1 default; 0: none (conv_psa_kernel); 1:
    // every eligible launch on the double-buffered halo (two teams where the grid fills the
    // chip); test-only through ubpl_set_psa_dispatch: 2: as 1, required (a 3x3 launch the
    // kernel cannot take is an error); 3: the one-buffer variant for every eligible split-piece
    // launch, required.  The tests compare the kernels in one process; the modes compute in
    // the same order, bit for bit.
    const Knobs::PsaDispatch pd = k.psa_dispatch();
    const int halo_mode = pd.halo;
    const bool split_np = npieces == 3 || npieces == 2;
    // (2xfp16 on double-buffered halos at two workgroups per CU — they fit 80 KB at W <= 64 —
    // measured slower than the one buffer: 122.4 vs 116.2 us, 426.5 vs 433.0 img/s, round 6)
    const bool one_buf = split_np && (halo_mode >= 3 || halo_mode < 0);
    // the 96-wide planes: 192-pixel tiles on 128 rows whatever the plan's row block (its
    // cost model is conv_psa_kernel's), the one-buffer variant only
    const bool w96 = W == 96 && Cout % 128 == 0 && H % 2 == 0 &&
                     ((split_np && one_buf) || (npieces == 1 && halo_mode > 0));   // (bf16: opt-in, slower)
    // unsplit 64-row 3x3 launches run on 256-pixel tiles with a 1 x 4 wave
    // layout (wave tile 64 x 64: +14-19 % on the 128x128 64-channel and the
    // 32x32 128-channel convs); UBPL_PSA_BM64W=0 keeps 64 x 128 tiles
    const bool bm64w = k.psa_bm64w;
    const bool halo_ok = KS == 3 && a.pad == 1 && pl.splits == 1 && !partials &&
                         (((pl.bm == 128 || bm64w) && (W == 32 || W == 64 || W == 128) && H % (256 / W) == 0) ||
                          w96);
    if ((halo_mode >= 2) && KS == 3 && !halo_ok) return (int)hipErrorInvalidValue;
    const bool halo = halo_mode < 0 ? ((npieces == 1 && W <= 64) || one_buf) : halo_mode != 0;
    if (halo && halo_ok) {
        c.halo = true;
        c.NHB = one_buf ? 1 : 2;   // one halo buffer, two workgroups per CU (split pieces), or double-buffered halos
        // two 4-wave teams per workgroup (512 pixels: one halo, one A ring for both,
        // two waves per SIMD) where the grid still fills the chip; UBPL_PSA_TEAMS=1 / 2
        const bool teams2 = !one_buf && (pd.teams > 0 ? pd.teams == 2 : (N / 512) * mt >= 256) && W <= 64 &&
                            H % (512 / W) == 0;
        if (teams2) {
            c.TEAMS = 2;
            c.grid = dim3((unsigned)(N / 512), (unsigned)mt);
        } else if (w96) {
            c.BM = 128;
            c.grid = dim3((unsigned)(N / 192), (unsigned)(Cout / 128));
        } else {
            c.grid = dim3((unsigned)(N / 256), (unsigned)mt);
        }
        return 0;
    }
    // conv_psa_kernel.  Unsplit launches run on 256-pixel tiles where they divide the pixels:
    // the 64-row ones (bm64w, above; 3x3, and the one-piece 1x1), and the 128-row ones
    // (+12 % on the 64x64-level 3x3 conv; tuning hook: UBPL_PSA_BN=128 keeps 128-pixel tiles
    // everywhere); the rest on 128-pixel tiles.
    const bool unsplit256 = pl.splits == 1 && N % 256 == 0;
    if (unsplit256 && ((bm64w && pl.bm == 64 && (KS == 3 || npieces == 1)) || (k.psa_bn256 && pl.bm == 128))) {
        c.BNT = 256;
        // the one-piece (bf16) path: KSUB 16-k steps per stage and barrier (UBPL_PSA_KSUB1 in 1..4)
        if (npieces == 1) c.KSUB = k.psa_ksub1;
    }
    c.grid = psa_grid();
    return 0;
}

int psa_launch(const PsaChoice& c, const PsaArgs& a) {
    if (c.halo) return launch_psah(c, a);
    return pick(
        [&](auto KS, auto NP, auto BM, auto BNT, auto KSUB) {
            if constexpr (psa_built(BM, KS, NP, BNT, KSUB)) return launch_psa<BM, KS, NP, BNT, KSUB>(c, a);
            return (int)hipErrorInvalidValue;
        },
        among<1, 3, 4>{a.KS}, among<1, 2, 3>{a.npieces}, among<128, 64>{c.BM}, among<128, 256>{c.BNT},
        among<1, 2, 3, 4>{c.KSUB});
}

}  // namespace

// Pre-split activations (PSA layout, see split_act_kernel): dst = npieces bf16
// planes `plane` elements apart of [B][C/16][H+2pad][W+2pad][16];
// v = relu(x*pscale + pshift) when pscale != nullptr, else x.  C % 16 == 0.
UBPL_API int ubpl_split_activation(const float* x, int B, int C, int H, int W, const float* pscale,
                                   const float* pshift, int pad, int npieces, uint16_t* dst, int64_t plane,
                                   uint16_t* dst3, int64_t plane3, void* stream) {
    if (C % 16 != 0 || npieces < 1 || npieces > 3 || pad < 0 || (plane % 8) != 0) return (int)hipErrorInvalidValue;
    if (dst3 != nullptr && (npieces != 2 || (plane3 % 8) != 0)) return (int)hipErrorInvalidValue;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    dim3 grid((unsigned)((Hp * Wp + 255) / 256), (unsigned)(C / 16), (unsigned)B);
    // npieces 1: the "bf16" precision, one piece = bf16(v); 2 with dst3: 2xfp16 (scaled) + the 6xbf16 image
    return pick(
        [&](auto NP, auto PRO, auto DUAL) {
            if constexpr (NP == 2 || !DUAL) {
                hipLaunchKernelGGL((split_act_kernel<NP, PRO != 0, DUAL != 0>), grid, dim3(256), 0, (hipStream_t)stream,
                                   x, C, H, W, pscale, pshift, pad, dst, plane, FP16_ACT_SCALE, dst3, plane3);
                UBPL_LAUNCH_CHECK();
                return 0;
            }
            return (int)hipErrorInvalidValue;
        },
        among<1, 2, 3>{npieces}, among<0, 1>{pscale != nullptr}, among<0, 1>{dst3 != nullptr});
}

UBPL_API int64_t ubpl_conv2d_forward_psa_workspace(int B, int Cin, int Cout, int KS, int H, int W, int npieces) {
    const Plan pl = psa_plan(B, Cin, Cout, KS, H, W, npieces);
    return pl.splits > 1 ? (int64_t)pl.splits * Cout * ((int64_t)B * H * W) : 0;
}

UBPL_API int ubpl_set_psa_dispatch(int halo_mode, int teams) {
    Knobs& k = knobs();
    if (halo_mode == -2 && teams == -2) {   // back to the environment's values (read again at the next launch)
        k.psa_halo.store(-2);
        k.psa_teams.store(-2);
        return 0;
    }
    if (halo_mode < -1 || halo_mode > 3 || teams < -1 || teams > 2) return (int)hipErrorInvalidValue;
    k.psa_dispatch();                     // the environment's values are read first, then replaced
    k.psa_halo.store(halo_mode);
    k.psa_teams.store(teams);
    return 0;
}

// y = conv(xs, w, stride 1, pad (KS-1)/2) + bias (+ res) with xs in the PSA
// layout (border pad >= (KS-1)/2) and w from ubpl_conv_weights_split (same
// npieces).  KS in {1, 3}, or 4 for the space-to-depth stem; Cin % 16 == 0; res may alias y.
UBPL_API int ubpl_conv2d_forward_psa(const uint16_t* xs, int64_t xplane, int B, int Cin, int H, int W, int pad,
                                     const uint16_t* wsplit, int64_t wplane, const float* bias, int Cout, int KS,
                                     const float* res, float* y, float* slab, int npieces, float* stat_part,
                                     const float* bn_x, const float* bn_coef, int bn_relu, float* bn_part,
                                     const float* act_scale, void* stream) {
    // validate
    if (Cin % 16 != 0 || npieces < 1 || npieces > 3 || pad < KS / 2 || (KS != 1 && KS != 3 && KS != 4))
        return (int)hipErrorInvalidValue;
    if ((((uintptr_t)wsplit) & 15) != 0 || (((uintptr_t)xs) & 15) != 0 || (wplane % 8) != 0 || (xplane % 8) != 0)
        return (int)hipErrorInvalidValue;
    // plan
    const Plan pl = psa_plan(B, Cin, Cout, KS, H, W, npieces);
    if (pl.splits > 1 && slab == nullptr) return (int)hipErrorInvalidValue;
    if (npieces == 2 && (stat_part || bn_part)) return (int)hipErrorInvalidValue;   // (6xbf16 / bf16 only)
    if (npieces != 2 && act_scale != nullptr) return (int)hipErrorInvalidValue;
    const PsaArgs a{xs, wsplit, xplane, wplane, bias, res, y, B, Cin, H, W, pad, Cout, KS, npieces, pl, slab,
                    stat_part, BnBwdEpi{bn_part ? bn_x : nullptr, bn_coef, bn_relu, bn_part},
                    psa_osc(npieces, Cin * KS * KS, act_scale != nullptr), act_scale, (hipStream_t)stream};
    // choose
    PsaChoice c;
    const int e = psa_choose(a, c);
    if (e) return e;
    // launch
    return psa_launch(c, a);
}
