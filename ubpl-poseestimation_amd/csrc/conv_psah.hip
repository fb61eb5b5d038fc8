// The 3x3 input-halo convolution over pre-split activations (conv_psah_kernel) and its
// launch.  ubpl_conv2d_forward_psa (conv_psa.hip) decides when it runs; the kernels build here,
// apart from conv_psa_kernel's.  Shared pieces: split_common.h.
#include "split_common.h"

namespace {

// ------------------------------------------------------------------ 3x3, input halo staged once per channel group
// The 3x3 stride-1 conv over PSA activations (pad 1: the PSA image's own zero
// border is the conv padding) with the B operand staged ONCE per 16-channel
// group instead of once per (group, tap): a workgroup's 256-pixel tile is
// R = 256 / W whole output rows of one image, whose 3x3 receptive field is
// PSA rows oh0 .. oh0 + R + 1 x all W + 2 columns — one contiguous
// (R + 2) (W + 2) x 32 B run per piece, copied by LDS-DMA as it lies.  The
// nine taps then read their B fragments from that halo image at a per-tap
// pixel offset (kh (W + 2) + kw).  conv_psa_kernel moves 9 x 256 pixels per
// group; this kernel (R + 2)(W + 2) (396 at W = 64: 5.8x fewer B bytes through
// the CU's L2 -> LDS path, 2.2x fewer bytes per K step in all, the weights
// included).  Weights: the A ring of conv_psa_kernel (3 stages, one per K step
// = (group, tap)); halo images double-buffered per group: the next group's
// halo is issued at the group's tap 0 and retired by tap 3 (counted vmcnt).
// One workgroup per CU (LDS 85-160 KB); BM 128: wave tile 64 x 128 (as
// conv_psa_kernel<128, 3, NP, 256, 2>), BM 64: 64 x 64 (4 waves along the
// pixels, as conv_psa_kernel<64, 3, NP, 256, 1>); the same ping-pong drains.
// Halo chunk swizzle as conv_psa_kernel's rows: pixel q's two 16-B halves
// swapped when (q >> 3) & 1 (applied on the DMA source and on the read).
// NHB = 1 (6xbf16, one team): ONE halo buffer and two workgroups per CU (<= 80 KB
// each): the next group's halo is loaded after every wave finished the group's last
// tap (a second barrier then), the partner workgroup's MFMAs covering that bubble.
// BNT1: pixels per team tile — 256, or 192 for the 96-wide planes (two rows; 128-row
// tiles only: wave tile 64 x 96, three 32-pixel fragments)
template <int WW, int NP, int BM, int TEAMS = 1, int NHB = 2, int BNT1 = 256>
__global__ void __launch_bounds__(NT * TEAMS, (NHB == 1 || (NP == 2 && TEAMS == 1)) ? 2 : 1) conv_psah_kernel(const uint16_t* __restrict__ xs, int64_t xplane,
                                                        const uint16_t* __restrict__ wp, int64_t wplane,
                                                        const float* __restrict__ bias, const float* res, float* y,
                                                        int B, int Cin, int H, int Cout, float osc,
                                                        const float* __restrict__ ascp) {
    if (ascp != nullptr) osc *= *ascp;   // (see conv_psa_kernel)
    constexpr int BNT = BNT1 * TEAMS, R = BNT / WW, W2 = WW + 2;
    static_assert(BNT1 == 256 || (BNT1 == 192 && BM == 128), "192-pixel tiles: 128 rows");
    constexpr int NW = 4 * TEAMS;              // waves (TEAMS 4-wave teams, one 256-pixel tile each)
    constexpr int HPX = (R + 2) * W2;          // halo pixels
    constexpr int HI = (HPX + 31) / 32;        // DMA instructions per piece (32 pixels each)
    constexpr int HB = HPX * 32;               // halo image bytes per piece (exact: the last chunk of a
                                               // piece starts at HPX - 32, rewriting pixels it overlaps)
    constexpr int HTOT = NP * HI;
    constexpr int NH = (HTOT + NW - 1) / NW;   // halo DMA instructions per wave (spares repeat the last one)
    constexpr int AB = NP * BM * 32;           // A bytes per K step
    constexpr int AI = AB / 1024;              // A DMA instructions per K step (1 KB each)
    constexpr int NAW = (AI + NW - 1) / NW;    // per wave (spares repeat the last one)
    // GS (the one-piece path): a stage is a whole channel group — its halo and the
    // nine taps' A images (one barrier per 9 K steps; 8 MFMAs per wave per K step
    // left the per-step ring bound by its barriers); NS_G slots.  Otherwise A per
    // K step in an NA-stage ring, halos double-buffered (NHB = 2) or one buffer
    // reloaded at each group boundary (NHB = 1).
    constexpr bool GS = NP == 1;
    constexpr int NS_G = 3 * (NP * HB + 9 * AB) <= 160 * 1024 ? 3 : 2;
    static_assert(NHB == 2 || (!GS && TEAMS == 1), "one halo buffer: split pieces, one team");
    // (one halo buffer: as many A stages, 2 .. UBPL_PSAH_NA_MAX, as fit two workgroups per CU)
    constexpr int NA1 = UBPL_PSAH_NA_MAX * AB + NP * HB <= 80 * 1024 ? UBPL_PSAH_NA_MAX
                        : (3 * AB + NP * HB <= 80 * 1024 ? 3 : 2);
    constexpr int NA = GS ? 9 * NS_G : (NHB == 1 ? NA1 : 3);   // A images
    constexpr int WGM = BM / 64, WGN = 4 / WGM;
    constexpr int TM = 2, TN = BNT1 / WGN / 32;
    static_assert(BM == 64 || BM == 128, "64- or 128-row tiles");
    constexpr int OFF_H = NA * AB, LDS_BYTES = OFF_H + (GS ? NS_G : NHB) * NP * HB;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(BNT % WW == 0 && WW % 32 == 0, "whole rows of 32-pixel fragments");
    __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];

    const int P = H * WW, Hp = H + 2, G = Cin >> 4;
    const int64_t N = (int64_t)B * P;
    const int Ktot = Cin * 9;
    // (wid wave-uniform in an SGPR: the DMA index math below stays scalar)
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = ((wid & 3) / WGN) * 64, wn = (wid >> 2) * BNT1 + ((wid & 3) % WGN) * (BNT1 / WGN);
    const int lam = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int by = lam % gridDim.y, bx = lam / gridDim.y;
    const int m0 = by * BM;
    const int64_t n0 = (int64_t)bx * BNT;
    const int tpi = H / R;                     // tiles per image
    const int b = bx / tpi, oh0 = (bx - b * tpi) * R;

    const int lr = lane >> 1;
    const int lchunk = (lane & 1) ^ ((lr >> 3) & 1);
    // A instruction i = u * NW + wid: piece i / (BM / 32), rows 32 (i % (BM / 32)) .. —
    // the row block depends on the wave only (NW % (BM / 32) == 0): one lane offset
    static_assert(NW % (BM / 32) == 0, "row block per wave");
    const uint32_t a_lane = (uint32_t)(((int64_t)min(m0 + 32 * (wid % (BM / 32)) + lr, Cout - 1) * Ktot +
                                        8 * lchunk) * 2);
    auto stage_a = [&](int slot, int s) {
        const char* base = reinterpret_cast<const char*>(wp + s * 16);
#pragma unroll
        for (int u = 0; u < NAW; ++u) {
            // (a spare repeats the last piece's instruction for the same row block: same bytes)
            const int i = u * NW + wid < AI ? u * NW + wid : (NP - 1) * (BM / 32) + wid % (BM / 32);
            const int p = i / (BM / 32), rb = i % (BM / 32);
            char* dst = lds + slot * AB + p * BM * 32 + rb * 1024;
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(base + (int64_t)p * wplane * 2 + a_lane),
                                             (lds_ptr_t)dst, 16, 0, 0);
        }
    };
    // halo of group cg: instruction i = wid * NH + u (piece i / HI, 32-pixel chunk i % HI)
    auto stage_h = [&](int buf, int cg) {
        const int64_t gpx = (((int64_t)b * G + cg) * Hp + oh0) * W2;   // first halo pixel (PSA pixel index)
        // (the lane terms made opaque here: otherwise the compiler keeps all NH per-lane
        // source offsets live across the K loop, ~20 VGPRs, and spills the tile)
        int lr = lane >> 1, lo = lane & 1;
        asm volatile("" : "+v"(lr), "+v"(lo));
#pragma unroll
        for (int u = 0; u < NH; ++u) {
            const int i = min(wid * NH + u, HTOT - 1);  // (a spare repeats the last: same bytes)
            const int p = i / HI, c0 = min((i - p * HI) * 32, HPX - 32);
            const int q = c0 + lr;
            const int ch = lo ^ ((q >> 3) & 1);
            const char* src = reinterpret_cast<const char*>(xs + p * xplane + (gpx + q) * 16) + ch * 16;
            char* dst = lds + OFF_H + (buf * NP + p) * HB + c0 * 32;
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)dst, 16, 0, 0);
        }
    };

    const int li = lane & 31, h = lane >> 5;
    // output offsets: computed for the seed and again for the stores (not live
    // across the K loop: register budget of the two-team variant)
    auto out_base = [&](int64_t (&obase)[TN], bool (&nok)[TN]) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t n = n0 + wn + 32 * j + li;
            nok[j] = n < N;
            const int64_t nc = nok[j] ? n : N - 1;
            const int bb = (int)(nc / P);
            const int pp = (int)(nc - (int64_t)bb * P);
            obase[j] = (int64_t)bb * Cout * P + pp;
        }
    };
    // halo pixel of tap (0, 0) for tile-local output pixel nt: row nt / WW, column nt % WW
    const int nt0 = wn + li;
    floatx16 acc[TM][TN];
    {
        int64_t obase[TN];
        bool nok[TN];
        out_base(obase, nok);
        ubpl::seed_acc<TM, TN, true>(acc, bias, res, obase, m0 + wm, Cout, P, osc);
    }

    // one K step (group cg's tap at pixel offset toff): fragments from the A image
    // at abase and the halo image at hbase
    auto step = [&](const char* abase, const char* hbase, int toff) {
        bf16x8 af[TM][NP], bfr[TN][NP];
        auto read_b = [&](int j) {
            const int nt = nt0 + 32 * j;
            const int q = nt + (nt / WW) * 2 + toff;
            const char* rp = hbase + q * 32 + 16 * (h ^ ((q >> 3) & 1));
#pragma unroll
            for (int p = 0; p < NP; ++p) bfr[j][p] = *reinterpret_cast<const bf16x8*>(rp + p * HB);
        };
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = wm + 32 * i + li;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                af[i][p] = *reinterpret_cast<const bf16x8*>(abase + p * BM * 32 + row * 32 + 16 * (h ^ ((row >> 3) & 1)));
        }
        if constexpr (NP == 1) {
            // one MFMA per tile, accumulated directly (conv_psa_kernel's one-piece path)
#pragma unroll
            for (int j = 0; j < TN; ++j) read_b(j);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) mfma_split<NP>(acc[i][j], af[i], bfr[j]);
        } else {
            // ping-pong chunks (conv_psa_kernel): tile q's chain with tile q-1's drain adds in its gaps
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
        }
    };

    if constexpr (GS) {
        // one stage per channel group (halo + the nine taps' A images), NS_G-slot
        // ring, one barrier per group
        auto stage_g = [&](int slot, int cg) {
            stage_h(slot, cg);
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) stage_a(slot * 9 + tp, cg * 9 + tp);
        };
        for (int c = 0; c < NS_G - 1 && c < G; ++c) stage_g(c, c);
        for (int cg = 0; cg < G; ++cg) {
            // group cg landed; (3 slots) group cg+1 may stay in flight
            if (NS_G == 3 && cg + 1 < G) vm_wait<NH + 9 * NAW>();
            else vm_wait<0>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (cg + NS_G - 1 < G) stage_g((cg + NS_G - 1) % NS_G, cg + NS_G - 1);
            const int slot = cg % NS_G;
            const char* hbase = lds + OFF_H + slot * NP * HB;
#pragma unroll 1
            for (int tp = 0; tp < 9; ++tp) {
                const int kh = tp / 3;
                step(lds + (slot * 9 + tp) * AB, hbase, kh * W2 + (tp - 3 * kh));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    } else {
        const int nk = G * 9;
        stage_h(0, 0);
        for (int a = 0; a < NA - 1 && a < nk; ++a) stage_a(a, a);
        for (int s = 0; s < nk; ++s) {
            const int cg = s / 9, tap = s - cg * 9;
            if (NHB == 1 && tap == 0 && cg > 0) {
                // every wave done with group cg - 1: reload the one halo buffer, wait for it
                vm_wait<(NA - 2) * NAW>();
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                stage_h(0, cg);
                vm_wait<0>();
            } else if (NHB == 1) {
                if (s + 1 < nk) vm_wait<(NA - 2) * NAW>();
                else vm_wait<0>();
            } else if (s + 1 < nk) {
                // A(s) and (tap 0) halo(cg) landed; the A images issued after A(s) (NA - 2
                // of them) and the next group's halo, when issued after A(s), may stay in flight
                if (tap >= 1 && tap <= NA - 1 && cg + 1 < G) vm_wait<(NA - 2) * NAW + NH>();
                else vm_wait<(NA - 2) * NAW>();
            } else {
                vm_wait<0>();
            }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (s + NA - 1 < nk) stage_a((s + NA - 1) % NA, s + NA - 1);
            if (NHB == 2 && tap == 0 && cg + 1 < G) stage_h((cg + 1) & 1, cg + 1);
            const int kh = tap / 3;
            step(lds + (s % NA) * AB, lds + OFF_H + (NHB == 2 ? (cg & 1) : 0) * NP * HB, kh * W2 + (tap - 3 * kh));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }

    int64_t obase[TN];
    bool nok[TN];
    out_base(obase, nok);
    store_tile<TM, TN>(acc, nok, obase, m0 + wm, Cout, P, y, m0 + BM <= Cout && n0 + BNT <= N, 1.f / osc);
}

// The instantiations that are built: two teams at W <= 64 on double-buffered halos; the
// 96-wide planes on 128 rows (one buffer for split pieces, two for the one-piece path);
// else one team, the one-buffer variant for split pieces only.
constexpr bool psah_built(int W, int NP, int BM, int TEAMS, int NHB) {
    if (TEAMS == 2) return W <= 64 && NHB == 2;
    if (W == 96) return BM == 128 && NHB == (NP == 1 ? 2 : 1);
    return NHB == 2 || NP != 1;
}

}  // namespace

int ubpl::launch_psah(const PsaChoice& c, const PsaArgs& a) {
    return pick(
        [&](auto W, auto NP, auto BM, auto TEAMS, auto NHB) {
            if constexpr (psah_built(W, NP, BM, TEAMS, NHB)) {
                hipLaunchKernelGGL((conv_psah_kernel<W, NP, BM, TEAMS, NHB, W == 96 ? 192 : 256>), c.grid,
                                   dim3(TEAMS * NT), 0, a.st, a.xs, a.xplane, a.wp, a.wplane, a.bias, a.res, a.y, a.B,
                                   a.Cin, a.H, a.Cout, a.osc, a.act_scale);
                UBPL_LAUNCH_CHECK();
                return 0;
            }
            return (int)hipErrorInvalidValue;
        },
        among<32, 64, 96, 128>{c.W}, among<1, 2, 3>{a.npieces}, among<128, 64>{c.BM}, among<1, 2>{c.TEAMS},
        among<1, 2>{c.NHB});
}
