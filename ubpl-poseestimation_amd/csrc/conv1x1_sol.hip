// The 1x1 convolution with the split on load (conv1x1_sol_kernel): forward and data gradient
// on the split paths with no pre-split image, and the planner that says which shapes it takes.
// Shared pieces: split_common.h.
#include "split_common.h"

namespace {

// ------------------------------------------------------------------ 1x1, split on load
// y[b,m,p] = sum_k w[m][k] v[b,k,p] + bias[m] (+ res), v = relu(x*pscale +
// pshift) (PRO) or x, on the 6xbf16 path without a pre-split operand: the f32
// activations (NCHW) go global -> LDS by LDS-DMA as the 16 k rows of a
// 256-pixel tile (1 KB each; rows 8-15 shifted 128 B so the two 32-lane halves
// of a fragment read sit in opposite bank halves), and each wave reads its own
// pixels' B fragments from that f32 image (lane (n, h): k = 8h..8h+7 of pixel
// n, 8 ds_read_b32), applies the prologue and splits into 3 bf16 pieces in
// registers.  Waves split the tile along pixels (wave w: all BM rows x pixels
// 64w..64w+63), so each value is split once per workgroup.  Weights: 3 bf16
// planes of [M][K] (ubpl_conv_weights_split with KS = 1), staged as in
// conv_psa_kernel.  2-stage ring, 2 workgroups per CU.  The activation read is
// the f32 tensor itself: no split pass, no 6-byte/element PSA image.
// BNT: pixels per tile, 256 (wave w: pixels 64w..64w+63) or 128 (32 per wave: half the
// LDS and accumulators, three workgroups per CU, so one workgroup's epilogue stores run
// beside the others' K loops)
template <int BM, bool PRO, bool EPI = false, int NP = 3, int NS = 2, int BNT = 256, int NSB = NS>
__global__ void __launch_bounds__(NT, BNT == 128 ? 3 : UBPL_SOL_LB) conv1x1_sol_kernel(const float* __restrict__ x,
                                                           const uint16_t* __restrict__ wp, int64_t wplane,
                                                           const float* __restrict__ bias,
                                                           const float* __restrict__ pscale,
                                                           const float* __restrict__ pshift, const float* res,
                                                           float* y, int B, int K, int P, int M,
                                                           float* __restrict__ stat_part, ubpl::BnBwdEpi bwd,
                                                           float asc, float osc) {
    // NP = 3: 6xbf16 (f32-equivalent); NP = 2: 2xfp16 (activations scaled by asc after the
    // prologue, accumulators by osc = weight scale x asc, undone at the stores); NP = 1: the
    // "bf16" precision (operands rounded to bf16, one MFMA per product, accumulated in f32)
    // NS: stages in the LDS ring (2, or 3 with 64-row tiles: two K steps' DMA in flight);
    // NSB = 3 with NS = 2: a deeper ring for the activation stream alone (HBM: two K
    // steps of it in flight per workgroup) beside the weights' two stages (L2-resident)
    static_assert(BNT == 256 || BNT == 128, "256- or 128-pixel tiles");
    static_assert(NSB == NS || (NS == 2 && NSB == 3), "B ring: as deep as A's, or 3 beside A's 2");
    constexpr int TM = BM / 32, TN = BNT / 128;
    constexpr int BQ = BNT / 64;             // B DMA instructions per wave per K step (1 KB each)
    constexpr int AB = NP * BM * 32;         // A stage bytes: [piece][BM rows][32 B]
    constexpr int BH = 8 * BNT * 4 + 128;    // one 8-row half of the B image (+ bank shift)
    constexpr int BB = 2 * BH;
    __shared__ __attribute__((aligned(16))) char lds[NS * AB + NSB * BB];   // A slots, then B slots
    // the prologue's (scale, shift) per input channel (K <= SOL_PRO_K), staged once:
    // a lane's 8 channels of a K step are 2 ds_read_b128 each, instead of scalar
    // loads of both 8-channel halves and 16 per-lane selects (48 VALU per K step)
    __shared__ __attribute__((aligned(16))) float lds_sc[PRO ? SOL_PRO_K : 4], lds_sh[PRO ? SOL_PRO_K : 4];

    const int64_t N = (int64_t)B * P;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: SGPR)
    const int wn = (BNT / 4) * wid;
    if (PRO) {
        for (int k = tid; k < K; k += NT) {
            lds_sc[k] = pscale[k];
            lds_sh[k] = pshift[k];
        }
        // a full barrier (waits for the LDS stores): the K loop's raw s_barrier does
        // not, and without it a wave could read another wave's coefficients of the
        // first K step before they land (before any DMA is issued: costs no overlap)
        __syncthreads();
    }
    const int lam = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int by = lam % gridDim.y, bx = lam / gridDim.y;
    const int m0 = by * BM;
    const int64_t n0 = (int64_t)bx * BNT;

    // A DMA (as conv_psa_kernel): wave w < BM/32 moves rows 32w..32w+31 of each piece
    const int lr = lane >> 1;
    const int lchunk = (lane & 1) ^ ((lr >> 3) & 1);
    const bool a_issue = BM / 32 >= NT / 64 || wid < BM / 32;   // every wave when BM >= 128
    const uint32_t a_lane = (uint32_t)(((int64_t)min(m0 + 32 * wid + lr, M - 1) * K + 8 * lchunk) * 2);
    // B DMA: wave w moves k rows 4w..4w+3; 256-pixel tiles: one row per instruction,
    // lane L pixels n0 + 4L .. +3; 128-pixel tiles: two rows per instruction, lanes
    // 32-63 the second (P % 4 == 0)
    uint32_t b_lane;
    {
        const int pl = BNT == 256 ? lane : (lane & 31);
        int64_t n = n0 + 4 * pl;
        n = n < N ? n : N - 4;
        const int64_t b = n / P;
        b_lane = (uint32_t)((b * K * P + (n - b * P) + (BNT == 256 ? 0 : (int64_t)(lane >> 5) * P)) * 4);
    }
    auto stage_a = [&](int buf, int kt) {
        char* base = lds + buf * AB;
        if (a_issue) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const char* ab = reinterpret_cast<const char*>(wp + p * wplane + kt);
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)(ab + a_lane),
                                                 (lds_ptr_t)(base + p * BM * 32 + wid * 1024), 16, 0, 0);
            }
        }
    };
    auto stage_b = [&](int buf, int kt) {
        char* base = lds + NS * AB + buf * BB;
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            const int r = 4 * wid + q * (4 / BQ);
            const char* bb = reinterpret_cast<const char*>(x + (int64_t)(kt + r) * P);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(bb + b_lane),
                                             (lds_ptr_t)(base + (r >> 3) * BH + (r & 7) * (BNT * 4)), 16, 0, 0);
        }
    };
    auto stage = [&](int buf, int kt) {
        stage_a(buf, kt);
        stage_b(buf, kt);
    };

    // accumulators start at bias (+ residual): see conv_psa_kernel
    const int li = lane & 31, h = lane >> 5;
    // output offsets: computed for the seed and again for the epilogue (not live
    // across the K loop: the tile spilled ~30 VGPRs to scratch with them)
    auto out_base = [&](int64_t (&ob)[TN], bool (&ok)[TN]) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t n = n0 + wn + 32 * j + li;
            ok[j] = n < N;
            const int64_t nc = ok[j] ? n : N - 1;
            const int b = (int)(nc / P);
            const int p = (int)(nc - (int64_t)b * P);
            ob[j] = (int64_t)b * M * P + p;
        }
    };
    int64_t obase[TN];
    bool nok[TN];
    out_base(obase, nok);
    floatx16 acc[TM][TN];
    // UBPL_SOL_TEPI (with a residual): the output tile leaves through LDS as
    // float4 rows (8 stores per lane per 32-row block instead of 32 scalar
    // stores) with the residual added there by float4 loads issued ahead of
    // the stores, instead of seeding the accumulators with 128 scalar loads per
    // lane before the K loop (128->256 + skip at 64x64 B=32: 101 -> 91 us);
    // without a residual the scalar epilogue measured faster
    const bool tepi = UBPL_SOL_TEPI && BNT == 256 && !EPI && res != nullptr &&
                      ((((uintptr_t)y) | (uintptr_t)res) & 15) == 0;
    ubpl::seed_acc<TM, TN>(acc, bias, tepi ? nullptr : res, obase, m0, M, P, osc);
    const float inv = 1.f / osc;

    const int nkt = K >> 4;
    constexpr bool deepb = NSB != NS;
    // this lane's k half of K step kt: 8 (scale, shift) pairs of the prologue
    auto load_coef = [&](int kt, float (&sc)[8], float (&sh)[8]) {
        if (PRO) {
            const float4* qs = reinterpret_cast<const float4*>(lds_sc + kt + 8 * h);
            const float4* qh = reinterpret_cast<const float4*>(lds_sh + kt + 8 * h);
            const float4 s0 = qs[0], s1 = qs[1], h0 = qh[0], h1 = qh[1];
            sc[0] = s0.x; sc[1] = s0.y; sc[2] = s0.z; sc[3] = s0.w;
            sc[4] = s1.x; sc[5] = s1.y; sc[6] = s1.z; sc[7] = s1.w;
            sh[0] = h0.x; sh[1] = h0.y; sh[2] = h0.z; sh[3] = h0.w;
            sh[4] = h1.x; sh[5] = h1.y; sh[6] = h1.z; sh[7] = h1.w;
        }
    };
    // this wave's B fragment of pixel column j (32 pixels) from a B stage: 8 f32 per lane,
    // prologue, split into NP bf16 pieces
    auto split_col = [&](const char* bbase, int j, const float (&sc)[8], const float (&sh)[8], bf16x8 (&out)[NP]) {
        const float* bs = reinterpret_cast<const float*>(bbase + h * BH) + wn + li;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] = bs[e * BNT + 32 * j];
            if (PRO) v[e] = fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f);
            if constexpr (NP == 2) v[e] *= asc;
        }
        uint32_t pk[NP][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            uint32_t o[NP];
            split2<NP>(v[2 * e], v[2 * e + 1], o);
#pragma unroll
            for (int p = 0; p < NP; ++p) pk[p][e] = o[p];
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const uint4 u = make_uint4(pk[p][0], pk[p][1], pk[p][2], pk[p][3]);
            out[p] = __builtin_bit_cast(bf16x8, u);
        }
    };
    stage(0, 0);
    if (NS == 3 && nkt > 1) stage(1, 16);
    if (deepb && nkt > 1) stage_b(1, 16);
    for (int t = 0; t < nkt; ++t) {
        // stage t landed for every wave (NS = 3: this wave's stage t+1 DMA may stay in
        // flight; deepb: B(t+1), issued after A(t), may stay in flight), every wave
        // done with stage t-1
        if (NS == 3 && t + 1 < nkt) {
            if (a_issue) vm_wait<NP + BQ>();
            else vm_wait<BQ>();
        } else if (deepb && t + 1 < nkt) {
            vm_wait<BQ>();
        } else {
            vm_wait<0>();
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (deepb) {
            // A(t+1) first, then B(t+2): the next wait leaves only B(t+2) in flight
            if (t + 1 < nkt) stage_a((t + 1) % NS, (t + 1) * 16);
            if (t + 2 < nkt) stage_b((t + 2) % NSB, (t + 2) * 16);
        } else if (t + NS - 1 < nkt) {
            stage((t + NS - 1) % NS, (t + NS - 1) * 16);
        }
        const int kt = t * 16;
        const char* base = lds + (t % NS) * AB;                       // A of stage t
        const char* bbase = lds + NS * AB + (t % NSB) * BB;           // B of stage t
        float sc[8], sh[8];
        load_coef(kt, sc, sh);
        bf16x8 bfr[TN][NP];
#pragma unroll
        for (int j = 0; j < TN; ++j) split_col(bbase, j, sc, sh, bfr[j]);
        if constexpr (NP == 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = 32 * i + li;
                bf16x8 af[NP];
                af[0] = *reinterpret_cast<const bf16x8*>(base + row * 32 + 16 * (h ^ ((row >> 3) & 1)));
#pragma unroll
                for (int j = 0; j < TN; ++j) mfma_split<NP>(acc[i][j], af, bfr[j]);
            }
        } else {
        auto lda = [&](int i, bf16x8 (&o)[NP]) {
            const int row = 32 * i + li;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                o[p] = *reinterpret_cast<const bf16x8*>(base + p * BM * 32 + row * 32 + 16 * (h ^ ((row >> 3) & 1)));
        };
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            bf16x8 af[NP];
            lda(i, af);
#pragma unroll
            for (int j = 0; j < TN; ++j) drain(acc[i][j], mfma_split0<NP>(af, bfr[j]));   // per-chunk accumulation
            // (register budget: one row block's A fragments live at a time)
            __builtin_amdgcn_sched_barrier(0);
        }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    out_base(obase, nok);
    if constexpr (EPI) {
        if (stat_part) ubpl::tile_bn_partials<TM, TN>(acc, nok, m0, M, n0 + wn, N, stat_part);
        if (bwd.part) ubpl::tile_bn_bwd_partials<TM, TN>(acc, nok, obase, m0, M, P, n0 + wn, N, bwd);
    }
    if constexpr (BNT == 256) if (tepi) {
        // every wave is done with the ring (its last reads waited on above); a
        // wave-private [32 rows][64 + 4 pixels] f32 image per 32-row block
        __syncthreads();
        constexpr int RS = 68;
        static_assert(NS * AB + NSB * BB >= 4 * 32 * RS * 4, "transposed epilogue image exceeds the ring");
        float* img = reinterpret_cast<float*>(lds) + wid * 32 * RS;
        const int rr = lane >> 4, c4 = (lane & 15) * 4;
        const int64_t n = n0 + wn + c4;   // 4 pixels of one image (P % 4 == 0)
        const bool ok = n < N;
        const int64_t b = ok ? n / P : 0;
        const int64_t ob = b * M * P + (n - b * P);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            // this block's residual rows first (8 loads in flight, ahead of the
            // stores, which may alias them)
            float4 q[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int m = m0 + 32 * i + rr + 4 * k;
                q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (res != nullptr && ok && m < M) q[k] = *reinterpret_cast<const float4*>(res + ob + (int64_t)m * P);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) img[((r & 3) + 8 * (r >> 2) + 4 * h) * RS + 32 * j + li] = acc[i][j][r];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int row = rr + 4 * k;
                const int m = m0 + 32 * i + row;
                float4 v = *reinterpret_cast<const float4*>(img + row * RS + c4);
                if (ok && m < M) {
                    v.x = fmaf(v.x, inv, q[k].x); v.y = fmaf(v.y, inv, q[k].y);
                    v.z = fmaf(v.z, inv, q[k].z); v.w = fmaf(v.w, inv, q[k].w);
                    *reinterpret_cast<float4*>(y + ob + (int64_t)m * P) = v;
                }
            }
        }
        return;
    }
    store_tile<TM, TN>(acc, nok, obase, m0, M, P, y, m0 + BM <= M && n0 + BNT <= N, inv);
}

using namespace ubpl;

bool sol_supported(int B, int Cin, int Cout, int P) {
    // Cout % 64 != 0 (the 16-channel heatmap projection, preds.*.conv): one
    // 64-row tile with the rows past Cout clamped on load and never stored
    return B > 0 && P > 0 && Cin % 16 == 0 && Cin > 0 && Cout % 16 == 0 && P % 4 == 0 && (int64_t)B * P >= 4 &&
           (int64_t)B * Cin * P * 4 < (1LL << 32) && (int64_t)Cout * Cin * 2 < (1LL << 31);
}

// Output-channel block: 128 rows (each pixel tile split once per 128 channels)
// unless that leaves CUs idle; then 64 (the 32x32-plane 256->128 convs at B=32:
// 128 -> 256 workgroups).  UBPL_SOL_BM=64: 64-row tiles everywhere (A/B knob)
int sol_bm(int64_t N, int Cout) {
    if (Cout % 128 != 0 || knobs().sol_bm64) return 64;
    return ((N + 255) / 256) * (Cout / 128) >= cu_count() ? 128 : 64;
}

dim3 sol_grid(int64_t N, int Cout, int bm) { return dim3((unsigned)((N + 255) / 256), (unsigned)((Cout + bm - 1) / bm)); }

// conv1x1_sol_kernel<BM, PRO, EPI, NP, NS, 256, NSB>
struct SolChoice {
    int BM, PRO, EPI, NP, NS, NSB;
};

SolChoice sol_choose(int bm, bool pro, bool epi, int npieces) {
    const Knobs& k = knobs();
    // the activation ring 3 stages deep beside the weights' 2 (two K steps of the HBM
    // stream in flight per workgroup; the default since round 5, measured even with the
    // 2-stage ring, profiles/r05_v1_sol_nsb.txt); UBPL_SOL_NSB=2: one ring of 2 stages
    const int nsb = k.sol_nsb3 ? 3 : 2;
    if (npieces != 3) return {bm, pro, 0, npieces, 2, nsb};
    if (bm == 64 && k.sol_ns3 && !epi) return {64, pro, 0, 3, 3, 3};   // UBPL_SOL_NS=3: 3-stage ring on 64-row tiles
    if (epi) return {bm, pro, 1, 3, 2, 2};                            // (epilogue partials: one ring of 2 stages)
    return {bm, pro, 0, 3, 2, nsb};
}

// the instantiations that are built: partials on 6xbf16 with one 2-stage ring; 3 stages on
// the 64-row 6xbf16 tiles
constexpr bool sol_built(int BM, int EPI, int NP, int NS, int NSB) {
    if (EPI) return NP == 3 && NS == 2 && NSB == 2;
    if (NS == 3) return BM == 64 && NP == 3 && NSB == 3;
    return true;
}

}  // namespace

// 1 when ubpl_conv1x1_forward_split_load takes this shape on a grid of at least min_wgs
// 256-pixel workgroups; 0: use the f32 1x1 kernel (split-K plans).
UBPL_API int ubpl_conv1x1_split_load_preferred_min(int B, int Cin, int Cout, int P, int min_wgs) {
    if (!sol_supported(B, Cin, Cout, P)) return 0;
    const int64_t N = (int64_t)B * P;
    const dim3 g = sol_grid(N, Cout, sol_bm(N, Cout));
    return (int64_t)g.x * g.y >= min_wgs ? 1 : 0;
}

// ... and fills the chip (>= one workgroup per CU)
UBPL_API int ubpl_conv1x1_split_load_preferred(int B, int Cin, int Cout, int P) {
    return ubpl_conv1x1_split_load_preferred_min(B, Cin, Cout, P, cu_count());
}

// y = conv1x1(relu(x*pscale + pshift) or x) + bias (+ res, may alias y) on the
// 6xbf16 path, x NCHW f32 split while it is staged (conv1x1_sol_kernel).
// wsplit: 3 bf16 planes (`wplane` elements apart) of [Cout][Cin] from
// ubpl_conv_weights_split (mode 0 of a 1x1 conv; mode 1 = its data gradient,
// then x = dy and Cin/Cout swap).  Cin % 16 == 0, Cout % 64 == 0, P % 4 == 0,
// x / wsplit 16-B aligned.  stat_part (nullable): BatchNorm partials of y.
UBPL_API int ubpl_conv1x1_forward_split_load(const float* x, int B, int Cin, int P, const uint16_t* wsplit,
                                             int64_t wplane, const float* bias, int Cout, const float* pscale,
                                             const float* pshift, const float* res, float* y, float* stat_part,
                                             const float* bn_x, const float* bn_coef, int bn_relu, float* bn_part,
                                             int npieces, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!sol_supported(B, Cin, Cout, P) || (((uintptr_t)x) & 15) || (((uintptr_t)wsplit) & 15) || (wplane % 8) ||
        npieces < 1 || npieces > 3)
        return (int)hipErrorInvalidValue;
    const bool pro = pscale != nullptr;
    if (pro && Cin > SOL_PRO_K) return (int)hipErrorInvalidValue;
    const int64_t N = (int64_t)B * P;
    const BnBwdEpi bwd{bn_part ? bn_x : nullptr, bn_coef, bn_relu, bn_part};
    const bool epi = stat_part != nullptr || bn_part != nullptr;
    if (epi && (npieces != 3 || Cout % 64 != 0)) return (int)hipErrorInvalidValue;   // (epilogue partials: 6xbf16, whole tiles)
    const int bm = sol_bm(N, Cout);
    const SolChoice c = sol_choose(bm, pro, epi, npieces);
    const dim3 grid = sol_grid(N, Cout, bm);
    const float asc = FP16_ACT_SCALE, osc = psa_osc(npieces, Cin);
    return pick(
        [&](auto BM, auto PRO, auto EPI, auto NP, auto NS, auto NSB) {
            if constexpr (sol_built(BM, EPI, NP, NS, NSB)) {
                hipLaunchKernelGGL((conv1x1_sol_kernel<BM, PRO != 0, EPI != 0, NP, NS, 256, NSB>), grid, dim3(NT), 0, st,
                                   x, wsplit, wplane, bias, pscale, pshift, res, y, B, Cin, P, Cout, stat_part, bwd,
                                   asc, osc);
                UBPL_LAUNCH_CHECK();
                return 0;
            }
            return (int)hipErrorInvalidValue;
        },
        among<128, 64>{c.BM}, among<0, 1>{c.PRO}, among<0, 1>{c.EPI}, among<1, 2, 3>{c.NP}, among<2, 3>{c.NS},
        among<2, 3>{c.NSB});
}
