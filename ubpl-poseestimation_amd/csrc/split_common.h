// Shared by the split-precision convolution files (conv_split_fwd.hip, conv_psa.hip,
// conv_psah.hip, conv1x1_sol.hip, conv_wgrad_split.hip, conv_stem_split.hip,
// conv_weights_split.hip): the device helpers of every kernel family, and on the host side
// the forward plan, the run-time knobs and the argument structs of the dispatch.
//
// Convolutions on the bf16 matrix cores with fp32 operands carried as sums of
// bf16 pieces ("split-bf16"): v = v0 + v1 (+ v2), v0 = bf16(v), v1 = bf16(v - v0),
// v2 = bf16(v - v0 - v1).  A product a*b is the sum of the piece products with
// pa + pb < NP (the dropped ones are below the fp32-relevant range for NP = 3,
// ~2^-16 relative for NP = 2), each exact in f32, summed by
// v_mfma_f32_32x32x16_bf16 into an f32 accumulator:
//   NP = 2: 3 MFMAs per 32x32x16 step (16/3 = 5.3x the v_mfma_f32_32x32x2_f32 rate);
//   NP = 3: 6 MFMAs (2.7x), rounding error at the level of an f32 fmaf chain.
// Same GEMM views, K order and epilogues as conv_f32.h (the Conv wrapper,
// models/base/layers.py:31-50): grouped tap-major k = (ci/16)*16T + tap*16 + ci%16.
//
// Operand images in LDS: [piece][row][4 x 16 B] with the row's 32 k of one
// K step in four 16-B chunks (chunk c = 2s + h holds k = 16s + 8h .. +7, the
// 8 bf16 lane (r, h) of MFMA k-step s reads) — A rows = output channels, B rows
// = output pixels n, both k-contiguous, chunk XOR-swizzled by (row >> 2) & 3
// (conflict-free ds_read_b128 for the 16-lane groups of a 32-row fragment read).
// Weights are split once per pass (ubpl_conv_weights_split, a batched
// re-layout into NP bf16 planes); activations are split while they are staged,
// after the fused BN+ReLU prologue.
#pragma once
#include <atomic>
#include <cstdlib>

#include "common.h"
using ubpl::xcd_remap;

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short short8 __attribute__((ext_vector_type(8)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// (the kernels and their helpers live in each file's own anonymous namespace)
namespace {

// the unguarded epilogues' stores non-temporal (UBPL_NT_EPI, below); the 1x1 split-load kernel's
// transposed residual epilogue (UBPL_SOL_TEPI); its launch-bounds occupancy (UBPL_SOL_LB); the
// one-buffer halo kernel's deepest A ring (UBPL_PSAH_NA_MAX) — build-time knobs, defaults measured
// (DESIGN.md §4, §6).  Round 6: the timing-only diagnostic builds and the variants that measured
// slower (the warp-specialized 1x1 and 3x3 kernels, the 16x16x32 halo forms, fair arbitration,
// clock stamps) were removed from the product source; they stay in the git history.
#ifndef UBPL_SOL_TEPI
#define UBPL_SOL_TEPI 1
#endif
#ifndef UBPL_PSAH_NA_MAX
#define UBPL_PSAH_NA_MAX 3
#endif
#ifndef UBPL_SOL_LB
#define UBPL_SOL_LB 2
#endif

constexpr int NT = 256;
constexpr int PSA_KSUB1 = 2;     // conv_psa_kernel on the bf16 path: 16-k steps per stage (measured)
constexpr int SOL_PRO_K = 512;   // conv1x1_sol_kernel: largest input channel count with a prologue
constexpr int BK = 32;
constexpr int BN = 128;

using ubpl::split2;

__device__ __forceinline__ int swz(int row, int c) { return c ^ ((row >> 2) & 3); }

// One 32x32x16 piece product: bf16 pieces (NP = 1, 3) or fp16 pieces (NP = 2, the
// 2xfp16 path: common.h split2); the fragments travel as 16-bit lanes either way.
template <int NP>
__device__ __forceinline__ floatx16 mfma_piece(const bf16x8 a, const bf16x8 b, const floatx16 c) {
    if constexpr (NP == 2)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c,
                                                      0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// element e of a piece fragment as f32 (fp16 pieces for NP = 2, bf16 otherwise)
template <int NP>
__device__ __forceinline__ float piece_elem(const bf16x8 v, int e) {
    if constexpr (NP == 2) return (float)__builtin_bit_cast(half8, v)[e];
    else return (float)v[e];
}

// acc += sum over piece pairs (pa, pb), pa + pb < NP, smallest terms first
template <int NP>
__device__ __forceinline__ void mfma_split(floatx16& acc, const bf16x8 (&a)[NP], const bf16x8 (&b)[NP]) {
#pragma unroll
    for (int d = NP - 1; d >= 0; --d)
#pragma unroll
        for (int pa = d; pa >= 0; --pa) acc = mfma_piece<NP>(a[pa], b[d - pa], acc);
}

// acc += t one element at a time.  The floatx16 `+=` lowers to v_pk_add_f32,
// which beside MFMAs costs ~13 cycles more per instruction than the two scalar
// adds it replaces (MI355X_MICROARCH.md, 'price of one filler beside MFMAs':
// packed f32 VALU is an anti-lever there); scalar v_add_f32 hide in the MFMA
// gaps.  Same rounding: one f32 add per element.  The empty asm on each sum
// keeps the SLP vectorizer from re-packing the adds (it emits no instruction).
__device__ __forceinline__ void drain(floatx16& acc, const floatx16 t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = acc[r] + t[r];
        asm("" : "+v"(v));
        acc[r] = v;
    }
}

// Ping-pong schedule of one chunk chain (its NP(NP+1)/2 MFMAs) with the previous
// tile's 16 drain adds spread over the MFMA gaps (6 x (1 MFMA : 3 VALU) for the
// 6-product chain, 3 x (1 : 6) for the 3-product one)
template <int NP>
__device__ __forceinline__ void pp_schedule() {
    constexpr int NMF = NP * (NP + 1) / 2;
    constexpr int NV = (16 + NMF - 1) / NMF;
#pragma unroll
    for (int g = 0; g < NMF; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// the same sum started from zero (one 16-k chunk of the chunked accumulation):
// the first MFMA takes C = 0 as an inline constant, no zeroed registers
template <int NP>
__device__ __forceinline__ floatx16 mfma_split0(const bf16x8 (&a)[NP], const bf16x8 (&b)[NP]) {
    const floatx16 zero = {};
    floatx16 t = mfma_piece<NP>(a[NP - 1], b[0], zero);
#pragma unroll
    for (int d = NP - 1; d >= 0; --d)
#pragma unroll
        for (int pa = d; pa >= 0; --pa)
            if (!(d == NP - 1 && pa == NP - 1)) t = mfma_piece<NP>(a[pa], b[d - pa], t);
    return t;
}


// The scalar epilogue of a TM x TN tile of 32 x 32 MFMA blocks (rows mrow0 + ..,
// output offsets obase[j] + m * P): when the whole tile is in range (`full`,
// wave-uniform) the stores go out unguarded — each guarded store had been a
// compare, an exec-mask branch and a restore.
// the unguarded epilogue's stores non-temporal (streamed past the caches: the output is
// read next by another kernel, far more than L2 holds): 207.5 vs 212.7 us on the 128-ch
// 64x64 halo conv, 238 vs 252 at 64 ch 128x128, 1x1 1-3 %, the step within noise
// (profiles/r04_psa_diag.txt); UBPL_NT_EPI=0 at build time: plain stores
#ifndef UBPL_NT_EPI
#define UBPL_NT_EPI 1
#endif
// inv: 1 / the accumulators' scale (seed_acc), applied exactly (a power of two)
template <int TM, int TN>
__device__ __forceinline__ void store_tile(const floatx16 (&acc)[TM][TN], const bool (&nok)[TN],
                                           const int64_t (&obase)[TN], int mrow0, int M, int P, float* y,
                                           bool full, float inv = 1.f) {
    const int h = (threadIdx.x & 63) >> 5;
    if (full) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float* d = y + obase[j] + (int64_t)(mrow0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h) * P;
                    if (UBPL_NT_EPI) __builtin_nontemporal_store(acc[i][j][r] * inv, d);
                    else *d = acc[i][j][r] * inv;
                }
        return;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        if (!nok[j]) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mrow0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < M) y[obase[j] + (int64_t)m * P] = acc[i][j][r] * inv;
            }
    }
}

}  // namespace

// ------------------------------------------------------------------ host side
namespace ubpl {

// The run-time knobs of the split paths: one field per environment name, read once at the
// first use (DESIGN.md §4 has the table with the measurements behind the defaults).
struct Knobs {
    static const char* env(const char* name) { return std::getenv(name); }
    static int env_int(const char* name, int dflt) {
        const char* e = env(name);
        return e ? atoi(e) : dflt;
    }
    static int in_range(int v, int lo, int hi, int dflt) { return v >= lo && v <= hi ? v : dflt; }

    // field = its environment name, the values that count, the default (what each does: DESIGN.md §4)
    const bool no_splitk = env("UBPL_NO_SPLITK") != nullptr && env("UBPL_NO_SPLITK")[0] == '1';   // (off)
    const bool psa_bn256 = env_int("UBPL_PSA_BN", 256) != 128;      // 128: 128-pixel tiles everywhere
    const bool psa_bm64w = env_int("UBPL_PSA_BM64W", 1) != 0;       // 0: 64 x 128 tiles on 64-row launches
    const int psa_ksub1 = in_range(env_int("UBPL_PSA_KSUB1", PSA_KSUB1), 1, 4, PSA_KSUB1);
    const bool sol_bm64 = env_int("UBPL_SOL_BM", 0) == 64;          // 64: 64-row tiles everywhere
    const bool sol_ns3 = env_int("UBPL_SOL_NS", 2) == 3;            // 3: 3-stage ring on 64-row 6xbf16 tiles
    const bool sol_nsb3 = env_int("UBPL_SOL_NSB", 3) == 3;          // any other value: 2 activation stages
    const int wgrad3_wgs = env_int("UBPL_WGRAD3_WGS", 512);         // two workgroups per CU
    const int wgrad1_wgs = env_int("UBPL_WGRAD1_WGS", 256);         // one workgroup per CU

    // The 3x3 halo kernel's dispatch: UBPL_PSA_HALO = 0 / 1 (anything else: -1, the default),
    // UBPL_PSA_TEAMS = 1 / 2 (unset: -1); diagnostics.  -2 = not read yet: ubpl_set_psa_dispatch
    // (tests) overrides both, and sends them back to the environment with (-2, -2).
    std::atomic<int> psa_halo{-2}, psa_teams{-2};
    struct PsaDispatch {
        int halo, teams;
    };
    PsaDispatch psa_dispatch() {
        if (psa_halo.load(std::memory_order_relaxed) == -2) {
            const int hv = env_int("UBPL_PSA_HALO", -1);
            int expect = -2;
            psa_halo.compare_exchange_strong(expect, hv == 0 || hv == 1 ? hv : -1);
            expect = -2;
            psa_teams.compare_exchange_strong(expect, env_int("UBPL_PSA_TEAMS", -1));
        }
        return {psa_halo.load(std::memory_order_relaxed), psa_teams.load(std::memory_order_relaxed)};
    }
};
inline Knobs& knobs() {
    static Knobs k;
    return k;
}

// Resident workgroups per CU of a family's 128- and 64-row forward kernels, [NP == 3]: each
// family's file queries its own kernels (the initial values stay where a query fails).
struct TileOcc {
    int o128[2], o64[2];
};
inline TileOcc query_tile_occ(TileOcc r, const void* k128_2, const void* k128_3, const void* k64_2,
                              const void* k64_3, int threads) {
    auto q = [&](const void* f, int& dst) {
        int o = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, f, threads, 0) == hipSuccess && o > 0) dst = o;
    };
    q(k128_2, r.o128[0]);
    q(k128_3, r.o128[1]);
    q(k64_2, r.o64[0]);
    q(k64_3, r.o64[1]);
    (void)hipGetLastError();
    return r;
}

// ------------------------------------------------------------------ planning
// Blocks spread evenly over the CUs; a CU with c blocks (r = min(c, occ)
// resident) runs them in c * (steps + 2) K steps at a rate that needs ~2
// resident blocks to hide latency.  Split-K adds the slab round trip + a launch.
inline double plan_cost(int64_t tiles, int s, int64_t nsteps, int occ, int ncu, double step_flops,
                        double slab_bytes) {
    const int64_t blocks = tiles * s;
    const int64_t per_cu = (blocks + ncu - 1) / ncu;
    const int64_t r = per_cu < occ ? per_cu : occ;
    const double eff = r >= 2 ? 1.0 : 0.6;
    const int64_t steps = (nsteps + s - 1) / s;
    const double rate = 2.0e12;   // split-bf16 flop/s per CU, sustained (model only)
    double t = (double)((per_cu + r - 1) / r) * r * (double)(steps + 2) * step_flops / (rate * eff);
    if (s > 1) t += 2.0 * s * slab_bytes / 5e12 + 4e-6;
    return t;
}

// bk: the kernel's K step (BK register-staged, 16 on pre-split activations); occ: its occupancy
inline Plan fwd_plan(int Cout, int64_t N, int Ktot, int np, int bk, const TileOcc& occ) {
    const int ncu = cu_count();
    const int nkt = (Ktot + bk - 1) / bk;
    const int maxs = knobs().no_splitk ? 1 : (nkt / 2 > 0 ? nkt / 2 : 1);
    Plan best{64, 1, 0};
    double bc = 1e30;
    for (int bm : {128, 64}) {
        if (bm == 128 && Cout <= 64) continue;
        const int64_t tiles = ((Cout + bm - 1) / bm) * ((N + BN - 1) / BN);
        const int o = bm == 128 ? occ.o128[np == 3] : occ.o64[np == 3];
        const double sf = 2.0 * bm * BN * bk;
        int s_best = 1;
        double c_best = plan_cost(tiles, 1, nkt, o, ncu, sf, 4.0 * Cout * N);
        for (int s = 2; s <= maxs; ++s) {
            const double c = plan_cost(tiles, s, nkt, o, ncu, sf, 4.0 * Cout * N);
            if (c < c_best * 0.97) {
                c_best = c;
                s_best = s;
            }
        }
        const double c = c_best / (bm == 128 ? 1.0 : 0.85);
        if (c < bc) {
            bc = c;
            best.bm = bm;
            best.splits = s_best;
        }
    }
    const int steps = (nkt + best.splits - 1) / best.splits;
    best.kchunk = steps * bk;
    best.splits = (nkt + steps - 1) / steps;
    return best;
}

// the accumulators' scale of a split conv: 2xfp16 (NP = 2) the weight scale of its contraction
// length x the activation scale (common.h split2), else 1
// (dev_act: the activation scale is read on the device, *ascp; the host part is the weight scale)
inline float psa_osc(int np, int ktot, bool dev_act = false) {
    return np == 2 ? fp16_wscale(ktot) * (dev_act ? 1.f : FP16_ACT_SCALE) : 1.f;
}

// ------------------------------------------------------------------ dispatch
// (the value selector pick / among: common.h)
// What every launch of ubpl_conv2d_forward_psa shares (conv_psa_kernel and conv_psah_kernel)
struct PsaArgs {
    const uint16_t *xs, *wp;
    int64_t xplane, wplane;
    const float *bias, *res;
    float* y;
    int B, Cin, H, W, pad, Cout, KS, npieces;
    Plan pl;
    float *slab, *stat_part;
    BnBwdEpi bwd;
    float osc;                // psa_osc of the launch
    const float* act_scale;   // (2xfp16: the image's scale on the device, or null)
    hipStream_t st;
};

// The kernel ubpl_conv2d_forward_psa runs: conv_psah_kernel<W, NP, BM, TEAMS, NHB> (halo; the
// 96-wide planes on 192-pixel tiles, the others on 256) or conv_psa_kernel<BM, KS, NP, BNT, WGM,
// EPI, KSUB> (WGM = 1 wave row on the 64 x 256 tiles, else 2; EPI where partials are asked
// for), and its grid.
struct PsaChoice {
    bool halo;
    int W, BM, TEAMS, NHB;   // conv_psah_kernel
    int BNT, KSUB;           // conv_psa_kernel (BM too)
    dim3 grid;
};

// (conv_psah.hip: its kernels build apart from conv_psa.hip's)
__attribute__((visibility("hidden"))) int launch_psah(const PsaChoice& c, const PsaArgs& a);

}  // namespace ubpl
