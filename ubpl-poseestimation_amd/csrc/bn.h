// BatchNorm2d (train-mode batch statistics, eval-mode running statistics) for
// the hourglass (models/base/layers.py:41,57-61; nn.BatchNorm2d momentum 0.1,
// eps 1e-5).  NCHW: a channel is B contiguous HW planes.  This header holds what
// the two BatchNorm files share; bn_fwd.hip has the forward side (statistics,
// eval coefficients, apply, the 64-pixel partials path), bn_bwd.hip the backward.
//
// Forward never materialises bn(x) for the residual branches: the statistics
// kernels produce per-channel (scale, shift) = (g*invstd, b - mean*g*invstd)
// — PyTorch's own transform form — and the consuming convolution applies
// relu(x*scale + shift) while staging its operand (conv_f32_fwd.hip prologue).
//
// Statistics: each (channel, batch-slice) workgroup accumulates sum and sum of
// squares of (x - x0) — x0 a sample of the channel, which removes the
// cancellation of E[x^2] - E[x]^2 — then reduces in f64.  Partials go to a
// slab; the channel's last-arriving workgroup (ticket counter) combines them
// in slice order: deterministic, one launch.
//
// Backward: dyp = dz * [x*scale + shift > 0] (ReLU mask recomputed bit-for-bit
// as the forward prologue computed it); per channel S1 = sum dyp,
// S2 = sum dyp*(x - mean); dbeta += S1, dgamma += S2*invstd;
// dx = a*dyp + b*(x - mean) + c with a = g*invstd, b = -g*invstd^3*S2/N,
// c = -g*invstd*S1/N, plus up to two addends (residual-gradient sums).
#pragma once
#include "common.h"
using ubpl::among;
using ubpl::pick;

namespace {

// ------------------------------------------------------------------ scratch
// The double scratch of the one-launch statistics (ubpl_bn_part_doubles doubles, ZEROED
// before first use), in order:
//   MAXBN arrival counters (a fixed place, whatever C a call has; every call leaves them
//     at zero again);
//   the slab: per channel its slices' partials, 2 or 4 doubles per slice, channels
//     chan_stride doubles apart — room for 4 per slice of MAX_SPLITS slices of MAXBN channels;
//   the bounded backward statistics' tensor ticket (back at zero after every launch) in
//     TCNT_DOUBLES doubles of its own, then MAXBN per-channel bounds (floats).
constexpr int MAXBN = 512;
constexpr int MAX_SPLITS = 2048 / 64 + 1;   // splits_for's bound for C >= 64 (and B)

// Doubles between two channels' slice partials: 2 per slice, rounded up to
// 256 B, so no two channels' partials share a cache line (their publishers
// and last arrivers may sit on different XCDs, each with its own L2).
__host__ __device__ constexpr int64_t chan_stride(int nsp) { return ((int64_t)2 * nsp + 31) / 32 * 32; }

constexpr int64_t CNT_DOUBLES = MAXBN / 2;
constexpr int64_t SLAB_DOUBLES = MAXBN * chan_stride(2 * MAX_SPLITS);
constexpr int64_t TCNT_DOUBLES = 32;
constexpr int64_t BND_DOUBLES = MAXBN / 2;
constexpr int64_t PART_DOUBLES = CNT_DOUBLES + SLAB_DOUBLES + TCNT_DOUBLES + BND_DOUBLES;

struct Scratch {
    unsigned* cnt;    // [MAXBN] channel tickets
    double* slab;
    unsigned* tcnt;   // the tensor ticket
    float* bnd;       // [MAXBN] per-channel bounds of |dx|
};

inline Scratch carve(double* p) {
    double* slab = p + CNT_DOUBLES;
    double* tail = slab + SLAB_DOUBLES;
    return {reinterpret_cast<unsigned*>(p), slab, reinterpret_cast<unsigned*>(tail),
            reinterpret_cast<float*>(tail + TCNT_DOUBLES)};
}

// ----------------------------------------------------------------- geometry
// The batch slices a statistics launch uses: enough (channel, slice) blocks to fill
// the chip (~2048), and at least 8192 elements per block — small planes get one
// block per channel (at 4x4 / B=32, 2048 blocks of 32 elements each were pure
// launch and ticket overhead).  (16384 / 32768 per block measured <= 1.4 us per
// launch faster and within noise on the training step: profiles/r05_v11_bn_stats.txt.)
inline int splits_for(int B, int C, int HW) {
    int s = (2048 + C - 1) / C;
    if (s > B) s = B;
    if (s < 1) s = 1;
    const int64_t per_slice = (int64_t)B * HW / 8192;
    if (s > per_slice) s = per_slice > 1 ? (int)per_slice : 1;
    return s;
}

// the (channel, batch slice) grid of a statistics launch: dim3(C, gs), bper images per slice
inline void stats_grid(int B, int C, int HW, int& bper, int& gs) {
    const int splits = splits_for(B, C, HW);
    bper = (B + splits - 1) / splits;
    gs = (B + bper - 1) / bper;
}

inline int grid_ew(int64_t n) {
    int64_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

// ----------------------------------------------------------------- hand-off
// Last-arriver hand-off (cdna_hip_programming.md §6 Guideline 16, split-K
// counter form with write-through payload): thread 0 of every (channel,
// slice) block stores its partials with agent-scope atomic stores (sc1,
// write-through: no release fence, which would write back the whole L2),
// drains them, and takes a ticket; the block drawing the last ticket reads the
// channel's partials with agent-scope atomic loads (sc1: past any stale L1
// line), one slice per lane, sums them in a fixed order (deterministic) and
// resets the counter.  The ticket itself is relaxed (an agent-scope acq_rel ticket —
// an L2 write-back before it, an invalidate after — was tried as a diagnostic for the
// packed-FP32 fault of DESIGN.md §6 and changed nothing there).
__device__ __forceinline__ void publish2(double* p, double a, double b) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(a),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p + 1), (unsigned long long)__double_as_longlong(b),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double consume(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p),
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

__device__ __forceinline__ bool last_arriver(unsigned* cnt, unsigned n) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old != n - 1) return false;
    __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// The one combine.  Wave 0 of every (channel c, slice sp) block publishes the slice's
// NS + NM values d[] (2 or 4: the slab holds that many doubles per slice, channels
// chan_stride(nsp) resp. chan_stride(2 * nsp) apart) and takes a ticket; in the channel's
// last block the 64 lanes read the slices in parallel (one round trip, not one per slice: a
// serial read chain here was ~10 % of the training step) and reduce them: the first NS
// values summed — lane-strided over the slices, then wave_sum: a fixed order,
// deterministic — the last NM max-reduced (order-free; values >= 0 that are floats).
// Returns true in every lane of wave 0 of the channel's last block (wave-uniform), false
// everywhere else; the totals t[] are valid in lane 0.
template <int NS, int NM>
__device__ __forceinline__ bool combine_slices(double* slab, int c, int sp, int nsp, unsigned* cnt,
                                               const double (&d)[NS + NM], double (&t)[NS + NM]) {
    constexpr int NV = NS + NM;
    static_assert(NV == 2 || NV == 4, "the slab layouts: 2 or 4 doubles per slice");
    if (threadIdx.x >= 64) return false;
    double* pc = slab + (int64_t)c * chan_stride(NV / 2 * nsp);
    const int lane = threadIdx.x;
    int last = 0;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; k += 2) publish2(pc + sp * NV + k, d[k], d[k + 1]);
        last = last_arriver(cnt + c, nsp) ? 1 : 0;
    }
    if (!__shfl(last, 0, 64)) return false;
#pragma unroll
    for (int k = 0; k < NV; ++k) t[k] = 0.0;
    for (int q = lane; q < nsp; q += 64) {
#pragma unroll
        for (int k = 0; k < NS; ++k) t[k] += consume(pc + q * NV + k);
#pragma unroll
        for (int k = NS; k < NV; ++k) t[k] = fmax(t[k], consume(pc + q * NV + k));
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) t[k] = ubpl::wave_sum(t[k]);
#pragma unroll
    for (int k = NS; k < NV; ++k) t[k] = (double)ubpl::wave_max((float)t[k]);
    return true;
}

// --------------------------------------------------------------- statistics
struct StatsOut {
    const float* gamma;
    const float* beta;
    float eps, momentum;
    float *rmean, *rvar, *mean_out, *invstd_out, *scale, *shift;
};

// One thread per channel: (mean, biased variance) over N elements -> the channel's
// statistics, coefficients and running-statistics update (one expression for every
// statistics path: the same rounding).
__device__ __forceinline__ void write_stats(const StatsOut& o, int c, double mean, double var, int64_t N) {
    const float invstd = (float)(1.0 / sqrt(var + (double)o.eps));
    const float sc = invstd * o.gamma[c];
    o.mean_out[c] = (float)mean;
    o.invstd_out[c] = invstd;
    o.scale[c] = sc;
    o.shift[c] = o.beta[c] - (float)mean * sc;
    if (o.rmean) {
        const double unb = N > 1 ? var * (double)N / (double)(N - 1) : var;
        o.rmean[c] = (float)((double)o.momentum * mean + (1.0 - (double)o.momentum) * (double)o.rmean[c]);
        o.rvar[c] = (float)((double)o.momentum * unb + (1.0 - (double)o.momentum) * (double)o.rvar[c]);
    }
}

// Lane 0 of a channel's last block: the totals of (x - x0) and (x - x0)^2 -> write_stats.
__device__ __forceinline__ void finalize_stats(const StatsOut& o, int c, float x0, double t1, double t2, int64_t N) {
    const double m1 = t1 / (double)N;
    double var = t2 / (double)N - m1 * m1;
    if (var < 0) var = 0;
    write_stats(o, c, (double)x0 + m1, var, N);
}

// One float4 of a channel into a thread's f32 sums of (x - x0) and (x - x0)^2.
__device__ __forceinline__ void acc_shifted(float4 v, float x0, float& s1, float& s2) {
    const float a = v.x - x0, q = v.y - x0, r = v.z - x0, d = v.w - x0;
    s1 += (a + q) + (r + d);
    s2 = fmaf(a, a, fmaf(q, q, fmaf(r, r, fmaf(d, d, s2))));
}

// Visits the float4 offsets of channel c over images [b0, b1) of an NCHW
// tensor (hw4 float4s per plane, 256-thread blocks), calling f(slot, offset)
// (slot = the position in a group of U).  When every plane is whole
// 256-float4 rows (hw4 = 256 * 2^k: the 32x32 planes and up) each thread walks
// the same elements in the same order as the flattened (image, offset) loop,
// with no index division and U independent loads in flight; otherwise that loop.
template <int U, typename F>
__device__ __forceinline__ void visit_chan4(int b0, int b1, int C, int c, int hw4, F&& f) {
    const int kq = hw4 >> 8;
    if (kq > 0 && (hw4 & 255) == 0 && (kq & (kq - 1)) == 0) {
        const int ksh = __builtin_ctz(kq);
        const int nj = (b1 - b0) << ksh;
        const int64_t bstride = (int64_t)C * hw4;
        const int64_t base = ((int64_t)b0 * C + c) * hw4 + threadIdx.x;
        int j = 0;
        for (; j + U <= nj; j += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int jj = j + u;
                f(u, base + (int64_t)(jj >> ksh) * bstride + ((int64_t)(jj & (kq - 1)) << 8));
            }
        }
        for (; j < nj; ++j) f(0, base + (int64_t)(j >> ksh) * bstride + ((int64_t)(j & (kq - 1)) << 8));
        return;
    }
    // (the small planes: U iterations' loads issued together — the loop was one
    // dependent load round trip per iteration, ~10 us per launch at 16x16 / B=32;
    // same elements, same order)
    const int n4 = (b1 - b0) * hw4;
    const int st = blockDim.x;
    int i = threadIdx.x;
    for (; i + (U - 1) * st < n4; i += U * st) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ii = i + u * st;
            const int bb = ii / hw4, o4 = ii - bb * hw4;
            f(u, ((int64_t)(b0 + bb) * C + c) * hw4 + o4);
        }
    }
    for (; i < n4; i += st) {
        const int bb = i / hw4, o4 = i - bb * hw4;
        f(0, ((int64_t)(b0 + bb) * C + c) * hw4 + o4);
    }
}

// Finalize kernels of the 64-pixel partials paths: one 1024-thread block per channel,
// NPT independent slice loads per thread before any add (a dependent load-add chain made
// each finalize launch latency-bound, ~15 us on the training step's critical path).
constexpr int FT = 1024, NPT = 8;

// ----------------------------------------------------------------- backward
struct BwdOut {
    const float* gamma;
    const float* invstd;
    float *dgamma, *dbeta, *ca, *cb, *cc;
    // BOUND: per channel a bound of |dx| (|a| max|g| + |b| max|x - mean| + |c|) into bnd[c],
    // and from the tensor's last channel the 2xfp16 scale of dx (fp16_scale_for) into *dxscale
    float* bnd;
    unsigned* tcnt;
    float* dxscale;
};

struct BwdCoef {
    float a, b, c;
};

// One thread per channel: the totals (S1, S2) over N elements -> dbeta += S1, dgamma +=
// S2*invstd and the coefficients of dx = a*dyp + b*(x - mean) + c, stored and returned
// (one expression for every backward statistics path: the same rounding).
__device__ __forceinline__ BwdCoef bwd_coeffs(const BwdOut& o, int c, double t1, double t2, double N) {
    const double is = o.invstd[c], g = o.gamma[c];
    if (o.dgamma) o.dgamma[c] += (float)(t2 * is);
    if (o.dbeta) o.dbeta[c] += (float)t1;
    const BwdCoef k{(float)(g * is), (float)(-g * is * is * is * t2 / N), (float)(-g * is * t1 / N)};
    o.ca[c] = k.a;
    o.cb[c] = k.b;
    o.cc[c] = k.c;
    return k;
}

__device__ __forceinline__ float bwd_one(float g, float xv, float sc, float sh, float mu, float a, float b, float c,
                                         int relu) {
    if (relu && !(fmaf(xv, sc, sh) > 0.f)) g = 0.f;
    return fmaf(a, g, fmaf(b, xv - mu, c));
}

__device__ __forceinline__ float4 bwd_one4(float4 g, float4 xv, float sc, float sh, float mu, float a, float b,
                                           float c, int relu) {
    return make_float4(bwd_one(g.x, xv.x, sc, sh, mu, a, b, c, relu), bwd_one(g.y, xv.y, sc, sh, mu, a, b, c, relu),
                       bwd_one(g.z, xv.z, sc, sh, mu, a, b, c, relu), bwd_one(g.w, xv.w, sc, sh, mu, a, b, c, relu));
}

__device__ __forceinline__ void add4(float4& v, float4 q) {
    v.x += q.x;
    v.y += q.y;
    v.z += q.z;
    v.w += q.w;
}

// ------------------------------------------------------------ pool geometry
// The hourglass resampling passes (pool.hip) folded into the BatchNorm kernel
// next to them in the chain, which already holds the tensor in registers:
//   stats_maxpool_kernel     statistics of x + MaxPool2d(2,2) of x + statistics of the pooled tensor
//   upadd_stats_kernel       out = up + upsample2x(low) + statistics of out
//   bwd_apply_*_kernel<true> the BN backward apply + the max-pool gradient + the second addend
// Geometry (pool_geom): planes of H x W floats, H a power of two >= 2, W/4 (float4s per
// row) a power of two <= 32.  Then a plane is hw4 = H*W/4 float4s, a power of two, and
//  * float4 `off` of the tensor is plane off >> lhw4, row (off & (hw4-1)) >> lw4, column
//    off & (W/4-1): shifts, no division;
//  * the float4 one row below / above (the other half of its two 2x2 windows) is float4
//    off ^ (W/4), held by lane ^ (W/4) of the same wave in the same iteration: on
//    visit_chan4's whole-row path and in bwd_apply_plane_kernel a thread's float4s sit
//    at threadIdx.x + 256 k of the plane, on the flattened paths at a multiple of 256 from
//    threadIdx.x with 256 a multiple of hw4 (or hw4 of 256) — and a lane is active exactly
//    when its partner is (the ranges end on plane boundaries);
//  * the half-resolution tensor's plane is hw4 floats = hw4/2 float2s, W/4 float2s a row.
struct PoolGeom {
    int lw4, lhw4;   // log2(W/4), log2(H*W/4)
};

inline bool pool_geom(int H, int W, PoolGeom& g) {
    if (H < 2 || W < 4 || (H & (H - 1)) || (W & 3)) return false;
    const int w4 = W >> 2;
    if ((w4 & (w4 - 1)) || w4 > 32) return false;
    g.lw4 = __builtin_ctz(w4);
    g.lhw4 = g.lw4 + __builtin_ctz(H);
    return g.lhw4 < 28;
}

// Maximum of a 2x2 window given in row-major order and its position: the first maximum,
// a NaN wins (maxpool_fwd_kernel / maxpool_bwd_kernel's rule).
__device__ __forceinline__ float max4(float a, float b, float c, float d, int& am) {
    float m = a;
    am = 0;
    if (b > m || isnan(b)) { m = b; am = 1; }
    if (c > m || isnan(c)) { m = c; am = 2; }
    if (d > m || isnan(d)) { m = d; am = 3; }
    return m;
}

__device__ __forceinline__ float4 shfl_xor4(float4 v, int m) {
    return make_float4(__shfl_xor(v.x, m, 64), __shfl_xor(v.y, m, 64), __shfl_xor(v.z, m, 64),
                       __shfl_xor(v.w, m, 64));
}

// float2 index, in the half-resolution tensor, of the two windows float4 `off` belongs to
__device__ __forceinline__ int64_t half_index(int64_t off, PoolGeom g) {
    const int o4 = (int)(off & ((1 << g.lhw4) - 1));
    return ((off >> g.lhw4) << (g.lhw4 - 1)) + (((o4 >> g.lw4) >> 1) << g.lw4) + (o4 & ((1 << g.lw4) - 1));
}

}  // namespace
