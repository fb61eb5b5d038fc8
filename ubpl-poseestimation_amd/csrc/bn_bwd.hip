// BatchNorm2d, the backward side (overview: bn.h): the one-launch statistics (plain, or
// BOUND: with the 2xfp16 scale of dx), the 64-pixel partials path the conv epilogues
// feed, and the apply kernels — f32 dx with up to two addends and the max-pool gradient,
// or dx straight into PSA planes.
#include "bn.h"

namespace {

// Power-of-two scale that puts a tensor whose |values| <= bound at <= 2^14 (the
// 2xfp16 split's operand range: common.h split2); 1 for an all-zero tensor.
__device__ __forceinline__ float fp16_scale_for(float bound) {
    if (!(bound > 0.f) || !isfinite(bound)) return 1.f;
    int e;
    frexpf(bound, &e);                     // bound < 2^e
    e = min(max(14 - e, -60), 60);
    return ldexpf(1.f, e);
}

// Per (channel, slice): S1 = sum dyp, S2 = sum dyp*(x - mean) with the ReLU
// mask recomputed; the channel's last block produces dgamma/dbeta and the
// coefficients of dx = a*dyp + b*(x - mean) + c.  BOUND: also max |dyp| and
// max |x - mean| through the same hand-off (4 values per slice), from them a bound
// of the channel's |dx|, and the tensor's last channel turns the bounds into the
// 2xfp16 scale of dx.
template <bool VEC, bool BOUND>
__global__ void __launch_bounds__(256) bwd_stats_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                       int B, int C, int HW, int bper,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const float* __restrict__ mean, int relu,
                                                       double* __restrict__ part, unsigned* __restrict__ cnt,
                                                       BwdOut o) {
    __shared__ double red[16];
    __shared__ float redf[16];
    const int c = blockIdx.x, sp = blockIdx.y;
    const int b0 = sp * bper, b1 = min(B, b0 + bper);
    const float sc = scale[c], sh = shift[c], mu = mean[c];
    float s1 = 0.f, s2 = 0.f;
    float mg = 0.f, mx = 0.f;   // BOUND: max |g|, max |x - mean| of the slice
    if (VEC) {
        // (visit_chan4 here measured 7 % slower: the flattened loop stays; on the small
        // planes — <= 8 iterations per thread — all of them load first, then accumulate
        // in the same order)
        const int hw4 = HW >> 2;
        const int n4 = (b1 - b0) * hw4;
        const float4* x4 = reinterpret_cast<const float4*>(x);
        const float4* d4 = reinterpret_cast<const float4*>(dz);
        auto acc1 = [&](float4 xv, float4 g) {
            if (relu) {
                g.x = fmaf(xv.x, sc, sh) > 0.f ? g.x : 0.f;
                g.y = fmaf(xv.y, sc, sh) > 0.f ? g.y : 0.f;
                g.z = fmaf(xv.z, sc, sh) > 0.f ? g.z : 0.f;
                g.w = fmaf(xv.w, sc, sh) > 0.f ? g.w : 0.f;
            }
            s1 += (g.x + g.y) + (g.z + g.w);
            s2 = fmaf(g.x, xv.x - mu, fmaf(g.y, xv.y - mu, fmaf(g.z, xv.z - mu, fmaf(g.w, xv.w - mu, s2))));
            if (BOUND) {
                mg = fmaxf(mg, fmaxf(fmaxf(fabsf(g.x), fabsf(g.y)), fmaxf(fabsf(g.z), fabsf(g.w))));
                mx = fmaxf(mx, fmaxf(fmaxf(fabsf(xv.x - mu), fabsf(xv.y - mu)),
                                     fmaxf(fabsf(xv.z - mu), fabsf(xv.w - mu))));
            }
        };
        auto off_of = [&](int i) {
            const int bb = i / hw4, o4 = i - bb * hw4;
            return ((int64_t)(b0 + bb) * C + c) * hw4 + o4;
        };
        const int st = blockDim.x;
        if (n4 <= 8 * st) {
            float4 xv[8], g[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = threadIdx.x + u * st;
                if (i < n4) {
                    const int64_t off = off_of(i);
                    xv[u] = x4[off];
                    g[u] = d4[off];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (threadIdx.x + u * st < n4) acc1(xv[u], g[u]);
        } else {
            for (int i = threadIdx.x; i < n4; i += st) {
                const int64_t off = off_of(i);
                acc1(x4[off], d4[off]);
            }
        }
    } else {
        const int n = (b1 - b0) * HW;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int bb = i / HW, o1 = i - bb * HW;
            const int64_t off = ((int64_t)(b0 + bb) * C + c) * HW + o1;
            const float xv = x[off];
            float g = dz[off];
            if (relu && !(fmaf(xv, sc, sh) > 0.f)) g = 0.f;
            s1 += g;
            s2 = fmaf(g, xv - mu, s2);
            if (BOUND) {
                mg = fmaxf(mg, fabsf(g));
                mx = fmaxf(mx, fabsf(xv - mu));
            }
        }
    }
    const double d1 = ubpl::block_sum((double)s1, red);
    const double d2 = ubpl::block_sum((double)s2, red);
    const double N = (double)((int64_t)B * HW);
    if constexpr (!BOUND) {
        const double d[2] = {d1, d2};
        double t[2];
        if (!combine_slices<2, 0>(part, c, sp, gridDim.y, cnt, d, t) || threadIdx.x != 0) return;
        bwd_coeffs(o, c, t[0], t[1], N);
    } else {
        const double d[4] = {d1, d2, (double)ubpl::block_max(mg, redf), (double)ubpl::block_max(mx, redf)};
        double t[4];
        if (!combine_slices<2, 2>(part, c, sp, gridDim.y, cnt, d, t)) return;
        // wave 0 of the channel's last block (converged); lane 0 holds the totals
        const int lane = threadIdx.x;
        int tlast = 0;
        if (lane == 0) {
            const BwdCoef k = bwd_coeffs(o, c, t[0], t[1], N);
            // |dx| <= |a| max|g| + |b| max|x - mean| + |c|, 1 % over for the f32 rounding of dx
            const float bound = 1.01f * (fabsf(k.a) * (float)t[2] + fabsf(k.b) * (float)t[3] + fabsf(k.c));
            __hip_atomic_store(reinterpret_cast<unsigned*>(o.bnd + c), __float_as_uint(bound), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            tlast = last_arriver(o.tcnt, C) ? 1 : 0;
        }
        if (!__shfl(tlast, 0, 64)) return;
        // the tensor's last channel: max over every channel's bound -> the scale of dx
        float m = 0.f;
        for (int q = lane; q < C; q += 64)
            m = fmaxf(m, __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned*>(o.bnd + q),
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
        m = ubpl::wave_max(m);
        if (lane == 0) *o.dxscale = fp16_scale_for(m);
    }
}

// Backward statistics partials, per (channel c, 64-pixel slice q of the flat
// (b, p) range): part[(c*np + q)*2 + {0,1}] = (S1, S2) = (sum g, sum g*(x -
// mean)), the layout the conv epilogues write (common.h tile_bn_bwd_partials),
// combined by bn_bwd_finalize_kernel.  One wave per 4 x IT slices of one
// channel: lane l takes pixels 4l..4l+3 of a 256-pixel chunk (float4; P % 4 ==
// 0), a 16-lane row is one slice (DPP row sums).  (The default statistics path
// is bwd_stats_kernel above — one launch; a partials pass + finalize launch
// measured 0.7 % slower on the training step.)
template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_partials_kernel(const float* __restrict__ dz,
                                                             const float* __restrict__ x, int C, int P, int64_t N,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             const float* __restrict__ mean, int relu,
                                                             float* __restrict__ part) {
    constexpr int IT = 4;   // 256-pixel chunks (4 slices each) per wave
    const int64_t np = (N + 63) / 64, nw = (np + 4 * IT - 1) / (4 * IT);
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (int64_t)C * nw) return;
    const int lane = threadIdx.x & 63;
    const int c = (int)(w / nw);
    const int64_t u0 = (w - (int64_t)c * nw) * IT;
    const float sc = scale[c], sh = shift[c], mu = mean[c];
    float g[IT][4], xv[IT][4];
#pragma unroll
    for (int it = 0; it < IT; ++it) {   // all loads first
        const int64_t n0 = (u0 + it) * 256 + 4 * lane;
        if (VEC) {   // P % 4 == 0, 16-B aligned: the lane's 4 pixels are one float4 of one image
            const int64_t nc = n0 < N ? n0 : 0;
            const int64_t b = nc / P;
            const int64_t off = (b * C + c) * P + (nc - b * P);
            const float4 gv = *reinterpret_cast<const float4*>(dz + off);
            const float4 xq = *reinterpret_cast<const float4*>(x + off);
            g[it][0] = gv.x, g[it][1] = gv.y, g[it][2] = gv.z, g[it][3] = gv.w;
            xv[it][0] = xq.x, xv[it][1] = xq.y, xv[it][2] = xq.z, xv[it][3] = xq.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t nc = n0 + e < N ? n0 + e : 0;
                const int64_t b = nc / P;
                const int64_t off = (b * C + c) * P + (nc - b * P);
                g[it][e] = dz[off];
                xv[it][e] = x[off];
            }
        }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int64_t n0 = (u0 + it) * 256 + 4 * lane;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float ge = n0 + e < N ? g[it][e] : 0.f;
            if (relu && !(fmaf(xv[it][e], sc, sh) > 0.f)) ge = 0.f;
            s1 += ge;
            s2 = fmaf(ge, xv[it][e] - mu, s2);
        }
        s1 = ubpl::row_sum16(s1);
        s2 = ubpl::row_sum16(s2);
        const int64_t q = (u0 + it) * 4 + (lane >> 4);
        if ((lane & 15) == 15 && q < np) {
            part[((int64_t)c * np + q) * 2] = s1;
            part[((int64_t)c * np + q) * 2 + 1] = s2;
        }
    }
}

// Channel totals of the backward partials in f64 (fixed order): dgamma +=
// S2*invstd, dbeta += S1, and the coefficients of dx = a*g + b*(x - mean) + c.
__global__ void __launch_bounds__(FT) bn_bwd_finalize_kernel(const float* __restrict__ part, int64_t np, int64_t N,
                                                            BwdOut o) {
    __shared__ double red[16];
    const int c = blockIdx.x;
    const float2* pc = reinterpret_cast<const float2*>(part) + (int64_t)c * np;
    double t1 = 0.0, t2 = 0.0;
    for (int64_t q0 = 0; q0 < np; q0 += (int64_t)FT * NPT) {
        float2 v[NPT];
#pragma unroll
        for (int k = 0; k < NPT; ++k) {   // independent loads first
            const int64_t q = q0 + threadIdx.x + (int64_t)k * FT;
            v[k] = q < np ? pc[q] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            t1 += (double)v[k].x;
            t2 += (double)v[k].y;
        }
    }
    t1 = ubpl::block_sum(t1, red);
    t2 = ubpl::block_sum(t2, red);
    if (threadIdx.x != 0) return;
    bwd_coeffs(o, c, t1, t2, (double)N);
}

// The max-pool gradient's share of one float4 of dx: pd holds the two windows' gradients;
// the float4's elements that are their windows' argmax (max4's rule over the window in
// row-major order, the other row from the partner lane) take them, every other element
// adds 0.f, as maxpool_bwd_kernel's accumulate does (-0 + 0 = +0: bit-identical).
__device__ __forceinline__ void add_pool_grad(float4& v, float4 xv, int64_t off, PoolGeom g, float2 pd) {
    const float4 w = shfl_xor4(xv, 1 << g.lw4);
    const bool bot = (off >> g.lw4) & 1;
    const float4 t = bot ? w : xv, b = bot ? xv : w;
    int a0, a1;
    max4(t.x, t.y, b.x, b.y, a0);
    max4(t.z, t.w, b.z, b.w, a1);
    const int q = bot ? 2 : 0;
    v.x += a0 == q ? pd.x : 0.f;
    v.y += a0 == q + 1 ? pd.x : 0.f;
    v.z += a1 == q ? pd.y : 0.f;
    v.w += a1 == q + 1 ? pd.y : 0.f;
}

// What only the POOL apply kernels read: the gradient of y = maxpool2x2(x), [B,C,H/2,W/2],
// and the planes' geometry.
struct PoolGrad {
    const float* dy;
    PoolGeom g;
};

// dx = a*dyp + b*(x - mean) + c (+ add1) (+ add2).  HW % 4 == 0: float4 lanes, one channel
// per 4-vector.  total4 = B*C*HW/4.  POOL: + the max-pool gradient,
// dx = ((bn + add1) + pool) + add2, the order of ubpl_bn_backward(add1),
// ubpl_maxpool2x2_backward(accumulate) and ubpl_add.
template <bool POOL>
__global__ void __launch_bounds__(256) bwd_apply_vec_kernel(const float* dz, const float* __restrict__ x, int C,
                                                           int HW4, int64_t total4, const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const float* __restrict__ mean, int relu,
                                                           const float* __restrict__ ca,
                                                           const float* __restrict__ cb,
                                                           const float* __restrict__ cc, const float* add1,
                                                           const float* add2, float* dx, PoolGrad p) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += stride) {
        const int c = (int)((POOL ? i >> p.g.lhw4 : i / HW4) % C);
        const float sc = scale[c], sh = shift[c], mu = mean[c], a = ca[c], b = cb[c], cx = cc[c];
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        const float4 g = reinterpret_cast<const float4*>(dz)[i];
        float2 pd;
        if (POOL) pd = reinterpret_cast<const float2*>(p.dy)[half_index(i, p.g)];
        float4 v = bwd_one4(g, xv, sc, sh, mu, a, b, cx, relu);
        if (add1) add4(v, reinterpret_cast<const float4*>(add1)[i]);
        if (POOL) add_pool_grad(v, xv, i, p.g, pd);
        if (add2) add4(v, reinterpret_cast<const float4*>(add2)[i]);
        reinterpret_cast<float4*>(dx)[i] = v;
    }
}

// The same per (image, channel) plane (HW4 % 256 == 0: planes of 32x32 and up): grid
// (HW4 / (256 U), B*C), so the channel and its six coefficients are block-uniform (scalar
// loads, no per-element 64-bit index division) and each thread issues its U float4s of
// every operand before computing (dx may alias dz / add1 / add2: same elements).
// (Against the grid-stride kernel above on these planes: profiles/r05_v2_bn_plane.txt.)
template <bool POOL, int U>
__global__ void __launch_bounds__(256) bwd_apply_plane_kernel(const float* dz, const float* __restrict__ x, int C,
                                                             int HW4, const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             const float* __restrict__ mean, int relu,
                                                             const float* __restrict__ ca,
                                                             const float* __restrict__ cb,
                                                             const float* __restrict__ cc, const float* add1,
                                                             const float* add2, float* dx, PoolGrad p) {
    const int pl = blockIdx.y;
    const int c = pl % C;
    const float sc = scale[c], sh = shift[c], mu = mean[c], a = ca[c], b = cb[c], cx = cc[c];
    const int64_t base = (int64_t)pl * HW4 + blockIdx.x * (256 * U) + threadIdx.x;
    const float4* x4 = reinterpret_cast<const float4*>(x) + base;
    const float4* d4 = reinterpret_cast<const float4*>(dz) + base;
    float4 xv[U], g[U], q1[U], q2[U];
    float2 pd[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        xv[u] = x4[u * 256];
        g[u] = d4[u * 256];
        if (POOL) pd[u] = reinterpret_cast<const float2*>(p.dy)[half_index(base + u * 256, p.g)];
        if (add1) q1[u] = reinterpret_cast<const float4*>(add1)[base + u * 256];
        if (add2) q2[u] = reinterpret_cast<const float4*>(add2)[base + u * 256];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float4 v = bwd_one4(g[u], xv[u], sc, sh, mu, a, b, cx, relu);
        if (add1) add4(v, q1[u]);
        if (POOL) add_pool_grad(v, xv[u], base + u * 256, p.g, pd[u]);
        if (add2) add4(v, q2[u]);
        reinterpret_cast<float4*>(dx)[base + u * 256] = v;
    }
}

__global__ void __launch_bounds__(256) bwd_apply_kernel(const float* dz, const float* __restrict__ x, int C, int HW,
                                                       int64_t total, const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const float* __restrict__ mean, int relu,
                                                       const float* __restrict__ ca, const float* __restrict__ cb,
                                                       const float* __restrict__ cc, const float* add1,
                                                       const float* add2, float* dx) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = (int)((i / HW) % C);
        float v = bwd_one(dz[i], x[i], scale[c], shift[c], mean[c], ca[c], cb[c], cc[c], relu);
        if (add1) v += add1[i];
        if (add2) v += add2[i];
        dx[i] = v;
    }
}

// dx of the BN backward written straight into the PSA layout (conv_psa.hip
// split_act_kernel's [B][C/16][H+2pad][W+2pad][16] bf16 planes, zero border):
// one thread per padded pixel of one 16-channel group, like split_act.
template <int NP>
__global__ void __launch_bounds__(256) bwd_apply_split_kernel(const float* __restrict__ dz,
                                                             const float* __restrict__ x, int C, int H, int W,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             const float* __restrict__ mean, int relu,
                                                             const float* __restrict__ ca,
                                                             const float* __restrict__ cb,
                                                             const float* __restrict__ cc, int pad,
                                                             uint16_t* __restrict__ dst, int64_t plane,
                                                             const float* __restrict__ dxscale) {
    // NP = 2 (2xfp16): the pieces of dx * (*dxscale), the power of two the statistics chose
    const int Hp = H + 2 * pad, Wp = W + 2 * pad, G = C >> 4;
    const int b = blockIdx.z, g = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= Hp * Wp) return;
    const int hp = pix / Wp, wq = pix - hp * Wp;
    const int h = hp - pad, w = wq - pad;
    const bool in = h >= 0 && h < H && w >= 0 && w < W;
    const int64_t HW = (int64_t)H * W;
    const int64_t o = ((int64_t)b * C + 16 * g) * HW + (in ? h * W + w : 0);
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = 16 * g + j;
        const float r = bwd_one(dz[o + j * HW], x[o + j * HW], scale[c], shift[c], mean[c], ca[c], cb[c], cc[c], relu);
        v[j] = in ? r : 0.f;
    }
    ubpl::store_psa_row<NP>(v, dst + (((int64_t)(b * G + g) * Hp + hp) * Wp + wq) * 16, plane,
                            NP == 2 ? *dxscale : 1.f);
}

// statistics -> coefficients (coef: ca | cb | cc, C floats each): the f64 finalize of the
// partials the producer's epilogue wrote (part != nullptr), or one bwd_stats_kernel
// launch.  bound: also the 2xfp16 scale of dx at coef[3C] (bwd_stats_kernel BOUND; coef:
// 3C + 1 floats), not to be had from partials.
int bwd_stats(const float* dz, const float* x, int B, int C, int HW, const float* gamma, const float* mean,
              const float* invstd, const float* scale, const float* shift, int relu, double* scratch,
              const float* part, float* coef, float* dgamma, float* dbeta, hipStream_t st, bool bound = false) {
    BwdOut o{gamma, invstd, dgamma, dbeta, coef, coef + C, coef + 2 * C, nullptr, nullptr, nullptr};
    if (part != nullptr) {
        if (bound) return (int)hipErrorInvalidValue;
        const int64_t N = (int64_t)B * HW;
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(FT), 0, st, part, (N + 63) / 64, N, o);
        UBPL_LAUNCH_CHECK();
        return 0;
    }
    if (C > MAXBN || scratch == nullptr) return (int)hipErrorInvalidValue;
    int bper, gs;
    stats_grid(B, C, HW, bper, gs);
    const Scratch s = carve(scratch);
    if (bound) {
        o.bnd = s.bnd;
        o.tcnt = s.tcnt;
        o.dxscale = coef + 3 * C;
    }
    const bool vec = (HW % 4 == 0) && ((((uintptr_t)dz | (uintptr_t)x) & 15) == 0);
    return pick(
        [&](auto VEC, auto BOUND) {
            hipLaunchKernelGGL((bwd_stats_kernel<VEC != 0, BOUND != 0>), dim3(C, gs), dim3(256), 0, st, dz, x, B, C,
                               HW, bper, scale, shift, mean, relu, s.slab, s.cnt, o);
            UBPL_LAUNCH_CHECK();
            return 0;
        },
        among<0, 1>{vec}, among<0, 1>{bound});
}

// The f32 apply on float4s (HW % 4 == 0, every operand 16-byte aligned): the plane kernel
// where a plane is whole 256-float4 rows, the grid-stride one elsewhere.
template <bool POOL>
int launch_apply4(const float* dz, const float* x, int B, int C, int HW, const float* scale, const float* shift,
                  const float* mean, int relu, const float* coef, const float* add1, const float* add2, float* dx,
                  PoolGrad p, hipStream_t st) {
    const float *ca = coef, *cb = coef + C, *cc = coef + 2 * C;
    const int hw4 = HW / 4;
    if (hw4 % 256 != 0 || (int64_t)B * C >= 65536) {
        const int64_t total4 = (int64_t)B * C * hw4;
        hipLaunchKernelGGL(bwd_apply_vec_kernel<POOL>, dim3(grid_ew(total4)), dim3(256), 0, st, dz, x, C, hw4, total4,
                           scale, shift, mean, relu, ca, cb, cc, add1, add2, dx, p);
        UBPL_LAUNCH_CHECK();
        return 0;
    }
    const int u = hw4 % 1024 == 0 ? 4 : (hw4 % 512 == 0 ? 2 : 1);
    return pick(
        [&](auto U) {
            hipLaunchKernelGGL((bwd_apply_plane_kernel<POOL, U>), dim3((unsigned)(hw4 / (256 * U)), (unsigned)(B * C)),
                               dim3(256), 0, st, dz, x, C, hw4, scale, shift, mean, relu, ca, cb, cc, add1, add2, dx,
                               p);
            UBPL_LAUNCH_CHECK();
            return 0;
        },
        among<4, 2, 1>{u});
}

}  // namespace

// Backward statistics partials of dz (ReLU mask from x's BN) alone: the layout
// ubpl_bn_backward's `part` takes; part: ubpl_bn_partial_floats(C, B*HW) floats.
UBPL_API int ubpl_bn_backward_partials(const float* dz, const float* x, int B, int C, int HW, const float* scale,
                                       const float* shift, const float* mean, int relu, float* part, void* stream) {
    const int64_t N = (int64_t)B * HW;
    const int64_t np = (N + 63) / 64;
    const bool vec = (HW % 4 == 0) && ((((uintptr_t)dz | (uintptr_t)x) & 15) == 0);
    const int64_t waves = (int64_t)C * ((np + 15) / 16);
    return pick(
        [&](auto VEC) {
            hipLaunchKernelGGL(bn_bwd_partials_kernel<VEC != 0>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0,
                               (hipStream_t)stream, dz, x, C, HW, N, scale, shift, mean, relu, part);
            UBPL_LAUNCH_CHECK();
            return 0;
        },
        among<0, 1>{vec});
}

// ubpl_bn_backward with dx delivered as PSA planes only (no f32 dx, no
// addends): statistics, then bwd_apply_split_kernel.  C % 16 == 0.
UBPL_API int ubpl_bn_backward_split(const float* dz, const float* x, int B, int C, int H, int W, const float* gamma,
                                    const float* mean, const float* invstd, const float* scale, const float* shift,
                                    int relu, double* scratch, const float* part, float* coef, float* dgamma,
                                    float* dbeta, int pad, int npieces, uint16_t* dst, int64_t plane, void* stream) {
    const int HW = H * W;
    if (C % 16 != 0 || npieces < 1 || npieces > 3 || pad < 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    // npieces 2 (2xfp16): dx scaled by the power of two its bound asks for (coef[3C]: coef holds 3C + 1 floats)
    const int e = bwd_stats(dz, x, B, C, HW, gamma, mean, invstd, scale, shift, relu, scratch, part, coef, dgamma,
                            dbeta, st, npieces == 2);
    if (e) return e;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    return pick(
        [&](auto NP) {
            hipLaunchKernelGGL(bwd_apply_split_kernel<NP>,
                               dim3((unsigned)((Hp * Wp + 255) / 256), (unsigned)(C / 16), (unsigned)B), dim3(256), 0,
                               st, dz, x, C, H, W, scale, shift, mean, relu, coef, coef + C, coef + 2 * C, pad, dst,
                               plane, coef + 3 * C);
            UBPL_LAUNCH_CHECK();
            return 0;
        },
        among<1, 2, 3>{npieces});
}

// dx = BatchNorm(+ReLU) backward of dz (+ add1 + add2; both nullable; dx may alias dz,
// add1 or add2), dgamma/dbeta ACCUMULATED (+=); statistics by one bwd_stats_kernel launch
// over `scratch` (ubpl_bn_part_doubles, zeroed before first use), or — part != nullptr —
// from the backward partials dz's producer wrote (then only the f64 finalize runs);
// coef: scratch of 3*C floats.
UBPL_API int ubpl_bn_backward(const float* dz, const float* x, int B, int C, int HW, const float* gamma,
                              const float* mean, const float* invstd, const float* scale, const float* shift,
                              int relu, double* scratch, const float* part, float* coef, float* dgamma,
                              float* dbeta, const float* add1, const float* add2, float* dx, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int e = bwd_stats(dz, x, B, C, HW, gamma, mean, invstd, scale, shift, relu, scratch, part, coef, dgamma,
                            dbeta, st);
    if (e) return e;
    const uintptr_t al = (uintptr_t)dz | (uintptr_t)x | (uintptr_t)dx | (uintptr_t)add1 | (uintptr_t)add2;
    if (HW % 4 == 0 && (al & 15) == 0)
        return launch_apply4<false>(dz, x, B, C, HW, scale, shift, mean, relu, coef, add1, add2, dx, PoolGrad{}, st);
    const int64_t total = (int64_t)B * C * HW;
    hipLaunchKernelGGL(bwd_apply_kernel, dim3(grid_ew(total)), dim3(256), 0, st, dz, x, C, HW, total, scale, shift,
                       mean, relu, coef, coef + C, coef + 2 * C, add1, add2, dx);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// ubpl_bn_backward of x [B,C,H,W] with the gradient of y = maxpool2x2(x) folded into the
// apply: dx = ((dL/dx + add1) + maxpool2x2_backward(x, pool_dy)) + add2, bit-identical to
// ubpl_bn_backward(add1), ubpl_maxpool2x2_backward(accumulate) and ubpl_add in turn.
// pool_dy [B,C,H/2,W/2] null: ubpl_bn_backward.  With it: geometry as
// ubpl_bn_forward_stats_maxpool's, every f32 operand 16-byte and pool_dy 8-byte aligned.
UBPL_API int ubpl_bn_backward_pool(const float* dz, const float* x, int B, int C, int H, int W, const float* gamma,
                                   const float* mean, const float* invstd, const float* scale, const float* shift,
                                   int relu, double* scratch, const float* part, float* coef, float* dgamma,
                                   float* dbeta, const float* add1, const float* pool_dy, const float* add2,
                                   float* dx, void* stream) {
    const int HW = H * W;
    if (pool_dy == nullptr)
        return ubpl_bn_backward(dz, x, B, C, HW, gamma, mean, invstd, scale, shift, relu, scratch, part, coef, dgamma,
                                dbeta, add1, add2, dx, stream);
    PoolGrad p{pool_dy, {}};
    const uintptr_t al = (uintptr_t)dz | (uintptr_t)x | (uintptr_t)dx | (uintptr_t)add1 | (uintptr_t)add2;
    if (B < 1 || C < 1 || !pool_geom(H, W, p.g) || (al & 15) || (((uintptr_t)pool_dy) & 7))
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int e = bwd_stats(dz, x, B, C, HW, gamma, mean, invstd, scale, shift, relu, scratch, part, coef, dgamma,
                            dbeta, st);
    if (e) return e;
    return launch_apply4<true>(dz, x, B, C, HW, scale, shift, mean, relu, coef, add1, add2, dx, p, st);
}
