// BatchNorm2d, the forward side (overview: bn.h): the one-launch train-mode statistics —
// plain, with the max-pool, with the upsample-add — the eval-mode coefficients, the
// stand-alone apply, and the statistics from 64-pixel partials.
#include "bn.h"

namespace {

// float4 loads a statistics thread keeps in flight (8 measured 0 - 0.6 us per launch faster,
// less than the training step's spread: profiles/r05_v11_bn_stats.txt)
constexpr int U = 4;

// One (channel c, batch slice) per block over the flattened (b, pixel) range:
// sum and sum of squares of (x - x0), x0 = x[0, c, 0]; f32 per thread, f64
// across the block and the slices.  The last block of channel c finalizes it.
template <bool VEC>
__global__ void __launch_bounds__(256) stats_kernel(const float* __restrict__ x, int B, int C, int HW, int bper,
                                                   double* __restrict__ part, unsigned* __restrict__ cnt,
                                                   StatsOut o) {
    __shared__ double red[16];
    const int c = blockIdx.x, sp = blockIdx.y;
    const int b0 = sp * bper, b1 = min(B, b0 + bper);
    const float x0 = x[(int64_t)c * HW];
    float s1 = 0.f, s2 = 0.f;
    if (VEC) {
        // one accumulator, elements in the flattened loop's order (bit-identical
        // statistics); only the loads run ahead
        const float4* x4 = reinterpret_cast<const float4*>(x);
        visit_chan4<U>(b0, b1, C, c, HW >> 2, [&](int, int64_t off) { acc_shifted(x4[off], x0, s1, s2); });
    } else {
        const int n = (b1 - b0) * HW;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int bb = i / HW, o1 = i - bb * HW;
            const float a = x[((int64_t)(b0 + bb) * C + c) * HW + o1] - x0;
            s1 += a;
            s2 = fmaf(a, a, s2);
        }
    }
    const double d[2] = {ubpl::block_sum((double)s1, red), ubpl::block_sum((double)s2, red)};
    double t[2];
    if (!combine_slices<2, 0>(part, c, sp, gridDim.y, cnt, d, t) || threadIdx.x != 0) return;
    finalize_stats(o, c, x0, t[0], t[1], (int64_t)B * HW);
}

// stats_kernel<true> over x (same elements per thread, same order: the statistics of x are
// bit-identical; `o` unused when o.scale is null) which also writes y = maxpool2x2(x) and
// accumulates the statistics of y for the BatchNorm `op` that consumes it: the thread
// holding the top row of two windows takes the bottom row from its partner lane, writes the
// two maxima (one float2) and adds them to its sums of (y - y0) and (y - y0)^2, y0 = y[0, c, 0],
// left window then right, in its visiting order; f64 across the block and the slices like
// x's sums.  The channel's last block finalizes both BatchNorms from the one ticket.
__global__ void __launch_bounds__(256) stats_maxpool_kernel(const float* __restrict__ x, int B, int C, int HW,
                                                           int bper, PoolGeom g, float* __restrict__ y,
                                                           double* __restrict__ part, unsigned* __restrict__ cnt,
                                                           StatsOut o, StatsOut op) {
    __shared__ double red[16];
    const int c = blockIdx.x, sp = blockIdx.y;
    const int b0 = sp * bper, b1 = min(B, b0 + bper);
    const float* xc = x + (int64_t)c * HW;
    const float x0 = xc[0];
    const int W = 4 << g.lw4, w4 = 1 << g.lw4;
    int am;
    const float y0 = max4(xc[0], xc[1], xc[W], xc[W + 1], am);
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float2* y2 = reinterpret_cast<float2*>(y);
    visit_chan4<U>(b0, b1, C, c, HW >> 2, [&](int, int64_t off) {
        const float4 v = x4[off];
        acc_shifted(v, x0, s1, s2);
        const float4 w = shfl_xor4(v, w4);
        if (!((off >> g.lw4) & 1)) {   // an even row: the top halves
            int t;
            const float m0 = max4(v.x, v.y, w.x, w.y, t), m1 = max4(v.z, v.w, w.z, w.w, t);
            y2[half_index(off, g)] = make_float2(m0, m1);
            const float e = m0 - y0, f = m1 - y0;
            s3 += e + f;
            s4 = fmaf(e, e, fmaf(f, f, s4));
        }
    });
    const double d[4] = {ubpl::block_sum((double)s1, red), ubpl::block_sum((double)s2, red),
                         ubpl::block_sum((double)s3, red), ubpl::block_sum((double)s4, red)};
    double t[4];
    if (!combine_slices<4, 0>(part, c, sp, gridDim.y, cnt, d, t) || threadIdx.x != 0) return;
    if (o.scale) finalize_stats(o, c, x0, t[0], t[1], (int64_t)B * HW);
    if (op.scale) finalize_stats(op, c, y0, t[2], t[3], (int64_t)B * (HW >> 2));
}

// upadd_fwd_vec_kernel's sum, out = up + upsample2x(low), on stats_kernel<true>'s grid and
// in its visiting order, followed by the statistics of out for the BatchNorm that consumes
// it: bit-identical to the two launches.  out may be up (each float4 read, then written, by
// one thread).  x0 = out[0, c, 0] is computed by every block from up and low; so that no
// block reads up[0, c, 0] after an in-place store, the float4 holding it is stored by the
// channel's last block, after the ticket (every block's x0 load has returned by then: its
// published sums depend on it).
__global__ void __launch_bounds__(256) upadd_stats_kernel(const float* up, const float* __restrict__ low, int B,
                                                         int C, int HW, int bper, PoolGeom g, float* out,
                                                         double* __restrict__ part, unsigned* __restrict__ cnt,
                                                         StatsOut o) {
    __shared__ double red[16];
    const int c = blockIdx.x, sp = blockIdx.y;
    const int b0 = sp * bper, b1 = min(B, b0 + bper);
    const int hw4 = HW >> 2;
    const int64_t first = (int64_t)c * hw4;   // the float4 of out[0, c, 0]
    const float x0 = up[(int64_t)c * HW] + low[(int64_t)c * hw4];
    float s1 = 0.f, s2 = 0.f;
    const float4* u4 = reinterpret_cast<const float4*>(up);
    const float2* l2 = reinterpret_cast<const float2*>(low);
    float4* o4 = reinterpret_cast<float4*>(out);
    auto sum_at = [&](int64_t off) {
        const float4 u = u4[off];
        const float2 l = l2[half_index(off, g)];
        return make_float4(u.x + l.x, u.y + l.x, u.z + l.y, u.w + l.y);
    };
    visit_chan4<U>(b0, b1, C, c, hw4, [&](int, int64_t off) {
        const float4 v = sum_at(off);
        if (off != first) o4[off] = v;
        acc_shifted(v, x0, s1, s2);
    });
    const double d[2] = {ubpl::block_sum((double)s1, red), ubpl::block_sum((double)s2, red)};
    double t[2];
    if (!combine_slices<2, 0>(part, c, sp, gridDim.y, cnt, d, t) || threadIdx.x != 0) return;
    o4[first] = sum_at(first);
    finalize_stats(o, c, x0, t[0], t[1], (int64_t)B * HW);
}

// Eval-mode scale / shift of one channel (one expression for both kernels below: the same rounding)
__device__ __forceinline__ void eval_coeff(float gamma, float beta, float rmean, float rvar, float eps, float& scale,
                                           float& shift) {
    const float invstd = (float)(1.0 / sqrt((double)rvar + (double)eps));
    const float sc = invstd * gamma;
    scale = sc;
    shift = beta - rmean * sc;
}

__global__ void eval_coeff_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                  const float* __restrict__ rmean, const float* __restrict__ rvar, float eps, int C,
                                  float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    eval_coeff(gamma[c], beta[c], rmean[c], rvar[c], eps, scale[c], shift[c]);
}

// The same for every BatchNorm of a network: one workgroup per row of `table`
// (gamma_off, beta_off, rmean_off, rvar_off, coef_off, C), see ubpl_bn_eval_coeffs_table.
__global__ void __launch_bounds__(256) eval_coeff_table_kernel(const float* __restrict__ params,
                                                              const float* __restrict__ stats,
                                                              const int64_t* __restrict__ table, float eps,
                                                              float* __restrict__ coef) {
    const int64_t* t = table + (int64_t)blockIdx.x * 6;
    const float* gamma = params + t[0];
    const float* beta = params + t[1];
    const float* rmean = stats + t[2];
    const float* rvar = stats + t[3];
    const int C = (int)t[5];
    float* scale = coef + t[4];
    float* shift = scale + C;
    for (int c = threadIdx.x; c < C; c += blockDim.x)
        eval_coeff(gamma[c], beta[c], rmean[c], rvar[c], eps, scale[c], shift[c]);
}

__global__ void __launch_bounds__(256) apply_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                   const float* __restrict__ shift, int C, int HW, int64_t total4,
                                                   int relu, float* __restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int hw4 = HW >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += stride) {
        const int c = (int)((i / hw4) % C);
        const float sc = scale[c], sh = shift[c];
        float4 v = reinterpret_cast<const float4*>(x)[i];
        v.x = fmaf(v.x, sc, sh);
        v.y = fmaf(v.y, sc, sh);
        v.z = fmaf(v.z, sc, sh);
        v.w = fmaf(v.w, sc, sh);
        if (relu) {
            v.x = fmaxf(v.x, 0.f);
            v.y = fmaxf(v.y, 0.f);
            v.z = fmaxf(v.z, 0.f);
            v.w = fmaxf(v.w, 0.f);
        }
        reinterpret_cast<float4*>(y)[i] = v;
    }
}

// ---- statistics from 64-pixel partials (conv-epilogue fused: common.h
// tile_bn_partials; or bn_partials_kernel below).  part [C][np][2] f32 =
// (S, M2) per slice, Chan's parallel form.
// One wave per (channel, 64-pixel slice): lane = pixel (coalesced along p),
// S and M2 by wave reductions.  4 waves per block.
__global__ void __launch_bounds__(256) bn_partials_kernel(const float* __restrict__ y, int C, int P, int64_t N,
                                                         float* __restrict__ part) {
    const int64_t np = (N + 63) / 64;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // (c, q)
    if (w >= (int64_t)C * np) return;
    const int lane = threadIdx.x & 63;
    const int c = (int)(w / np);
    const int64_t q = w - (int64_t)c * np;
    const int64_t n = q * 64 + lane;
    const bool ok = n < N;
    const int64_t nc = ok ? n : N - 1;
    const int64_t b = nc / P;
    const float v = y[(b * C + c) * P + (nc - b * P)];
    const float cnt = (float)(N - q * 64 < 64 ? N - q * 64 : 64);
    const float s = ubpl::wave_sum(ok ? v : 0.f);
    const float d = ok ? v - s / cnt : 0.f;
    const float m2 = ubpl::wave_sum(d * d);
    if (lane == 0) {
        part[w * 2] = s;
        part[w * 2 + 1] = m2;
    }
}

// mean = sum S / N; M2 = sum M2_q + sum n_q (S_q/n_q - mean)^2, in f64.
__global__ void __launch_bounds__(FT) bn_finalize_partials_kernel(const float* __restrict__ part, int64_t np,
                                                                 int64_t N, StatsOut o) {
    __shared__ double red[16];
    const int c = blockIdx.x;
    const float2* pc = reinterpret_cast<const float2*>(part) + (int64_t)c * np;
    auto nq_of = [&](int64_t q) { return (double)(N - q * 64 < 64 ? N - q * 64 : 64); };
    double t1 = 0.0;
    float2 v[NPT];   // the first FT*NPT slices stay in registers for the second pass
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int64_t q = threadIdx.x + (int64_t)k * FT;
        v[k] = q < np ? pc[q] : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k) t1 += (double)v[k].x;
    for (int64_t q0 = (int64_t)FT * NPT; q0 < np; q0 += (int64_t)FT * NPT) {
        float w[NPT];
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int64_t q = q0 + threadIdx.x + (int64_t)k * FT;
            w[k] = q < np ? pc[q].x : 0.f;
        }
#pragma unroll
        for (int k = 0; k < NPT; ++k) t1 += (double)w[k];
    }
    t1 = ubpl::block_sum(t1, red);
    const double mean = t1 / (double)N;
    double t2 = 0.0;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int64_t q = threadIdx.x + (int64_t)k * FT;
        if (q < np) {
            const double nq = nq_of(q);
            const double dm = (double)v[k].x / nq - mean;
            t2 += (double)v[k].y + nq * dm * dm;
        }
    }
    for (int64_t q0 = (int64_t)FT * NPT; q0 < np; q0 += (int64_t)FT * NPT) {
        float2 w[NPT];
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int64_t q = q0 + threadIdx.x + (int64_t)k * FT;
            w[k] = q < np ? pc[q] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int64_t q = q0 + threadIdx.x + (int64_t)k * FT;
            if (q < np) {
                const double nq = nq_of(q);
                const double dm = (double)w[k].x / nq - mean;
                t2 += (double)w[k].y + nq * dm * dm;
            }
        }
    }
    t2 = ubpl::block_sum(t2, red);
    if (threadIdx.x != 0) return;
    write_stats(o, c, mean, t2 / (double)N, N);
}

}  // namespace

// Doubles of the statistics scratch (bn.h: the layout), the same for every B and C.
UBPL_API int64_t ubpl_bn_part_doubles(int B, int C) {
    (void)B;
    (void)C;
    return PART_DOUBLES;
}

// Train-mode statistics of x [B,C,H,W] -> mean, invstd, (scale, shift) and the
// running-stat update (rmean/rvar nullable: track_running_stats off).
UBPL_API int ubpl_bn_forward_stats(const float* x, int B, int C, int HW, const float* gamma, const float* beta,
                                   float eps, float momentum, float* rmean, float* rvar, double* part,
                                   float* mean_out, float* invstd_out, float* scale, float* shift, void* stream) {
    if (C > MAXBN) return (int)hipErrorInvalidValue;
    int bper, gs;
    stats_grid(B, C, HW, bper, gs);
    const Scratch s = carve(part);
    const StatsOut o{gamma, beta, eps, momentum, rmean, rvar, mean_out, invstd_out, scale, shift};
    const bool vec = (HW % 4 == 0) && (((uintptr_t)x & 15) == 0);
    return pick(
        [&](auto VEC) {
            hipLaunchKernelGGL(stats_kernel<VEC != 0>, dim3(C, gs), dim3(256), 0, (hipStream_t)stream, x, B, C, HW,
                               bper, s.slab, s.cnt, o);
            UBPL_LAUNCH_CHECK();
            return 0;
        },
        among<0, 1>{vec});
}

// ubpl_bn_forward_stats(x) for the BatchNorm of (gamma, beta, ...) — all eight null: no
// BatchNorm on x — with y = maxpool2x2(x) [B,C,H/2,W/2] and the statistics of y for the
// BatchNorm of (pgamma, pbeta, ...) — all eight null: not wanted — from the same launch.  H a power of two, W/4 a power
// of two <= 32, C <= 512, x 16-byte and y 8-byte aligned; anything else is refused.
UBPL_API int ubpl_bn_forward_stats_maxpool(const float* x, int B, int C, int H, int W, float* y, const float* gamma,
                                           const float* beta, float* rmean, float* rvar, float* mean_out,
                                           float* invstd_out, float* scale, float* shift, const float* pgamma,
                                           const float* pbeta, float* prmean, float* prvar, float* pmean_out,
                                           float* pinvstd_out, float* pscale, float* pshift, float eps,
                                           float momentum, double* part, void* stream) {
    PoolGeom g;
    if (B < 1 || C < 1 || C > MAXBN || !pool_geom(H, W, g) || (((uintptr_t)x) & 15) || (((uintptr_t)y) & 7) ||
        part == nullptr || y == nullptr)
        return (int)hipErrorInvalidValue;
    const bool own = scale != nullptr;
    if (own ? !(gamma && beta && mean_out && invstd_out && shift) : (gamma || beta || rmean || rvar || mean_out ||
                                                                    invstd_out || shift) != 0)
        return (int)hipErrorInvalidValue;
    if (pscale ? !(pgamma && pbeta && pmean_out && pinvstd_out && pshift) : (pgamma || pbeta || prmean || prvar ||
                                                                             pmean_out || pinvstd_out || pshift) != 0)
        return (int)hipErrorInvalidValue;
    int bper, gs;
    stats_grid(B, C, H * W, bper, gs);
    const Scratch s = carve(part);
    const StatsOut o{gamma, beta, eps, momentum, rmean, rvar, mean_out, invstd_out, scale, shift};
    const StatsOut op{pgamma, pbeta, eps, momentum, prmean, prvar, pmean_out, pinvstd_out, pscale, pshift};
    hipLaunchKernelGGL(stats_maxpool_kernel, dim3(C, gs), dim3(256), 0, (hipStream_t)stream, x, B, C, H * W, bper, g,
                       y, s.slab, s.cnt, o, op);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// out = up + upsample2x(low) (ubpl_upsample2x_add_forward; out may be up) and
// ubpl_bn_forward_stats(out) in one launch, both bit-identical.  Geometry as above; up /
// out 16-byte, low 8-byte aligned.
UBPL_API int ubpl_upsample2x_add_forward_bnstats(const float* up, const float* low, int B, int C, int H, int W,
                                                 float* out, const float* gamma, const float* beta, float eps,
                                                 float momentum, float* rmean, float* rvar, double* part,
                                                 float* mean_out, float* invstd_out, float* scale, float* shift,
                                                 void* stream) {
    PoolGeom g;
    if (B < 1 || C < 1 || C > MAXBN || !pool_geom(H, W, g) || ((((uintptr_t)up) | ((uintptr_t)out)) & 15) ||
        (((uintptr_t)low) & 7) || part == nullptr || out == nullptr)
        return (int)hipErrorInvalidValue;
    if (!(gamma && beta && mean_out && invstd_out && scale && shift)) return (int)hipErrorInvalidValue;
    int bper, gs;
    stats_grid(B, C, H * W, bper, gs);
    const Scratch s = carve(part);
    const StatsOut o{gamma, beta, eps, momentum, rmean, rvar, mean_out, invstd_out, scale, shift};
    hipLaunchKernelGGL(upadd_stats_kernel, dim3(C, gs), dim3(256), 0, (hipStream_t)stream, up, low, B, C, H * W, bper,
                       g, out, s.slab, s.cnt, o);
    UBPL_LAUNCH_CHECK();
    return 0;
}

UBPL_API int ubpl_bn_eval_coeffs(const float* gamma, const float* beta, const float* rmean, const float* rvar,
                                 float eps, int C, float* scale, float* shift, void* stream) {
    hipLaunchKernelGGL(eval_coeff_kernel, dim3(ubpl::cdiv(C, 64)), dim3(64), 0, (hipStream_t)stream, gamma, beta,
                       rmean, rvar, eps, C, scale, shift);
    UBPL_LAUNCH_CHECK();
    return 0;
}

UBPL_API int ubpl_bn_eval_coeffs_table(const float* params, const float* stats, const int64_t* table, int nbn,
                                       float eps, float* coef, void* stream) {
    if (nbn < 0) return (int)hipErrorInvalidValue;
    if (nbn == 0) return 0;
    hipLaunchKernelGGL(eval_coeff_table_kernel, dim3(nbn), dim3(256), 0, (hipStream_t)stream, params, stats, table,
                       eps, coef);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// y = [relu](x*scale + shift); HW must be a multiple of 4, x/y 16-B aligned.
UBPL_API int ubpl_bn_apply(const float* x, int B, int C, int HW, const float* scale, const float* shift, int relu,
                           float* y, void* stream) {
    if ((HW & 3) || (((uintptr_t)x | (uintptr_t)y) & 15)) return (int)hipErrorInvalidValue;
    const int64_t total4 = (int64_t)B * C * HW / 4;
    hipLaunchKernelGGL(apply_kernel, dim3(grid_ew(total4)), dim3(256), 0, (hipStream_t)stream, x, scale, shift, C, HW,
                       total4, relu, y);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// Floats of a partial-statistics buffer for C channels over N = B*P pixels.
UBPL_API int64_t ubpl_bn_partial_floats(int C, int64_t N) { return 2 * (int64_t)C * ((N + 63) / 64); }

// part [C][ceil(N/64)][2] = per 64-pixel slice (S, M2) of y [B,C,P]: the layout
// conv epilogues produce themselves.
UBPL_API int ubpl_bn_partials(const float* y, int B, int C, int P, float* part, void* stream) {
    const int64_t N = (int64_t)B * P;
    const int64_t n = (int64_t)C * ((N + 63) / 64);
    hipLaunchKernelGGL(bn_partials_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, y, C,
                       P, N, part);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// Train-mode BatchNorm statistics from partials (outputs as ubpl_bn_forward_stats).
UBPL_API int ubpl_bn_stats_from_partials(const float* part, int C, int64_t N, const float* gamma,
                                         const float* beta, float eps, float momentum, float* rmean, float* rvar,
                                         float* mean_out, float* invstd_out, float* scale, float* shift_out,
                                         void* stream) {
    StatsOut o{gamma, beta, eps, momentum, rmean, rvar, mean_out, invstd_out, scale, shift_out};
    hipLaunchKernelGGL(bn_finalize_partials_kernel, dim3(C), dim3(FT), 0, (hipStream_t)stream, part,
                       (N + 63) / 64, N, o);
    UBPL_LAUNCH_CHECK();
    return 0;
}
