// The deterministic reduces of the convolutions' split slabs: the split-K reduce of every
// forward path (f32 and split precisions: ubpl::launch_split_reduce) and the weight-gradient
// slab reduce (ubpl_wgrad_slab_reduce).
#include "common.h"

namespace {

// y[b,m,p] = sum_z slab[z][m][b*P+p] + bias[m] (+ res)
__global__ void __launch_bounds__(256) split_reduce_kernel(const float* __restrict__ slab, int splits, int Cout, int P,
                                                          int64_t N, const float* __restrict__ bias, const float* res,
                                                          float* y) {
    const int64_t total = (int64_t)Cout * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        // i enumerates the output in NCHW order: i = (b*Cout + m)*P + p
        const int p = (int)(i % P);
        const int64_t t = i / P;
        const int m = (int)(t % Cout);
        const int64_t b = t / Cout;
        const int64_t n = b * P + p;
        float s = 0.f;
        for (int z = 0; z < splits; ++z) s += slab[((int64_t)z * Cout + m) * N + n];
        if (bias) s += bias[m];
        if (res) s += res[i];
        y[i] = s;
    }
}

// slab columns are tap-major (n = tap*Cin + ci); dw is the reference layout
// [Cout][Cin][KS][KS] (ci*KS*KS + tap).  R split-lanes per output element
// (256/R elements per block) sum interleaved splits with two accumulators;
// the R partials are combined in a fixed order (deterministic).  The sums are
// f64, rounded once: with hundreds of splits (the 1x1 weight gradients over
// 128x128 planes: K = B*16384 pixels in 8-step slices) an f32 sum of the
// partials would add more rounding than the slices themselves carry.
template <int R>
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ slab, int splits, int Cout,
                                                          int Cin, int T, int with_bias, float* __restrict__ dw,
                                                          float* __restrict__ db, int accumulate) {
    constexpr int C = 256 / R;
    __shared__ double red[R][C];
    const int Ntot = Cin * T;
    const int Nt = Ntot + 1;
    const int64_t total = (int64_t)Cout * Nt;
    const int c = threadIdx.x % C, r = threadIdx.x / C;
    for (int64_t i0 = (int64_t)blockIdx.x * C; i0 < total; i0 += (int64_t)gridDim.x * C) {
        const int64_t i = i0 + c;
        const int64_t ic = i < total ? i : total - 1;
        double s0 = 0.0, s1 = 0.0;
        int z = r;
        for (; z + R < splits; z += 2 * R) {
            s0 += (double)slab[(int64_t)z * total + ic];
            s1 += (double)slab[(int64_t)(z + R) * total + ic];
        }
        if (z < splits) s0 += (double)slab[(int64_t)z * total + ic];
        double sd = s0 + s1;
        if (R > 1) {
            red[r][c] = sd;
            __syncthreads();
            if (r == 0) {
                sd = red[0][c];
#pragma unroll
                for (int q = 1; q < R; ++q) sd += red[q][c];
            }
            __syncthreads();
        }
        const float s = (float)sd;
        if (r != 0 || i >= total) continue;
        const int m = (int)(i / Nt), n = (int)(i - (int64_t)m * Nt);
        if (n < Ntot) {
            const int tap = n / Cin, ci = n - tap * Cin;
            float* d = dw + (int64_t)m * Ntot + (int64_t)ci * T + tap;
            *d = accumulate ? *d + s : s;
        } else if (with_bias && db) {
            db[m] = accumulate ? db[m] + s : s;
        }
    }
}

}  // namespace

void ubpl::launch_split_reduce(const float* slab, int splits, int Cout, int P, int64_t N, const float* bias,
                               const float* res, float* y, hipStream_t st) {
    const int64_t total = (int64_t)Cout * N;
    int gsz = (int)((total + 255) / 256);
    if (gsz > 8192) gsz = 8192;
    hipLaunchKernelGGL(split_reduce_kernel, dim3(gsz), dim3(256), 0, st, slab, splits, Cout, P, N, bias, res, y);
}

// Reduce a weight-gradient slab [splits][Cout][Cin*T + 1] (columns tap-major
// n = tap*Cin + ci, the last = bias) into dw (reference layout) and db (nullable).
UBPL_API int ubpl_wgrad_slab_reduce(const float* slab, int splits, int Cout, int Cin, int T, int with_bias, float* dw,
                                    float* db, int accumulate, void* stream) {
    const int64_t total = (int64_t)Cout * (Cin * T + 1);
    int R = 1;
    while (R < 16 && R * 32 < splits) R *= 2;           // <= ~32 loads per thread
    const int C = 256 / R;
    int64_t g = (total + C - 1) / C;
    if (g > 8192) g = 8192;
    return ubpl::pick(
        [&](auto R_) {
            hipLaunchKernelGGL(wgrad_reduce_kernel<R_>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, slab,
                               splits, Cout, Cin, T, with_bias, dw, db, accumulate);
            UBPL_LAUNCH_CHECK();
            return 0;
        },
        ubpl::among<1, 2, 4, 8, 16>{R});
}
