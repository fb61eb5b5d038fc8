// Weight re-layouts of the exact-f32 convolutions: the grouped tap-major forward layout, the
// flipped / transposed data-gradient layout, and both batched over a model's segment table.
#include "common.h"
using ubpl::conv_kgroup;

namespace {

// Forward weight layout (grouped tap-major): wt[co][ci/G][tap][ci%G] = w[co][ci][tap].
__device__ __forceinline__ int64_t fwd_layout_src(int64_t i, int Cout, int Cin, int T) {
    const int G = conv_kgroup(Cin);
    const int gi = (int)(i % G);
    const int64_t t1 = i / G;
    const int tap = (int)(t1 % T);
    const int64_t t2 = t1 / T;
    const int cb = (int)(t2 % (Cin / G));
    const int co = (int)(t2 / (Cin / G));
    return ((int64_t)co * Cin + cb * G + gi) * T + tap;
}

// dgrad weights = the forward layout of the flipped, transposed kernel:
// wd[ci][co/G][tap][co%G] = w[co][ci][T-1-tap]  (G = conv_kgroup(Cout)).
__device__ __forceinline__ int64_t dgrad_layout_src(int64_t i, int Cout, int Cin, int T) {
    const int G = conv_kgroup(Cout);
    const int gi = (int)(i % G);
    const int64_t t1 = i / G;
    const int tap = (int)(t1 % T);
    const int64_t t2 = t1 / T;
    const int cb = (int)(t2 % (Cout / G));
    const int ci = (int)(t2 / (Cout / G));
    return ((int64_t)(cb * G + gi) * Cin + ci) * T + (T - 1 - tap);
}

__global__ void tapmajor_kernel(const float* __restrict__ w, int Cout, int Cin, int T, float* __restrict__ wt) {
    const int64_t total = (int64_t)Cout * Cin * T;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        wt[i] = w[fwd_layout_src(i, Cout, Cin, T)];
}

__global__ void flip_tapmajor_kernel(const float* __restrict__ w, int Cout, int Cin, int T, float* __restrict__ wd) {
    const int64_t total = (int64_t)Cout * Cin * T;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        wd[i] = w[dgrad_layout_src(i, Cout, Cin, T)];
}

// Batched weight re-layout over a segment table (int64 [nseg][5]:
// src_off, dst_off, Cout, Cin, T), one segment per blockIdx.y.
// mode 0: forward layout, mode 1: dgrad layout (above).
__global__ void __launch_bounds__(256) relayout_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                      const int64_t* __restrict__ table, int mode) {
    const int64_t* e = table + (int64_t)blockIdx.y * 5;
    const int64_t so = e[0], dof = e[1];
    const int Cout = (int)e[2], Cin = (int)e[3], T = (int)e[4];
    const int64_t total = (int64_t)Cout * Cin * T;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        dst[dof + i] = src[so + (mode == 0 ? fwd_layout_src(i, Cout, Cin, T) : dgrad_layout_src(i, Cout, Cin, T))];
}

}  // namespace

// Forward weight layout: wt[co][ci/G][tap][ci%G] = w[co][ci][tap], G = 16 if it
// divides Cin, else Cin (plain tap-major); for KS == 1 it is w itself.
UBPL_API int ubpl_conv_weight_tapmajor(const float* w, int Cout, int Cin, int KS, float* wt, void* stream) {
    const int64_t total = (int64_t)Cout * Cin * KS * KS;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(tapmajor_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, KS * KS, wt);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// dgrad weights (stride 1): the forward layout of the flipped, transposed
// kernel, wd[ci][co/G][tap][co%G] = w[co][ci][KS*KS-1-tap]: dx = conv(dy, wd).
UBPL_API int ubpl_conv_weight_flip(const float* w, int Cout, int Cin, int KS, float* wt, void* stream) {
    const int64_t total = (int64_t)Cout * Cin * KS * KS;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(flip_tapmajor_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, KS * KS,
                       wt);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// All conv weights of a model re-laid out in one launch (see relayout_kernel).
UBPL_API int ubpl_conv_weights_relayout(const float* src, float* dst, const int64_t* table, int nseg, int mode,
                                        void* stream) {
    if (nseg <= 0) return 0;
    hipLaunchKernelGGL(relayout_kernel, dim3(64, nseg), dim3(256), 0, (hipStream_t)stream, src, dst, table, mode);
    UBPL_LAUNCH_CHECK();
    return 0;
}
