// The split paths' weights: one batched re-layout into npieces 16-bit planes per pass.
#include "common.h"

namespace {

// ------------------------------------------------------------------ weights
// Batched split re-layout over a segment table (int64 [nseg][5]: src_off,
// dst_off, Cout, Cin, T), one segment per blockIdx.y; NP bf16 planes of
// `plane` elements.  mode 0: forward layout wt[co][ci/G][tap][ci%G] =
// w[co][ci][tap]; mode 1: data-gradient layout wd[ci][co/G][tap][co%G] =
// w[co][ci][T-1-tap] (G = 16 when it divides the contraction channels).
__global__ void __launch_bounds__(256) split_relayout_kernel(const float* __restrict__ src,
                                                            uint16_t* __restrict__ dst, int64_t plane,
                                                            const int64_t* __restrict__ table, int mode, int np) {
    const int64_t* e = table + (int64_t)blockIdx.y * 5;
    const int64_t so = e[0], dof = e[1];
    const int Cout = (int)e[2], Cin = (int)e[3], T = (int)e[4];
    const int64_t total = (int64_t)Cout * Cin * T;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t s;
        if (mode == 0) {
            const int G = ubpl::conv_kgroup(Cin);
            const int gi = (int)(i % G);
            const int64_t t1 = i / G;
            const int tap = (int)(t1 % T);
            const int64_t t2 = t1 / T;
            const int cbk = (int)(t2 % (Cin / G));
            const int co = (int)(t2 / (Cin / G));
            s = ((int64_t)co * Cin + cbk * G + gi) * T + tap;
        } else {
            const int G = ubpl::conv_kgroup(Cout);
            const int gi = (int)(i % G);
            const int64_t t1 = i / G;
            const int tap = (int)(t1 % T);
            const int64_t t2 = t1 / T;
            const int cbk = (int)(t2 % (Cout / G));
            const int ci = (int)(t2 / (Cout / G));
            s = ((int64_t)(cbk * G + gi) * Cin + ci) * T + (T - 1 - tap);
        }
        float v = src[so + s];
        if (np == 2) {
            // 2xfp16: the fp16 pieces of w * fp16_wscale(contraction length) (common.h split2)
            v *= ubpl::fp16_wscale((mode == 0 ? Cin : Cout) * T);
            const _Float16 hv = (_Float16)v;
            dst[dof + i] = __builtin_bit_cast(uint16_t, hv);
            dst[plane + dof + i] = __builtin_bit_cast(uint16_t, (_Float16)(v - (float)hv));
            continue;
        }
        for (int p = 0; p < np; ++p) {
            const __bf16 hv = (__bf16)v;
            dst[(int64_t)p * plane + dof + i] = __builtin_bit_cast(uint16_t, hv);
            v -= (float)hv;
        }
    }
}

}  // namespace

// Split re-layout of many convs in one launch (table as ubpl_conv_weights_relayout;
// dst_off multiples of 8).  dst: npieces planes of `plane` bf16 elements.
UBPL_API int ubpl_conv_weights_split(const float* src, uint16_t* dst, int64_t plane, const int64_t* table, int nseg,
                                     int mode, int npieces, void* stream) {
    if (nseg <= 0) return 0;
    if (npieces < 1 || npieces > 3) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(split_relayout_kernel, dim3(64, nseg), dim3(256), 0, (hipStream_t)stream, src, dst, plane,
                       table, mode, npieces);
    UBPL_LAUNCH_CHECK();
    return 0;
}
