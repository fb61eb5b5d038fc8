// The argmax decode's order and its per-map finish, shared by the decode kernels
// (decode.hip, decode_warp.hip).
#pragma once
#include "common.h"

namespace ubpl {

__device__ __forceinline__ bool beats(float v, int i, float bv, int bi) {
    const bool vn = isnan(v), bn = isnan(bv);
    if (vn != bn) return vn;
    if (vn && bn) return i < bi;
    return v > bv || (v == bv && i < bi);
}

// The lanes' (value, first index) candidates of one map -> its decoded point,
// written by lane 0 (the rules in decode.hip's header comment).  Returns the map's
// maximum (every lane holds it after the xor butterfly).
__device__ __forceinline__ float finish_map(float bv, int bi, int lane, int map, int W, const double* __restrict__ tinv,
                                           int K, float* __restrict__ raw, float* __restrict__ preds,
                                           float* __restrict__ scores) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (beats(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane != 0) return bv;
    const float on = bv > 0.f ? 1.f : 0.f;
    const float px = (float)(bi % W + 1) * on;   // utils/udaap/evaluation.py:25,28-29
    const float py = (float)(bi / W + 1) * on;   // :26
    if (raw) {
        raw[map * 2 + 0] = px;
        raw[map * 2 + 1] = py;
    }
    if (scores) scores[map] = bv;
    if (preds) {
        const double* t = tinv + (int64_t)(map / K) * 6;
        const double vx = (double)px - 1.0, vy = (double)py - 1.0;  // transforms.py:156
        const double rx = __dadd_rn(__dadd_rn(__dmul_rn(t[0], vx), __dmul_rn(t[1], vy)), t[2]);
        const double ry = __dadd_rn(__dadd_rn(__dmul_rn(t[3], vx), __dmul_rn(t[4], vy)), t[5]);
        preds[map * 2 + 0] = (float)((long long)rx + 1);  // astype(int) + 1 (:158)
        preds[map * 2 + 1] = (float)((long long)ry + 1);
    }
    return bv;
}

}  // namespace ubpl
