// The one bilinear sampling rule of the view kernels (include/ubpl_hip.h states it), shared by
// decode_warp.hip (one matrix per view) and view_merge.hip (one per view pair and sample).
//
// One rounding per product, sum and quotient (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn in
// meaning).  The toolchain's own helpers of those names are plain operators compiled with
// contraction allowed, and after inlining the compiler fuses their products and sums into FMAs,
// which the numpy restatement (tests/tta_ref.py) cannot follow; contraction is off from here to
// the end of every file that includes this one.
//
// The rule is cut in two so that a kernel can keep the first half: locate() is everything that
// depends on the matrix and the pixel alone (position, tap index, weights, which taps are inside),
// cover_of() and blend() are the formula over the in-bounds indicators and over a plane's four
// taps.  sample() is the three in a row.
#pragma once
#include "common.h"

namespace ubpl {

#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }

struct Mat6 {
    float m[6];
};

__device__ __forceinline__ Mat6 load_mat6(const float* __restrict__ p) {
    Mat6 a;
#pragma unroll
    for (int j = 0; j < 6; ++j) a.m[j] = p[j];
    return a;
}

__device__ __forceinline__ bool is_identity(const Mat6& a) {
    return a.m[0] == 1.f && a.m[1] == 0.f && a.m[2] == 0.f && a.m[3] == 0.f && a.m[4] == 1.f && a.m[5] == 0.f;
}

// a (1 - t) + b t, every product and sum its own rounding
__device__ __forceinline__ float lerp_rn(float a, float b, float t, float u) {
    return add_rn(mul_rn(a, u), mul_rn(b, t));
}

// Where an output pixel samples a plane [H,W]: tap (0,0) at element idx = y0*W + x0 (it may lie
// outside the plane: read a tap only where its bit of `in` is set), the weights of the second
// column and row, and in = bit 0..3 for the taps (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1)
// inside the plane.  in == 0 is "outside": a position inside always has one tap inside.
struct alignas(16) Taps {
    int idx;
    int in;
    float ax, ay;
};

// The source position of output pixel (x, y) under matrix a.  Outside — sx not in (-1, W) or sy
// not in (-1, H), which a NaN or an infinity is not — in = 0; the test comes before the float ->
// int conversion.
__device__ __forceinline__ Taps locate(int H, int W, const Mat6& a, int x, int y) {
    const float fx = (float)x, fy = (float)y;
    const float sx = add_rn(add_rn(mul_rn(a.m[0], fx), mul_rn(a.m[1], fy)), a.m[2]);
    const float sy = add_rn(add_rn(mul_rn(a.m[3], fx), mul_rn(a.m[4], fy)), a.m[5]);
    Taps t = {0, 0, 0.f, 0.f};
    if (!(sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H)) return t;
    const float x0f = floorf(sx), y0f = floorf(sy);
    t.ax = sub_rn(sx, x0f);
    t.ay = sub_rn(sy, y0f);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const bool l = x0 >= 0, r = x0 + 1 < W, u = y0 >= 0, d = y0 + 1 < H;
    t.idx = y0 * W + x0;
    t.in = (int)(u && l) | (int)(u && r) << 1 | (int)(d && l) << 2 | (int)(d && r) << 3;
    return t;
}

// The bilinear formula over the taps' in-bounds indicators (1 / 0); 0 outside.
__device__ __forceinline__ float cover_of(const Taps& t) {
    if (t.in == 0) return 0.f;
    const float bx = sub_rn(1.f, t.ax), by = sub_rn(1.f, t.ay);
    const float c00 = t.in & 1 ? 1.f : 0.f, c01 = t.in & 2 ? 1.f : 0.f;
    const float c10 = t.in & 4 ? 1.f : 0.f, c11 = t.in & 8 ? 1.f : 0.f;
    return lerp_rn(lerp_rn(c00, c01, t.ax, bx), lerp_rn(c10, c11, t.ax, bx), t.ay, by);
}

// The bilinear sample of plane p [H,W] (row length W) under t, a tap outside the plane 0; 0 outside.
__device__ __forceinline__ float blend(const float* __restrict__ p, int W, const Taps& t) {
    if (t.in == 0) return 0.f;
    const float bx = sub_rn(1.f, t.ax), by = sub_rn(1.f, t.ay);
    const float v00 = t.in & 1 ? p[t.idx] : 0.f, v01 = t.in & 2 ? p[t.idx + 1] : 0.f;
    const float v10 = t.in & 4 ? p[t.idx + W] : 0.f, v11 = t.in & 8 ? p[t.idx + W + 1] : 0.f;
    return lerp_rn(lerp_rn(v00, v01, t.ax, bx), lerp_rn(v10, v11, t.ax, bx), t.ay, by);
}

// sample and its coverage (cov) in one: the rule as include/ubpl_hip.h writes it
__device__ __forceinline__ float sample(const float* __restrict__ p, int H, int W, const Mat6& a, int x, int y,
                                        float& cov) {
    const Taps t = locate(H, W, a, x, y);
    cov = cover_of(t);
    return blend(p, W, t);
}

}  // namespace ubpl
