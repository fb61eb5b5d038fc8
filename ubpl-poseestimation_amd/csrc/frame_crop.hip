// Crop from raw frames — the reference's evaluation crop on the device.
//
// AugmentUtils.affine_image(img, center, scale, [R, R]) with angle == 0
// (utils/augment.py:91-137) is what turns a camera frame and a box into the
// network's input: for sf = scale * 200 / R >= 2 the WHOLE frame is first resized
// by 1 / sf (skimage.transform.resize), then the integer box transform([0, 0] /
// [R, R], invert=1) is cut out with zero fill and resized to R x R (a second
// skimage.transform.resize).  skimage's resize is a Gaussian of sigma = (in/out - 1)
// / 2 per shrinking axis (truncate 4, ndimage 'mirror' edges) followed by a bilinear
// sample at pixel centres with mirrored indices; both are separable and linear.
//
// Both branches are ONE computation per axis, stated by six ints of the host plan
// (ubpl_amd/frames.py crop_plan; include/ubpl_hip.h ubpl_crop_frames):
//
//   virtual source  ls pixels, pixel i = frame pixel org + i, 0 outside the frame
//   zoom            Gaussian radius r (weights from the host, f64 -> f32) then the
//                   bilinear sample at (g + 0.5) * ls / lo - 0.5 onto lo pixels —
//                   merged into 2r + 2 taps around the floor of that coordinate
//   box             lb pixels of the zoom grid from index off on, 0 outside the grid,
//                   resized to R pixels (two taps; lb == R: one, the identity)
//
// sf < 2: the virtual source is the box itself, lo = lb = R, off = 0.  sf >= 2: the
// virtual source is the frame, lo its pre-resized size and (off, lb) the box; lb is
// R up to the int truncation of the reference's transform, so the last resize has no
// Gaussian (the host refuses a plan where it would).
//
// Numerics: every source coordinate and its floor in float64 (a float32 coordinate
// on a 2000-pixel axis is 1e-4 px off), weights and sums in float32 in a fixed
// order — no atomics, two launches give equal bits.  u8 -> [0, 1] is v * (1/255.f),
// the value mouse.to_device_images computes (torch divides by a host scalar as a
// multiplication by its float32 reciprocal), so a box that is the whole frame at
// sf = 1 reproduces it bit for bit: every weight there is exactly 1 or 0.
//
// Two passes through a float32 intermediate: rows first (a thread per intermediate
// pixel, neighbours along x, the interleaved BGR bytes of a tap read once for the
// three channels), then columns.  Memory per box: the source rows the box needs
// (plan rows 13 / 14) x R x 3 floats written and read once.
#include "common.h"

namespace {

constexpr int PLAN_INTS = 16;

struct Axis {
    int org, ls, lo, off, lb, r;
};

__device__ __forceinline__ Axis load_axis(const int* p) { return Axis{p[0], p[1], p[2], p[3], p[4], p[5]}; }

// ndimage 'mirror' (d c b | a b c d | c b a), continued periodically: period 2 (n - 1)
__device__ __forceinline__ int mirror_p(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// floor and fraction of the sample coordinate of output pixel o of a resize in -> out (product
// and difference rounded separately, as the host plan computes its row ranges)
__device__ __forceinline__ int sample_at(int o, int in, int out, float& w) {
#pragma clang fp contract(off)
    const double q = ((double)o + 0.5) * ((double)in / (double)out) - 0.5;
    const double f = floor(q);
    w = (float)(q - f);
    return (int)f;
}

// weight of merged tap k (-r .. r + 1) around the floor: the Gaussian of the lower bilinear
// neighbour at k and of the upper one at k - 1 (gw[j] = 0 beyond the radius)
__device__ __forceinline__ float tap_weight(const float* gw, int r, int k, float wq) {
    const int a = k < 0 ? -k : k, b = k - 1 < 0 ? 1 - k : k - 1;
    const float ga = a <= r ? gw[a] : 0.f, gb = b <= r ? gw[b] : 0.f;
    return (1.f - wq) * ga + wq * gb;
}

// Pass 1: inter[b][c][rr][ox] = row (row_lo + rr) of box b's virtual source, resampled along x.
__global__ void __launch_bounds__(256) crop_rows_kernel(const uint8_t* __restrict__ bank,
                                                        const int64_t* __restrict__ off,
                                                        const int* __restrict__ hw, const int* __restrict__ plan,
                                                        const float* __restrict__ gauss, int gw, int rows_max,
                                                        int R, float* __restrict__ inter) {
    const int b = blockIdx.y;
    const int* pl = plan + PLAN_INTS * b;
    const int rows = pl[14];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= rows * R) return;
    const int rr = p / R, ox = p - rr * R;
    const Axis ax = load_axis(pl + 1);
    const int frame = pl[0], ht = hw[2 * frame], wd = hw[2 * frame + 1];
    const int y = pl[7] + pl[13] + rr;                       // frame row of this virtual-source row
    const float* g = gauss + (int64_t)(2 * b) * gw;
    float acc[3] = {0.f, 0.f, 0.f};
    if (y >= 0 && y < ht) {
        const uint8_t* row = bank + off[frame] + (int64_t)y * wd * 3;
        float wo;
        const int fo = sample_at(ox, ax.lb, R, wo);
        for (int t = 0; t < 2; ++t) {
            const float wt = t ? wo : 1.f - wo;
            if (wt == 0.f) continue;
            const int gi = ax.off + mirror_p(fo + t, ax.lb);
            if (gi < 0 || gi >= ax.lo) continue;              // the box leaves the zoom grid: 0
            float wq;
            const int fq = sample_at(gi, ax.ls, ax.lo, wq);
            float s[3] = {0.f, 0.f, 0.f};
            for (int k = -ax.r; k <= ax.r + 1; ++k) {
                const float wk = tap_weight(g, ax.r, k, wq);
                const int x = ax.org + mirror_p(fq + k, ax.ls);
                if (x < 0 || x >= wd) continue;               // the virtual source leaves the frame: 0
                const uint8_t* px = row + x * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c] += wk * ((float)px[c] * (1.f / 255.f));
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wt * s[c];
        }
    }
    const int64_t plane = (int64_t)rows_max * R;
    float* o = inter + (int64_t)b * 3 * plane + (int64_t)rr * R + ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = acc[c];
}

// Pass 2: out[b][c][oy][ox] = the intermediate resampled along y, minus chan_mean[c].
__global__ void __launch_bounds__(256) crop_cols_kernel(const float* __restrict__ inter,
                                                        const int* __restrict__ plan,
                                                        const float* __restrict__ gauss, int gw, int rows_max,
                                                        int R, const float* __restrict__ chan_mean,
                                                        float* __restrict__ out) {
    const int b = blockIdx.y;
    const int* pl = plan + PLAN_INTS * b;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= R * R) return;
    const int oy = p / R, ox = p - oy * R;
    const Axis ay = load_axis(pl + 7);
    const int row_lo = pl[13], rows = pl[14];
    const float* g = gauss + (int64_t)(2 * b + 1) * gw;
    const int64_t plane = (int64_t)rows_max * R;
    const float* src = inter + (int64_t)b * 3 * plane + ox;
    float acc[3] = {0.f, 0.f, 0.f};
    float wo;
    const int fo = sample_at(oy, ay.lb, R, wo);
    for (int t = 0; t < 2; ++t) {
        const float wt = t ? wo : 1.f - wo;
        if (wt == 0.f) continue;
        const int gi = ay.off + mirror_p(fo + t, ay.lb);
        if (gi < 0 || gi >= ay.lo) continue;
        float wq;
        const int fq = sample_at(gi, ay.ls, ay.lo, wq);
        float s[3] = {0.f, 0.f, 0.f};
        for (int k = -ay.r; k <= ay.r + 1; ++k) {
            const float wk = tap_weight(g, ay.r, k, wq);
            const int rr = mirror_p(fq + k, ay.ls) - row_lo;
            // memory safety only: the wrapper's host check (_check._crop_plan) recomputes every tap
            // and refuses a plan whose row range misses one, so no tap is ever dropped here
            if (rr < 0 || rr >= rows) continue;
            const float* q = src + (int64_t)rr * R;
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += wk * q[c * plane];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += wt * s[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(((int64_t)b * 3 + c) * R + oy) * R + ox] = acc[c] - chan_mean[c];
}

}  // namespace

UBPL_API int64_t ubpl_crop_frames_workspace(int n, int rows, int R) {
    if (n <= 0 || rows <= 0 || R <= 0) return 0;
    return (int64_t)n * 3 * rows * R;
}

UBPL_API int ubpl_crop_frames(const uint8_t* bank, const int64_t* off, const int* hw, const int* plan,
                              const float* gauss, int gw, const float* chan_mean, int n, int rows, int R,
                              float* inter, float* out, void* stream) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    if (rows <= 0 || R <= 0 || gw < 2 || (int64_t)rows * R > INT32_MAX || (int64_t)R * R > INT32_MAX || n > 65535)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(crop_rows_kernel, dim3(ubpl::cdiv((int64_t)rows * R, 256), n), dim3(256), 0,
                       (hipStream_t)stream, bank, off, hw, plan, gauss, gw, rows, R, inter);
    UBPL_LAUNCH_CHECK();
    hipLaunchKernelGGL(crop_cols_kernel, dim3(ubpl::cdiv((int64_t)R * R, 256), n), dim3(256), 0, (hipStream_t)stream,
                       inter, plan, gauss, gw, rows, R, chan_mean, out);
    UBPL_LAUNCH_CHECK();
    return 0;
}
