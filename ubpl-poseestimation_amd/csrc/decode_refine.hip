// D5 — sub-pixel refinement of the decoded peaks (ubpl_refine_peaks), a post-pass after
// the decodes of decode.hip, which stay as they are.
//
// The integer argmax puts every prediction on the heatmap's pixel lattice.  Two classical
// refinements move it off the lattice, per map, from the values around the peak the decode
// wrote (the rule in full: include/ubpl_hip.h):
//
//   quarter  a quarter pixel toward the larger neighbour, per axis — the stacked-hourglass
//            step the reference carries commented out (utils/udaap/evaluation.py:218-228),
//            with its indexing made right and without its +0.5;
//   Taylor   the distribution-aware decode (DARK): a Newton step on the log of the
//            (optionally blurred) map, from the gradient and Hessian at the peak; falls
//            back to quarter where the Hessian is not that of a maximum, the step is longer
//            than a pixel, the peak is within two cells of the border or anything in the
//            window is not finite.
//
// The sampled value v(y, x) is the decode's own: hm alone, or (hm + hm_flip[perm[k]]
// mirrored) * 0.5f — same expression, same rounding, same addressing (batch stride sb), so
// the refinement sees the bits the argmax saw.  Outside the map v = 0.
//
// One wave per map, four maps per block.  Quarter needs five loads by lane 0 and no LDS.
// Taylor stages the (5 + 2 radius)^2 window around the peak in the wave's LDS region, blurs
// it separably (rows, then columns) down to the 5 x 5 neighbourhood, takes logs, and lane 0
// finishes.  The block's barriers are reached by every wave — also by the idle waves of the
// tail block and by the waves whose map takes no Taylor step: the work between the barriers
// is guarded, nothing returns early.  No atomics; every sum has a fixed order, so repeated
// launches give equal bits.
#include "common.h"

namespace {

constexpr int MAX_RADIUS = 5;
constexpr int MAX_SIDE = 5 + 2 * MAX_RADIUS;   // 15

// One map's sampler: v(y, x) as the decode computed it, 0 outside the map.
struct MapView {
    const float* a;
    const float* b;   // the flipped set's (pair-swapped) map, or null
    int H, W;
    __device__ __forceinline__ float at(int y, int x) const {
        if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0.f;
        float v = a[y * W + x];
        if (b != nullptr) v = (v + b[y * W + (W - 1 - x)]) * 0.5f;
        return v;
    }
};

// sign with sign(0) = sign(NaN) = 0
__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// symmetric blur of one output: w[0] p[0] + sum_{j=1..radius} w[j] (p[-j st] + p[+j st]), f32, ascending j
__device__ __forceinline__ float blur_at(const float* p, int st, const float* w, int radius) {
    float acc = w[0] * p[0];
    for (int j = 1; j <= radius; ++j) acc += w[j] * (p[-j * st] + p[j * st]);
    return acc;
}

template <bool TAYLOR>
__global__ void __launch_bounds__(256) refine_peaks_kernel(const float* __restrict__ hm,
                                                          const float* __restrict__ hm_flip, int64_t sb, int maps,
                                                          int K, int H, int W, const int* __restrict__ perm,
                                                          const float* __restrict__ raw,
                                                          const float* __restrict__ taps, int radius,
                                                          const double* __restrict__ tinv,
                                                          float* __restrict__ raw_sub, float* __restrict__ preds_sub,
                                                          float* __restrict__ how) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int map = blockIdx.x * 4 + wid;
    const bool live = map < maps;

    // the peak the decode wrote, and rule 0 (every comparison fails on a NaN)
    MapView m = {nullptr, nullptr, H, W};
    float rx = 0.f, ry = 0.f;
    int c = 0, r = 0;
    bool peak = false;
    if (live) {
        const int n = map / K, k = map - n * K;
        m.a = hm + n * sb + (int64_t)k * H * W;
        if (hm_flip != nullptr) {
            int pk = perm != nullptr ? perm[k] : k;
            if ((unsigned)pk >= (unsigned)K) pk = k;          // (a bad table must not read out of bounds)
            m.b = hm_flip + n * sb + (int64_t)pk * H * W;
        }
        rx = raw[(int64_t)map * 2];
        ry = raw[(int64_t)map * 2 + 1];
        if (rx >= 1.f && rx <= (float)W && ry >= 1.f && ry <= (float)H) {
            c = (int)rx - 1;
            r = (int)ry - 1;
            peak = m.at(r, c) > 0.f;
        }
    }

    float ox = 0.f, oy = 0.f, rule = 0.f;
    if constexpr (TAYLOR) {
        // per wave: the window, its row-blurred 5 columns, the 5 x 5 logs; per block: the taps
        __shared__ float s_win[4][MAX_SIDE * MAX_SIDE];
        __shared__ float s_row[4][MAX_SIDE * 5];
        __shared__ float s_log[4][25];
        __shared__ float w[MAX_RADIUS + 1];
        const bool tay = peak && c >= 2 && c <= W - 3 && r >= 2 && r <= H - 3;   // wave-uniform
        const int side = 5 + 2 * radius, org = 2 + radius;
        if (threadIdx.x <= MAX_RADIUS) w[threadIdx.x] = (int)threadIdx.x <= radius ? taps[threadIdx.x] : 0.f;
        if (tay)
            for (int i = lane; i < side * side; i += 64) {
                const int wy = i / side, wx = i - wy * side;
                s_win[wid][i] = m.at(r - org + wy, c - org + wx);
            }
        __syncthreads();
        if (tay)
            for (int i = lane; i < side * 5; i += 64) {          // rows: [side][5]
                const int wy = i / 5, dx = i - wy * 5;
                s_row[wid][i] = blur_at(&s_win[wid][wy * side + radius + dx], 1, w, radius);
            }
        __syncthreads();
        if (tay && lane < 25) {                                  // columns: [5][5], then the log
            const int dy = lane / 5, dx = lane - dy * 5;
            s_log[wid][lane] = logf(fmaxf(blur_at(&s_row[wid][(radius + dy) * 5 + dx], 5, w, radius), 1e-10f));
        }
        __syncthreads();
        if (tay && lane == 0) {
            const float* L = s_log[wid];                         // L(dy, dx) = L[(dy + 2) * 5 + dx + 2]
            const float gx = 0.5f * (L[13] - L[11]), gy = 0.5f * (L[17] - L[7]);
            const float dxx = 0.25f * (L[14] - 2.f * L[12] + L[10]);
            const float dyy = 0.25f * (L[22] - 2.f * L[12] + L[2]);
            const float dxy = 0.25f * (L[18] - L[8] - L[16] + L[6]);
            const float det = dxx * dyy - dxy * dxy;
            if (dxx < 0.f && det > 0.f) {
                const float tx = -(dyy * gx - dxy * gy) / det, ty = -(dxx * gy - dxy * gx) / det;
                if (fabsf(tx) <= 1.f && fabsf(ty) <= 1.f) {      // max(|tx|, |ty|) <= 1, false on a NaN
                    ox = tx;
                    oy = ty;
                    rule = 2.f;
                }
            }
        }
    }
    if (!live || lane != 0) return;                              // (past the last barrier)
    if (peak && rule == 0.f) {                                   // quarter, on the unblurred values
        const bool ex = c >= 1 && c <= W - 2, ey = r >= 1 && r <= H - 2;
        if (ex) ox = 0.25f * sgn(m.at(r, c + 1) - m.at(r, c - 1));
        if (ey) oy = 0.25f * sgn(m.at(r + 1, c) - m.at(r - 1, c));
        rule = (ex || ey) ? 1.f : 0.f;
    }
    const float sx = rx + ox, sy = ry + oy;
    raw_sub[(int64_t)map * 2] = sx;
    raw_sub[(int64_t)map * 2 + 1] = sy;
    if (how) how[map] = rule;
    if (preds_sub) {
        // finish_map's transform (decode.hip) without its truncation
        const double* t = tinv + (int64_t)(map / K) * 6;
        const double vx = (double)sx - 1.0, vy = (double)sy - 1.0;
        const double px = __dadd_rn(__dadd_rn(__dmul_rn(t[0], vx), __dmul_rn(t[1], vy)), t[2]);
        const double py = __dadd_rn(__dadd_rn(__dmul_rn(t[3], vx), __dmul_rn(t[4], vy)), t[5]);
        preds_sub[(int64_t)map * 2] = (float)__dadd_rn(px, 1.0);
        preds_sub[(int64_t)map * 2 + 1] = (float)__dadd_rn(py, 1.0);
    }
}

}  // namespace

// Sub-pixel refinement of decoded peaks (see include/ubpl_hip.h).
UBPL_API int ubpl_refine_peaks(const float* hm, const float* hm_flip, int64_t sb, int N, int K, int H, int W,
                               const int* perm, const float* raw, int mode, const float* taps, int radius,
                               const double* tinv, float* raw_sub, float* preds_sub, float* how, void* stream) {
    if (N < 0 || K < 1 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff || (int64_t)N * K > 0x3fffffff ||
        (N > 1 && sb < (int64_t)K * H * W) || (preds_sub != nullptr && tinv == nullptr) || (mode != 1 && mode != 2) ||
        radius < 0 || radius > MAX_RADIUS || hm == nullptr || raw == nullptr || taps == nullptr || raw_sub == nullptr)
        return (int)hipErrorInvalidValue;
    const int maps = N * K;
    if (maps == 0) return 0;
    if (mode == 2)
        hipLaunchKernelGGL(refine_peaks_kernel<true>, dim3(ubpl::cdiv(maps, 4)), dim3(256), 0, (hipStream_t)stream, hm,
                           hm_flip, sb, maps, K, H, W, perm, raw, taps, radius, tinv, raw_sub, preds_sub, how);
    else
        hipLaunchKernelGGL(refine_peaks_kernel<false>, dim3(ubpl::cdiv(maps, 4)), dim3(256), 0, (hipStream_t)stream,
                           hm, hm_flip, sb, maps, K, H, W, perm, raw, taps, radius, tinv, raw_sub, preds_sub, how);
    UBPL_LAUNCH_CHECK();
    return 0;
}
