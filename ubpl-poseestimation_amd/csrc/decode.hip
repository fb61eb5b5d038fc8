// D1-D4 — argmax decoder, affine back-transform and PCK.
//
// Replaces get_preds / final_preds / transform_preds (utils/udaap/evaluation.py:13-30,215-238;
// utils/udaap/transforms.py:119-168) and EvaluationUtils.acc_pck (utils/evaluation.py:91-139),
// which the reference runs on the host after a D2H copy of every heatmap, with
// per-point Python loops.
//
// decode: one wave per (sample, keypoint) map.  Each lane scans a strided
// slice keeping the FIRST maximal index (strict >), then a wave reduction
// keeps the larger value and, on ties, the smaller index — torch.max's
// documented first-index rule.  NaN ranks above every number, as in torch.
// The 1-based (col, row) is zeroed where the max is not > 0, then mapped
// through the host-computed float64 inverse transform (same entries as the
// reference: float32 arithmetic for h = 200*scale, np.linalg.inv in f64) with
// un-fused f64 multiply/add in np.dot's order, truncated toward zero, + 1.
//
// decode with the flip test (ubpl_decode_heatmaps_flip): the same decode of
// (hm + flipped-back, pair-swapped hm_flip) / 2 — fliplr_back / flip_back
// (utils/augment.py:239-252, utils/udaap/transforms.py:20-57) and the average
// fused into the one read of both heatmap sets, which are addressed through a
// batch stride (the last stack of a [B,S,K,H,W] network output, in place).
//
// ensemble pseudo-labels (ubpl_ensemble_pseudo): JointPseudoLoss3's target and mask
// (utils/losses.py:176-210) at inference.  One read of M members' maps gives, per map,
// the decode of their per-pixel mean T (:179), every member's peak (:187), its mean
// squared distance from T (:184) and the two-sided threshold mask (:187-193).
#include "decode_common.h"

namespace {

using ubpl::beats;        // (decode_common.h: shared with decode_warp.hip)
using ubpl::finish_map;

__global__ void __launch_bounds__(256) argmax_kernel(const float* __restrict__ hm, int maps, int H, int W,
                                                    const double* __restrict__ tinv, int K,
                                                    float* __restrict__ raw, float* __restrict__ preds,
                                                    float* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const int map = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (map >= maps) return;
    const int HW = H * W;
    const float* m = hm + (int64_t)map * HW;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < HW; i += 64) {
        const float v = m[i];
        if (beats(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
    finish_map(bv, bi, lane, map, W, tinv, K, raw, preds, scores);
}

// Flip test (ubpl_decode_heatmaps_flip): map (n, k) = (hm[n,k] + mirror(hm_flip[n,perm[k]])) / 2,
// stored to `merged` (nullable) and decoded from the registers.  One wave per map, as above; a
// wave's 64 consecutive pixels of a row read 64 consecutive floats of hm_flip's row in
// descending order, so both loads stay contiguous.  FLIP false: hm alone (batch stride sb).
template <bool FLIP>
__global__ void __launch_bounds__(256) argmax_flip_kernel(const float* __restrict__ hm,
                                                         const float* __restrict__ hm_flip, int64_t sb, int maps,
                                                         int H, int W, const int* __restrict__ perm,
                                                         const double* __restrict__ tinv, int K,
                                                         float* __restrict__ merged, float* __restrict__ raw,
                                                         float* __restrict__ preds, float* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const int map = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (map >= maps) return;
    const int HW = H * W;
    const int n = map / K, k = map - n * K;
    const float* a = hm + n * sb + (int64_t)k * HW;
    const float* b = nullptr;
    if (FLIP) {
        int pk = perm != nullptr ? perm[k] : k;
        if ((unsigned)pk >= (unsigned)K) pk = k;      // (a bad table must not read out of bounds)
        b = hm_flip + n * sb + (int64_t)pk * HW;
    }
    float* mo = merged != nullptr ? merged + (int64_t)map * HW : nullptr;
    // pixel i = lane + 64 t at (y, x), stepped without a division per element
    const int dy = 64 / W, dx = 64 - dy * W;
    int y = lane / W, x = lane - y * W;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < HW; i += 64) {
        float v = a[i];
        if (FLIP) v = (v + b[y * W + (W - 1 - x)]) * 0.5f;
        if (mo != nullptr) mo[i] = v;
        if (beats(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
        y += dy;
        x += dx;
        if (x >= W) {
            x -= W;
            y += 1;
        }
    }
    finish_map(bv, bi, lane, map, W, tinv, K, raw, preds, scores);
}

// max with torch.max's NaN rule: a NaN, once seen, stays.
__device__ __forceinline__ float nanmax(float a, float b) { return (b > a || isnan(b)) ? b : a; }

// ubpl_ensemble_pseudo: one wave per map (n, k), the M members' values of a pixel in registers.
// T = (((p_0 + p_1) + ...) + p_{M-1}) / (float)M, a sequential f32 sum in member order and one
// division (targets.mean(0), utils/losses.py:179); T goes to mean_hm (nullable) and, from the
// same registers, into the argmax and into (p_m - T)^2.  The squared distances are summed per
// lane in pixel order and then by a fixed xor butterfly, so repeated launches give equal bits.
template <int M>
__global__ void __launch_bounds__(256) ensemble_pseudo_kernel(
    const float* __restrict__ hm, int64_t sm, int64_t sb, int maps, int H, int W, const double* __restrict__ tinv,
    int K, const float* __restrict__ thr, float* __restrict__ mean_hm, float* __restrict__ ens_raw,
    float* __restrict__ ens_preds, float* __restrict__ ens_score, float* __restrict__ member_score,
    float* __restrict__ disagree, float* __restrict__ select) {
    const int lane = threadIdx.x & 63;
    const int map = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (map >= maps) return;
    const int HW = H * W;
    const int n = map / K, k = map - n * K;
    const float* a = hm + n * sb + (int64_t)k * HW;
    float* mo = mean_hm != nullptr ? mean_hm + (int64_t)map * HW : nullptr;
    float mx[M], sq[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        mx[m] = -INFINITY;
        sq[m] = 0.f;
    }
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < HW; i += 64) {
        float p[M];
#pragma unroll
        for (int m = 0; m < M; ++m) p[m] = a[m * sm + i];
        float t = p[0];
#pragma unroll
        for (int m = 1; m < M; ++m) t += p[m];
        t /= (float)M;
        if (mo != nullptr) mo[i] = t;
        if (beats(t, i, bv, bi)) {
            bv = t;
            bi = i;
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            mx[m] = nanmax(mx[m], p[m]);
            const float d = p[m] - t;
            sq[m] += d * d;
        }
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mx[m] = nanmax(mx[m], __shfl_xor(mx[m], o, 64));
            sq[m] += __shfl_xor(sq[m], o, 64);
        }
    const float es = finish_map(bv, bi, lane, map, W, tinv, K, ens_raw, ens_preds, ens_score);
    if (lane != 0) return;
    const float th = thr[0];
    const bool eok = es >= th;                                      // :190-193 (a NaN never selects)
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int64_t o = (int64_t)m * maps + map;
        if (member_score) member_score[o] = mx[m];
        if (disagree) disagree[o] = sq[m] / (float)HW;               // :184
        select[o] = (mx[m] >= th && eok) ? 1.f : 0.f;                // :187-189
    }
}

template <int M>
void launch_ensemble_pseudo(hipStream_t st, const float* hm, int64_t sm, int64_t sb, int maps, int H, int W,
                            const double* tinv, int K, const float* thr, float* mean_hm, float* ens_raw,
                            float* ens_preds, float* ens_score, float* member_score, float* disagree,
                            float* select) {
    hipLaunchKernelGGL(ensemble_pseudo_kernel<M>, dim3(ubpl::cdiv(maps, 4)), dim3(256), 0, st, hm, sm, sb, maps, H, W,
                       tinv, K, thr, mean_hm, ens_raw, ens_preds, ens_score, member_score, disagree, select);
}

// PCK (utils/evaluation.py:91-139).  One workgroup; thread per keypoint.
__global__ void __launch_bounds__(256) pck_kernel(const float* __restrict__ preds, const float* __restrict__ gts,
                                                 int N, int K, int ref0, int ref1, float thr,
                                                 float* __restrict__ errs, float* __restrict__ accs,
                                                 int* __restrict__ hits, int* __restrict__ valid) {
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        float esum = 0.f;
        int nh = 0, nv = 0;
        for (int b = 0; b < N; ++b) {
            const float* g = gts + ((int64_t)b * K) * 3;
            const float nx = g[ref0 * 3] - g[ref1 * 3], ny = g[ref0 * 3 + 1] - g[ref1 * 3 + 1];
            const float norm = sqrtf(nx * nx + ny * ny);          // torch.dist (:121)
            const float gx = g[k * 3], gy = g[k * 3 + 1];
            float d = -1.f;
            if (gx > 1.f && gy > 1.f) {                          // :123
                const float dx = preds[((int64_t)b * K + k) * 2] - gx;
                const float dy = preds[((int64_t)b * K + k) * 2 + 1] - gy;
                d = sqrtf(dx * dx + dy * dy);
                const float dr = d / norm;
                nv += 1;
                nh += dr < thr;                                   // _acc_counting (:134-139)
            }
            esum += d;                                           // -1 sentinels included (:99-101)
        }
        errs[k] = esum / (float)N;
        accs[k] = nv > 0 ? (float)((double)nh / (double)nv) : -1.f;
        if (hits) hits[k] = nh;
        if (valid) valid[k] = nv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float es = 0.f, as = 0.f;
        int an = 0;
        for (int k = 0; k < K; ++k) es += errs[k];
        errs[K] = es / (float)K;                                 // :102-104
        for (int k = 0; k < K; ++k)
            if (accs[k] >= 0.f) {
                as += accs[k];
                an += 1;
            }
        accs[K] = an != 0 ? as / (float)an : 0.f;                // :110-114
    }
}

}  // namespace

// hm [N,K,H,W]; tinv [N,6] f64 (rows 0-1 of the inverse of get_transform) or
// null; raw/preds [N,K,2] f32 (nullable), scores [N,K] (nullable).
UBPL_API int ubpl_decode_heatmaps(const float* hm, int N, int K, int H, int W, const double* tinv, float* raw,
                                  float* preds, float* scores, void* stream) {
    const int maps = N * K;
    if (maps == 0) return 0;
    hipLaunchKernelGGL(argmax_kernel, dim3(ubpl::cdiv(maps, 4)), dim3(256), 0, (hipStream_t)stream, hm, maps, H, W,
                       tinv, K, raw, preds, scores);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// Flip-test decode (see include/ubpl_hip.h): hm / hm_flip maps at n*sb + k*H*W.
UBPL_API int ubpl_decode_heatmaps_flip(const float* hm, const float* hm_flip, int64_t sb, int N, int K, int H, int W,
                                       const int* perm, const double* tinv, float* merged, float* raw, float* preds,
                                       float* scores, void* stream) {
    if (N < 0 || K < 1 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff || (int64_t)N * K > 0x3fffffff ||
        (N > 1 && sb < (int64_t)K * H * W) || (preds != nullptr && tinv == nullptr))
        return (int)hipErrorInvalidValue;
    const int maps = N * K;
    if (maps == 0) return 0;
    if (hm_flip != nullptr)
        hipLaunchKernelGGL(argmax_flip_kernel<true>, dim3(ubpl::cdiv(maps, 4)), dim3(256), 0, (hipStream_t)stream, hm,
                           hm_flip, sb, maps, H, W, perm, tinv, K, merged, raw, preds, scores);
    else
        hipLaunchKernelGGL(argmax_flip_kernel<false>, dim3(ubpl::cdiv(maps, 4)), dim3(256), 0, (hipStream_t)stream,
                           hm, hm_flip, sb, maps, H, W, perm, tinv, K, merged, raw, preds, scores);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// Ensemble pseudo-labels (see include/ubpl_hip.h): member m's map (n, k) at hm + m*sm + n*sb + k*H*W.
UBPL_API int ubpl_ensemble_pseudo(const float* hm, int64_t sm, int64_t sb, int M, int N, int K, int H, int W,
                                  const double* tinv, const float* thr, float* mean_hm, float* ens_raw,
                                  float* ens_preds, float* ens_score, float* member_score, float* disagree,
                                  float* select, void* stream) {
    if (M < 1 || M > 8 || N < 0 || K < 1 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff ||
        (int64_t)N * K > 0x3fffffff || (N > 1 && sb < (int64_t)K * H * W) || (M > 1 && sm < (int64_t)K * H * W) ||
        (ens_preds != nullptr && tinv == nullptr) || hm == nullptr || thr == nullptr || select == nullptr)
        return (int)hipErrorInvalidValue;
    const int maps = N * K;
    if (maps == 0) return 0;
    // one instantiation per member count: the M values of a pixel stay in registers
    static constexpr decltype(&launch_ensemble_pseudo<1>) by_members[8] = {
        launch_ensemble_pseudo<1>, launch_ensemble_pseudo<2>, launch_ensemble_pseudo<3>, launch_ensemble_pseudo<4>,
        launch_ensemble_pseudo<5>, launch_ensemble_pseudo<6>, launch_ensemble_pseudo<7>, launch_ensemble_pseudo<8>};
    by_members[M - 1]((hipStream_t)stream, hm, sm, sb, maps, H, W, tinv, K, thr, mean_hm, ens_raw, ens_preds, ens_score,
                      member_score, disagree, select);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// preds [N,K,2], gts [N,K,3]; errs/accs [K+1]; hits/valid [K] int32 (nullable).
UBPL_API int ubpl_pck(const float* preds, const float* gts, int N, int K, int ref0, int ref1, float thr, float* errs,
                      float* accs, int* hits, int* valid, void* stream) {
    hipLaunchKernelGGL(pck_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, preds, gts, N, K, ref0, ref1, thr,
                       errs, accs, hits, valid);
    UBPL_LAUNCH_CHECK();
    return 0;
}
