// D6 — multi-view test-time augmentation: ubpl_warp_views makes the rotated / zoomed / mirrored
// views of an image batch, ubpl_decode_heatmaps_views warps every view's heatmaps back into the
// original frame, merges them per pixel and decodes the merged maps from the same registers.
//
// The reference computes a view's warp matrix (utils/augment.py:158-164 affine_getWarpmat) and
// can warp heatmaps back (affine_back2, :36-47: F.affine_grid / F.grid_sample with
// align_corners=True, then the flip-back), but calls it from a debug drawing only
// (projects/MT_UBPL.py:186-205).  Here both directions are pixel-space 2x3 matrices, output
// pixel -> source pixel, with the mirror folded in (kernels.view_matrices).
//
// One sampling rule for both kernels (include/ubpl_hip.h states it; warp_sample.h is its code,
// shared with view_merge.hip): un-fused f32 products and sums, so the numpy restatement
// (tests/tta_ref.py) gives the same bits; zero taps outside; an exactly-identity matrix takes the
// value itself.
//
// decode: one 256-thread block per map (n, k).  A map is 16 KB, so the four bilinear taps of
// every view are gathers that stay in the cache; what a map costs is the latency of V rounds of
// gathers per pixel, and four waves per map instead of the decode family's one put four times
// as many of them in flight where the batch is small (N = 1: K blocks in all).  Each thread
// keeps its (value, first index) candidate; the four waves' candidates of a lane meet in LDS
// and wave 0 finishes the map with the decode family's finish_map.  beats() is a total order
// on (value, index), so the result does not depend on how the pixels are dealt to threads.
#include "decode_common.h"
#include "warp_sample.h"

namespace {

using namespace ubpl;   // beats, finish_map; Mat6, is_identity, sample and the *_rn helpers (warp_sample.h)

constexpr int MAX_VIEWS = 16;

// (the merge's sums and its quotient below are un-fused like the header's)
#pragma clang fp contract(off)

// out[v, plane, y, x] = sample of src[plane] under mat[v]; thread per output pixel.
__global__ void __launch_bounds__(256) warp_views_kernel(const float* __restrict__ src, int64_t planes, int H, int W,
                                                        const float* __restrict__ mat, int V,
                                                        float* __restrict__ out) {
    const int HW = H * W;
    const int64_t per_view = planes * HW, total = per_view * V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int v = (int)(i / per_view);
        const int64_t r = i - (int64_t)v * per_view;
        const int64_t pl = r / HW;
        const int px = (int)(r - pl * HW);
        const int y = px / W, x = px - y * W;
        const Mat6 a = load_mat6(mat + v * 6);
        const float* p = src + pl * HW;
        float cov;
        out[i] = is_identity(a) ? p[px] : sample(p, H, W, a, x, y, cov);
    }
}

__global__ void __launch_bounds__(256) decode_views_kernel(const float* __restrict__ hm, int64_t sv, int64_t sb,
                                                          int V, int H, int W, const float* __restrict__ mat,
                                                          const int* __restrict__ swap, const int* __restrict__ perm,
                                                          const double* __restrict__ tinv, int K,
                                                          float* __restrict__ merged, float* __restrict__ raw,
                                                          float* __restrict__ preds, float* __restrict__ scores) {
    __shared__ float cand_v[4][64];
    __shared__ int cand_i[4][64];
    const int map = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = H * W;
    const int n = map / K, k = map - n * K;
    int pk = perm != nullptr ? perm[k] : k;
    if ((unsigned)pk >= (unsigned)K) pk = k;          // (a bad table must not read out of bounds)
    const float* base = hm + n * sb;
    float* mo = merged != nullptr ? merged + (int64_t)map * HW : nullptr;
    // pixel i = tid + 256 t at (y, x), stepped without a division per element
    const int dy = 256 / W, dx = 256 - dy * W;
    int y = tid / W, x = tid - y * W;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < HW; i += 256) {
        float num = 0.f, den = 0.f;
        for (int v = 0; v < V; ++v) {                  // (block-uniform: the matrices are scalar loads)
            const Mat6 a = load_mat6(mat + v * 6);
            const int kv = (swap != nullptr && swap[v] != 0) ? pk : k;
            const float* p = base + v * sv + (int64_t)kv * HW;
            float s, c;
            if (is_identity(a)) {
                s = p[i];
                c = 1.f;
            } else {
                s = sample(p, H, W, a, x, y, c);
            }
            num = v == 0 ? s : add_rn(num, s);
            den = v == 0 ? c : add_rn(den, c);
        }
        const float m = den > 0.f ? div_rn(num, den) : 0.f;
        if (mo != nullptr) mo[i] = m;
        if (beats(m, i, bv, bi)) {
            bv = m;
            bi = i;
        }
        y += dy;
        x += dx;
        if (x >= W) {
            x -= W;
            y += 1;
        }
    }
    cand_v[wave][lane] = bv;
    cand_i[wave][lane] = bi;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float ov = cand_v[w][lane];
        const int oi = cand_i[w][lane];
        if (beats(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    finish_map(bv, bi, lane, map, W, tinv, K, raw, preds, scores);
}

}  // namespace

// Views of an image batch (see include/ubpl_hip.h): out[v] = src sampled under mat[v].
UBPL_API int ubpl_warp_views(const float* src, int N, int C, int H, int W, const float* mat, int V, float* out,
                             void* stream) {
    if (N < 0 || C < 1 || H < 1 || W < 1 || V < 0 || (int64_t)H * W > 0x7fffffff || src == nullptr ||
        mat == nullptr || out == nullptr)
        return (int)hipErrorInvalidValue;
    const int64_t planes = (int64_t)N * C, total = planes * H * W * V;
    if (total == 0) return 0;
    const int64_t blocks = (total + 255) / 256, cap = (int64_t)ubpl::cu_count() * 16;
    hipLaunchKernelGGL(warp_views_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0,
                       (hipStream_t)stream, src, planes, H, W, mat, V, out);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// Multi-view decode (see include/ubpl_hip.h): view v's map (n, k) at hm + v*sv + n*sb + k'*H*W.
UBPL_API int ubpl_decode_heatmaps_views(const float* hm, int64_t sv, int64_t sb, int V, int N, int K, int H, int W,
                                        const float* mat, const int* swap, const int* perm, const double* tinv,
                                        float* merged, float* raw, float* preds, float* scores, void* stream) {
    if (V < 1 || V > MAX_VIEWS || N < 0 || K < 1 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff ||
        (int64_t)N * K > 0x3fffffff || (N > 1 && sb < (int64_t)K * H * W) || (V > 1 && sv < (int64_t)K * H * W) ||
        sb < 0 || sv < 0 || (preds != nullptr && tinv == nullptr) || hm == nullptr || mat == nullptr)
        return (int)hipErrorInvalidValue;
    const int maps = N * K;
    if (maps == 0) return 0;
    hipLaunchKernelGGL(decode_views_kernel, dim3(maps), dim3(256), 0, (hipStream_t)stream, hm, sv, sb, V, H, W, mat,
                       swap, perm, tinv, K, merged, raw, preds, scores);
    UBPL_LAUNCH_CHECK();
    return 0;
}
