// Cross-view pseudo-label targets: ubpl_merge_views_samples warps every member's heatmaps of
// every view into every other view's frame and merges them per pixel, where each (target view,
// source view, sample) has its own matrix — the training step's augmented views, each with its
// own random flip, scale and rotation.  It is to ubpl_decode_heatmaps_views' merge what
// ubpl_view_uncertainty_samples is to ubpl_view_uncertainty.
//
// The reference hands every view's warp matrix to the step (utils/augment.py:158-164) and can
// warp heatmaps back (affine_back2, :36-47), but calls it from a debug drawing only
// (projects/MT_UBPL.py:186-205); its pseudo loss takes the teachers' maps of the student's own
// view (:279).  kernels.train_pair_matrices composes the pair matrices from the views' own.
//
// The sampling rule is warp_sample.h's, the merge rule ubpl_decode_heatmaps_views' (num / den
// over the views in ascending order, sequential un-fused f32 sums, 0 where no view covers), so the
// numpy restatement (tests/cross_view_ref.py on tests/tta_ref.py) gives the same bits.
//
// The work: a plane is small (64x64: 16 KB), the taps are gathers that stay in cache, the stores
// stream; the kernel is bound by latency and bandwidth, not arithmetic.  Where a pixel samples
// (tap index, weights, which taps are inside) and its coverage den depend on (target view, source
// view, sample, pixel) only, not on the M*K planes.  So a block is 256 pixels of one (target view,
// sample, member): each thread locates its pixel in every other view once, keeps the V-1 results
// in LDS (16 bytes each, the thread's own slots: no barrier), and then walks the K planes eight at
// a time — per source view one LDS read serves eight planes' gathers.  A row's two taps are
// neighbours in memory and come as one 8-byte load (blend_pairs), so a sample is two loads, not
// four, and sixteen are in flight per thread.  The matrices and the identity test are
// block-uniform (scalar loads, scalar branches).  cover is written by member 0's blocks.
// Measured at A = 2, M = 2, B = 32, K = 16, 64x64 (tools/view_merge_bench.py): four
// planes at a time with four 4-byte taps 52.5 us, eight planes 58.9 us; with paired taps two,
// four and eight planes 42.1, 42.3 and 38.8 us.
#include "warp_sample.h"

namespace {

using namespace ubpl;

constexpr int MAX_VIEWS = 16, MAX_MEMBERS = 8, BLOCK = 256, PLANES = 8;

// (the merge's sums and its quotient are un-fused like the header's)
#pragma clang fp contract(off)

typedef float float2u __attribute__((ext_vector_type(2), aligned(4)));

// blend() with each row's two taps in one 8-byte load (4-byte aligned; W >= 2): the same taps, the
// same arithmetic, the same bits.  A row's pair starts at x0; where x0 is -1 or W - 1 the pair is
// moved one cell into the row, so it never leaves the row, and the tap outside reads as 0.
__device__ __forceinline__ float blend_pairs(const float* __restrict__ p, int W, const Taps& t) {
    if (t.in == 0) return 0.f;
    const float bx = sub_rn(1.f, t.ax), by = sub_rn(1.f, t.ay);
    const bool l = t.in & 5, r = t.in & 10;
    const int base = t.idx + (l ? (r ? 0 : -1) : 1);
    float2u e0 = {0.f, 0.f}, e1 = {0.f, 0.f};
    if (t.in & 3) e0 = *reinterpret_cast<const float2u*>(p + base);
    if (t.in & 12) e1 = *reinterpret_cast<const float2u*>(p + base + W);
    const float v00 = l ? (r ? e0.x : e0.y) : 0.f, v01 = r ? (l ? e0.y : e0.x) : 0.f;
    const float v10 = l ? (r ? e1.x : e1.y) : 0.f, v11 = r ? (l ? e1.y : e1.x) : 0.f;
    return lerp_rn(lerp_rn(v00, v01, t.ax, bx), lerp_rn(v10, v11, t.ax, bx), t.ay, by);
}

// PAIR: a row's two taps in one load (rows of at least two cells)
template <bool PAIR>
__global__ void __launch_bounds__(BLOCK) merge_views_samples_kernel(
    const float* __restrict__ hm, int64_t sv, int64_t sm, int64_t sb, int V, int N, int K, int H, int W, int tiles,
    const float* __restrict__ mat, int include_self, float* __restrict__ out, float* __restrict__ cover) {
    extern __shared__ Taps taps[];                     // [V - 1][BLOCK]: slot of view v != a is v - (v > a)
    const int tid = threadIdx.x;
    const int an = blockIdx.x / tiles, tile = blockIdx.x - an * tiles;
    const int a = an / N, n = an - a * N, m = blockIdx.y, M = gridDim.y;
    const int HW = H * W;
    const int i = tile * BLOCK + tid;
    if (i >= HW) return;
    const int y = i / W, x = i - y * W;
    // ---- per (a, v, n, pixel): where it samples, and the pixel's coverage
    unsigned direct = 0;                               // bit v: view v contributes its own value p[i]
    unsigned skip = 0;                                 // bit v: view v does not contribute
    float den = 0.f;
    bool first = true;
    for (int v = 0; v < V; ++v) {
        float c = 1.f;
        if (v == a) {
            if (include_self == 0) {
                skip |= 1u << v;
                continue;
            }
            direct |= 1u << v;
        } else {
            const Mat6 q = load_mat6(mat + (((int64_t)a * V + v) * N + n) * 6);
            if (is_identity(q)) {
                direct |= 1u << v;
            } else {
                const Taps t = locate(H, W, q, x, y);
                taps[(v - (v > a)) * BLOCK + tid] = t;
                c = cover_of(t);
            }
        }
        den = first ? c : add_rn(den, c);
        first = false;
    }
    if (cover != nullptr && m == 0) cover[(int64_t)an * HW + i] = den;
    // ---- the K planes of member m, PLANES at a time
    const float* src = hm + m * sm + n * sb;
    float* dst = out + (((int64_t)a * M + m) * N + n) * K * HW;
    for (int k0 = 0; k0 < K; k0 += PLANES) {
        float num[PLANES];
        const float* p[PLANES];
#pragma unroll
        for (int j = 0; j < PLANES; ++j) {             // (a plane past the last: the last one again, not stored)
            p[j] = src + (int64_t)(k0 + j < K ? k0 + j : K - 1) * HW;
            num[j] = 0.f;
        }
        first = true;
        for (int v = 0; v < V; ++v) {
            if (skip >> v & 1) continue;
            float s[PLANES];
            if (direct >> v & 1) {
#pragma unroll
                for (int j = 0; j < PLANES; ++j) s[j] = p[j][v * sv + i];
            } else {
                const Taps t = taps[(v - (v > a)) * BLOCK + tid];
#pragma unroll
                for (int j = 0; j < PLANES; ++j)
                    s[j] = PAIR ? blend_pairs(p[j] + v * sv, W, t) : blend(p[j] + v * sv, W, t);
            }
#pragma unroll
            for (int j = 0; j < PLANES; ++j) num[j] = first ? s[j] : add_rn(num[j], s[j]);
            first = false;
        }
#pragma unroll
        for (int j = 0; j < PLANES; ++j)
            if (k0 + j < K) dst[(int64_t)(k0 + j) * HW + i] = den > 0.f ? div_rn(num[j], den) : 0.f;
    }
}

}  // namespace

// Per-sample cross-view merge (see include/ubpl_hip.h): view v, member m, sample n, joint k is the
// plane at hm + v*sv + m*sm + n*sb + k*H*W; mat [V][V][N][6], target view cell -> source view cell.
UBPL_API int ubpl_merge_views_samples(const float* hm, int64_t sv, int64_t sm, int64_t sb, int V, int M, int N, int K,
                                      int H, int W, const float* mat, int include_self, float* out, float* cover,
                                      void* stream) {
    if (V < 1 || V > MAX_VIEWS || M < 1 || M > MAX_MEMBERS || N < 0 || K < 1 || H < 1 || W < 1 ||
        (int64_t)H * W > 0x7fffffff || (include_self == 0 && V < 2) || sv < 0 || sm < 0 || sb < 0)
        return (int)hipErrorInvalidValue;
    const int64_t plane = (int64_t)K * H * W;
    if ((V > 1 && sv < plane) || (M > 1 && sm < plane) || (N > 1 && sb < plane) || hm == nullptr || out == nullptr ||
        (V > 1 && mat == nullptr))
        return (int)hipErrorInvalidValue;
    const int64_t tiles = ((int64_t)H * W + BLOCK - 1) / BLOCK, blocks = tiles * V * N;
    if (blocks > 0x7fffffff) return (int)hipErrorInvalidValue;
    if (blocks == 0) return 0;
    const auto kernel = W >= 2 ? merge_views_samples_kernel<true> : merge_views_samples_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, (unsigned)M), dim3(BLOCK),
                       (size_t)(V - 1) * BLOCK * sizeof(Taps), (hipStream_t)stream, hm, sv, sm, sb, V, N, K, H, W,
                       (int)tiles, mat, include_self, out, cover);
    UBPL_LAUNCH_CHECK();
    return 0;
}
