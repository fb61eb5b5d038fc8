// U1 — view-consistency uncertainty of multi-view predictions (ubpl_view_uncertainty).
//
// The reference estimates how far a pseudo-label can be trusted from geometry alone
// (utils/business.py: pseudo_cal_unc :220-234, _initKSample :302-318, _calKSampleExterData
// :320-346, pseudo_filter_mixUnc :237-264, assess_pseudo_unc2 :109-161; utils/process.py:53-68
// coord_distance / coord_avgDistance): how far one teacher's predictions on several augmented
// copies of an image lie from each other (intDist), how far the teachers lie from one another
// (extDist on the image itself, aExtDist on the means over the copies), folded into
// unc = 1 - exp(-mixDist / 5) and thresholded on the distances.  It does that on the host, in
// Python loops over dictionaries, from predictions made one augmented batch at a time.
//
// Here the per-view peaks of the test-time-augmentation batch (the strided plain decode of the
// view-major network output, optionally refined) are mapped back into the original frame and
// folded in one launch; the rule in full, with every rounding, is in include/ubpl_hip.h, and
// tests/unc_ref.py restates it in numpy.  Two things of the reference are left out: the running
// average over epochs (_lma_variables, :397-406) is the identity on a first call, which is what
// one inference pass is, so the *_lma values are the values themselves and no history is kept;
// and the scores of _initKSample (:309-311) index batch row 0 and feed no distance.
//
// One 64-thread block (one wave) per (n, k).  The lanes map the M*V <= 128 points into LDS; lane
// m then runs member m's sequential sums; lane 0 folds the member pairs; lane m finishes member
// m.  The data is a few hundred bytes per block: what matters is one launch inside the captured
// graph and summation orders that a restatement can reproduce.  No atomics; contraction is off,
// so every product and sum is its own f32 rounding; repeated launches give equal bits.
//
// The kernel is a template on how the points are addressed.  SAMPLES = false is the layout above:
// one back[V,6] for all samples, view-major member blocks, the joint swap and tinv.  SAMPLES = true
// (ubpl_view_uncertainty_samples) is the training step's: every (view, sample) has its own random
// flip, scale and rotation, so back is [V][N][6]; raw has a member and a view stride (one decode
// launch per view fills a [V][M][N][K][2] buffer); no joint swap and no tinv (points come out in
// source-image pixels through back); and gate[N,K] = 1 iff every member is selected.
#include "common.h"

namespace {

constexpr int MAX_MEMBERS = 8;
constexpr int MAX_VIEWS = 16;
constexpr float SENTINEL = 999.f;                  // the reference's "no value" (business.py:121, 344)

#pragma clang fp contract(off)
// coord_distance (utils/process.py:53-54) in f32
__device__ __forceinline__ float dist2(float ax, float ay, float bx, float by) {
    const float dx = ax - bx, dy = ay - by;
    return sqrtf(dx * dx + dy * dy);
}

template <bool SAMPLES>
__global__ void __launch_bounds__(64) view_uncertainty_kernel(
    const float* __restrict__ raw, int64_t sm, int64_t sv, int M, int V, int N, int K,
    const float* __restrict__ back, const int* __restrict__ swap, const int* __restrict__ perm,
    const double* __restrict__ tinv, const float* __restrict__ dist_thr, float* __restrict__ pts,
    float* __restrict__ legal, float* __restrict__ int_dist, float* __restrict__ aug_coord,
    float* __restrict__ ext_dist, float* __restrict__ aext_dist, float* __restrict__ ext_views,
    float* __restrict__ mix_dist, float* __restrict__ unc, float* __restrict__ select,
    float* __restrict__ gate) {
    __shared__ float s_x[MAX_MEMBERS * MAX_VIEWS], s_y[MAX_MEMBERS * MAX_VIEWS];
    __shared__ int s_ok[MAX_MEMBERS * MAX_VIEWS];
    __shared__ float s_int[MAX_MEMBERS], s_ax[MAX_MEMBERS], s_ay[MAX_MEMBERS];
    __shared__ int s_leg[MAX_MEMBERS];
    __shared__ float s_pair[3];
    __shared__ int s_sel[MAX_MEMBERS];
    const int map = blockIdx.x, lane = threadIdx.x;
    const int n = map / K, k = map - n * K;
    const int64_t maps = (int64_t)N * K;

    // the points, in the original frame (heatmap cells, or image coordinates with tinv)
    for (int i = lane; i < M * V; i += 64) {
        const int m = i / V, v = i - m * V;
        const float *p, *b;
        if (SAMPLES) {
            p = raw + m * sm + v * sv + ((int64_t)n * K + k) * 2;
            b = back + ((int64_t)v * N + n) * 6;
        } else {
            int kk = k;
            if (swap != nullptr && swap[v] != 0 && perm != nullptr) {
                const int pk = perm[k];
                if ((unsigned)pk < (unsigned)K) kk = pk;  // (a bad table must not read out of bounds)
            }
            p = raw + m * sm + (((int64_t)v * N + n) * K + kk) * 2;
            b = back + v * 6;
        }
        const float rx = p[0], ry = p[1];
        const float u = rx - 1.f, w = ry - 1.f;
        const float ox = (b[0] * u + b[1] * w) + b[2];
        const float oy = (b[3] * u + b[4] * w) + b[5];
        float px, py;
        if (!SAMPLES && tinv != nullptr) {
            // ubpl_refine_peaks' preds_sub expression at (ox, oy): f64, un-fused, + 1, not truncated
            const double* t = tinv + (int64_t)n * 6;
            const double du = (double)ox, dw = (double)oy;
            const double qx = __dadd_rn(__dadd_rn(__dmul_rn(t[0], du), __dmul_rn(t[1], dw)), t[2]);
            const double qy = __dadd_rn(__dadd_rn(__dmul_rn(t[3], du), __dmul_rn(t[4], dw)), t[5]);
            px = (float)__dadd_rn(qx, 1.0);
            py = (float)__dadd_rn(qy, 1.0);
        } else {
            px = ox + 1.f;
            py = oy + 1.f;
        }
        const bool peak = !(rx == 0.f && ry == 0.f);
        const bool finite = fabsf(px) < INFINITY && fabsf(py) < INFINITY;      // false on a NaN
        const bool ok = peak && finite && (SAMPLES || tinv == nullptr || (px >= 0.f && py >= 0.f));   // business.py:31
        s_x[i] = px;
        s_y[i] = py;
        s_ok[i] = ok ? 1 : 0;
        if (pts != nullptr) {
            const int64_t o = (((int64_t)m * V + v) * maps + map) * 2;
            pts[o] = px;
            pts[o + 1] = py;
        }
    }
    __syncthreads();

    // member m: _checkGroupLegal, coord_avgDistance over the view pairs, the mean point
    bool leg = false;
    float id = SENTINEL, ax = -1.f, ay = -1.f;
    if (lane < M) {
        const float* x = s_x + lane * V;
        const float* y = s_y + lane * V;
        leg = true;
        for (int v = 0; v < V; ++v) leg = leg && s_ok[lane * V + v] != 0;
        if (leg) {
            float ds = 0.f, sx = 0.f, sy = 0.f;
            for (int a = 0; a < V; ++a)
                for (int b = a + 1; b < V; ++b) ds += dist2(x[a], y[a], x[b], y[b]);   // combinations order
            for (int v = 0; v < V; ++v) {
                sx += x[v];
                sy += y[v];
            }
            id = ds / (float)(V * (V - 1) / 2);
            ax = sx / (float)V;
            ay = sy / (float)V;
        }
        s_int[lane] = id;
        s_ax[lane] = ax;
        s_ay[lane] = ay;
        s_leg[lane] = leg ? 1 : 0;
    }
    __syncthreads();

    // the member pairs a < b with both legal, ascending
    if (lane == 0) {
        float se = 0.f, sa = 0.f, sv = 0.f;
        int cnt = 0;
        for (int a = 0; a < M; ++a)
            for (int b = a + 1; b < M; ++b) {
                if (!(s_leg[a] && s_leg[b])) continue;
                se += dist2(s_x[a * V], s_y[a * V], s_x[b * V], s_y[b * V]);                  // :322
                sa += dist2(s_ax[a], s_ay[a], s_ax[b], s_ay[b]);                              // :323
                float dv = 0.f;
                for (int v = 0; v < V; ++v)
                    dv += dist2(s_x[a * V + v], s_y[a * V + v], s_x[b * V + v], s_y[b * V + v]);   // :144-149
                sv += dv / (float)V;
                cnt += 1;
            }
        const float none = M >= 2 ? SENTINEL : 0.f;
        const float e = cnt > 0 ? se / (float)cnt : none;
        const float ae = cnt > 0 ? sa / (float)cnt : none;
        const float ev = cnt > 0 ? sv / (float)cnt : none;
        s_pair[0] = e;
        s_pair[1] = ae;
        s_pair[2] = ev;
        if (ext_dist != nullptr) ext_dist[map] = e;
        if (aext_dist != nullptr) aext_dist[map] = ae;
        if (ext_views != nullptr) ext_views[map] = ev;
    }
    __syncthreads();

    if (lane < M) {
        const float e = s_pair[0], ae = s_pair[1], t = dist_thr[0];
        float mix = SENTINEL, un = SENTINEL;
        bool sel = false;
        if (leg) {
            mix = id + (e > 0.f ? (e + ae) / 2.f : ae);                // :328
            un = 1.f - expf(-mix / 5.f);                               // _calUncValue (:375-376)
            sel = id <= t && e <= t && ae <= t && mix <= 3.f * t;      // :331-345, :242-247 on the distance
        }
        const int64_t o = (int64_t)lane * maps + map;
        if (legal != nullptr) legal[o] = leg ? 1.f : 0.f;
        if (int_dist != nullptr) int_dist[o] = id;
        if (aug_coord != nullptr) {
            aug_coord[o * 2] = ax;
            aug_coord[o * 2 + 1] = ay;
        }
        if (mix_dist != nullptr) mix_dist[o] = mix;
        if (unc != nullptr) unc[o] = un;
        select[o] = sel ? 1.f : 0.f;
        if (SAMPLES) s_sel[lane] = sel ? 1 : 0;
    }
    if (!SAMPLES || gate == nullptr) return;                           // (uniform over the block)
    __syncthreads();
    if (lane == 0) {
        bool all = true;                                               // unc_select.all(0)
        for (int m = 0; m < M; ++m) all = all && s_sel[m] != 0;
        gate[map] = all ? 1.f : 0.f;
    }
}

}  // namespace

// View-consistency uncertainty (see include/ubpl_hip.h): member m's point of view v, sample n,
// joint k at raw + m*sm + ((v*N + n)*K + k')*2.
UBPL_API int ubpl_view_uncertainty(const float* raw, int64_t sm, int M, int V, int N, int K, const float* back,
                                   const int* swap, const int* perm, const double* tinv, const float* dist_thr,
                                   float* pts, float* legal, float* int_dist, float* aug_coord, float* ext_dist,
                                   float* aext_dist, float* ext_views, float* mix_dist, float* unc, float* select,
                                   void* stream) {
    if (M < 1 || M > MAX_MEMBERS || V < 2 || V > MAX_VIEWS || N < 0 || K < 1 || (int64_t)N * K > 0x3fffffff ||
        (int64_t)V * N * K > 0x3fffffff || (M > 1 && sm < (int64_t)V * N * K * 2) || raw == nullptr ||
        back == nullptr || dist_thr == nullptr || select == nullptr)
        return (int)hipErrorInvalidValue;
    const int maps = N * K;
    if (maps == 0) return 0;
    hipLaunchKernelGGL(view_uncertainty_kernel<false>, dim3(maps), dim3(64), 0, (hipStream_t)stream, raw, sm,
                       (int64_t)0, M, V, N, K, back, swap, perm, tinv, dist_thr, pts, legal, int_dist, aug_coord,
                       ext_dist, aext_dist, ext_views, mix_dist, unc, select, (float*)nullptr);
    UBPL_LAUNCH_CHECK();
    return 0;
}

// The same rule with per-sample matrices (see include/ubpl_hip.h): member m's point of view v,
// sample n, joint k at raw + m*sm + v*sv + (n*K + k)*2, its matrix at back + (v*N + n)*6.
UBPL_API int ubpl_view_uncertainty_samples(const float* raw, int64_t sm, int64_t sv, int M, int V, int N, int K,
                                           const float* back, const float* dist_thr, float* pts, float* legal,
                                           float* int_dist, float* aug_coord, float* ext_dist, float* aext_dist,
                                           float* ext_views, float* mix_dist, float* unc, float* select,
                                           float* gate, void* stream) {
    if (M < 1 || M > MAX_MEMBERS || V < 2 || V > MAX_VIEWS || N < 0 || K < 1 || (int64_t)N * K > 0x3fffffff ||
        (int64_t)V * N * K > 0x3fffffff || raw == nullptr || back == nullptr || dist_thr == nullptr ||
        select == nullptr)
        return (int)hipErrorInvalidValue;
    // a view's block of one member holds N*K points; the members' and the views' blocks do not
    // interleave: member-major (sm >= the V views of a member) or view-major (sv >= the M members)
    // (strides are bounded first, so that the products below cannot wrap)
    const int64_t blk = (int64_t)N * K * 2, max_stride = (int64_t)1 << 40;
    if (sm > max_stride || sv > max_stride || sv < blk || sm < 0 || (M > 1 && sm < blk) ||
        (M > 1 && sm < (V - 1) * sv + blk && sv < (M - 1) * sm + blk))
        return (int)hipErrorInvalidValue;
    const int maps = N * K;
    if (maps == 0) return 0;
    hipLaunchKernelGGL(view_uncertainty_kernel<true>, dim3(maps), dim3(64), 0, (hipStream_t)stream, raw, sm, sv, M,
                       V, N, K, back, (const int*)nullptr, (const int*)nullptr, (const double*)nullptr, dist_thr,
                       pts, legal, int_dist, aug_coord, ext_dist, aext_dist, ext_views, mix_dist, unc, select, gate);
    UBPL_LAUNCH_CHECK();
    return 0;
}
