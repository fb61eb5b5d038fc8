// Rank-based and softmax-score pseudo-label selection (utils/losses.py:73-166, 213-243:
// JointPseudoLoss, JointPseudoLoss2, JointDistLoss_mt).
//
// The reference scores a map by the softmax ACROSS the keypoint axis at every pixel, then the
// per-map maximum (:137-138), sorts the batch's B*K scores of a stack and keeps the rows at or
// above the int(N*(1-selRate))-th smallest (:139-141) — per-element Python loops and a
// torch.sort per stack.  Here:
//   softmax_peak   lanes along the pixels, the K maps of a pixel held in registers: one HBM
//                  read of the maps; the pixels of a (b,s) are split over workgroups and
//                  combined by an integer atomic max on the scores' bits (they are >= 0, so
//                  the bit order is the value order, and max is order-independent);
//   rank_select    one workgroup per group: the rank-th smallest by counting (no sort);
//   finalize       the shared finalize body (finalize_rows, loss_rows.h) for kinds 1 and 2 with
//                  the scores given and the thresholds read per stack from device memory;
//   finalize_rank  the step's form: the rank selections folded into the finalize launch, the
//                  same body reading its thresholds from LDS.
// The member mean of an ensemble target is loss_rows.h's member_mean, as in loss.hip's kernels.
// The mask carries no gradient, so ubpl_heatmap_row_grad serves the backward with out_w.
#include "loss_rows.h"

namespace {

constexpr int QNAN_BITS = 0x7fc00000;   // above every finite score's and +inf's bits as an int

__global__ void __launch_bounds__(256) zero_fill_kernel(int* __restrict__ p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

// grid (nchunk, B*S): block (c, bs) scores pixels [c*per, min((c+1)*per, HW)) of the K maps of (b,s)
template <int KT>
__global__ void __launch_bounds__(256) softmax_peak_kernel(const float* __restrict__ x, int64_t x_sb, int64_t x_ss,
                                                           int64_t x_sm, int M, int S, int K, int HW, int per,
                                                           int* __restrict__ score_bits) {
    __shared__ int red[4][KT];
    const int bs = blockIdx.y, b = bs / S, s = bs % S;
    const float* base = x + b * x_sb + s * x_ss;
    const int p0 = blockIdx.x * per, p1 = min(p0 + per, HW);
    float best[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) best[k] = 0.f;
    for (int i = p0 + threadIdx.x; i < p1; i += blockDim.x) {
        float v[KT];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            if (k < K) {
                v[k] = member_mean(base + (int64_t)k * HW + i, x_sm, M);
                mx = fmaxf(mx, v[k]);
            }
        }
        float sum = 0.f;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            if (k < K) {
                bad = bad || v[k] != v[k];          // (fmaxf drops a NaN: carry it by hand)
                v[k] = expf(v[k] - mx);
                sum += v[k];
            }
        }
        bad = bad || sum != sum;                    // +inf among the maps: exp(inf - inf)
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            if (k < K) {
                const float p = bad ? NAN : v[k] / sum;
                best[k] = (p > best[k] || p != p) ? p : best[k];   // NaN sticks
            }
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        if (k < K) {
            int bits = best[k] != best[k] ? QNAN_BITS : __float_as_int(best[k]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) bits = max(bits, __shfl_xor(bits, o, 64));
            if (lane == 0) red[wid][k] = bits;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        const int bits = max(max(red[0][k], red[1][k]), max(red[2][k], red[3][k]));
        atomicMax(score_bits + (int64_t)bs * K + k, bits);
    }
}

// The order torch.sort gives floats, as a signed integer key: ascending, -0 ties +0, NaNs last
// and tied with each other (no float's bits map to INT_MAX but a NaN's own).
__device__ __forceinline__ int order_key(float x) {
    if (x != x) return 0x7fffffff;
    const int b = x == 0.f ? 0 : __float_as_int(x);
    return b ^ ((b >> 31) & 0x7fffffff);
}

constexpr int RANK_MAX = 8192;   // one group's keys in LDS
constexpr int RANK_NT = 1024;

// The rank-th smallest (0-based) of the N scores x[(e / inner) * outer + e % inner], e < N, by the
// whole workgroup, without a sort: element i is the rank-th of the stable ascending order iff
// #{j : (key_j, j) < (key_i, i)} == rank — one 64-bit compare per pair, exactly one i, so one
// writer, and the value is exact under ties (a tie is a value; only -0 / +0 differ in bits, and
// the index order settles them as a stable sort does).  keys: RANK_MAX ints of LDS; *res (LDS or
// global) is valid after the caller's next barrier.
__device__ __forceinline__ void select_rank(const float* __restrict__ x, int inner, int64_t outer, int N, int rank,
                                            int* keys, float* res) {
    const int NP = (N + 3) & ~3;
    __syncthreads();                                   // (keys may still be read for the previous group)
    for (int e = threadIdx.x; e < NP; e += blockDim.x)
        keys[e] = e < N ? order_key(x[(int64_t)(e / inner) * outer + e % inner]) : 0x7fffffff;
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const int64_t ci = ((int64_t)keys[i] << 32) | (uint32_t)i;
        int cnt = 0;
        for (int j = 0; j < NP; j += 4) {              // the same address in every lane: a broadcast
            const int4 kj = *reinterpret_cast<const int4*>(keys + j);
            cnt += ((((int64_t)kj.x << 32) | (uint32_t)j) < ci) + ((((int64_t)kj.y << 32) | (uint32_t)(j + 1)) < ci) +
                   ((((int64_t)kj.z << 32) | (uint32_t)(j + 2)) < ci) + ((((int64_t)kj.w << 32) | (uint32_t)(j + 3)) < ci);
        }
        if (cnt == rank) *res = x[(int64_t)(i / inner) * outer + i % inner];
    }
}

// One workgroup per group of N <= RANK_MAX contiguous scores.
__global__ void __launch_bounds__(RANK_NT) rank_select_kernel(const float* __restrict__ scores, int N, int rank,
                                                              float* __restrict__ thr) {
    __shared__ __attribute__((aligned(16))) int keys[RANK_MAX];
    select_rank(scores + (int64_t)blockIdx.x * N, N, 0, N, rank, keys, thr + blockIdx.x);
}

// finalize_rows (loss_rows.h) for kinds 1 and 2 with the scores given and the thresholds per stack.
__global__ void __launch_bounds__(256) finalize_ranked_kernel(int kind, const float* __restrict__ sq_mean,
                                                             const float* __restrict__ ascore,
                                                             const float* __restrict__ tscore,
                                                             const float* __restrict__ athr,
                                                             const float* __restrict__ tthr,
                                                             const float* __restrict__ gate,
                                                             const float* __restrict__ sw, int use_gate, int use_sw,
                                                             int B, int S, int K, float* __restrict__ out_sum,
                                                             int* __restrict__ out_cnt, float* __restrict__ out_score,
                                                             float* __restrict__ out_w) {
    finalize_rows(kind, sq_mean, ascore, tscore, S, athr, tthr, gate, sw, use_gate, use_sw, B, S, K, out_sum, out_cnt,
                  out_score, out_w);
}

constexpr int RANK_MAX_STACKS = 16;

// The training step's form: the rank selection of every stack of both inputs folded into the
// finalize launch.  Per stack s the thresholds are the rank-th smallest of the batch's B*K scores
// ascore[b][s][k] (kind 2) and tscore[b][s or 0][k]; thr[0..S) = athr (NaN for kind 1), thr[S..2S) = tthr.
__global__ void __launch_bounds__(RANK_NT) finalize_rank_kernel(int kind, const float* __restrict__ sq_mean,
                                                                const float* __restrict__ ascore,
                                                                const float* __restrict__ tscore, int TS, int rank,
                                                                const float* __restrict__ gate,
                                                                const float* __restrict__ sw, int use_gate,
                                                                int use_sw, int B, int S, int K,
                                                                float* __restrict__ thr, float* __restrict__ out_sum,
                                                                int* __restrict__ out_cnt,
                                                                float* __restrict__ out_score,
                                                                float* __restrict__ out_w) {
    __shared__ __attribute__((aligned(16))) int keys[RANK_MAX];
    __shared__ float thr_s[2 * RANK_MAX_STACKS];
    const int N = B * K;
    if (threadIdx.x < S) thr_s[threadIdx.x] = NAN;
    for (int s = 0; s < S && kind == 2; ++s)
        select_rank(ascore + s * K, K, (int64_t)S * K, N, rank, keys, thr_s + s);
    for (int s = 0; s < TS; ++s) select_rank(tscore + s * K, K, (int64_t)TS * K, N, rank, keys, thr_s + S + s);
    __syncthreads();
    if (TS == 1 && threadIdx.x > 0 && (int)threadIdx.x < S) thr_s[S + threadIdx.x] = thr_s[S];
    __syncthreads();
    if ((int)threadIdx.x < 2 * S) thr[threadIdx.x] = thr_s[threadIdx.x];
    const float* athr = thr_s;
    finalize_rows(kind, sq_mean, ascore, tscore, TS, athr, athr + S, gate, sw, use_gate, use_sw, B, S, K, out_sum,
                  out_cnt, out_score, out_w);
}

}  // namespace

UBPL_API int ubpl_softmax_peak_scores(const float* x, int64_t x_sb, int64_t x_ss, int64_t x_sm, int M, int B, int S,
                                      int K, int HW, float* score, void* stream) {
    if (K < 1 || K > 32 || M < 1 || M > 8 || B < 0 || S < 0 || HW < 1) return (int)hipErrorInvalidValue;
    const int groups = B * S;
    if (groups == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    int* bits = reinterpret_cast<int*>(score);
    hipLaunchKernelGGL(zero_fill_kernel, dim3(ubpl::cdiv(groups * K, 256)), dim3(256), 0, st, bits, groups * K);
    UBPL_LAUNCH_CHECK();
    // enough workgroups to cover the chip a few times over, at least 256 pixels each
    const int want = ubpl::cdiv(4 * ubpl::cu_count(), groups);
    const int nchunk = max(1, min(ubpl::cdiv(HW, 256), want));
    const int per = ubpl::cdiv(ubpl::cdiv(HW, nchunk), 256) * 256;
    const dim3 grid(ubpl::cdiv(HW, per), groups);
    if (K <= 16)
        hipLaunchKernelGGL(softmax_peak_kernel<16>, grid, dim3(256), 0, st, x, x_sb, x_ss, x_sm, M, S, K, HW, per,
                           bits);
    else
        hipLaunchKernelGGL(softmax_peak_kernel<32>, grid, dim3(256), 0, st, x, x_sb, x_ss, x_sm, M, S, K, HW, per,
                           bits);
    UBPL_LAUNCH_CHECK();
    return 0;
}

UBPL_API int ubpl_rank_threshold(const float* scores, int G, int N, int rank, float* thr, void* stream) {
    if (G < 0 || N < 1 || N > RANK_MAX || rank < 0 || rank >= N) return (int)hipErrorInvalidValue;
    if (G == 0) return 0;
    hipLaunchKernelGGL(rank_select_kernel, dim3(G), dim3(RANK_NT), 0, (hipStream_t)stream, scores, N, rank, thr);
    UBPL_LAUNCH_CHECK();
    return 0;
}

UBPL_API int ubpl_loss_finalize_ranked(int kind, const float* sq_mean, const float* ascore, const float* tscore,
                                       const float* athr, const float* tthr, const float* gate, const float* sw,
                                       int use_gate, int use_sw, int B, int S, int K, float* out_sum, int* out_cnt,
                                       float* out_score, float* out_w, void* stream) {
    if (kind != 1 && kind != 2) return (int)hipErrorInvalidValue;
    if (tscore == nullptr || tthr == nullptr || (kind == 2 && (ascore == nullptr || athr == nullptr)))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(finalize_ranked_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, kind, sq_mean, ascore,
                       tscore, athr, tthr, gate, sw, use_gate, use_sw, B, S, K, out_sum, out_cnt, out_score, out_w);
    UBPL_LAUNCH_CHECK();
    return 0;
}

UBPL_API int ubpl_loss_finalize_rank(int kind, const float* sq_mean, const float* ascore, const float* tscore,
                                     int t_stacks, int rank, const float* gate, const float* sw, int use_gate,
                                     int use_sw, int B, int S, int K, float* thr, float* out_sum, int* out_cnt,
                                     float* out_score, float* out_w, void* stream) {
    if (kind != 1 && kind != 2) return (int)hipErrorInvalidValue;
    if (tscore == nullptr || thr == nullptr || (kind == 2 && ascore == nullptr)) return (int)hipErrorInvalidValue;
    if (B < 1 || K < 1 || S < 1 || S > RANK_MAX_STACKS || (t_stacks != 1 && t_stacks != S))
        return (int)hipErrorInvalidValue;
    if ((int64_t)B * K > RANK_MAX || rank < 0 || rank >= B * K) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(finalize_rank_kernel, dim3(1), dim3(RANK_NT), 0, (hipStream_t)stream, kind, sq_mean, ascore,
                       tscore, t_stacks, rank, gate, sw, use_gate, use_sw, B, S, K, thr, out_sum, out_cnt, out_score,
                       out_w);
    UBPL_LAUNCH_CHECK();
    return 0;
}
