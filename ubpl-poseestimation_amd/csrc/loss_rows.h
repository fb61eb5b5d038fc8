// What loss.hip and loss_rate.hip share: the row geometry of a (prediction, target) pair, the
// member-order mean of a target element, and the ONE finalize body behind ubpl_loss_finalize,
// ubpl_loss_finalize_ranked and ubpl_loss_finalize_rank.  Each entry keeps its own __global__
// kernel and block size, so every block_sum order is the entry's own; what a row's loss, mask,
// weight and counts ARE is written here once.
#pragma once
#include "common.h"

namespace {

struct RowGeom {
    const float* a;
    int64_t a_sb, a_ss;  // a row (b,s,k) at a + b*a_sb + s*a_ss + k*HW
    const float* t;
    int64_t t_sb, t_ss, t_sm;  // target row (b,s,k) = mean over m of t + m*t_sm + b*t_sb + s*t_ss + k*HW
    int M;
};

// Mean of the M members p[0], p[sm], ..., p[(M-1)*sm]: summed in member order, then one divide
// (none for M == 1).  Every kernel that reads an ensemble target goes through here, so a row's
// target and its softmax score see the same float.
__device__ __forceinline__ float member_mean(const float* p, int64_t sm, int M) {
    float acc = p[0];
    for (int m = 1; m < M; ++m) acc += p[(int64_t)m * sm];
    return M == 1 ? acc : acc / (float)M;
}

// The thresholds of a finalize, read as thr[s]: one scalar for every stack (ThrConst), or per
// stack from global memory or LDS (a plain const float*).
struct ThrConst {
    float v;
    __device__ __forceinline__ float operator[](int) const { return v; }
};

// kind 0: MSE / consistency   w = gate? * sw?                          (utils/losses.py:16-53)
// kind 1: teacher-confidence  w = gate? * sw? * [tscore >= tthr]       (utils/losses.py:255-286, 213-243)
// kind 2: UBPL pseudo mask    w = sw * [ascore >= athr] * [tscore >= tthr]  (utils/losses.py:73-210)
// kind 3: kind 2 with a given selection: w = sw * [gate > 0] * [ascore >= athr] * [tscore >= tthr];
//         the gate [B,K] is a row mask only (cnt[0] stays kind 2's S*B*K)
// cnt[0] = S * #{gate > 0}, cnt[1] = n_pseudo = #{pre-mask loss > 0},
// cnt[2] = n_sel = #{mask > 0}, cnt[3] = #{rows with sw > 0}.
// The scores are whatever the entry masks by (per-map maxima or softmax scores).  tscore holds TS
// stacks: S, or 1 when one target score per (b,k) serves every stack.  Any block size up to 1024.
template <class Thr>
__device__ __forceinline__ void finalize_rows(int kind, const float* __restrict__ sq_mean,
                                              const float* __restrict__ ascore, const float* __restrict__ tscore,
                                              int TS, Thr athr, Thr tthr, const float* __restrict__ gate,
                                              const float* __restrict__ sw, int use_gate, int use_sw, int B, int S,
                                              int K, float* __restrict__ out_sum, int* __restrict__ out_cnt,
                                              float* __restrict__ out_score, float* __restrict__ out_w) {
    __shared__ double dred[16];
    __shared__ int ired[16];
    const int rows = B * S * K;
    const bool both = kind >= 2;
    double lsum = 0.0;
    int n_pos = 0, n_sel = 0, n_gate = 0;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const int k = r % K, s = (r / K) % S, b = r / (K * S);
        const float gv = gate ? gate[b * K + k] : 1.f;
        const float sv = sw ? sw[b] : 1.f;
        float l = sq_mean[r];
        float m = 1.f;   // (a product of 0/1 factors: exact in any order)
        if (kind != 0) m = tscore[TS == 1 ? b * K + k : r] >= tthr[s] ? 1.f : 0.f;
        if (both) m *= ascore[r] >= athr[s] ? 1.f : 0.f;
        if (kind == 3) m *= gv > 0.f ? 1.f : 0.f;
        float wv = m;
        if (both) {
            if (sw) {
                l = l * sv;
                wv *= sv;
            }
        } else {
            if (use_gate) {
                l = l * gv;
                wv *= gv;
            }
            if (use_sw && sw) {
                l = l * sv;
                wv *= sv;
            }
        }
        n_pos += l > 0.f;
        n_sel += m > 0.f;
        lsum += (double)(l * m);
        out_w[r] = wv;
    }
    for (int r = threadIdx.x; r < B * K; r += blockDim.x) n_gate += (gate && kind != 3 ? gate[r] : 1.f) > 0.f;
    lsum = ubpl::block_sum(lsum, dred);
    n_pos = ubpl::block_sum(n_pos, ired);
    n_sel = ubpl::block_sum(n_sel, ired);
    n_gate = ubpl::block_sum(n_gate, ired);
    int n_rows = 0;
    for (int b = 0; b < B; ++b) n_rows += (sw ? sw[b] : 1.f) > 0.f;
    if (threadIdx.x == 0) {
        out_sum[0] = (float)lsum;
        out_cnt[0] = S * n_gate;
        out_cnt[1] = n_pos;
        out_cnt[2] = n_sel;
        out_cnt[3] = n_rows;
    }
    // per-keypoint mean score over rows with sw > 0 (utils/losses.py:152-159, :196-208, :275-285)
    if (out_score != nullptr && kind != 0) {
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            float acc_s = 0.f;
            for (int s = 0; s < S; ++s) {
                float sa = 0.f, st = 0.f;
                for (int b = 0; b < B; ++b) {
                    if ((sw ? sw[b] : 1.f) > 0.f) {
                        const int r = (b * S + s) * K + k;
                        if (both) sa += ascore[r];
                        st += tscore[TS == 1 ? b * K + k : r];
                    }
                }
                const float ma = n_rows > 0 ? sa / (float)n_rows : 0.f;
                const float mt = n_rows > 0 ? st / (float)n_rows : 0.f;
                acc_s += both ? (ma + mt) / 2.f : mt;
            }
            out_score[k] = acc_s / (float)S;
        }
    }
}

}  // namespace
