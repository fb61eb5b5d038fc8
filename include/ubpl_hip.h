/*
 * ubpl_hip.h — C-ABI of libubpl_hip.so, the MI355X (gfx950) hot path of
 * Qi2019KB/UBPL-PoseEstimation's semi-supervised pose training step.
 *
 * Conventions
 *   - plain pointers to DEVICE memory, sizes as int / int64_t, no torch types;
 *   - every function enqueues on `stream` (a hipStream_t, NULL = default
 *     stream), never synchronises, never allocates: scratch is caller-owned;
 *   - return 0 on success, otherwise a hipError_t code (e.g. 1 =
 *     hipErrorInvalidValue for an unsupported shape);
 *   - layouts are the reference's: NCHW float32 tensors, contiguous.
 *
 * Reference interfaces replaced (paths relative to the reference root) are
 * cited per entry.
 *
 * Argument annotations: the comment `/ *@ name:type[extent] ... * /` right
 * before a declaration gives each pointer argument its element type (f32,
 * f64, i32, i64, u16 = bf16 pieces, u8) and the number of elements the call
 * may touch, as a C expression of the integer arguments ("?" = not derivable
 * from them).
 *
 * This header is the only description of the ABI.  Its one parser,
 * ubpl-poseestimation_amd/ubpl_amd/_abi.py, derives both bindings from it: the
 * build generates the torch ops (one per entry; the annotations become their
 * argument checks of dtype, contiguity and storage extent, so a short tensor
 * raises there instead of being written out of bounds), through which the
 * Python host layer (ubpl-poseestimation_amd/ubpl_amd) makes every launch and
 * re-exposes the reference's module API; and the library loader builds the
 * ctypes signatures used for the host-only queries and the ABI tests.  The
 * parser reads declarations that start a line with their return type (int or
 * int64_t) and take int, int64_t, float, double and pointer parameters.
 */
#ifndef UBPL_HIP_H
#define UBPL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- R1 ----
 * ProcessUtils.kps_heatmap / kps_heatmap_mulKps (utils/process.py:252-318).
 * kps [N,K,3] (x, y, vis) in image pixels -> hm [N,K,size_h,size_w] with
 * size = int(img / (inp_res/out_res)); kps_out[...,2] = vis * visible
 * (may alias kps: the reference mutates kpsMap in place, :267). */
/*@ kps:f32[N*K*3] hm:f32[(int64_t)N*K*(int)(img_h/((double)inp_res/out_res))*(int)(img_w/((double)inp_res/out_res))] kps_out:f32[N*K*3] */
int ubpl_render_heatmaps(const float* kps, float* hm, float* kps_out, int N, int K, int img_h, int img_w,
                         int inp_res, int out_res, float kernel_size, float sigma, float cutoff, void* stream);

/* ---------------------------------------------------------------- L1-L4 --
 * Row statistics of mean_px((a - t)^2): a row (b,s,k) at a + b*a_sb + s*a_ss + k*HW;
 * target = mean over m < M of t + m*t_sm + b*t_sb + s*t_ss + k*HW.
 * Outputs [B*S*K]: sq_mean; amax = max_px a (nullable); tmax = max_px target (nullable).
 * JointMSELoss / JointDistLoss / JointDistLoss_mt2 / JointPseudoLoss3 forward
 * (utils/losses.py:16-53, 255-286, 176-210). */
/*@ a:f32[(B-1)*a_sb+(S-1)*a_ss+(int64_t)K*HW] t:f32[(M-1)*t_sm+(B-1)*t_sb+(S-1)*t_ss+(int64_t)K*HW] sq_mean:f32[B*S*K] amax:f32[B*S*K] tmax:f32[B*S*K] */
int ubpl_heatmap_row_stats(const float* a, int64_t a_sb, int64_t a_ss, const float* t, int64_t t_sb, int64_t t_ss,
                           int64_t t_sm, int M, int B, int S, int K, int HW, float* sq_mean, float* amax,
                           float* tmax, void* stream);
/* Loss reduction + counts on device.  kind 0 MSE/consistency, 1 teacher-
 * confidence mask (mt2), 2 UBPL pseudo mask, 3 UBPL pseudo mask with a given
 * selection: kind 2 in everything (l *= sw, the counts, out_score, out_w) but the
 * row mask, (gate[b*K+k] > 0) * (amax >= thr) * (tmax >= thr) — with thr = -inf
 * the selection alone decides (a NaN score still never selects); gate [B,K] is
 * required (hipErrorInvalidValue without).  out_sum[1] f32; out_cnt[4] int32 =
 * {nStack*#gate>0, n_pseudo, n_sel, #rows sw>0}; out_score[K] (kinds 1,2);
 * out_w[B*S*K] per-row weight for the backward. */
/*@ sq_mean:f32[B*S*K] amax:f32[B*S*K] tmax:f32[B*S*K] gate:f32[B*K] sw:f32[B] out_sum:f32[1] out_cnt:i32[4] out_score:f32[K] out_w:f32[B*S*K] */
int ubpl_loss_finalize(int kind, const float* sq_mean, const float* amax, const float* tmax, const float* gate,
                       const float* sw, int use_gate, int use_sw, int B, int S, int K, float thr, float* out_sum,
                       int* out_cnt, float* out_score, float* out_w, void* stream);
/* d a (+)= w_row * (*gscale) * extra * (a - target); gscale device scalar (nullable = 1). */
/*@ a:f32[(B-1)*a_sb+(S-1)*a_ss+(int64_t)K*HW] t:f32[(M-1)*t_sm+(B-1)*t_sb+(S-1)*t_ss+(int64_t)K*HW] w:f32[B*S*K] gscale:f32[1] da:f32[(B-1)*a_sb+(S-1)*a_ss+(int64_t)K*HW] */
int ubpl_heatmap_row_grad(const float* a, int64_t a_sb, int64_t a_ss, const float* t, int64_t t_sb, int64_t t_ss,
                          int64_t t_sm, int M, int B, int S, int K, int HW, const float* w, const float* gscale,
                          float extra, float* da, int accumulate, void* stream);

/* ------------------------------------------------------------- L2b-L2d ---
 * Softmax-score and rank-based pseudo-label selection: JointPseudoLoss, JointPseudoLoss2,
 * JointDistLoss_mt (utils/losses.py:73-115, 118-166, 213-243).
 *
 * The reference's confidence score of a map (:137-138): softmax ACROSS the K maps of (b,s) at
 * every pixel, then the per-map maximum.  Map (b,s,k) = mean over m < M of
 * x + m*x_sm + b*x_sb + s*x_ss + k*HW, summed in member order and divided by (float)M (the
 * target addressing of ubpl_heatmap_row_stats; M = 1: the maps themselves).
 * score[B*S*K] = max_px exp(v_k - max_j v_j) / sum_j exp(v_j - max_j v_j).  One read of x.
 * 1 <= K <= 32, 1 <= M <= 8 (hipErrorInvalidValue outside).  A NaN or +inf at a pixel makes
 * the K scores of its (b,s) NaN. */
/*@ x:f32[(M-1)*x_sm+(B-1)*x_sb+(S-1)*x_ss+(int64_t)K*HW] score:f32[B*S*K] */
int ubpl_softmax_peak_scores(const float* x, int64_t x_sb, int64_t x_ss, int64_t x_sm, int M, int B, int S, int K,
                             int HW, float* score, void* stream);
/* thr[g] = the rank-th smallest (0-based) of scores[g*N .. g*N+N), bit for bit
 * torch.sort(scores[g])[0][rank]: ties are values, NaNs order last.  One workgroup per group,
 * by counting.  1 <= N <= 8192, 0 <= rank < N (hipErrorInvalidValue outside). */
/*@ scores:f32[(int64_t)G*N] thr:f32[G] */
int ubpl_rank_threshold(const float* scores, int G, int N, int rank, float* thr, void* stream);
/* ubpl_loss_finalize for kinds 1 and 2 with the scores given and the thresholds read from
 * device memory per stack: row mask (ascore >= athr[s]) * (tscore >= tthr[s]) for kind 2,
 * tscore >= tthr[s] for kind 1 (ascore, athr nullable).  A NaN score or threshold never
 * selects.  Outputs as ubpl_loss_finalize's (out_score from the given scores, nullable), so
 * ubpl_heatmap_row_grad serves the backward with out_w. */
/*@ sq_mean:f32[B*S*K] ascore:f32[B*S*K] tscore:f32[B*S*K] athr:f32[S] tthr:f32[S] gate:f32[B*K] sw:f32[B] out_sum:f32[1] out_cnt:i32[4] out_score:f32[K] out_w:f32[B*S*K] */
int ubpl_loss_finalize_ranked(int kind, const float* sq_mean, const float* ascore, const float* tscore,
                              const float* athr, const float* tthr, const float* gate, const float* sw,
                              int use_gate, int use_sw, int B, int S, int K, float* out_sum, int* out_cnt,
                              float* out_score, float* out_w, void* stream);
/* The training step's form of the two above in one launch: per stack s the thresholds are the
 * rank-th smallest of the batch's B*K scores ascore[b][s][k] (kind 2) and tscore[b][s][k];
 * tscore holds t_stacks = S stacks, or 1 when one target map per (b,k) serves every stack.
 * thr[2*S] receives them: athr[S] (NaN for kind 1), then tthr[S].  Everything else as
 * ubpl_loss_finalize_ranked.  B*K <= 8192, 0 <= rank < B*K, S <= 16 (hipErrorInvalidValue outside). */
/*@ sq_mean:f32[B*S*K] ascore:f32[B*S*K] tscore:f32[B*t_stacks*K] gate:f32[B*K] sw:f32[B] thr:f32[2*S] out_sum:f32[1] out_cnt:i32[4] out_score:f32[K] out_w:f32[B*S*K] */
int ubpl_loss_finalize_rank(int kind, const float* sq_mean, const float* ascore, const float* tscore, int t_stacks,
                            int rank, const float* gate, const float* sw, int use_gate, int use_sw, int B, int S,
                            int K, float* thr, float* out_sum, int* out_cnt, float* out_score, float* out_w,
                            void* stream);

/* ---------------------------------------------------------------- L5 ----
 * ProcessUtils.features_cov (utils/process.py:18-31) over rows whose
 * rowmask[b] > 0 (the caller's labeled-row selection, projects/MT_UBPL.py:309-320).
 * f1,f2 [B,S,C,HW]; cov/mu1/mu2 [B*S*C] scratch; out_val[1] = mean |cov|;
 * out_cnt[1] = #selected * S * C. */
/*@ f1:f32[(int64_t)B*S*C*HW] f2:f32[(int64_t)B*S*C*HW] rowmask:f32[B] cov:f32[B*S*C] mu1:f32[B*S*C] mu2:f32[B*S*C] out_val:f32[1] out_cnt:i32[1] */
int ubpl_fdl_cov_forward(const float* f1, const float* f2, const float* rowmask, int B, int S, int C, int HW,
                         float* cov, float* mu1, float* mu2, float* out_val, int* out_cnt, void* stream);
/*@ f1:f32[(int64_t)B*S*C*HW] f2:f32[(int64_t)B*S*C*HW] rowmask:f32[B] cov:f32[B*S*C] mu1:f32[B*S*C] mu2:f32[B*S*C] cnt:i32[1] gscale:f32[1] d1:f32[(int64_t)B*S*C*HW] d2:f32[(int64_t)B*S*C*HW] */
int ubpl_fdl_cov_backward(const float* f1, const float* f2, const float* rowmask, const float* cov, const float* mu1,
                          const float* mu2, const int* cnt, const float* gscale, int B, int S, int C, int HW,
                          float* d1, float* d2, int accumulate, void* stream);

/* ---------------------------------------------------------------- D1-D4 --
 * get_preds + final_preds + kps_fromHeatmap (utils/udaap/evaluation.py:13-30,215-238;
 * utils/process.py:320-327).  tinv [N,6] f64 = rows 0-1 of inv(get_transform)
 * (nullable: no transform).  raw/preds [N,K,2], scores [N,K] (each nullable). */
/*@ hm:f32[(int64_t)N*K*H*W] tinv:f64[N*6] raw:f32[N*K*2] preds:f32[N*K*2] scores:f32[N*K] */
int ubpl_decode_heatmaps(const float* hm, int N, int K, int H, int W, const double* tinv, float* raw, float* preds,
                         float* scores, void* stream);
/* Flip test fused into the decode: the heatmaps of the mirrored image flipped
 * back (utils/augment.py:239-252 fliplr_back / fliplr_back_tensor), their
 * left/right joints swapped (utils/udaap/transforms.py:20-57 flip_back),
 * averaged with the image's own and decoded as ubpl_decode_heatmaps does, in
 * one read of both sets.  Map (n, k) of hm starts at hm + n*sb + k*H*W (sb: the
 * batch stride in floats, so the last stack of a [B,S,K,H,W] output is decoded
 * in place); hm_flip likewise.  merged[n,k,y,x] = (hm[n,k,y,x] +
 * hm_flip[n,perm[k],y,W-1-x]) * 0.5f; perm int32 [K], null = identity (the
 * reference's own convention: kps_fliplr, utils/process.py:239-242, mirrors x
 * and swaps nothing), entries in [0, K); hm_flip null: merged = hm (a strided
 * plain decode).  merged [N,K,H,W] contiguous, raw, preds, scores, tinv nullable. */
/*@ hm:f32[(N-1)*sb+(int64_t)K*H*W] hm_flip:f32[(N-1)*sb+(int64_t)K*H*W] perm:i32[K] tinv:f64[N*6] merged:f32[(int64_t)N*K*H*W] raw:f32[N*K*2] preds:f32[N*K*2] scores:f32[N*K] */
int ubpl_decode_heatmaps_flip(const float* hm, const float* hm_flip, int64_t sb, int N, int K, int H, int W,
                              const int* perm, const double* tinv, float* merged, float* raw, float* preds,
                              float* scores, void* stream);
/* UBPL ensemble pseudo-labels at inference: JointPseudoLoss3's target and mask
 * (utils/losses.py:176-210) from one read of M members' heatmaps.  Member m's
 * map (n, k) starts at hm + m*sm + n*sb + k*H*W (strides in floats: a
 * [M,N,K,H,W] buffer, or the last stacks of [M,B,S,K,H,W], in place);
 * 1 <= M <= 8 (hipErrorInvalidValue otherwise).  Per pixel
 * T = (((p_0 + p_1) + ...) + p_{M-1}) / (float)M (targets.mean(0), :179), to
 * mean_hm [N,K,H,W].  Per map: ens_raw / ens_preds [N,K,2], ens_score [N,K] =
 * the decode of T as ubpl_decode_heatmaps does; member_score [M,N,K] =
 * max_px p_m (s1 of :187, the member in the student's place); disagree
 * [M,N,K] = mean_px (p_m - T)^2 (:184), f32, a fixed summation order; select
 * [M,N,K] = (member_score >= thr) * (ens_score >= thr) as 0/1 (:187-193; a
 * NaN score never selects).  thr: device f32[1], read by the kernel, so a
 * captured graph serves every threshold.  tinv, mean_hm and every output but
 * select are nullable (ens_preds needs tinv). */
/*@ hm:f32[(M-1)*sm+(N-1)*sb+(int64_t)K*H*W] tinv:f64[N*6] thr:f32[1] mean_hm:f32[(int64_t)N*K*H*W] ens_raw:f32[N*K*2] ens_preds:f32[N*K*2] ens_score:f32[N*K] member_score:f32[(int64_t)M*N*K] disagree:f32[(int64_t)M*N*K] select:f32[(int64_t)M*N*K] */
int ubpl_ensemble_pseudo(const float* hm, int64_t sm, int64_t sb, int M, int N, int K, int H, int W,
                         const double* tinv, const float* thr, float* mean_hm, float* ens_raw, float* ens_preds,
                         float* ens_score, float* member_score, float* disagree, float* select, void* stream);
/* Sub-pixel refinement of decoded peaks, a post-pass after any of the decodes
 * above.  hm, hm_flip, sb and perm as in ubpl_decode_heatmaps_flip; the value
 * at (y, x) of map (n, k) is v(y,x) = (hm[..] + hm_flip[n,perm[k],y,W-1-x]) *
 * 0.5f (hm_flip null: hm[..]) — the decode's own expression — and 0 outside
 * the map.  raw [N,K,2]: the 1-based integer peaks the decode wrote, (0,0) =
 * no peak.  mode 1 = quarter, 2 = Taylor (anything else:
 * hipErrorInvalidValue).  taps: device f32 w[0..radius], the half of a
 * symmetric separable blur kernel (radius 0, taps {1}: no blur), 0 <= radius
 * <= 5.  Per map, with c = raw_x - 1, r = raw_y - 1; every comparison is
 * false on a NaN, so a non-finite window only falls back:
 *   rule 0   raw outside [1,W]x[1,H] (the (0,0) of no peak included) or not
 *            v(r,c) > 0: how = 0, raw_sub = raw.
 *   Taylor   (mode 2, 2 <= c <= W-3 and 2 <= r <= H-3) b(dy,dx), dy, dx in
 *            [-2,2]: v blurred along x, then along y; each pass is w[0] x(0) +
 *            sum_{j=1..radius} w[j] (x(-j) + x(+j)) in f32, ascending j.
 *            L = logf(fmaxf(b, 1e-10f));
 *            gx = (L(0,1) - L(0,-1))/2, gy = (L(1,0) - L(-1,0))/2,
 *            dxx = (L(0,2) - 2 L(0,0) + L(0,-2))/4, dyy likewise,
 *            dxy = (L(1,1) - L(-1,1) - L(1,-1) + L(-1,-1))/4, det = dxx dyy -
 *            dxy^2.  If dxx < 0 and det > 0: ox = -(dyy gx - dxy gy)/det, oy =
 *            -(dxx gy - dxy gx)/det, and if |ox| <= 1 and |oy| <= 1: how = 2.
 *            (The distribution-aware decode; the blurred map's rescale to the
 *            original maximum is a constant in log space and is dropped.)
 *   quarter  (otherwise: mode 1, and the fallback of mode 2) on unblurred
 *            values: ox = 0.25 sign(v(r,c+1) - v(r,c-1)) when 1 <= c <= W-2,
 *            else 0; oy likewise on rows; sign(0) = sign(NaN) = 0; how = 1 if
 *            either axis was eligible, else 0.
 * raw_sub [N,K,2] = (raw_x + ox, raw_y + oy); preds_sub [N,K,2] = (t0 u + t1 v +
 * t2 + 1, t3 u + t4 v + t5 + 1), u = raw_sub_x - 1, v = raw_sub_y - 1, in f64
 * with the decode's un-fused multiply/add order, rounded to f32 and NOT
 * truncated (the decode's preds is the truncation of this expression at ox =
 * oy = 0); how [N,K] = the rule taken, {0, 1, 2} as floats.  tinv, preds_sub
 * and how are nullable (preds_sub needs tinv).  No atomics, fixed summation
 * order: repeated launches give equal bits. */
/*@ hm:f32[(N-1)*sb+(int64_t)K*H*W] hm_flip:f32[(N-1)*sb+(int64_t)K*H*W] perm:i32[K] raw:f32[N*K*2] taps:f32[radius+1] tinv:f64[N*6] raw_sub:f32[N*K*2] preds_sub:f32[N*K*2] how:f32[N*K] */
int ubpl_refine_peaks(const float* hm, const float* hm_flip, int64_t sb, int N, int K, int H, int W,
                      const int* perm, const float* raw, int mode, const float* taps, int radius,
                      const double* tinv, float* raw_sub, float* preds_sub, float* how, void* stream);
/* Multi-view test-time augmentation.  The reference computes a warp matrix per
 * augmented view (utils/augment.py:158-164 affine_getWarpmat) and can warp a
 * view's heatmaps back (affine_back2, :36-47: F.affine_grid / F.grid_sample
 * with align_corners=True, then the flip-back), used by a debug drawing only
 * (projects/MT_UBPL.py:186-205).  Both entries take PIXEL-space 2x3 matrices,
 * output pixel -> source pixel, row-major (m0 .. m5), built on the host in f64
 * and rounded to f32, the mirror folded in (kernels.view_matrices;
 * kernels.affine_theta_to_pixels converts affine_grid's normalised convention).
 * The one sampling rule of a plane p [H,W] at output pixel (x, y) under m, every
 * product, sum and quotient its own f32 rounding (no FMA):
 *   sx = (m0*x + m1*y) + m2,  sy = (m3*x + m4*y) + m5;
 *   outside unless -1 < sx < W and -1 < sy < H (a NaN or an infinity is
 *   outside; tested before any float -> int conversion): s = 0, cov = 0;
 *   x0 = floorf(sx), ax = sx - x0, bx = 1 - ax, y0, ay, by likewise; the taps
 *   v00 = p[y0,x0], v01 = p[y0,x0+1], v10 = p[y0+1,x0], v11 = p[y0+1,x0+1],
 *   each 0 where its index is outside the plane;
 *   top = v00*bx + v01*ax, bot = v10*bx + v11*ax, s = top*by + bot*ay;
 *   cov = the same formula over the taps' in-bounds indicators (1 / 0);
 *   a matrix that is exactly (1,0,0,0,1,0): s = p[y,x], cov = 1, no arithmetic.
 * ubpl_warp_views: src [N,C,H,W], mat [V,6] -> out [V,N,C,H,W], out[v] = s of
 * every plane under mat[v] (an identity view is a copy). */
/*@ src:f32[(int64_t)N*C*H*W] mat:f32[V*6] out:f32[(int64_t)V*N*C*H*W] */
int ubpl_warp_views(const float* src, int N, int C, int H, int W, const float* mat, int V, float* out,
                    void* stream);
/* ubpl_decode_heatmaps_views: view v's map (n, k) starts at hm + v*sv + n*sb +
 * k'*H*W (strides in floats: the last stacks of a view-major [V*N,S,K,H,W]
 * output in place with sv = N*sb), k' = perm[k] where swap[v] != 0, else k
 * (swap int32 [V], null = none; perm int32 [K], null = identity, an entry
 * outside [0, K) falls back to k).  1 <= V <= 16 (hipErrorInvalidValue
 * otherwise).  Per output pixel, views in ascending v: num = s_0, den = cov_0,
 * then num = num + s_v, den = den + cov_v (sequential f32 sums); merged = num /
 * den (one IEEE f32 division) where den > 0, else 0 — a pixel a rotated or
 * zoomed view does not cover is averaged over the views that cover it.  So V =
 * 1 with the identity matrix is the plain strided decode (NaN and inf rules
 * included), and identity + mirror is ubpl_decode_heatmaps_flip's (a + b) *
 * 0.5f.  merged [N,K,H,W] (nullable); raw, preds, scores, tinv as in
 * ubpl_decode_heatmaps_flip, decoded from the same registers.  No atomics, no
 * cross-pixel sums: repeated launches give equal bits. */
/*@ hm:f32[(V-1)*sv+(N-1)*sb+(int64_t)K*H*W] mat:f32[V*6] swap:i32[V] perm:i32[K] tinv:f64[N*6] merged:f32[(int64_t)N*K*H*W] raw:f32[N*K*2] preds:f32[N*K*2] scores:f32[N*K] */
int ubpl_decode_heatmaps_views(const float* hm, int64_t sv, int64_t sb, int V, int N, int K, int H, int W,
                               const float* mat, const int* swap, const int* perm, const double* tinv,
                               float* merged, float* raw, float* preds, float* scores, void* stream);
/* View-consistency uncertainty of multi-view predictions: the reference's
 * geometric pseudo-label uncertainty (utils/business.py: pseudo_cal_unc
 * :220-234, _initKSample :302-318, _calKSampleExterData :320-346,
 * pseudo_filter_mixUnc :237-264, assess_pseudo_unc2 :109-161;
 * utils/process.py:53-68 coord_distance / coord_avgDistance) from the per-view
 * peaks of M members (teachers) on V views of N samples, in one launch.
 * Member m's point of view v, sample n, output joint k is the pair of floats
 * at raw + m*sm + ((v*N + n)*K + k')*2 (sm: the member stride in floats; per
 * member a view-major [V*N,K,2] block as ubpl_decode_heatmaps_flip or
 * ubpl_refine_peaks writes it with N' = V*N), k' = perm[k] where swap[v] != 0,
 * else k (swap int32 [V], null = none; perm int32 [K], null = identity, an
 * entry outside [0, K) falls back to k: ubpl_decode_heatmaps_views' rule).
 * Points are 1-based heatmap coordinates in the view's own frame, integer or
 * sub-pixel; (0,0) = no peak.  1 <= M <= 8 and 2 <= V <= 16
 * (hipErrorInvalidValue otherwise).  back [V,6] f32: view heatmap pixel ->
 * original-frame heatmap pixel, the f64 inverse of ubpl_decode_heatmaps_views'
 * mat rounded once (kernels.view_back_matrices).  dist_thr: device f32[1], read
 * by the kernel, so a captured graph serves every threshold.  Every product,
 * sum, quotient and square root below is its own f32 rounding (no FMA) unless
 * f64 is named; every comparison is false on a NaN.
 * Per point:  u = raw_x - 1, v = raw_y - 1;  ox = (b0*u + b1*v) + b2,
 *   oy = (b3*u + b4*v) + b5.  Without tinv the point is p = (ox + 1, oy + 1),
 *   heatmap cells.  With tinv [N,6] it is ubpl_refine_peaks' preds_sub
 *   expression at u = ox, v = oy: (t0 u + t1 v + t2 + 1, t3 u + t4 v + t5 + 1)
 *   in f64 with the decode's un-fused order, rounded to f32, not truncated:
 *   image coordinates.  pts [M,V,N,K,2] = p, whatever its legality.  A point is
 *   legal iff raw is not (0,0), both coordinates of p are finite and, with
 *   tinv, both are >= 0 (coord_legal, business.py:31).
 * Per member (m, n, k):  legal [M,N,K] = 1 iff all V points are legal
 *   (_checkGroupLegal), else 0.  With d(p, q) = sqrtf(dx*dx + dy*dy):
 *   int_dist [M,N,K] = (sum of d over the V(V-1)/2 view pairs (a, b), a < b, in
 *   itertools.combinations order, sequentially from 0) / (float)pairs
 *   (coord_avgDistance); aug_coord [M,N,K,2] = (sequential sum of the V points
 *   from 0) / (float)V (coord_aug, :313).  Not legal: int_dist = mix_dist = unc
 *   = 999 (the reference's sentinel), aug_coord = (-1,-1), select = 0.
 * Per (n, k), over the member pairs a < b with both legal, ascending, each a
 *   sequential sum from 0 divided by (float)count:  ext_dist [N,K] = mean of
 *   d(p_a0, p_b0), the view-0 points (extDist, :322); aext_dist [N,K] = mean of
 *   d(aug_coord_a, aug_coord_b) (aExtDist, :323); ext_views [N,K] = mean over
 *   pairs of ((sum over views v of d(p_av, p_bv), sequentially from 0) /
 *   (float)V) (assess_pseudo_unc2's extDist, :144-149).  For M = 2 each is the
 *   reference's value.  M >= 2 and no legal pair: all three 999; M = 1: all 0.
 * Per legal member:  mix_dist [M,N,K] = int_dist + (ext_dist > 0 ? (ext_dist +
 *   aext_dist)/2 : aext_dist) (:328); unc [M,N,K] = 1 - expf(-mix_dist/5)
 *   (_calUncValue); select [M,N,K] = 1 iff int_dist <= t, ext_dist <= t,
 *   aext_dist <= t (:331-345) and mix_dist <= 3*t, t = dist_thr[0], else 0.
 *   1 - exp(-x/5) is monotonic, so the last condition is the reference's
 *   unc <= _calUncValue(3 * distThrMax) (:242-247) decided on the distance,
 *   where no rounding of expf can flip it.
 * The reference's running average over epochs (_lma_variables, :397-406) is
 * the identity on a first call, which is what one inference pass is: the
 * *_lma values are the values themselves and no history is kept.  The scores
 * of _initKSample (:309-311) index batch row 0 and feed no distance: left out.
 * tinv and every output but select are nullable.  No atomics, fixed summation
 * orders: repeated launches give equal bits. */
/*@ raw:f32[(M-1)*sm+(int64_t)V*N*K*2] back:f32[V*6] swap:i32[V] perm:i32[K] tinv:f64[N*6] dist_thr:f32[1] pts:f32[(int64_t)M*V*N*K*2] legal:f32[(int64_t)M*N*K] int_dist:f32[(int64_t)M*N*K] aug_coord:f32[(int64_t)M*N*K*2] ext_dist:f32[N*K] aext_dist:f32[N*K] ext_views:f32[N*K] mix_dist:f32[(int64_t)M*N*K] unc:f32[(int64_t)M*N*K] select:f32[(int64_t)M*N*K] */
int ubpl_view_uncertainty(const float* raw, int64_t sm, int M, int V, int N, int K, const float* back,
                          const int* swap, const int* perm, const double* tinv, const float* dist_thr, float* pts,
                          float* legal, float* int_dist, float* aug_coord, float* ext_dist, float* aext_dist,
                          float* ext_views, float* mix_dist, float* unc, float* select, void* stream);
/* The same rule where every (view, sample) has its own matrix: the training
 * step's two augmented views, each with its own random flip, scale and
 * rotation (the setting utils/business.py pseudo_cal_unc was written for).  It
 * shares ubpl_view_uncertainty's device code and differs in four things:
 *   back [V][N][6] f32: point (m, v, n, k) is mapped by back + (v*N + n)*6;
 *   raw has a member stride sm and a view stride sv, in floats: the point is the
 *   pair at raw + m*sm + v*sv + (n*K + k)*2, so a [V][M][N][K][2] buffer (sm =
 *   N*K*2, sv = M*N*K*2) is filled by one decode launch per view, and
 *   ubpl_view_uncertainty's view-major member blocks are sm = V*N*K*2, sv =
 *   N*K*2.  sv >= N*K*2; with M > 1, sm >= N*K*2 and the blocks nest one way or
 *   the other: sm >= (V-1)*sv + N*K*2 or sv >= (M-1)*sm + N*K*2
 *   (hipErrorInvalidValue otherwise);
 *   no swap / perm (the reference's training flip, kps_fliplr, mirrors x and
 *   swaps no joints) and no tinv: p = (ox + 1, oy + 1), in whatever frame back
 *   maps to (kernels.train_back_matrices: source-image pixels), legal iff raw is
 *   not (0,0) and p is finite;
 *   gate [N,K] (nullable) = 1 iff select is 1 for every member m < M, else 0:
 *   the unc_select.all(0) of Predictor.pseudo_label(rule="uncertainty").
 * Everything else — legality, the 999 sentinel, int_dist, aug_coord, ext_dist,
 * aext_dist, ext_views, mix_dist, unc, select, the sequential f32 sums without
 * FMA, dist_thr read from the device, 1 <= M <= 8, 2 <= V <= 16, no atomics — is
 * the rule above, word for word.  Every output but select is nullable. */
/*@ raw:f32[(M-1)*sm+(V-1)*sv+(int64_t)N*K*2] back:f32[(int64_t)V*N*6] dist_thr:f32[1] pts:f32[(int64_t)M*V*N*K*2] legal:f32[(int64_t)M*N*K] int_dist:f32[(int64_t)M*N*K] aug_coord:f32[(int64_t)M*N*K*2] ext_dist:f32[N*K] aext_dist:f32[N*K] ext_views:f32[N*K] mix_dist:f32[(int64_t)M*N*K] unc:f32[(int64_t)M*N*K] select:f32[(int64_t)M*N*K] gate:f32[N*K] */
int ubpl_view_uncertainty_samples(const float* raw, int64_t sm, int64_t sv, int M, int V, int N, int K,
                                  const float* back, const float* dist_thr, float* pts, float* legal,
                                  float* int_dist, float* aug_coord, float* ext_dist, float* aext_dist,
                                  float* ext_views, float* mix_dist, float* unc, float* select, float* gate,
                                  void* stream);
/* Cross-view pseudo-label targets: ubpl_decode_heatmaps_views' merge where every
 * (target view, source view, sample) has its own matrix, and every view is a
 * target — the training step's augmented views warped into one another's frames
 * (the plumbing the reference ships and calls from a debug drawing only:
 * warpmat per view, utils/augment.py:158-164; affine_back2, :36-47).
 * View v, member m, sample n, joint k is the plane at hm + v*sv + m*sm + n*sb +
 * k*H*W (strides in floats: the last stacks of [.., S, K, H, W] outputs are read
 * in place).  mat [V][V][N][6] f32: mat[a][v][n] maps a 0-based cell of target
 * view a to a 0-based cell of source view v, a pixel matrix in the convention
 * above (kernels.train_pair_matrices).  Per element out[a][m][n][k][y][x], over
 * the source views in ascending v:
 *   v == a: with include_self != 0, s = p[y,x], c = 1 (the diagonal of mat is
 *           never read); with include_self == 0 the view is skipped;
 *   v != a: an exactly-identity matrix takes s = p[y,x], c = 1; otherwise (s, c)
 *           = (s, cov) of the one sampling rule above under mat[a][v][n] (un-fused
 *           f32, zero taps outside, a NaN or infinite position is outside).
 *   The first contributing view sets num = s, den = c; later ones num = num + s,
 *   den = den + c (sequential f32 sums); out = num / den (one IEEE f32 division)
 *   where den > 0, else 0: ubpl_decode_heatmaps_views' rule, word for word.
 * cover [V][N][H][W] (nullable) = den, written once, not per plane.
 * 1 <= V <= 16, 1 <= M <= 8, include_self == 0 needs V >= 2, strides >= 0 and
 * >= K*H*W wherever their count exceeds 1, out non-null (hipErrorInvalidValue
 * otherwise).  out must not overlap hm.  No atomics, no cross-pixel sums:
 * repeated launches give equal bits. */
/*@ hm:f32[(V-1)*sv+(M-1)*sm+(N-1)*sb+(int64_t)K*H*W] mat:f32[(int64_t)V*V*N*6] out:f32[(int64_t)V*M*N*K*H*W] cover:f32[(int64_t)V*N*H*W] */
int ubpl_merge_views_samples(const float* hm, int64_t sv, int64_t sm, int64_t sb, int V, int M, int N, int K,
                             int H, int W, const float* mat, int include_self, float* out, float* cover, void* stream);
/* EvaluationUtils.acc_pck (utils/evaluation.py:91-139).  errs/accs [K+1];
 * hits/valid [K] int32 (nullable) for cross-rank aggregation. */
/*@ preds:f32[N*K*2] gts:f32[N*K*3] errs:f32[K+1] accs:f32[K+1] hits:i32[K] valid:i32[K] */
int ubpl_pck(const float* preds, const float* gts, int N, int K, int ref0, int ref1, float thr, float* errs,
             float* accs, int* hits, int* valid, void* stream);

/* ---------------------------------------------------------------- E1 ----
 * update_ema_variables (utils/parameters.py:4-8) on a flat parameter buffer. */
/*@ ema:f32[n] p:f32[n] */
int ubpl_ema_update(float* ema, const float* p, int64_t n, double alpha, void* stream);
/* torch.optim.AdamW step (the optimizer projects/MT_UBPL.py:48 builds) on flat buffers. */
/*@ p:f32[n] g:f32[n] m:f32[n] v:f32[n] */
int ubpl_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                    double eps, double weight_decay, int64_t step, void* stream);
/* The same step with the 1-based step count on the device (incremented by the
 * call), so a captured HIP graph of the training step replays it; coef: 4 floats. */
/*@ p:f32[n] g:f32[n] m:f32[n] v:f32[n] step:i64[1] coef:f32[4] */
int ubpl_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1,
                        double beta2, double eps, double weight_decay, int64_t* step, float* coef, void* stream);
/* ubpl_adamw_step_dev on p[0, nlive) fused with ubpl_ema_update(ema, p, n) in
 * one pass (the optimizer step of projects/MT_UBPL.py:338-340 followed by
 * update_ema_variables, utils/parameters.py:4-8); bit-identical to the two
 * calls.  nlive, n multiples of 4; buffers 16-B aligned. */
/*@ p:f32[n] g:f32[nlive] m:f32[nlive] v:f32[nlive] step:i64[1] coef:f32[4] ema:f32[n] */
int ubpl_adamw_ema_step_dev(float* p, const float* g, float* m, float* v, int64_t nlive, double lr, double beta1,
                            double beta2, double eps, double weight_decay, int64_t* step, float* coef, float* ema,
                            int64_t n, double alpha, void* stream);
/*@ x:f32[n] */
int ubpl_scale_(float* x, int64_t n, float s, void* stream);

/* Guarded optimizer step: global gradient-norm clip (torch.nn.utils.clip_grad_norm_)
 * and a non-finite guard, all through device memory so a captured step replays it.
 * ubpl_grad_guard reads the gradient prefix g[0, n) once (n a multiple of 4, g 16-B
 * aligned; part: ubpl_grad_guard_scratch(n) doubles of caller-owned scratch) and writes
 * guard[4] = {c, norm, skip, 0}: the squares are summed in f64 in a fixed order (equal
 * input, equal bits); skip = 1.0 iff the sum is not finite (some element is inf or NaN);
 * c = min(1, max_norm / (norm + 1e-6)) in f64 rounded once, 1 when max_norm <= 0 or the
 * step is skipped; norm is the f32 rounding of the f64 L2 norm.  n == 0: {1, 0, 0, 0}. */
int64_t ubpl_grad_guard_scratch(int64_t n);
/*@ g:f32[n] part:f64[ubpl_grad_guard_scratch(n)] guard:f32[4] */
int ubpl_grad_guard(const float* g, int64_t n, double max_norm, double* part, float* guard, void* stream);
/* ubpl_adamw_step_dev / ubpl_adamw_ema_step_dev under such a guard: the gradient is
 * taken as g * guard[0] (one f32 product in registers; g is not written), so guard[0] == 1
 * is bit-identical to the unguarded entry and any other value to ubpl_scale_(g, c)
 * followed by it.  When guard[2] != 0 the step count, p, m and v are untouched and
 * skipped[0] (total) and skipped[1] (consecutive) are incremented; a step that runs
 * zeroes skipped[1].  The EMA half runs either way (toward the unchanged student on a
 * skipped step: ubpl_ema_update alone). */
/*@ p:f32[n] g:f32[n] m:f32[n] v:f32[n] step:i64[1] coef:f32[4] guard:f32[4] skipped:i64[2] */
int ubpl_adamw_step_guarded_dev(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1,
                                double beta2, double eps, double weight_decay, int64_t* step, float* coef,
                                const float* guard, int64_t* skipped, void* stream);
/*@ p:f32[n] g:f32[nlive] m:f32[nlive] v:f32[nlive] step:i64[1] coef:f32[4] ema:f32[n] guard:f32[4] skipped:i64[2] */
int ubpl_adamw_ema_step_guarded_dev(float* p, const float* g, float* m, float* v, int64_t nlive, double lr,
                                    double beta1, double beta2, double eps, double weight_decay, int64_t* step,
                                    float* coef, float* ema, int64_t n, double alpha, const float* guard,
                                    int64_t* skipped, void* stream);
/* dst[0, n) = saved[0, n) when guard[2] != 0, else nothing (BatchNorm running
 * statistics after a skipped step). */
/*@ dst:f32[n] saved:f32[n] guard:f32[4] */
int ubpl_restore_if(float* dst, const float* saved, int64_t n, const float* guard, void* stream);

/* ---------------------------------------------------------------- H2-H4 --
 * BatchNorm2d (models/base/layers.py:41,57-61), train-mode statistics.
 * part: scratch of ubpl_bn_part_doubles(B,C) doubles, ZEROED before its first
 * use (arrival counters for C <= 512 channels at its head, which each call
 * leaves at zero, then the partial sums; one call at a time per scratch).  rmean/rvar updated with momentum
 * (nullable).  scale = gamma*invstd, shift = beta - mean*scale. */
int64_t ubpl_bn_part_doubles(int B, int C);
/*@ x:f32[(int64_t)B*C*HW] gamma:f32[C] beta:f32[C] rmean:f32[C] rvar:f32[C] part:f64[ubpl_bn_part_doubles(B,C)] mean_out:f32[C] invstd_out:f32[C] scale:f32[C] shift:f32[C] */
int ubpl_bn_forward_stats(const float* x, int B, int C, int HW, const float* gamma, const float* beta, float eps,
                          float momentum, float* rmean, float* rvar, double* part, float* mean_out,
                          float* invstd_out, float* scale, float* shift, void* stream);
/*@ gamma:f32[C] beta:f32[C] rmean:f32[C] rvar:f32[C] scale:f32[C] shift:f32[C] */
int ubpl_bn_eval_coeffs(const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                        int C, float* scale, float* shift, void* stream);
/* Eval-mode coefficients of EVERY BatchNorm of a network in one launch (the
 * frozen inference path: models/base/layers.py:41,57-61 in eval mode, once per
 * weight snapshot instead of once per BN per forward).  table int64 [nbn][6] =
 * (gamma_off, beta_off, rmean_off, rvar_off, coef_off, C): offsets in floats
 * into params (gamma, beta), stats (rmean, rvar) and coef; row i writes scale
 * at coef + coef_off and shift at coef + coef_off + C, bit-identical to
 * ubpl_bn_eval_coeffs per BN.  The extents below are the least any table needs
 * (C >= 1); the caller owns the table's offsets. */
/*@ params:f32[2*nbn] stats:f32[2*nbn] table:i64[6*nbn] coef:f32[2*nbn] */
int ubpl_bn_eval_coeffs_table(const float* params, const float* stats, const int64_t* table, int nbn, float eps,
                              float* coef, void* stream);
/*@ x:f32[(int64_t)B*C*HW] scale:f32[C] shift:f32[C] y:f32[(int64_t)B*C*HW] */
int ubpl_bn_apply(const float* x, int B, int C, int HW, const float* scale, const float* shift, int relu, float* y,
                  void* stream);
/* Statistics from 64-pixel partials: part [C][ceil(N/64)][2] f32 = (S, M2) =
 * (sum y, sum (y - S/n)^2) over each 64-pixel slice of the flat (b, p) pixels of
 * y [B,C,P] (Chan's parallel form); the conv kernels write it from their
 * accumulators (stat_part arguments), ubpl_bn_partials from a tensor.
 * ubpl_bn_stats_from_partials: outputs as ubpl_bn_forward_stats, f64 combine. */
int64_t ubpl_bn_partial_floats(int C, int64_t N);
/*@ y:f32[(int64_t)B*C*P] part:f32[ubpl_bn_partial_floats(C,(int64_t)B*P)] */
int ubpl_bn_partials(const float* y, int B, int C, int P, float* part, void* stream);
/*@ part:f32[ubpl_bn_partial_floats(C,N)] gamma:f32[C] beta:f32[C] rmean:f32[C] rvar:f32[C] mean_out:f32[C] invstd_out:f32[C] scale:f32[C] shift_out:f32[C] */
int ubpl_bn_stats_from_partials(const float* part, int C, int64_t N, const float* gamma,
                                const float* beta, float eps, float momentum, float* rmean, float* rvar,
                                float* mean_out, float* invstd_out, float* scale, float* shift_out, void* stream);
/* Backward of y = [relu](bn(x)); dgamma/dbeta accumulate; dx = add1 + add2 + dL/dx.
 * Statistics: one launch over `scratch` (ubpl_bn_part_doubles(B, C) doubles,
 * zeroed before first use, as ubpl_bn_forward_stats), or — part != nullptr —
 * from backward partials dz's producer wrote: per (channel, 64-pixel slice)
 * (S1, S2) = (sum g, sum g*(x - mean)), g = dz under the recomputed ReLU mask,
 * ubpl_bn_partial_floats(C, B*HW) floats (a conv epilogue's bn_part argument,
 * or ubpl_bn_backward_partials); coef: 3*C floats of scratch. */
/*@ dz:f32[(int64_t)B*C*HW] x:f32[(int64_t)B*C*HW] gamma:f32[C] mean:f32[C] invstd:f32[C] scale:f32[C] shift:f32[C] scratch:f64[ubpl_bn_part_doubles(B,C)] part:f32[ubpl_bn_partial_floats(C,(int64_t)B*HW)] coef:f32[3*C] dgamma:f32[C] dbeta:f32[C] add1:f32[(int64_t)B*C*HW] add2:f32[(int64_t)B*C*HW] dx:f32[(int64_t)B*C*HW] */
int ubpl_bn_backward(const float* dz, const float* x, int B, int C, int HW, const float* gamma, const float* mean,
                     const float* invstd, const float* scale, const float* shift, int relu, double* scratch,
                     const float* part, float* coef, float* dgamma, float* dbeta, const float* add1,
                     const float* add2, float* dx, void* stream);
/* The same backward with dx delivered only as PSA planes (ubpl_split_activation
 * layout, border `pad`, npieces 1, 2 or 3) — the operand of a split-path 3x3 data /
 * weight gradient; no addends; C % 16 == 0.  npieces 2 (2xfp16): the statistics
 * pass also bounds |dx| and picks the power-of-two scale of the fp16 pieces,
 * written to coef[3C] (coef: 3C + 1 floats) for the consumers (act_scale of
 * ubpl_conv2d_forward_psa / dscale of ubpl_wgrad3_psa); not with `part`. */
/*@ dz:f32[(int64_t)B*C*H*W] x:f32[(int64_t)B*C*H*W] gamma:f32[C] mean:f32[C] invstd:f32[C] scale:f32[C] shift:f32[C] scratch:f64[ubpl_bn_part_doubles(B,C)] part:f32[ubpl_bn_partial_floats(C,(int64_t)B*H*W)] coef:f32[3*C+1] dgamma:f32[C] dbeta:f32[C] dst:u16[(npieces-1)*plane+(int64_t)B*C*(H+2*pad)*(W+2*pad)] */
int ubpl_bn_backward_split(const float* dz, const float* x, int B, int C, int H, int W, const float* gamma,
                           const float* mean, const float* invstd, const float* scale, const float* shift, int relu,
                           double* scratch, const float* part, float* coef, float* dgamma, float* dbeta, int pad,
                           int npieces, uint16_t* dst, int64_t plane, void* stream);
/* The backward statistics partials alone (the layout above). */
/*@ dz:f32[(int64_t)B*C*HW] x:f32[(int64_t)B*C*HW] scale:f32[C] shift:f32[C] mean:f32[C] part:f32[ubpl_bn_partial_floats(C,(int64_t)B*HW)] */
int ubpl_bn_backward_partials(const float* dz, const float* x, int B, int C, int HW, const float* scale,
                              const float* shift, const float* mean, int relu, float* part, void* stream);

/* Conv (models/base/layers.py:31-50): 1x1/s1, 3x3/s1, 7x7/s2, pad (KS-1)/2,
 * optional fused pre-activation relu(x*pscale + pshift), bias, residual add
 * (res may alias y).  MFMA f32 implicit GEMM over a grouped tap-major K,
 * k = (ci/G)*G*T + tap*G + ci%G (T = KS*KS, G = 16 if 16 | Cin else Cin):
 * for KS > 1 the weights must be in the layout ubpl_conv_weight_tapmajor makes,
 * [Cout][Cin/G][T][G] (for KS == 1 that is the reference layout itself).
 * Small grids split K over workgroups: slab = ubpl_conv2d_forward_workspace
 * floats (nullable when that is 0). */
int64_t ubpl_conv2d_forward_workspace(int B, int Cin, int Cout, int KS, int Ho, int Wo);
/*@ x:f32[(int64_t)B*Cin*H*W] w:f32[(int64_t)Cout*Cin*KS*KS] bias:f32[Cout] pscale:f32[Cin] pshift:f32[Cin] res:f32[(int64_t)B*Cout*Ho*Wo] y:f32[(int64_t)B*Cout*Ho*Wo] slab:f32[ubpl_conv2d_forward_workspace(B,Cin,Cout,KS,Ho,Wo)] */
int ubpl_conv2d_forward(const float* x, int B, int Cin, int H, int W, const float* w, const float* bias, int Cout,
                        int KS, int stride, const float* pscale, const float* pshift, const float* res, float* y,
                        int Ho, int Wo, float* slab, void* stream);
/*@ w:f32[(int64_t)Cout*Cin*KS*KS] wt:f32[(int64_t)Cout*Cin*KS*KS] */
int ubpl_conv_weight_tapmajor(const float* w, int Cout, int Cin, int KS, float* wt, void* stream);
/* 1x1 stride-1 conv fed by LDS-DMA, k-major weights wk [Cin][Cout] (the
 * data-gradient re-layout of the conv; for a data gradient, the reference
 * weights themselves): same semantics as ubpl_conv2d_forward with KS = 1.
 * Cin % 16 == 0, Cout % 4 == 0, P % 4 == 0, x / wk 16-B aligned, Cin <= 256 with a
 * prologue. */
int64_t ubpl_conv1x1_kmajor_workspace(int B, int Cin, int Cout, int P);
/*@ x:f32[(int64_t)B*Cin*P] wk:f32[(int64_t)Cin*Cout] bias:f32[Cout] pscale:f32[Cin] pshift:f32[Cin] res:f32[(int64_t)B*Cout*P] y:f32[(int64_t)B*Cout*P] slab:f32[ubpl_conv1x1_kmajor_workspace(B,Cin,Cout,P)] stat_part:f32[ubpl_bn_partial_floats(Cout,(int64_t)B*P)] */
int ubpl_conv1x1_forward_kmajor(const float* x, int B, int Cin, int P, const float* wk, const float* bias, int Cout,
                                const float* pscale, const float* pshift, const float* res, float* y, float* slab,
                                float* stat_part, void* stream);
/* Weight gradient (+ bias gradient), reference weight layout. */
int64_t ubpl_conv2d_wgrad_workspace(int B, int Cin, int Cout, int KS, int Ho, int Wo);
/*@ dy:f32[(int64_t)B*Cout*Ho*Wo] x:f32[(int64_t)B*Cin*H*W] pscale:f32[Cin] pshift:f32[Cin] slab:f32[ubpl_conv2d_wgrad_workspace(B,Cin,Cout,KS,Ho,Wo)] dw:f32[(int64_t)Cout*Cin*KS*KS] db:f32[Cout] */
int ubpl_conv2d_wgrad(const float* dy, const float* x, int B, int Cin, int H, int W, int Cout, int KS, int stride,
                      const float* pscale, const float* pshift, int Ho, int Wo, float* slab, float* dw, float* db,
                      int accumulate, void* stream);
/* Data-gradient weights (stride 1): the forward layout of the flipped,
 * transposed kernel ([Cin][Cout/G][T][G], G from Cout), so
 * dx = ubpl_conv2d_forward(dy, wt). */
/*@ w:f32[(int64_t)Cout*Cin*KS*KS] wt:f32[(int64_t)Cout*Cin*KS*KS] */
int ubpl_conv_weight_flip(const float* w, int Cout, int Cin, int KS, float* wt, void* stream);
/* Reduce a weight-gradient slab [splits][Cout][Cin*T + 1] (columns n = tap*Cin + ci,
 * last = bias) into dw (reference layout, (+)=) and db (nullable). */
/*@ slab:f32[(int64_t)splits*Cout*((int64_t)Cin*T+1)] dw:f32[(int64_t)Cout*Cin*T] db:f32[Cout] */
int ubpl_wgrad_slab_reduce(const float* slab, int splits, int Cout, int Cin, int T, int with_bias, float* dw,
                           float* db, int accumulate, void* stream);
/* Both re-layouts for many convs in one launch: table int64 [nseg][5] =
 * (src_off, dst_off, Cout, Cin, KS*KS) in floats; mode 0 tap-major, 1 dgrad. */
/*@ src:f32[?] dst:f32[?] table:i64[nseg*5] */
int ubpl_conv_weights_relayout(const float* src, float* dst, const int64_t* table, int nseg, int mode, void* stream);

/* Split MFMA path of the same Conv (split_common.h and the conv_*split*, conv_psa*,
 * conv1x1_sol files): every f32 operand carried
 * as npieces 16-bit pieces, the piece products with pa + pb < npieces summed by
 * the 32x32x16 MFMA in f32: npieces 3 = three bf16 pieces ("6xbf16", exact
 * operands, 6 products), 2 = two fp16 pieces of the operand times a power-of-two
 * scale ("2xfp16", 3 products on v_mfma_f32_32x32x16_f16; weights scaled by
 * 2^(9 + ceil(log2 sqrt K)) for contraction length K, activations by 32, the
 * accumulators unscaled exactly before the stores), 1 = bf16 operands.  Weights:
 * ubpl_conv_weights_split writes npieces planes (`plane` elements apart)
 * of the mode-0 (forward, grouped tap-major) or mode-1 (data-gradient) layout
 * for many convs in one launch (table as above, dst_off % 8 == 0).
 * ubpl_conv2d_forward_split (the register-staged kernel, npieces 3): (KS, stride)
 * in {(1,1), (3,1)}, Cin % 16 == 0, wsplit 16-B aligned; other arguments as
 * ubpl_conv2d_forward. */
/*@ src:f32[?] dst:u16[npieces*plane] table:i64[nseg*5] */
int ubpl_conv_weights_split(const float* src, uint16_t* dst, int64_t plane, const int64_t* table, int nseg, int mode,
                            int npieces, void* stream);
int64_t ubpl_conv2d_forward_split_workspace(int B, int Cin, int Cout, int KS, int Ho, int Wo, int npieces);
/*@ x:f32[(int64_t)B*Cin*H*W] wsplit:u16[(npieces-1)*plane+(int64_t)Cout*Cin*KS*KS] bias:f32[Cout] pscale:f32[Cin] pshift:f32[Cin] res:f32[(int64_t)B*Cout*Ho*Wo] y:f32[(int64_t)B*Cout*Ho*Wo] slab:f32[ubpl_conv2d_forward_split_workspace(B,Cin,Cout,KS,Ho,Wo,npieces)] */
int ubpl_conv2d_forward_split(const float* x, int B, int Cin, int H, int W, const uint16_t* wsplit, int64_t plane,
                              const float* bias, int Cout, int KS, int stride, const float* pscale,
                              const float* pshift, const float* res, float* y, int Ho, int Wo, float* slab,
                              int npieces, void* stream);
/* Pre-split activations ("PSA"): npieces 16-bit planes (`plane` elements apart)
 * of [B][C/16][H+2pad][W+2pad][16] holding relu(x*pscale + pshift) (or x when
 * pscale is null) with a zero border; C % 16 == 0.  npieces 2 (2xfp16): the
 * pieces of v * 32; dst3 (nullable, npieces 2 only): also the 3-piece bf16
 * image of v (planes `plane3` apart) from the same read. */
/*@ x:f32[(int64_t)B*C*H*W] pscale:f32[C] pshift:f32[C] dst:u16[(npieces-1)*plane+(int64_t)B*C*(H+2*pad)*(W+2*pad)] dst3:u16[2*plane3+(int64_t)B*C*(H+2*pad)*(W+2*pad)] */
int ubpl_split_activation(const float* x, int B, int C, int H, int W, const float* pscale, const float* pshift,
                          int pad, int npieces, uint16_t* dst, int64_t plane, uint16_t* dst3, int64_t plane3,
                          void* stream);
/* Stride-1 conv (KS 1 or 3) of PSA activations (pad >= (KS-1)/2) with split
 * weights: both operands DMA'd global -> LDS; y = conv + bias (+ res, may alias y). */
int64_t ubpl_conv2d_forward_psa_workspace(int B, int Cin, int Cout, int KS, int H, int W, int npieces);
/* Test hook (host-only): the 3x3 input-halo kernel dispatch of
 * ubpl_conv2d_forward_psa.  halo_mode -1 default, 0 off, 1 on where eligible,
 * 2 on and required (an ineligible 3x3 launch returns hipErrorInvalidValue),
 * 3 the one-buffer variant required; teams -1 default, 1 / 2 teams per
 * workgroup.  The environment (UBPL_PSA_HALO = 0 / 1, UBPL_PSA_TEAMS) sets the
 * initial values, read once; (-2, -2) returns to the environment's values. */
int ubpl_set_psa_dispatch(int halo_mode, int teams);
/* 3x3 weight gradient (+ bias gradient, db nullable) on the split path from PSA
 * operands with a 1-pixel border: dys = split(dy), xs = split(conv input),
 * npieces 3 (6xbf16), 1 (bf16) or 2 (2xfp16: dys the pieces of dy * *dscale —
 * ubpl_bn_backward_split's coef[3C] — and xs of x * 32, the forward's image;
 * dscale required exactly then); Cin % 64 == 0, Cout % 64 == 0, W % 16 == 0. */
int64_t ubpl_wgrad3_psa_workspace(int B, int Cin, int Cout, int H, int W);
/*@ dys:u16[(npieces-1)*dplane+(int64_t)B*Cout*(H+2)*(W+2)] xs:u16[(npieces-1)*xplane+(int64_t)B*Cin*(H+2)*(W+2)] slab:f32[ubpl_wgrad3_psa_workspace(B,Cin,Cout,H,W)] dw:f32[(int64_t)Cout*Cin*9] db:f32[Cout] dscale:f32[1] */
int ubpl_wgrad3_psa(const uint16_t* dys, int64_t dplane, const uint16_t* xs, int64_t xplane, int B, int Cin,
                    int Cout, int H, int W, float* slab, float* dw, float* db, int accumulate, int npieces,
                    const float* dscale, void* stream);
/* The 7x7 stride-2 stem's weight gradient (+ bias gradient, db nullable) on the
 * split path, as the weight gradient of its space-to-depth form (replaces the
 * exact-f32 ubpl_conv2d_wgrad for models/pose/hourglass.py pre.0 / layers.py:31-50):
 * dys = split(dy) (PSA, pad 1, Cout channels at the H x W output), xs = the
 * forward's phase image (ubpl_stem_s2d_split, 16 channels, pad 2); KS = 7, C <= 4
 * input channels, Cout % 64 == 0, W % 16 == 0, npieces 3 or 1.  _workspace: slab floats. */
int64_t ubpl_wgrad_stem_psa_workspace(int B, int Cout, int H, int W);
/*@ dys:u16[(npieces-1)*dplane+(int64_t)B*Cout*(H+2)*(W+2)] xs:u16[(npieces-1)*xplane+(int64_t)B*16*(H+4)*(W+4)] slab:f32[ubpl_wgrad_stem_psa_workspace(B,Cout,H,W)] dw:f32[(int64_t)Cout*C*KS*KS] db:f32[Cout] */
int ubpl_wgrad_stem_psa(const uint16_t* dys, int64_t dplane, const uint16_t* xs, int64_t xplane, int B, int C,
                        int Cout, int H, int W, int KS, float* slab, float* dw, float* db, int accumulate,
                        int npieces, void* stream);
/* 1x1 weight gradient (+ bias gradient, db nullable) on the split path with
 * both f32 operands (dy [B,Cout,P], x [B,Cin,P], prologue relu(x*pscale +
 * pshift) when pscale != nullptr) split while staged: npieces 3 = 6xbf16,
 * 1 = bf16 operands with f32 accumulation.  _workspace: slab floats,
 * 0 = shape not supported (needs Cin % 64 == 0, Cout % 64 == 0, P % 16 == 0). */
int64_t ubpl_wgrad1x1_split_load_workspace(int B, int Cin, int Cout, int P);
/*@ dy:f32[(int64_t)B*Cout*P] x:f32[(int64_t)B*Cin*P] pscale:f32[Cin] pshift:f32[Cin] slab:f32[ubpl_wgrad1x1_split_load_workspace(B,Cin,Cout,P)] dw:f32[(int64_t)Cout*Cin] db:f32[Cout] */
int ubpl_wgrad1x1_split_load(const float* dy, const float* x, int B, int Cin, int Cout, int P, const float* pscale,
                             const float* pshift, float* slab, float* dw, float* db, int accumulate, int npieces,
                             void* stream);
/*@ xs:u16[(npieces-1)*xplane+(int64_t)B*Cin*(H+2*pad)*(W+2*pad)] wsplit:u16[(npieces-1)*wplane+(int64_t)Cout*Cin*KS*KS] bias:f32[Cout] res:f32[(int64_t)B*Cout*H*W] y:f32[(int64_t)B*Cout*H*W] slab:f32[ubpl_conv2d_forward_psa_workspace(B,Cin,Cout,KS,H,W,npieces)] stat_part:f32[ubpl_bn_partial_floats(Cout,(int64_t)B*H*W)] bn_x:f32[(int64_t)B*Cout*H*W] bn_coef:f32[3*Cout] bn_part:f32[ubpl_bn_partial_floats(Cout,(int64_t)B*H*W)] act_scale:f32[1] */
int ubpl_conv2d_forward_psa(const uint16_t* xs, int64_t xplane, int B, int Cin, int H, int W, int pad,
                            const uint16_t* wsplit, int64_t wplane, const float* bias, int Cout, int KS,
                            const float* res, float* y, float* slab, int npieces, float* stat_part,
                            const float* bn_x, const float* bn_coef, int bn_relu, float* bn_part,
                            const float* act_scale, void* stream);
/* bn_part (nullable; with bn_x [B,Cout,P], bn_coef = scale|shift|mean, Cout
 * floats each, bn_relu): when y is the data gradient dz of a BatchNorm(+ReLU)
 * with input bn_x, its backward statistics partials (ubpl_bn_backward layout),
 * from the epilogue — then ubpl_bn_backward(..., part_ready = 1) needs no pass.
 * act_scale (nullable, npieces 2 only): the device-side scale of xs's pieces (a
 * data gradient's, ubpl_bn_backward_split coef[3C]); null: xs from
 * ubpl_split_activation (scale 32). */
/* The 7x7 stride-2 stem (Cin <= 4) on the split path by space-to-depth: the
 * phase images of x as a 16-channel PSA image with a `pad` (>= 2) border, and
 * the equivalent 4x4 stride-1 weights (Cin' = 16, KS' = 4) split into npieces
 * (3: 6xbf16; 1: the bf16 precision) planes of Cout*256 bf16; then
 * ubpl_conv2d_forward_psa(..., KS = 4). */
/*@ x:f32[(int64_t)B*C*H*W] dst:u16[(npieces-1)*plane+(int64_t)B*16*(H/2+2*pad)*(W/2+2*pad)] */
int ubpl_stem_s2d_split(const float* x, int B, int C, int H, int W, int pad, int npieces, uint16_t* dst,
                        int64_t plane, void* stream);
/*@ w:f32[(int64_t)Cout*C*KS*KS] dst:u16[(npieces-1)*plane+(int64_t)Cout*256] */
int ubpl_stem_weight_s2d_split(const float* w, int Cout, int C, int KS, int npieces, uint16_t* dst, int64_t plane,
                               void* stream);
/* 1x1 stride-1 conv on the split path with the f32 activations split while
 * they are staged (no pre-split image): y = conv(relu(x*pscale + pshift) or x)
 * + bias (+ res, may alias y); wsplit = npieces planes of [Cout][Cin] from
 * ubpl_conv_weights_split (KS = 1); npieces 3 = 6xbf16, 2 = 2xfp16 (no epilogue
 * partials), 1 = bf16 operands (one plane; no epilogue partials).  Cin % 16 == 0, Cout % 16 == 0, P % 4 == 0.
 * stat_part (nullable): BatchNorm partials of y (ubpl_bn_partials layout).
 * _preferred: 1 when the shape is supported and fills the chip (a grid of at least
 * one workgroup per CU); _preferred_min: ... and its grid has at least min_wgs workgroups. */
int ubpl_conv1x1_split_load_preferred(int B, int Cin, int Cout, int P);
int ubpl_conv1x1_split_load_preferred_min(int B, int Cin, int Cout, int P, int min_wgs);
/*@ x:f32[(int64_t)B*Cin*P] wsplit:u16[(npieces-1)*wplane+(int64_t)Cout*Cin] bias:f32[Cout] pscale:f32[Cin] pshift:f32[Cin] res:f32[(int64_t)B*Cout*P] y:f32[(int64_t)B*Cout*P] stat_part:f32[ubpl_bn_partial_floats(Cout,(int64_t)B*P)] bn_x:f32[(int64_t)B*Cout*P] bn_coef:f32[3*Cout] bn_part:f32[ubpl_bn_partial_floats(Cout,(int64_t)B*P)] */
int ubpl_conv1x1_forward_split_load(const float* x, int B, int Cin, int P, const uint16_t* wsplit, int64_t wplane,
                                    const float* bias, int Cout, const float* pscale, const float* pshift,
                                    const float* res, float* y, float* stat_part, const float* bn_x,
                                    const float* bn_coef, int bn_relu, float* bn_part, int npieces, void* stream);

/* MaxPool2d(2,2) (models/base/layers.py:93), Upsample(x2, nearest) + add
 * (layers.py:110-111), AvgPool2d(2,2) projection (models/pose/hourglass.py:226). */
/*@ x:f32[planes*H*W] y:f32[planes*(H/2)*(W/2)] */
int ubpl_maxpool2x2_forward(const float* x, int64_t planes, int H, int W, float* y, void* stream);
/*@ x:f32[planes*H*W] dy:f32[planes*(H/2)*(W/2)] dx:f32[planes*H*W] */
int ubpl_maxpool2x2_backward(const float* x, const float* dy, int64_t planes, int H, int W, float* dx,
                             int accumulate, void* stream);
/*@ x:f32[planes*H*W] y:f32[planes*(H/2)*(W/2)] */
int ubpl_avgpool2x2_forward(const float* x, int64_t planes, int H, int W, float* y, void* stream);
/*@ dy:f32[planes*(H/2)*(W/2)] dx:f32[planes*H*W] */
int ubpl_avgpool2x2_backward(const float* dy, int64_t planes, int H, int W, float* dx, int accumulate, void* stream);
/*@ up:f32[planes*H*W] low:f32[planes*(H/2)*(W/2)] out:f32[planes*H*W] */
int ubpl_upsample2x_add_forward(const float* up, const float* low, int64_t planes, int H, int W, float* out,
                                void* stream);
/*@ dout:f32[planes*H*W] dlow:f32[planes*(H/2)*(W/2)] */
int ubpl_upsample2x_add_backward(const float* dout, int64_t planes, int H, int W, float* dlow, int accumulate,
                                 void* stream);
/*@ a:f32[n] b:f32[n] out:f32[n] */
int ubpl_add(const float* a, const float* b, int64_t n, float* out, void* stream);
/* ProcessUtils.image_fliplr (utils/process.py:200-207) on device planes:
 * y[p,r,c] = x[p,r,W-1-c], y != x, any W >= 1, 4-byte alignment. */
/*@ x:f32[planes*H*W] y:f32[planes*H*W] */
int ubpl_fliplr(const float* x, int64_t planes, int H, int W, float* y, void* stream);
/* The same forwards + BatchNorm partials of the output for the BN that
 * consumes it (ubpl_bn_partials layout); output planes of a multiple of 64 pixels. */
/*@ x:f32[(int64_t)B*C*H*W] y:f32[(int64_t)B*C*(H/2)*(W/2)] part:f32[ubpl_bn_partial_floats(C,(int64_t)B*(H/2)*(W/2))] */
int ubpl_maxpool2x2_forward_stats(const float* x, int B, int C, int H, int W, float* y, float* part, void* stream);
/*@ up:f32[(int64_t)B*C*H*W] low:f32[(int64_t)B*C*(H/2)*(W/2)] out:f32[(int64_t)B*C*H*W] part:f32[ubpl_bn_partial_floats(C,(int64_t)B*H*W)] */
int ubpl_upsample2x_add_forward_stats(const float* up, const float* low, int B, int C, int H, int W, float* out,
                                      float* part, void* stream);
/* The hourglass resampling passes folded into the BatchNorm kernel next to them
 * (bn_fwd.hip, bn_bwd.hip).  Planes of H x W with H a power of two >= 2 and W/4 a power of two
 * <= 32, C <= 512, f32 operands 16-byte aligned (half-resolution ones 8-byte);
 * anything else returns hipErrorInvalidValue.  `part`: the statistics scratch of
 * ubpl_bn_forward_stats.
 * ubpl_bn_forward_stats_maxpool: ubpl_bn_forward_stats(x) for the BatchNorm of
 * gamma .. shift (bit-identical; all eight null: x has no BatchNorm), y =
 * ubpl_maxpool2x2_forward(x) (bit-identical) and the statistics of y for the
 * BatchNorm of pgamma .. pshift (all eight null: not taken; f32 per thread about y[0,c,0], f64 across
 * threads and slices, in a fixed order) in one launch. */
/*@ x:f32[(int64_t)B*C*H*W] y:f32[(int64_t)B*C*(H/2)*(W/2)] gamma:f32[C] beta:f32[C] rmean:f32[C] rvar:f32[C] mean_out:f32[C] invstd_out:f32[C] scale:f32[C] shift:f32[C] pgamma:f32[C] pbeta:f32[C] prmean:f32[C] prvar:f32[C] pmean_out:f32[C] pinvstd_out:f32[C] pscale:f32[C] pshift:f32[C] part:f64[ubpl_bn_part_doubles(B,C)] */
int ubpl_bn_forward_stats_maxpool(const float* x, int B, int C, int H, int W, float* y, const float* gamma,
                                  const float* beta, float* rmean, float* rvar, float* mean_out, float* invstd_out,
                                  float* scale, float* shift, const float* pgamma, const float* pbeta, float* prmean,
                                  float* prvar, float* pmean_out, float* pinvstd_out, float* pscale, float* pshift,
                                  float eps, float momentum, double* part, void* stream);
/* out = ubpl_upsample2x_add_forward(up, low) (out may be up) and
 * ubpl_bn_forward_stats(out) in one launch, both bit-identical. */
/*@ up:f32[(int64_t)B*C*H*W] low:f32[(int64_t)B*C*(H/2)*(W/2)] out:f32[(int64_t)B*C*H*W] gamma:f32[C] beta:f32[C] rmean:f32[C] rvar:f32[C] part:f64[ubpl_bn_part_doubles(B,C)] mean_out:f32[C] invstd_out:f32[C] scale:f32[C] shift:f32[C] */
int ubpl_upsample2x_add_forward_bnstats(const float* up, const float* low, int B, int C, int H, int W, float* out,
                                        const float* gamma, const float* beta, float eps, float momentum,
                                        float* rmean, float* rvar, double* part, float* mean_out, float* invstd_out,
                                        float* scale, float* shift, void* stream);
/* ubpl_bn_backward of x [B,C,H,W] with the gradient of y = maxpool2x2(x) folded
 * into the apply: dx = ((dL/dx + add1) + maxpool2x2_backward(x, pool_dy)) + add2,
 * bit-identical to ubpl_bn_backward(add1), ubpl_maxpool2x2_backward(accumulate)
 * and ubpl_add in turn.  pool_dy [B,C,H/2,W/2] null: ubpl_bn_backward. */
/*@ dz:f32[(int64_t)B*C*H*W] x:f32[(int64_t)B*C*H*W] gamma:f32[C] mean:f32[C] invstd:f32[C] scale:f32[C] shift:f32[C] scratch:f64[ubpl_bn_part_doubles(B,C)] part:f32[ubpl_bn_partial_floats(C,(int64_t)B*H*W)] coef:f32[3*C] dgamma:f32[C] dbeta:f32[C] add1:f32[(int64_t)B*C*H*W] pool_dy:f32[(int64_t)B*C*(H/2)*(W/2)] add2:f32[(int64_t)B*C*H*W] dx:f32[(int64_t)B*C*H*W] */
int ubpl_bn_backward_pool(const float* dz, const float* x, int B, int C, int H, int W, const float* gamma,
                          const float* mean, const float* invstd, const float* scale, const float* shift, int relu,
                          double* scratch, const float* part, float* coef, float* dgamma, float* dbeta,
                          const float* add1, const float* pool_dy, const float* add2, float* dx, void* stream);

/* ---------------------------------------------------------------- f1 ----
 * Two-view training augmentation (DS_mds.__getitem__, datasets/dataset_mds.py:41-201:
 * fliplr utils/augment.py:216-227, noisy_mean :261-267, affine :86-156,
 * image_colorNorm utils/process.py:151-160) on images resident in HBM.
 * imgs uint8 BGR [N][H][W][3].  ubpl_image_mean_u8: out[n] = mean of image n / 255
 * (the noisy_mean mu).  ubpl_augment_warp: view v samples image src_idx[v] at
 * (mat[6v..6v+2] . (x,y,1), mat[6v+3..6v+5] . (x,y,1)) — flip and the inverse
 * crop/scale/rotate transform folded by the host — bilinear, zero outside;
 * noise[3v..3v+2] = (alpha, beta, enabled) of noisy_mean; out [V][3][Ho][Wo]
 * float32 minus chan_mean[3]. */
/*@ imgs:u8[N*n_per_image] out:f32[N] */
int ubpl_image_mean_u8(const uint8_t* imgs, int N, int64_t n_per_image, float* out, void* stream);
/*@ imgs:u8[?] src_idx:i32[V] mat:f32[6*V] noise:f32[3*V] img_mean:f32[?] chan_mean:f32[3] out:f32[(int64_t)V*3*Ho*Wo] */
int ubpl_augment_warp(const uint8_t* imgs, int H, int W, const int* src_idx, const float* mat, const float* noise,
                      const float* img_mean, const float* chan_mean, int V, int Ho, int Wo, float* out, void* stream);

/* ubpl_augment_chain: the same views with the reference's TWO resamplings
 * (utils/augment.py:119-137) instead of one: stage 1, skimage.transform.rotate
 * (order 1, constant 0) of the integer crop of the flipped, noise-adjusted image
 * about the padded crop's centre, pad stripped, into inter [V][3][Hm][Wm]
 * (Hc x Wc used per view); stage 2, skimage.transform.resize to Ho x Wo (order
 * 1, pixel centres, mirror edges), minus chan_mean[3] -> out [V][3][Ho][Wo].
 * geo int [V][8] = (src_idx, flip, ul_x, ul_y, Hp, Wp, Hc, Wc): the grown crop
 * box corner and size, the stripped size (Hp - Hc = Wp - Wc = 2 * pad, Hc <= Hm,
 * Wc <= Wm); cs [V][2] = (cos, sin) of the angle; noise as ubpl_augment_warp. */
/*@ imgs:u8[?] geo:i32[8*V] cs:f32[2*V] noise:f32[3*V] img_mean:f32[?] chan_mean:f32[3] inter:f32[(int64_t)V*3*Hm*Wm] out:f32[(int64_t)V*3*Ho*Wo] */
int ubpl_augment_chain(const uint8_t* imgs, int H, int W, const int* geo, const float* cs, const float* noise,
                       const float* img_mean, const float* chan_mean, int V, int Hm, int Wm, float* inter, int Ho,
                       int Wo, float* out, void* stream);

/* Random occlusion of augmented views (utils/udaap/utils_augment.py:21-25,116-163:
 * augment_occlu / occlude_with_objects / resize_by_factor / paste_over), after
 * ubpl_augment_warp: out [V][3][H][W] (colorNorm'ed) gets, in draw order, each
 * paste alpha * (color - chan_mean) + (1 - alpha) * out.  bank: RGBA float
 * occluders (16-B aligned, [h][w][4] each at bank + off[o], hw[2o..2o+1] = h, w);
 * pastes int [P][9] = (view, occluder, w1, h1, x0, y0, x1, y1, sx0 | sy0 << 16)
 * sorted by view, view_first [V+1] the first paste of each view; the occluder is
 * resized to w1 x h1 by pixel-area averaging (cv2.INTER_AREA). */
/*@ out:f32[(int64_t)V*3*H*W] bank:f32[?] off:i64[?] hw:i32[?] pastes:i32[?] view_first:i32[V+1] chan_mean:f32[3] */
int ubpl_occlude(float* out, int V, int H, int W, const float* bank, const int64_t* off, const int* hw,
                 const int* pastes, const int* view_first, const float* chan_mean, void* stream);

/* Crop from raw frames: the evaluation crop of affine_image (utils/augment.py:91-137 with
 * angle == 0) for n boxes out of a ragged bank of uint8 BGR frames: frame f is [h][w][3] at
 * bank + off[f], hw[2f..2f+1] = h, w.  Box b reads frame plan[16b] and writes out[b] =
 * [3][R][R] float32, channel c = BGR channel c of u8 * (1/255.f), resampled, minus
 * chan_mean[c].  Per axis (x: plan[16b+1..6], y: plan[16b+7..12]) the six ints
 * (org, ls, lo, off, lb, r) state both branches of the reference as one computation:
 *   a virtual source of ls pixels whose pixel i is frame pixel org + i (0 outside the frame);
 *   skimage.transform.resize of it to lo pixels — a Gaussian of radius r with the weights
 *   gauss[(2b + axis)*gw + |k|] (normalised, 0 at |k| = r + 1; ndimage 'mirror' edges, periodic),
 *   then the bilinear sample at (g + 0.5) * ls/lo - 0.5 with mirrored indices;
 *   a box of lb pixels of that grid from grid index off on (0 outside the grid), resized to
 *   R pixels by the bilinear sample at (o + 0.5) * lb/R - 0.5 with mirrored indices.
 * sf < 2: the virtual source is the integer crop box and lo = lb = R, off = 0 (the last
 * resize is the identity); sf >= 2: the virtual source is the whole frame, lo the pre-resized
 * size and (off, lb) the crop box in it.  Coordinates and floors in float64, weights and sums
 * in float32, in a fixed order (no atomics).  Two passes: rows first, into inter — per box
 * [3][rows][R] floats of which the box uses its own plan[16b+14] rows, virtual-source rows
 * plan[16b+13] on —, then columns.  _workspace: the floats of inter. */
int64_t ubpl_crop_frames_workspace(int n, int rows, int R);
/*@ bank:u8[?] off:i64[?] hw:i32[?] plan:i32[16*n] gauss:f32[(int64_t)n*2*gw] chan_mean:f32[3] inter:f32[ubpl_crop_frames_workspace(n,rows,R)] out:f32[(int64_t)n*3*R*R] */
int ubpl_crop_frames(const uint8_t* bank, const int64_t* off, const int* hw, const int* plan, const float* gauss,
                     int gw, const float* chan_mean, int n, int rows, int R, float* inter, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UBPL_HIP_H */
