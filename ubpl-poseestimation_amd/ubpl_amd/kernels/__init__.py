"""Tensor-level wrappers over the C-ABI (no autograd here), one module per kernel family.

A device wrapper validates device / dtype / contiguity (`_check`), allocates outputs with the
torch caching allocator on the input's device and enqueues on torch's current stream; it
computes nothing on the host.  `view_geometry` and the small table builders (`flip_perm`,
`blur_taps`, `bn_coeff_table`, `_occlude_check`) do compute on the host, in float64 or integers.

The launch seam is `ubpl_amd._lib.call`, read at call time: every wrapper launches through the
module attribute `_lib.call(...)`, so replacing that one name intercepts every launch of every
family.  `call` below is an alias for direct launches (`Kn.call("ubpl_...", ...)`) that no wrapper
reads; likewise the wrappers read the tensor check as `_check._chk`, and `_chk` here is an alias.
Callers use `from ubpl_amd import kernels as Kn`: the imports below are the whole surface.
"""
from .._lib import call  # noqa: F401
from ._check import F32, _chk, _chk_entries, _chk_maps, _outs, _same_shape  # noqa: F401
from .augment import (CROP_MAX_BOXES, CROP_WORKSPACE_BYTES, _crop_chunks, _occlude_check, augment_chain,  # noqa: F401
                      augment_warp, crop_frames, image_mean_u8, occlude)
from .bn import (_fuse_geometry, bn_apply, bn_backward, bn_backward_pool, bn_backward_split,  # noqa: F401
                 bn_bwd_partials, bn_coeff_table, bn_eval_coeffs, bn_eval_coeffs_table, bn_forward_stats,
                 bn_forward_stats_maxpool, bn_part, bn_partial_buffer, bn_partials, bn_stats_from_partials,
                 pool_fuse_ok, upsample2x_add_bnstats)
from .conv import (_NO_SOL, _SOL_MINWG, _bnb, _slab, _workspace, conv1x1_forward_kmajor,  # noqa: F401
                   conv1x1_forward_split_load, conv1x1_kmajor_ok, conv1x1_split_load_ok, conv2d_dgrad,
                   conv2d_forward, conv2d_forward_psa, conv2d_forward_split, conv2d_wgrad,
                   conv2d_wgrad1x1_split_load, conv2d_wgrad3_psa, conv2d_wgrad_stem_psa, conv_out_hw,
                   conv_weight_flip, conv_weight_split, conv_weight_tapmajor, conv_weights_relayout,
                   conv_weights_split, split_activation, stem_s2d_ok, stem_s2d_split, stem_weight_s2d_split,
                   wgrad1x1_split_load_ok, wgrad3_psa_ok, wgrad_stem_psa_ok)
from .decode import (MAX_BLUR_RADIUS, REFINE_MODES, blur_taps, decode_heatmaps, decode_heatmaps_flip,  # noqa: F401
                     ensemble_pseudo, flip_perm, fliplr, pck, refine_peaks)
from .optim import (adamw_ema_step_dev_, adamw_ema_step_guarded_dev_, adamw_step_, adamw_step_dev_,  # noqa: F401
                    adamw_step_guarded_dev_, ema_update_, grad_guard_, grad_guard_scratch, restore_if_, scale_)
from .pool import (add, avgpool2x2, avgpool2x2_backward, maxpool2x2, maxpool2x2_backward, stats_ok,  # noqa: F401
                   upsample2x_add, upsample2x_add_backward)
from .render_loss import (MAX_RANK_GROUP, MAX_SCORE_MAPS, MAX_SCORE_MEMBERS, RowSpec, fdl_cov_backward,  # noqa: F401
                          fdl_cov_forward, loss_finalize, loss_finalize_rank, loss_finalize_ranked, pred_rows,
                          rank_threshold, render_heatmaps, row_grad, row_stats, softmax_peak_scores)
from .split_operands import (CONV_PRECISIONS, DEFAULT_CONV_PRECISION, SplitAct, SplitWeights,  # noqa: F401
                             backward_pieces, conv_precision_name, conv_precision_pieces)
from .view_geometry import (F64, MAX_VIEWS, _about_centre, _mat6, affine_pixels_to_theta,  # noqa: F401
                            affine_theta_to_pixels, compose_pixels, mirror_pixels, train_back_matrices,
                            train_pair_matrices, view_back_matrices, view_matrices)
from .views import (UNC_OUTPUTS, decode_heatmaps_views, merge_views_samples, view_uncertainty,  # noqa: F401
                    view_uncertainty_samples, warp_views)
