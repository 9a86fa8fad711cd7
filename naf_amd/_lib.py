"""ctypes binding of libnaf_hip.so (the C ABI declared in include/naf_hip.h).

The product path has NO fallback: if the shared library is missing or does not export every symbol,
``load()`` raises and every op built on it raises with it.  ``import torch`` happens first on purpose:
the library's DT_NEEDED libamdhip64.so.7 then resolves to the HIP runtime torch already mapped.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch  # noqa: F401  (must be imported before the HIP library is dlopen'ed)

# NAF_HIP_LIB lets an experiment point at an alternative build of the SAME library (A/B kernel variants)
LIB_PATH = os.environ.get("NAF_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnaf_hip.so")

HEADER_VERSION = 403          # NAF_HIP_VERSION of the include/naf_hip.h these ctypes mirrors were written against
NAF_BF16, NAF_F32 = 0, 1
NAF_F16 = 2     # IEEE half: values / output of the attention forward only (naf_dtype_supported)
DT_XNA_VALUES, DT_XNA_OUT, DT_PACK_SRC, DT_FWD_FEAT, DT_FWD_OUT = range(5)     # naf_dtype_arg
XNA_AUTO, XNA_MFMA, XNA_GENERIC, XNA_UNION, XNA_ROWS = 0, 1, 2, 3, 4
XNA_HEAD_AUTO, XNA_HEAD_FUSED = 0, 1            # naf_xna_head_path

I64x4 = C.c_int64 * 4


class RopePoolArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("q", C.c_void_p), ("k_lr", C.c_void_p), ("tab_y", C.c_void_p), ("tab_x", C.c_void_p),
        ("x_dtype", C.c_int32), ("B", C.c_int32), ("Cq", C.c_int32), ("heads", C.c_int32), ("Ho", C.c_int32),
        ("Wo", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("x_stride", I64x4), ("q_stride", I64x4), ("k_stride", I64x4),
    ]


class XnaArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k_lr", C.c_void_p), ("v_lr", C.c_void_p), ("out", C.c_void_p), ("logits", C.c_void_p),
        ("idx_y", C.c_void_p), ("idx_x", C.c_void_p), ("rope_tab_y", C.c_void_p), ("rope_tab_x", C.c_void_p),
        ("B", C.c_int32), ("heads", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("h", C.c_int32),
        ("w", C.c_int32), ("Dq", C.c_int32), ("Dv", C.c_int32), ("ky", C.c_int32), ("kx", C.c_int32),
        ("out_dtype", C.c_int32), ("path", C.c_int32), ("scale", C.c_float), ("reserved", C.c_int32),
        ("q_stride", I64x4), ("k_stride", I64x4), ("v_stride", I64x4), ("o_stride", I64x4),
    ]


I64x3 = C.c_int64 * 3


class XnaHeadArgs(C.Structure):
    """naf_xna_head_args (added after 0.4.3, detected by symbol): the attention with a linear head folded in."""
    _fields_ = [
        ("q", C.c_void_p), ("k_lr", C.c_void_p), ("pv_lr", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
        ("rope_tab_y", C.c_void_p), ("rope_tab_x", C.c_void_p),
        ("B", C.c_int32), ("heads", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("h", C.c_int32),
        ("w", C.c_int32), ("Dq", C.c_int32), ("N", C.c_int32), ("ky", C.c_int32), ("kx", C.c_int32),
        ("out_dtype", C.c_int32), ("path", C.c_int32), ("scale", C.c_float), ("reserved", C.c_int32),
        ("q_stride", I64x4), ("k_stride", I64x4), ("pv_stride", I64x4), ("o_stride", I64x3),
    ]


class XnaHeadCEArgs(C.Structure):
    """naf_xna_head_ce_args (added after the head entries, detected by symbol): naf_xna_head_args plus the classification epilogue's maps."""
    _fields_ = [
        ("head", XnaHeadArgs), ("target", C.c_void_p), ("loss", C.c_void_p), ("labels", C.c_void_p), ("dlogits", C.c_void_p),
        ("ignore_index", C.c_int64), ("dlogits_channels", C.c_int32), ("reserved", C.c_int32),
        ("t_stride", I64x3), ("loss_stride", I64x3), ("labels_stride", I64x3), ("dlogits_stride", I64x3),
    ]


class XnaHeadCMArgs(C.Structure):
    """naf_xna_head_cm_args (added after the classification entries, detected by symbol): naf_xna_head_ce_args plus the confusion matrix."""
    _fields_ = [("ce", XnaHeadCEArgs), ("confusion", C.c_void_p), ("cm_stride", C.c_int64), ("reserved", C.c_int64 * 2)]


HEAD_REG_STATS = 10                                   # NAF_HEAD_REG_STATS
HEAD_REG_KINDS = {"l1": 0, "mse": 1, "smooth_l1": 2}  # naf_head_reg_kind


class XnaHeadRegArgs(C.Structure):
    """naf_xna_head_reg_args (added after the k-means entries, detected by symbol): naf_xna_head_args plus the regression epilogue's target,
    mask, maps and error statistics.  ctypes zero-initialises it, as the header asks."""
    _fields_ = [
        ("head", XnaHeadArgs), ("target", C.c_void_p), ("valid", C.c_void_p), ("loss", C.c_void_p), ("dlogits", C.c_void_p),
        ("errors", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("dlogits_channels", C.c_int32), ("kind", C.c_int32), ("beta", C.c_float), ("clamp_lo", C.c_float), ("clamp_hi", C.c_float),
        ("reserved", C.c_int32 * 3),
        ("t_stride", I64x4), ("valid_stride", I64x3), ("loss_stride", I64x3), ("dlogits_stride", I64x3),
    ]


class XnaCosArgs(C.Structure):
    """naf_xna_cos_args (added after the image-preparation entries, detected by symbol): the attention with a cosine head folded in."""
    _fields_ = [
        ("q", C.c_void_p), ("k_lr", C.c_void_p), ("pv_lr", C.c_void_p), ("v_lr", C.c_void_p), ("out", C.c_void_p), ("norms", C.c_void_p),
        ("rope_tab_y", C.c_void_p), ("rope_tab_x", C.c_void_p),
        ("B", C.c_int32), ("heads", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("Dq", C.c_int32), ("Dv", C.c_int32), ("N", C.c_int32), ("ky", C.c_int32), ("kx", C.c_int32),
        ("path", C.c_int32), ("scale", C.c_float), ("logit_scale", C.c_float), ("reserved", C.c_int32 * 2),
        ("q_stride", I64x4), ("k_stride", I64x4), ("pv_stride", I64x4), ("v_stride", I64x4), ("o_stride", I64x3), ("norms_stride", I64x3),
    ]


class XnaCosCEArgs(C.Structure):
    """naf_xna_cos_ce_args (added after the cosine entries, detected by symbol): naf_xna_cos_args plus the classification epilogue's maps."""
    _fields_ = [
        ("cos", XnaCosArgs), ("target", C.c_void_p), ("loss", C.c_void_p), ("labels", C.c_void_p), ("dlogits", C.c_void_p),
        ("dscale", C.c_void_p), ("logit_scale_ptr", C.c_void_p),
        ("ignore_index", C.c_int64), ("dlogits_channels", C.c_int32), ("reserved", C.c_int32),
        ("t_stride", I64x3), ("loss_stride", I64x3), ("labels_stride", I64x3), ("dlogits_stride", I64x3), ("dscale_stride", I64x3),
    ]


class XnaCosPeaksArgs(C.Structure):
    """naf_xna_cos_peaks_args (added after the mask-pooling entries, detected by symbol): naf_xna_cos_args plus the cell peaks."""
    _fields_ = [
        ("cos", XnaCosArgs), ("peak", C.c_void_p), ("where", C.c_void_p), ("peak_stride", I64x3), ("where_stride", I64x3),
        ("reserved", C.c_int64 * 2),
    ]


MASK_BF16, MASK_U8 = 0, 1     # naf_mask_dtype


class XnaMaskPoolArgs(C.Structure):
    """naf_xna_maskpool_args (added after the cosine entries, detected by symbol): the attention summed under K masks."""
    _fields_ = [
        ("q", C.c_void_p), ("k_lr", C.c_void_p), ("masks", C.c_void_p), ("A", C.c_void_p), ("mass", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("rope_tab_y", C.c_void_p), ("rope_tab_x", C.c_void_p),
        ("B", C.c_int32), ("heads", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("Dq", C.c_int32), ("K", C.c_int32), ("ky", C.c_int32), ("kx", C.c_int32),
        ("mask_dtype", C.c_int32), ("path", C.c_int32), ("scale", C.c_float), ("reserved", C.c_int32),
        ("q_stride", I64x4), ("k_stride", I64x4), ("m_stride", I64x4),
    ]


class XnaKmeansArgs(C.Structure):
    """naf_xna_kmeans_args (added after the peak-search entries, detected by symbol): one k-means step, assign and accumulate in one launch."""
    _fields_ = [
        ("q", C.c_void_p), ("k_lr", C.c_void_p), ("pv_lr", C.c_void_p), ("bias", C.c_void_p), ("labels", C.c_void_p),
        ("A", C.c_void_p), ("mass", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("rope_tab_y", C.c_void_p), ("rope_tab_x", C.c_void_p),
        ("B", C.c_int32), ("heads", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("Dq", C.c_int32), ("K", C.c_int32), ("ky", C.c_int32), ("kx", C.c_int32),
        ("path", C.c_int32), ("scale", C.c_float), ("bias_stride_b", C.c_int64),
        ("q_stride", I64x4), ("k_stride", I64x4), ("pv_stride", I64x4), ("labels_stride", I64x3), ("reserved", C.c_int64 * 2),
    ]


class XnaMSEArgs(C.Structure):
    """naf_xna_mse_args (added after the PCA entries, detected by symbol): naf_xna_args plus the regression target of the training objective."""
    _fields_ = [
        ("a", XnaArgs), ("target", C.c_void_p), ("loss", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("target_dtype", C.c_int32), ("reserved", C.c_int32), ("target_stride", I64x4),
    ]


PROPAGATE_MAX_FRAMES = 16


class PropagateArgs(C.Structure):
    """naf_propagate_args (added after the confusion entries, detected by symbol): label propagation over a queue of context frames."""
    _fields_ = [
        ("target", C.c_void_p), ("target_inv", C.c_void_p),
        ("context", C.c_void_p * PROPAGATE_MAX_FRAMES), ("context_inv", C.c_void_p * PROPAGATE_MAX_FRAMES),
        ("segs", C.c_void_p), ("out", C.c_void_p),
        ("n", C.c_int32), ("C", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("K", C.c_int32), ("radius", C.c_int32),
        ("topk", C.c_int32), ("temperature", C.c_float), ("reserved", C.c_int32 * 2),
    ]


DAVIS_TILE_W, DAVIS_TILE_H = 64, 32             # NAF_DAVIS_TILE_W / _H: the tile one workgroup of naf_davis_jf owns
DAVIS_MAX_OBJECTS, DAVIS_MAX_HALF_WIDTH = 32, 32


class DavisJFArgs(C.Structure):
    """naf_davis_jf_args (added after the objective entries, detected by symbol): the counts behind the DAVIS J and F measures."""
    _fields_ = [
        ("annotation", C.c_void_p), ("segmentation", C.c_void_p), ("counts", C.c_void_p),
        ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("N", C.c_int32), ("r2", C.c_int32), ("half_width", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


MASK_LABELS_MAX_CHANNELS, MASK_LABELS_MAX_SIZE, MASK_LABELS_WORKSPACE_BYTES = 64, 16384, 8192     # NAF_MASK_LABELS_*


class MaskLabelsArgs(C.Structure):
    """naf_mask_labels_args (added after the DAVIS entries, detected by symbol): a propagated frame's soft masks to its label map."""
    _fields_ = [
        ("seg", C.c_void_p), ("tab_y", C.c_void_p), ("tab_x", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t), ("seg_stride", I64x3), ("out_stride", C.c_int64),
        ("K", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("mid_h", C.c_int32), ("mid_w", C.c_int32), ("out_h", C.c_int32),
        ("out_w", C.c_int32), ("reserved", C.c_int32),
    ]


class XnaPointsArgs(C.Structure):
    """naf_xna_points_args (added after the label-map entries, detected by symbol): the attention's scores, weights and features at N pixels."""
    _fields_ = [
        ("q", C.c_void_p), ("k_lr", C.c_void_p), ("v_lr", C.c_void_p), ("points", C.c_void_p), ("idx_y", C.c_void_p), ("idx_x", C.c_void_p),
        ("rope_tab_y", C.c_void_p), ("rope_tab_x", C.c_void_p), ("logits", C.c_void_p), ("probs", C.c_void_p), ("out", C.c_void_p),
        ("N", C.c_int32), ("B", C.c_int32), ("heads", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("Dq", C.c_int32), ("Dv", C.c_int32), ("ky", C.c_int32), ("kx", C.c_int32), ("v_dtype", C.c_int32), ("scale", C.c_float),
        ("reserved", C.c_int32),
        ("q_stride", I64x4), ("k_stride", I64x4), ("v_stride", I64x4),
    ]


IMAGE_PREP_MAX_VIEWS, IMAGE_PREP_MAX_SIZE, IMAGE_PREP_U8 = 4, 16384, 3      # NAF_IMAGE_PREP_*
PREP_NONE, PREP_BILINEAR, PREP_BICUBIC = 0, 1, 2                          # naf_prep_mode


class ImagePrepView(C.Structure):
    """naf_image_prep_view: one derived image of naf_image_prep -- first resize, normalise, second resize, store."""
    _fields_ = [
        ("out", C.c_void_p), ("out_stride", I64x4), ("out_dtype", C.c_int32), ("h1", C.c_int32), ("w1", C.c_int32), ("mode1", C.c_int32),
        ("normalise", C.c_int32), ("h2", C.c_int32), ("w2", C.c_int32), ("mode2", C.c_int32),
        ("mean", C.c_float * 3), ("std", C.c_float * 3), ("reserved", C.c_int32 * 2),
    ]


class ImagePrepArgs(C.Structure):
    """naf_image_prep_args (added after the point queries, detected by symbol): up to four views of one source image from one launch."""
    _fields_ = [
        ("src", C.c_void_p), ("src_stride", I64x4), ("src_dtype", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("hflip", C.c_int32), ("n_views", C.c_int32), ("reserved", C.c_int32 * 2), ("view", ImagePrepView * IMAGE_PREP_MAX_VIEWS),
    ]


DENOISE_LOSS, DENOISE_METRICS = 0, 1            # naf_denoise_mode


class DenoiseArgs(C.Structure):
    """naf_denoise_args (added after the propagation entries, detected by symbol): the denoising loss with its gradient, or the metrics."""
    _fields_ = [
        ("pred", C.c_void_p), ("target", C.c_void_p), ("grad", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t),
        ("pred_dtype", C.c_int32), ("target_dtype", C.c_int32), ("grad_dtype", C.c_int32), ("mode", C.c_int32),
        ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("clamp", C.c_int32), ("reserved", C.c_int32),
        ("l1_weight", C.c_double), ("l2_weight", C.c_double), ("ssim_weight", C.c_double),
        ("pred_stride", I64x4), ("target_stride", I64x4), ("grad_stride", I64x4),
    ]


MOMENTS_CHAIN = 65536                           # NAF_MOMENTS_CHAIN: most fp32 additions between a product and the fp64 sum
MOMENTS_WORKSPACE_CAP = 256 << 20               # NAF_MOMENTS_WORKSPACE_CAP
PCA_MAX_C, PCA_MAX_COMPONENTS = 4096, 8


class FeatureMomentsArgs(C.Structure):
    """naf_feature_moments_args (added after the denoising entries, detected by symbol): Gram matrix and channel sums of one feature map."""
    _fields_ = [
        ("x", C.c_void_p), ("gram", C.c_void_p), ("sum", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("P", C.c_int64), ("ld", C.c_int64), ("C", C.c_int32), ("reserved", C.c_int32),
    ]


class PcaProjectArgs(C.Structure):
    """naf_pca_project_args: a map's projection on n components with the components' minima and maxima."""
    _fields_ = [
        ("x", C.c_void_p), ("V", C.c_void_p), ("b", C.c_void_p), ("y", C.c_void_p), ("minmax", C.c_void_p), ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t), ("P", C.c_int64), ("ld", C.c_int64), ("C", C.c_int32), ("n", C.c_int32), ("reserved", C.c_int32 * 2),
    ]


class PcaMinmaxArgs(C.Structure):
    """naf_pca_minmax_args: minima and maxima of an existing fp32 projection."""
    _fields_ = [
        ("y", C.c_void_p), ("minmax", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("P", C.c_int64), ("ld", C.c_int64), ("n", C.c_int32), ("reserved", C.c_int32),
    ]


class StemConv0Args(C.Structure):
    _fields_ = [
        ("image", C.c_void_p), ("y", C.c_void_p), ("weight", C.c_void_p), ("bias", C.c_void_p), ("stats_out", C.c_void_p),
        ("image_dtype", C.c_int32), ("ksize", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("channels", C.c_int32), ("image_stride", I64x4), ("y_stride", I64x3), ("flags", C.c_int32), ("reserved", C.c_int32),
    ]


CONV0_EXACT = 1                                  # naf_stem_conv0_args.flags
FWD_CONV0_EXACT, FWD_ONE_STREAM, FWD_TWO_STREAMS = 1, 2, 4   # naf_forward_ex flags


class StemConvArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("w_packed", C.c_void_p), ("bias", C.c_void_p), ("gn_weight", C.c_void_p),
        ("gn_bias", C.c_void_p), ("stats_in", C.c_void_p), ("stats_out", C.c_void_p),
        ("ksize", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("eps", C.c_float),
        ("channels", C.c_int32), ("x_stride", I64x3), ("y_stride", I64x3), ("first", C.POINTER(StemConv0Args)),
    ]


class KeyPoolArgs(C.Structure):
    _fields_ = [
        ("k_lr", C.c_void_p), ("tab_y", C.c_void_p), ("tab_x", C.c_void_p), ("h", C.c_int32), ("w", C.c_int32),
        ("k_stride", I64x3),
    ]


class RopePoolBwdArgs(C.Structure):
    _fields_ = [
        ("dq", C.c_void_p), ("dk_lr", C.c_void_p), ("dx", C.c_void_p), ("tab_y", C.c_void_p), ("tab_x", C.c_void_p),
        ("B", C.c_int32), ("Cq", C.c_int32), ("heads", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("h", C.c_int32),
        ("w", C.c_int32), ("dq_stride", I64x4), ("dk_stride", I64x4), ("dx_stride", I64x4),
    ]


class StemWgradArgs(C.Structure):
    _fields_ = [
        ("dy", C.c_void_p), ("x", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p), ("gn_weight", C.c_void_p), ("gn_bias", C.c_void_p),
        ("stats_in", C.c_void_p), ("ksize", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("eps", C.c_float),
        ("channels", C.c_int32), ("dy_stride", I64x3), ("x_stride", I64x3),
    ]


class StemConv0WgradArgs(C.Structure):
    _fields_ = [
        ("dy", C.c_void_p), ("image", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p), ("image_dtype", C.c_int32),
        ("ksize", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32), ("dy_stride", I64x3),
        ("image_stride", I64x4),
    ]


class StemConv0DgradArgs(C.Structure):
    _fields_ = [
        ("dy", C.c_void_p), ("weight", C.c_void_p), ("dimage", C.c_void_p), ("ksize", C.c_int32), ("B", C.c_int32), ("H", C.c_int32),
        ("W", C.c_int32), ("channels", C.c_int32), ("accumulate", C.c_int32), ("dy_stride", I64x3), ("dimage_stride", I64x4),
    ]


class StemActArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("a", C.c_void_p), ("gn_weight", C.c_void_p), ("gn_bias", C.c_void_p), ("stats_in", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32), ("pad", C.c_int32), ("eps", C.c_float),
        ("x_stride", I64x3), ("a_stride", I64x3),
    ]


class StemActBwdArgs(C.Structure):
    _fields_ = [
        ("da", C.c_void_p), ("x", C.c_void_p), ("dx", C.c_void_p), ("gn_weight", C.c_void_p), ("gn_bias", C.c_void_p),
        ("stats_in", C.c_void_p), ("sums", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32), ("fold", C.c_int32), ("phase", C.c_int32),
        ("eps", C.c_float), ("da_stride", I64x3), ("x_stride", I64x3), ("dx_stride", I64x3),
    ]


class XnaBwdArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k_lr", C.c_void_p), ("v_lr", C.c_void_p), ("dout", C.c_void_p), ("dq", C.c_void_p),
        ("dk_lr", C.c_void_p), ("dv_lr", C.c_void_p), ("idx_y", C.c_void_p), ("idx_x", C.c_void_p),
        ("B", C.c_int32), ("heads", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("h", C.c_int32),
        ("w", C.c_int32), ("Dq", C.c_int32), ("Dv", C.c_int32), ("ky", C.c_int32), ("kx", C.c_int32),
        ("scale", C.c_float), ("path", C.c_int32),
        ("q_stride", I64x4), ("k_stride", I64x4), ("v_stride", I64x4), ("dout_stride", I64x4), ("dq_stride", I64x4),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class XnaBwdScoresArgs(C.Structure):
    """naf_xna_bwd_scores_args (0.4.3): the gradient of naf_xna_fwd's logits for naf_xna_bwd_scores."""
    _fields_ = [("dlogits", C.c_void_p), ("dlogits_stride", I64x4)]


MAX_STEM_LAYERS = 8


class StemBranch(C.Structure):
    _fields_ = [
        ("conv0_weight", C.c_void_p), ("conv0_bias", C.c_void_p), ("conv0_ksize", C.c_int32), ("ksize", C.c_int32),
        ("gn_weight", C.c_void_p * MAX_STEM_LAYERS), ("gn_bias", C.c_void_p * MAX_STEM_LAYERS),
        ("conv_weight_packed", C.c_void_p * MAX_STEM_LAYERS), ("conv_bias", C.c_void_p * MAX_STEM_LAYERS),
    ]


class ForwardArgs(C.Structure):
    _fields_ = [
        ("image", C.c_void_p), ("features", C.c_void_p), ("out", C.c_void_p), ("tab_y", C.c_void_p), ("tab_x", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("events", C.c_void_p * 2), ("logits", C.c_void_p),
        ("branch", StemBranch * 2),
        ("nlayer", C.c_int32), ("image_dtype", C.c_int32), ("feat_dtype", C.c_int32), ("out_dtype", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("C", C.c_int32),
        ("heads", C.c_int32), ("ksize", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("heads_rope", C.c_int32), ("reserved", C.c_int32), ("gn_eps", C.c_float), ("scale", C.c_float),
        ("image_stride", I64x4), ("feat_stride", I64x4), ("phase_events", C.c_void_p * 8),
    ]


class ForwardAux(C.Structure):
    """naf_forward_aux: the second stream and the fork / join events the caller lends to naf_forward_ex."""
    _fields_ = [("stream", C.c_void_p), ("fork_event", C.c_void_p), ("join_event", C.c_void_p)]


# Entry points that read or write GroupNorm-sum buffers are EXPORTED under names that carry the copy count (naf_hip.h, 0.4.0: a
# binary built for another buffer layout fails to resolve them instead of overrunning its buffers); header name -> exported name
STATS_SLOTS_ABI = 16
EXPORTED_AS = {n: f"{n}_s{STATS_SLOTS_ABI}" for n in ("naf_stem_conv0_fwd", "naf_stem_conv_fwd", "naf_stem_conv_keys_fwd",
                                                      "naf_stem_act_fwd", "naf_stem_act_bwd", "naf_stem_wgrad")}

# symbol -> (restype, argtypes); must list every function include/naf_hip.h declares
SIGNATURES = {
    "naf_version": (C.c_int, []),
    "naf_last_error": (C.c_char_p, []),
    "naf_abi_check": (C.c_int, [C.c_int]),
    "naf_dtype_supported": (C.c_int, [C.c_int, C.c_int]),
    "naf_stem_stats_bytes": (C.c_size_t, [C.c_int32]),
    "naf_forward_aux_create": (C.c_int, [C.POINTER(ForwardAux)]),
    "naf_forward_aux_destroy": (C.c_int, [C.POINTER(ForwardAux)]),
    "naf_forward_streams": (C.c_int, [C.POINTER(ForwardArgs), C.c_uint32]),
    "naf_forward_workspace_view": (C.c_int, [C.POINTER(ForwardArgs), C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "naf_forward_ex": (C.c_int, [C.POINTER(ForwardArgs), C.POINTER(ForwardAux), C.c_uint32, C.c_void_p]),
    "naf_axis_index_table": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32]),
    "naf_stem_weight_index": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "naf_axis_index_table_device": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "naf_stem_conv0_fwd": (C.c_int, [C.POINTER(StemConv0Args), C.c_void_p]),
    "naf_stem_conv_fwd": (C.c_int, [C.POINTER(StemConvArgs), C.c_void_p]),
    "naf_stem_conv_keys_supported": (C.c_int, [C.POINTER(StemConvArgs), C.POINTER(KeyPoolArgs)]),
    "naf_stem_conv_keys_fwd": (C.c_int, [C.POINTER(StemConvArgs), C.POINTER(KeyPoolArgs), C.c_void_p]),
    "naf_rope_pool_bwd": (C.c_int, [C.POINTER(RopePoolBwdArgs), C.c_void_p]),
    "naf_stem_wgrad": (C.c_int, [C.POINTER(StemWgradArgs), C.c_void_p]),
    "naf_stem_conv0_wgrad": (C.c_int, [C.POINTER(StemConv0WgradArgs), C.c_void_p]),
    "naf_stem_conv0_dgrad": (C.c_int, [C.POINTER(StemConv0DgradArgs), C.c_void_p]),
    "naf_stem_act_fwd": (C.c_int, [C.POINTER(StemActArgs), C.c_void_p]),
    "naf_stem_act_bwd": (C.c_int, [C.POINTER(StemActBwdArgs), C.c_void_p]),
    "naf_rope_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "naf_rope_pool_fwd": (C.c_int, [C.POINTER(RopePoolArgs), C.c_void_p]),
    "naf_preshrink_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(I64x4), C.c_void_p]),
    "naf_pool_guidance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "naf_pool_guidance_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "naf_preshrink_image_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(I64x4), C.c_void_p]),
    "naf_pack_values": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.POINTER(C.c_int64), C.c_void_p]),
    "naf_xna_select": (C.c_int, [C.POINTER(XnaArgs)]),
    "naf_xna_union_plan": (C.c_int, [C.POINTER(XnaArgs), C.POINTER(C.c_int32)]),
    "naf_workspace_bytes": (C.c_size_t, [C.POINTER(XnaArgs)]),
    "naf_xna_fwd": (C.c_int, [C.POINTER(XnaArgs), C.c_void_p]),
    "naf_xna_head_select": (C.c_int, [C.POINTER(XnaHeadArgs)]),
    "naf_xna_head_workspace_bytes": (C.c_size_t, [C.POINTER(XnaHeadArgs)]),
    "naf_xna_head_fwd": (C.c_int, [C.POINTER(XnaHeadArgs), C.c_void_p]),
    "naf_xna_head_ce_select": (C.c_int, [C.POINTER(XnaHeadCEArgs)]),
    "naf_xna_head_ce_fwd": (C.c_int, [C.POINTER(XnaHeadCEArgs), C.c_void_p]),
    "naf_xna_head_cm_select": (C.c_int, [C.POINTER(XnaHeadCMArgs)]),
    "naf_xna_head_cm_fwd": (C.c_int, [C.POINTER(XnaHeadCMArgs), C.c_void_p]),
    "naf_xna_head_reg_select": (C.c_int, [C.POINTER(XnaHeadRegArgs)]),
    "naf_xna_head_reg_workspace_bytes": (C.c_size_t, [C.POINTER(XnaHeadRegArgs)]),
    "naf_xna_head_reg_fwd": (C.c_int, [C.POINTER(XnaHeadRegArgs), C.c_void_p]),
    "naf_xna_cos_select": (C.c_int, [C.POINTER(XnaCosArgs)]),
    "naf_xna_cos_fwd": (C.c_int, [C.POINTER(XnaCosArgs), C.c_void_p]),
    "naf_xna_cos_ce_select": (C.c_int, [C.POINTER(XnaCosCEArgs)]),
    "naf_xna_cos_ce_fwd": (C.c_int, [C.POINTER(XnaCosCEArgs), C.c_void_p]),
    "naf_xna_maskpool_select": (C.c_int, [C.POINTER(XnaMaskPoolArgs)]),
    "naf_xna_maskpool_workspace_bytes": (C.c_size_t, [C.POINTER(XnaMaskPoolArgs)]),
    "naf_xna_maskpool_fwd": (C.c_int, [C.POINTER(XnaMaskPoolArgs), C.c_void_p]),
    "naf_maskpool_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(C.c_int64), C.c_int32, C.c_void_p]),
    "naf_xna_cos_peaks_select": (C.c_int, [C.POINTER(XnaCosPeaksArgs)]),
    "naf_xna_cos_peaks_fwd": (C.c_int, [C.POINTER(XnaCosPeaksArgs), C.c_void_p]),
    "naf_peaks_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                 C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]),
    "naf_xna_kmeans_select": (C.c_int, [C.POINTER(XnaKmeansArgs)]),
    "naf_xna_kmeans_workspace_bytes": (C.c_size_t, [C.POINTER(XnaKmeansArgs)]),
    "naf_xna_kmeans_fwd": (C.c_int, [C.POINTER(XnaKmeansArgs), C.c_void_p]),
    "naf_propagate_select": (C.c_int, [C.POINTER(PropagateArgs)]),
    "naf_propagate_fwd": (C.c_int, [C.POINTER(PropagateArgs), C.c_void_p]),
    "naf_propagate_plan": (C.c_int, [C.POINTER(PropagateArgs), C.POINTER(C.c_int32)]),
    "naf_feature_inv_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "naf_denoise_workspace_bytes": (C.c_size_t, [C.POINTER(DenoiseArgs)]),
    "naf_denoise_objective": (C.c_int, [C.POINTER(DenoiseArgs), C.c_void_p]),
    "naf_feature_moments_workspace_bytes": (C.c_size_t, [C.POINTER(FeatureMomentsArgs)]),
    "naf_feature_moments_plan": (C.c_int, [C.POINTER(FeatureMomentsArgs), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "naf_feature_moments": (C.c_int, [C.POINTER(FeatureMomentsArgs), C.c_void_p]),
    "naf_pca_project_workspace_bytes": (C.c_size_t, [C.POINTER(PcaProjectArgs)]),
    "naf_pca_project": (C.c_int, [C.POINTER(PcaProjectArgs), C.c_void_p]),
    "naf_pca_minmax": (C.c_int, [C.POINTER(PcaMinmaxArgs), C.c_void_p]),
    "naf_xna_mse_supported": (C.c_int, [C.POINTER(XnaMSEArgs)]),
    "naf_xna_mse_workspace_bytes": (C.c_size_t, [C.POINTER(XnaMSEArgs)]),
    "naf_xna_mse_fwd": (C.c_int, [C.POINTER(XnaMSEArgs), C.c_void_p]),
    "naf_davis_jf_select": (C.c_int, [C.POINTER(DavisJFArgs)]),
    "naf_davis_jf": (C.c_int, [C.POINTER(DavisJFArgs), C.c_void_p]),
    "naf_mask_labels_select": (C.c_int, [C.POINTER(MaskLabelsArgs)]),
    "naf_mask_labels": (C.c_int, [C.POINTER(MaskLabelsArgs), C.c_void_p]),
    "naf_nearest_resize_table": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.c_int32]),
    "naf_xna_points": (C.c_int, [C.POINTER(XnaPointsArgs), C.c_void_p]),
    "naf_image_prep_select": (C.c_int, [C.POINTER(ImagePrepArgs)]),
    "naf_image_prep": (C.c_int, [C.POINTER(ImagePrepArgs), C.c_void_p]),
    "naf_xna_bwd_supported": (C.c_int, [C.POINTER(XnaBwdArgs)]),
    "naf_xna_bwd_workspace_bytes": (C.c_size_t, [C.POINTER(XnaBwdArgs)]),
    "naf_xna_bwd_chunk_plan": (C.c_int, [C.POINTER(XnaBwdArgs), C.POINTER(C.c_int32), C.c_int]),
    "naf_xna_bwd": (C.c_int, [C.POINTER(XnaBwdArgs), C.c_void_p]),
    "naf_xna_bwd_scores_supported": (C.c_int, [C.POINTER(XnaBwdArgs), C.POINTER(XnaBwdScoresArgs)]),
    "naf_xna_bwd_scores": (C.c_int, [C.POINTER(XnaBwdArgs), C.POINTER(XnaBwdScoresArgs), C.c_void_p]),
    "naf_forward_workspace_bytes": (C.c_size_t, [C.POINTER(ForwardArgs)]),
    "naf_forward_workspace_bytes_ex": (C.c_size_t, [C.POINTER(ForwardArgs), C.c_uint32]),
    "naf_forward_supported": (C.c_int, [C.POINTER(ForwardArgs)]),
    "naf_forward": (C.c_int, [C.POINTER(ForwardArgs), C.c_void_p]),
}

_lib = None
_lock = threading.Lock()


class NafHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """dlopen libnaf_hip.so and bind every declared symbol; raises NafHipError when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NafHipError(
                f"{LIB_PATH} not found: build it with `python -m naf_amd.build` (hipcc, gfx950). "
                "naf_amd has no CPU or PyTorch fallback for its kernels.")
        try:
            lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        except OSError as e:  # pragma: no cover
            raise NafHipError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            exported = EXPORTED_AS.get(name, name)
            try:
                fn = getattr(lib, exported)
            except AttributeError as e:
                raise NafHipError(f"{LIB_PATH} does not export {exported}; rebuild with `python -m naf_amd.build --force`") from e
            fn.restype, fn.argtypes = res, args
            if exported != name:
                setattr(lib, name, fn)           # callers use the header's names
        rc = lib.naf_abi_check(HEADER_VERSION)
        if rc != 0:
            raise NafHipError(f"{LIB_PATH}: {lib.naf_last_error().decode('utf-8', 'replace')}")
        _lib = lib
    return _lib


def last_error() -> str:
    return load().naf_last_error().decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = last_error()
        if rc == 1:
            raise ValueError(f"{what}: {msg}")
        raise NafHipError(f"{what} failed (status {rc}): {msg}")
