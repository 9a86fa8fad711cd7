"""naf_amd -- MI355X-native (gfx950 / CDNA4) implementation of NAF's cross-scale neighbourhood
attention filtering forward, behind the reference's own API (valeoai/NAF: src/model/naf.py).

    from naf_amd import NAF            # same constructor / state_dict as the reference
    naf = NAF().to("cuda").eval()
    hr = naf(image, lr_features, (H, W))
    loss = naf.train()(image, lr_features, (H, W), regress=hr_features)   # the training step's objective, from the attention kernel
    g = naf.guide(image); hr_b = naf(g, other_features, (H, W))           # encode the image once: no stem for the next backbone / size
    r = naf.query(g, points, features=lr_features, output_size=(H, W))    # scores, weights and features at N pixels, nothing dense
    loss = naf(image, lr_features, (H, W), head=probe, dense_target=depth, valid=mask)      # a depth probe's L1 loss, from the attention kernel

Kernels live in naf_amd/csrc (HIP, C ABI in include/naf_hip.h); build with ``python -m naf_amd.build``.
"""
from .model import NAF, CrossAttention, GraphedForward, Guidance, ImageEncoder, KMeans, Match, Peaks, PointQuery, RoPE  # noqa: F401
from .ops import ConfusionMetrics, FrameFeatures, confusion_metrics, pack_frame, propagate_labels  # noqa: F401
from .ops import DepthMetrics, depth_metrics  # noqa: F401
from .ops import DenoisingLoss, denoising_loss, denoising_metrics  # noqa: F401
from .ops import DavisJF, davis_jf, davis_statistics  # noqa: F401
from .ops import VideoTracker, labels_to_masks, masks_to_labels, nearest_index_table  # noqa: F401
from .ops import PrepView, davis_frame_views, lr_image_size, prepare_views, probing_views, training_views  # noqa: F401
from .feature_pca import FeaturePCA, pca  # noqa: F401

__all__ = ["NAF", "CrossAttention", "GraphedForward", "Guidance", "PointQuery", "Peaks", "Match", "KMeans", "ImageEncoder", "RoPE", "ConfusionMetrics", "confusion_metrics",
           "DepthMetrics", "depth_metrics",
           "FrameFeatures", "pack_frame", "propagate_labels", "DenoisingLoss", "denoising_loss", "denoising_metrics",
           "FeaturePCA", "pca", "DavisJF", "davis_jf", "davis_statistics",
           "VideoTracker", "labels_to_masks", "masks_to_labels", "nearest_index_table",
           "PrepView", "prepare_views", "davis_frame_views", "training_views", "probing_views", "lr_image_size"]
__version__ = "0.1.0"
