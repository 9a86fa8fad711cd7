"""Host-side operators over libnaf_hip.so: thin, typed wrappers that hand raw device pointers, element
strides and torch's current HIP stream to the C ABI.  torch is plumbing here (device memory, streams);
every kernel is the library's.  There is no CPU / eager fallback: CPU tensors raise.

Reference counterparts (paths relative to the reference repo):
  axis_index_table   NATTEN neighbourhood rule + nearest-exact map      src/layers/attentions.py:48-61
  stem_conv0/stem_conv  encoder() conv + GroupNorm + SiLU chain         src/layers/convolutions.py:6-92
  rope_tables        RoPE.create_coordinate / angle, sin, cos           src/layers/rope.py:84-105,137-146
  rope_pool          RoPE.forward rotation + KeyEncoder pooling         src/layers/rope.py:147-174, src/model/naf.py:63-69
  pack_values        CrossAttention._resize layout/dtype part           src/layers/attentions.py:50-51
  xna_forward        legacy_attention / na2d                            src/layers/attentions.py:16-29,72
  xna_points         the same at N query pixels (the attention viewer's read)    notebooks/attention_maps.ipynb cell 11
  xna_head_forward   the same with the probe's 1x1 convolution folded in  evaluation/eval_seg_probing.py:56,104-111
  propagate_labels   label_propagation after feature extraction          evaluation/eval_video_seg.py:499-561
  davis_jf / davis_statistics  davis_db_eval_iou, davis_db_eval_boundary, davis_db_statistics  evaluation/eval_video_seg.py:145-269
  masks_to_labels / labels_to_masks / VideoTracker  the upsample, norm_mask, argmax and PIL resize of a propagated frame; read_seg + to_one_hot;
                     the queue of eval_video_tracking_davis                 evaluation/eval_video_seg.py:389-457,488-496,611-643
  prepare_views / PrepView / davis_frame_views / training_views / probing_views  the resizes and normalisations in front of the model
                     evaluation/eval_video_seg.py:577-597, train.py:115-126, utils/training.py:24-47, evaluation/eval_seg_probing.py:97-98
  denoising_loss     DenoisingLoss.forward and its backward               denoising.py:129-177
  denoising_metrics  MetricsCalculator.calculate_batch_metrics            denoising.py:61-126,302
  feature_moments / pca_project / pca_minmax  pca() and TorchPCA          utils/visualization.py:135-190
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import math
import threading
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import XnaArgs, XnaHeadArgs, XnaBwdArgs, XnaBwdScoresArgs, RopePoolArgs, StemConv0Args, StemConvArgs, KeyPoolArgs, ForwardArgs, I64x3, I64x4

_DT = {torch.bfloat16: _lib.NAF_BF16, torch.float32: _lib.NAF_F32}
# The VALUES and the output of the attention forward also come as float16 (naf_dtype_supported): a map of its own, because _DT
# gates image dtypes, targets and every other entry, none of which takes half.
_DT_VALUES = {**_DT, torch.float16: _lib.NAF_F16}

# Optional kernel timer (bench.py): an object with start(name) / stop(name) that records HIP events on
# the CURRENT stream tightly around one C-ABI launch.  None in normal operation.
KERNEL_TIMER = None


class _Timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if KERNEL_TIMER is not None:
            KERNEL_TIMER.start(self.name)

    def __exit__(self, *exc):
        if KERNEL_TIMER is not None:
            KERNEL_TIMER.stop(self.name)
        return False
_PATH = {"auto": _lib.XNA_AUTO, "mfma": _lib.XNA_MFMA, "generic": _lib.XNA_GENERIC, "union": _lib.XNA_UNION, "rows": _lib.XNA_ROWS}
_PATH_NAME = {_lib.XNA_MFMA: "mfma", _lib.XNA_GENERIC: "generic", _lib.XNA_UNION: "union", _lib.XNA_ROWS: "rows"}


def _gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"naf_amd: `{name}` is on {t.device}; the NAF hot path only exists as HIP kernels for a "
                           "ROCm device (no CPU fallback). Move the module and its inputs to 'cuda'.")


def _stream(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _strides4(t: torch.Tensor, dims) -> I64x4:
    return I64x4(*[int(t.stride(d)) for d in dims])


def _strides3(t: torch.Tensor) -> I64x3:
    return I64x3(int(t.stride(0)), int(t.stride(1)), int(t.stride(2)))


def _ksize(kernel_size):
    """(ky, kx) of an int or a pair."""
    return (int(kernel_size), int(kernel_size)) if isinstance(kernel_size, int) else (int(kernel_size[0]), int(kernel_size[1]))


# ------------------------------------------------------------------------------------------------
def axis_index_table(L_out: int, L_in: int, k: int) -> torch.Tensor:
    """[L_out, k] int32 CPU tensor of low-res indices (host function of the library, no GPU needed)."""
    lib = _lib.load()
    if L_out <= 0 or k <= 0:
        raise ValueError(f"axis_index_table: bad sizes L_out={L_out} k={k}")
    out = torch.empty((int(L_out), int(k)), dtype=torch.int32)
    rc = lib.naf_axis_index_table(C.cast(out.data_ptr(), C.POINTER(C.c_int32)), int(L_out), int(L_in), int(k))
    _lib.check(rc, "naf_axis_index_table")
    return out


_table_cache = {}


def device_index_table(L_out: int, L_in: int, k: int, device) -> torch.Tensor:
    key = (int(L_out), int(L_in), int(k), str(device))
    t = _table_cache.get(key)
    if t is None:
        if len(_table_cache) > 64:
            _table_cache.clear()
        t = axis_index_table(L_out, L_in, k).to(device)
        _table_cache[key] = t
    return t


# ------------------------------------------------------------------------------------------------
STATS_SLOTS = 16   # NAF_STATS_SLOTS of include/naf_hip.h: partial copies of every GroupNorm-sum buffer


def new_stats(B: int, device, lead: Tuple[int, ...] = ()) -> torch.Tensor:
    """Zeroed GroupNorm-sum buffer(s) ``[*lead, STATS_SLOTS, B, 8, 2]`` (f64): a producing workgroup adds into one of the
    ``STATS_SLOTS`` copies, consumers add them up (include/naf_hip.h, "guidance conv stem")."""
    return torch.zeros((*lead, STATS_SLOTS, B, 8, 2), dtype=torch.float64, device=device)


def stats_total(stats: torch.Tensor) -> torch.Tensor:
    """``[..., STATS_SLOTS, B, 8, 2]`` -> the sums ``[..., B, 8, 2]``."""
    return stats.sum(dim=-4)


def stats_from_total(total: torch.Tensor) -> torch.Tensor:
    """Sums ``[B, 8, 2]`` (e.g. computed by torch) as a buffer the stem entries read: copy 0 holds them, the rest is zero."""
    st = new_stats(total.shape[0], total.device)
    st[0] = total
    return st


def _stats_ptr(t: Optional[torch.Tensor], B: int, what: str):
    if t is None:
        return None
    if tuple(t.shape) != (STATS_SLOTS, B, 8, 2) or t.dtype != torch.float64 or not t.is_contiguous():
        raise ValueError(f"{what}: GroupNorm sums must be a contiguous f64 [{STATS_SLOTS}, {B}, 8, 2] tensor (ops.new_stats), "
                         f"got {tuple(t.shape)} {t.dtype}")
    return t.data_ptr()


def pack_conv_weight(weight: torch.Tensor) -> torch.Tensor:
    """``w_packed`` of ``naf_stem_conv_fwd`` for a Conv2d weight ``[oc, ic, k, k]`` (k in {1, 3}, oc == ic): bf16 ``[k*k, oc, ic]``
    -- for the 3x3 layers of the default width (128 channels) holding the elements in the order the kernel's lanes keep them,
    ``[9 taps][4 blocks of 32 oc][8 steps of 16 ic][2 halves of 8 ic][32 oc][8 ic]`` (``naf_stem_weight_index``), otherwise
    plain ``weight.permute(2, 3, 0, 1)``.  The data gradient of a layer is the same kernel on
    ``pack_conv_weight(weight.flip(2, 3).transpose(0, 1))``."""
    oc, ic, k, k2 = weight.shape
    if oc != ic or k != k2 or k not in (1, 3):
        raise ValueError(f"pack_conv_weight: expected [C, C, k, k] with k in {{1, 3}}, got {tuple(weight.shape)}")
    w = weight.detach().permute(2, 3, 0, 1).reshape(k * k, oc, ic)
    if k == 3 and oc == 128:
        # (t, wave, n32, ks, half, e) -> (t, wave, ks, half, n32, e)
        w = w.reshape(9, 4, 32, 8, 2, 8).permute(0, 1, 3, 4, 2, 5).reshape(9, 128, 128)
    return w.contiguous().to(torch.bfloat16)


def unpack_conv_weight(w_packed: torch.Tensor) -> torch.Tensor:
    """Inverse of ``pack_conv_weight``: the Conv2d weight ``[oc, ic, k, k]`` (bf16 values as fp32)."""
    taps, oc, ic = w_packed.shape
    k = {1: 1, 9: 3}[int(taps)]
    w = w_packed.float()
    if k == 3 and oc == 128:
        w = w.reshape(9, 4, 8, 2, 32, 8).permute(0, 1, 4, 2, 3, 5).reshape(9, 128, 128)
    return w.reshape(k, k, oc, ic).permute(2, 3, 0, 1).contiguous()


def _fill_stem_conv0(image, weight, bias, y, stats_out) -> StemConv0Args:
    B, Cin, H, W = image.shape
    Cout = int(weight.shape[0])
    if Cin != 3 or weight.shape[1] != 3 or Cout % 16 or not (16 <= Cout <= 256) or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise ValueError(f"stem_conv0: expected a 3-channel image and an f32 [C,3,k,k] weight with C a multiple of 16 up to 256, "
                         f"got {tuple(image.shape)} / {tuple(weight.shape)}")
    a = StemConv0Args()
    a.channels = Cout
    a.image, a.weight, a.bias = image.data_ptr(), weight.data_ptr(), bias.data_ptr()
    a.y = y.data_ptr() if y is not None else None
    a.stats_out = _stats_ptr(stats_out, B, "stem_conv0")
    a.image_dtype, a.ksize, a.B, a.H, a.W = _DT[image.dtype], int(weight.shape[-1]), B, H, W
    a.image_stride = _strides4(image, (0, 1, 2, 3))
    a.y_stride = _strides3(y) if y is not None else I64x3(0, 0, 0)
    return a


def stem_conv0(image: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, y: Optional[torch.Tensor],
               stats_out: torch.Tensor, exact: bool = False) -> None:
    """Conv2d(3 -> 128, k in {1, 3}, reflect) + bias.  image [B,3,H,W] f32/bf16 (any strides); weight f32
    [128,3,k,k]; y: bf16 [B,H,W,128] view (128 channels contiguous) or None (statistics only);
    stats_out: ``new_stats(B, device)`` (f64 [STATS_SLOTS,B,8,2], zeroed).  ``exact=True`` sets ``NAF_CONV0_EXACT``: the 3x3
    kernel of the default width then sums all six terms of the bf16 split (exact fp32 products) instead of three."""
    _gpu(image, "image")
    lib = _lib.load()
    if image.dtype not in _DT:
        image = image.float()
    a = _fill_stem_conv0(image, weight, bias, y, stats_out)
    a.flags = _lib.CONV0_EXACT if exact else 0
    with torch.cuda.device(image.device), _Timed("stem_conv0"):
        rc = lib.naf_stem_conv0_fwd(C.byref(a), _stream(image))
    _lib.check(rc, "naf_stem_conv0_fwd")


def stem_conv(x: Optional[torch.Tensor], stats_in: torch.Tensor, gn_weight: torch.Tensor, gn_bias: torch.Tensor, eps: float,
              w_packed: torch.Tensor, bias: torch.Tensor, y: torch.Tensor, stats_out: Optional[torch.Tensor],
              first=None, keys=None) -> None:
    """GroupNorm(8,128) -> SiLU -> Conv2d(128 -> 128, k in {1,3}, reflect) + bias on bf16 [B,H,W,128] views.
    w_packed: ``pack_conv_weight(conv.weight)`` (bf16 [k*k, C, C]); stats: f64 [STATS_SLOTS,B,8,2] buffers of ``new_stats`` (stats_out zeroed, or None).
    ``first=(image, conv0_weight, conv0_bias)`` (1x1 layers only, ``x=None``): the input is bf16(conv0(image))
    recomputed on the fly; ``stats_in`` then come from ``stem_conv0(..., y=None, ...)``.
    ``keys=(k_slice, tab_y, tab_x)`` (a branch's LAST layer, ``stats_out=None``): ``naf_stem_conv_keys_fwd`` -- the layer also
    writes its 128 channels of the pooled, RoPE'd keys into the bf16 ``[B, h, w, 128]`` view ``k_slice`` (16 x 16 pixel cells);
    raises when the library does not serve the geometry (``stem_conv_keys_supported``)."""
    lib = _lib.load()
    f0 = None
    if first is not None:
        image, w0, b0 = first
        _gpu(image, "image")
        if image.dtype not in _DT:
            image = image.float()
        f0 = _fill_stem_conv0(image, w0, b0, None, None)
        x = y                                                        # shape / device donor only
    _gpu(x, "x")
    B, H, W, Cc = x.shape
    if Cc % 16 or not (16 <= Cc <= 256) or x.dtype != torch.bfloat16 or x.stride(3) != 1 or y.stride(3) != 1:
        raise ValueError("stem_conv: activations must be bf16 [B,H,W,C] with channels contiguous, C a multiple of 16 up to 256")
    if tuple(w_packed.shape[1:]) != (Cc, Cc):
        raise ValueError(f"stem_conv: packed weight {tuple(w_packed.shape)} does not match {Cc} channels")
    taps = w_packed.shape[0]
    a = StemConvArgs()
    a.x, a.y, a.w_packed, a.bias = (None if first is not None else x.data_ptr()), y.data_ptr(), w_packed.data_ptr(), bias.data_ptr()
    if f0 is not None:
        a.first = C.pointer(f0)
    a.gn_weight, a.gn_bias, a.stats_in = gn_weight.data_ptr(), gn_bias.data_ptr(), _stats_ptr(stats_in, B, "stem_conv")
    a.stats_out = _stats_ptr(stats_out, B, "stem_conv")
    a.ksize = {1: 1, 9: 3}[int(taps)]
    a.channels = Cc
    a.B, a.H, a.W, a.eps = B, H, W, float(eps)
    a.x_stride = _strides3(x)
    a.y_stride = _strides3(y)
    if keys is not None:
        kp = _fill_key_pool(keys, x)
        with torch.cuda.device(x.device), _Timed("stem_conv%d_keys" % a.ksize):
            rc = lib.naf_stem_conv_keys_fwd(C.byref(a), C.byref(kp), _stream(x))
        _lib.check(rc, "naf_stem_conv_keys_fwd")
        return
    with torch.cuda.device(x.device), _Timed("stem_conv%d" % a.ksize):
        rc = lib.naf_stem_conv_fwd(C.byref(a), _stream(x))
    _lib.check(rc, "naf_stem_conv_fwd")


def _fill_key_pool(keys, x) -> KeyPoolArgs:
    k_slice, tab_y, tab_x = keys
    _gpu(k_slice, "k_slice")
    if k_slice.dtype != torch.bfloat16 or k_slice.dim() != 4 or k_slice.shape[0] != x.shape[0] or k_slice.shape[3] != 128 or k_slice.stride(3) != 1:
        raise ValueError("stem_conv: keys must be a bf16 [B, h, w, 128] view with channels contiguous")
    if tab_y.dtype != torch.float32 or tab_x.dtype != torch.float32 or tab_y.shape[-1] != 16 or tab_x.shape[-1] != 16:
        raise ValueError("stem_conv: keys need the fp32 RoPE tables of 16 periods (heads of 64 channels)")
    kp = KeyPoolArgs()
    kp.k_lr, kp.tab_y, kp.tab_x = k_slice.data_ptr(), tab_y.data_ptr(), tab_x.data_ptr()
    kp.h, kp.w = int(k_slice.shape[1]), int(k_slice.shape[2])
    kp.k_stride = _strides3(k_slice)
    return kp


def stem_conv_plain(x: torch.Tensor, w_packed: torch.Tensor, y: torch.Tensor, bias: Optional[torch.Tensor] = None) -> None:
    """y = conv(x) (+ bias): ``naf_stem_conv_fwd`` without GroupNorm / SiLU, bf16 [B,H,W,C] views (any width the stem serves), reflect padding for the
    3x3 kernel.  With ``w_packed = pack_conv_weight(weight.flip(2, 3).transpose(0, 1))`` it is a layer's data gradient (see include/naf_hip.h)."""
    lib = _lib.load()
    _gpu(x, "x")
    B, H, W, Cc = x.shape
    if Cc % 16 or not (16 <= Cc <= 256) or x.dtype != torch.bfloat16 or y.dtype != torch.bfloat16 or x.stride(3) != 1 or y.stride(3) != 1:
        raise ValueError("stem_conv_plain: bf16 [B,H,W,C] activations with channels contiguous, C a multiple of 16 up to 256")
    if tuple(w_packed.shape[1:]) != (Cc, Cc) or w_packed.dtype != torch.bfloat16 or not w_packed.is_contiguous():
        raise ValueError(f"stem_conv_plain: packed weight {tuple(w_packed.shape)} / {w_packed.dtype}")
    a = StemConvArgs()
    a.x, a.y, a.w_packed = x.data_ptr(), y.data_ptr(), w_packed.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.gn_weight = a.gn_bias = a.stats_in = a.stats_out = None
    a.ksize = {1: 1, 9: 3}[int(w_packed.shape[0])]
    a.channels = Cc
    a.B, a.H, a.W, a.eps = B, H, W, 0.0
    a.x_stride = _strides3(x)
    a.y_stride = _strides3(y)
    with torch.cuda.device(x.device), _Timed("stem_dgrad%d" % a.ksize):
        rc = lib.naf_stem_conv_fwd(C.byref(a), _stream(x))
    _lib.check(rc, "naf_stem_conv_fwd")


def stem_act(x: torch.Tensor, stats_in: torch.Tensor, gn_weight: torch.Tensor, gn_bias: torch.Tensor, eps: float,
             pad: int = 0) -> torch.Tensor:
    """SiLU(GroupNorm(8, C)(x)) as bf16 [B, H + 2 pad, W + 2 pad, C] with a reflected border (``naf_stem_act_fwd``)."""
    lib = _lib.load()
    _gpu(x, "x")
    B, H, W, Cc = x.shape
    out = torch.empty((B, H + 2 * pad, W + 2 * pad, Cc), dtype=torch.bfloat16, device=x.device)
    a = _lib.StemActArgs()
    a.x, a.a, a.gn_weight, a.gn_bias, a.stats_in = x.data_ptr(), out.data_ptr(), gn_weight.data_ptr(), gn_bias.data_ptr(), _stats_ptr(stats_in, B, "stem_act")
    a.B, a.H, a.W, a.channels, a.pad, a.eps = B, H, W, Cc, int(pad), float(eps)
    a.x_stride = _strides3(x)
    a.a_stride = _strides3(out)
    with torch.cuda.device(x.device), _Timed("stem_act"):
        rc = lib.naf_stem_act_fwd(C.byref(a), _stream(x))
    _lib.check(rc, "naf_stem_act_fwd")
    return out


def stem_wgrad(dy: torch.Tensor, x: torch.Tensor, stats_in: Optional[torch.Tensor], gn_weight: Optional[torch.Tensor],
               gn_bias: Optional[torch.Tensor], eps: float, ksize: int, with_bias: bool = False, out: Optional[torch.Tensor] = None):
    """Weight gradient [C, C, k, k] (fp32) of y = conv_k(SiLU(GroupNorm(x))) + b: ``naf_stem_wgrad``; dy, x bf16 [B,H,W,C]
    (C = 128: the hand-scheduled kernel of stem_wgrad.hip; other multiples of 16 up to 256: stem_generic_bwd.hip).
    ``stats_in=None``: x already is the activation SiLU(GroupNorm(.)) (``stem_act(..., pad=0)``).  ``with_bias``: also returns
    the bias gradient [128] (sum of dy over pixels, accumulated by the same kernel).  ``out``: a ZEROED fp32 buffer of
    ``k*k*C*C + C`` elements to accumulate into (a training step zeroes one buffer for all its layers) instead of a new one."""
    lib = _lib.load()
    _gpu(x, "x")
    B, H, W, Cc = x.shape
    if (Cc % 16 or not (16 <= Cc <= 256) or tuple(dy.shape) != (B, H, W, Cc) or dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16
            or dy.stride(3) != 1 or x.stride(3) != 1):
        raise ValueError("stem_wgrad: bf16 [B,H,W,C] tensors with channels contiguous, C a multiple of 16 up to 256")
    n_out = ksize * ksize * Cc * Cc + Cc
    if out is not None:
        if out.dtype != torch.float32 or out.numel() != n_out or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"stem_wgrad: out must be a contiguous zeroed f32 buffer of {n_out} elements")
        buf = out.view(-1)
    else:
        buf = torch.zeros((n_out,), dtype=torch.float32, device=x.device)   # one memset for both
    dw = buf[: ksize * ksize * Cc * Cc].view(ksize, ksize, Cc, Cc)                       # taps outermost: coalesced atomics
    db = buf[ksize * ksize * Cc * Cc:]
    a = _lib.StemWgradArgs()
    a.dy, a.x, a.dw = dy.data_ptr(), x.data_ptr(), dw.data_ptr()
    a.db = db.data_ptr() if with_bias else None
    if stats_in is not None:
        a.gn_weight, a.gn_bias, a.stats_in = gn_weight.data_ptr(), gn_bias.data_ptr(), _stats_ptr(stats_in, B, "stem_wgrad")
    else:
        a.gn_weight = a.gn_bias = a.stats_in = None
    a.ksize, a.B, a.H, a.W, a.eps, a.channels = int(ksize), B, H, W, float(eps), Cc
    a.dy_stride = _strides3(dy)
    a.x_stride = _strides3(x)
    with torch.cuda.device(x.device), _Timed("stem_wgrad%d" % ksize):
        rc = lib.naf_stem_wgrad(C.byref(a), _stream(x))
    _lib.check(rc, "naf_stem_wgrad")
    return (dw.permute(2, 3, 0, 1), db) if with_bias else dw.permute(2, 3, 0, 1)


def stem_conv0_wgrad(dy: torch.Tensor, image: torch.Tensor, ksize: int, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dW [C, 3, k, k], db [C]) of the first convolution (``naf_stem_conv0_wgrad``): dy bf16 [B,H,W,C], image [B,3,H,W]."""
    lib = _lib.load()
    _gpu(dy, "dy")
    B, H, W, Cc = dy.shape
    if Cc % 16 or not (16 <= Cc <= 256) or dy.dtype != torch.bfloat16 or dy.stride(3) != 1 or tuple(image.shape) != (B, 3, H, W):
        raise ValueError(f"stem_conv0_wgrad: dy {tuple(dy.shape)} / image {tuple(image.shape)}")
    if image.dtype not in _DT:
        image = image.float()
    nt = 3 * ksize * ksize
    if out is not None:      # a ZEROED contiguous f32 buffer of (3 k k + 1) C elements (see stem_wgrad)
        if out.dtype != torch.float32 or out.numel() != (nt + 1) * Cc or not out.is_contiguous() or out.device != dy.device:
            raise ValueError(f"stem_conv0_wgrad: out must be a contiguous zeroed f32 buffer of {(nt + 1) * Cc} elements")
        buf = out.view(-1)
    else:
        buf = torch.zeros(((nt + 1) * Cc,), dtype=torch.float32, device=dy.device)
    a = _lib.StemConv0WgradArgs()
    a.dy, a.image, a.dw, a.db = dy.data_ptr(), image.data_ptr(), buf.data_ptr(), buf[nt * Cc:].data_ptr()
    a.image_dtype, a.ksize, a.B, a.H, a.W, a.channels = _DT[image.dtype], int(ksize), B, H, W, Cc
    a.dy_stride = _strides3(dy)
    a.image_stride = _strides4(image, (0, 1, 2, 3))
    with torch.cuda.device(dy.device), _Timed("stem_conv0_wgrad"):
        rc = lib.naf_stem_conv0_wgrad(C.byref(a), _stream(dy))
    _lib.check(rc, "naf_stem_conv0_wgrad")
    return buf[: nt * Cc].view(3, ksize, ksize, Cc).permute(3, 0, 1, 2), buf[nt * Cc:]


def stem_conv0_dgrad(dy: torch.Tensor, weight: torch.Tensor, dimage: torch.Tensor, accumulate: bool = False) -> None:
    """Gradient of the first convolution Conv2d(3 -> C, k in {1, 3}, reflect) w.r.t. the image (``naf_stem_conv0_dgrad``):
    dy bf16 [B,H,W,C], weight f32 [C,3,k,k] (the parameter), dimage f32 [B,3,H,W] written or -- ``accumulate`` -- added to."""
    lib = _lib.load()
    _gpu(dy, "dy")
    B, H, W, Cc = dy.shape
    k = int(weight.shape[-1])
    if (Cc % 16 or not (16 <= Cc <= 256) or dy.dtype != torch.bfloat16 or dy.stride(3) != 1 or tuple(dimage.shape) != (B, 3, H, W)
            or dimage.dtype != torch.float32 or tuple(weight.shape) != (Cc, 3, k, k) or weight.dtype != torch.float32 or not weight.is_contiguous()):
        raise ValueError(f"stem_conv0_dgrad: dy {tuple(dy.shape)} / weight {tuple(weight.shape)} / dimage {tuple(dimage.shape)} {dimage.dtype}")
    a = _lib.StemConv0DgradArgs()
    a.dy, a.weight, a.dimage = dy.data_ptr(), weight.data_ptr(), dimage.data_ptr()
    a.ksize, a.B, a.H, a.W, a.channels, a.accumulate = k, B, H, W, Cc, int(bool(accumulate))
    a.dy_stride = _strides3(dy)
    a.dimage_stride = _strides4(dimage, (0, 1, 2, 3))
    with torch.cuda.device(dy.device), _Timed("stem_conv0_dgrad"):
        rc = lib.naf_stem_conv0_dgrad(C.byref(a), _stream(dy))
    _lib.check(rc, "naf_stem_conv0_dgrad")


def stem_act_bwd(da: torch.Tensor, x: torch.Tensor, stats_in: torch.Tensor, gn_weight: torch.Tensor, gn_bias: torch.Tensor,
                 eps: float, dx: torch.Tensor, fold: bool = False, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward of SiLU(GroupNorm(x)) (``naf_stem_act_bwd``): writes dx (bf16 [B,H,W,C] view) and returns the fp64 sums
    [B, C, 2] = per sample {d gn_bias, d gn_weight}.  ``fold``: da is [B, H+2, W+2, C], the gradient on the reflect-padded
    domain."""
    lib = _lib.load()
    _gpu(x, "x")
    B, H, W, Cc = x.shape
    want = (B, H + 2, W + 2, Cc) if fold else (B, H, W, Cc)
    if tuple(da.shape) != want or da.dtype != torch.bfloat16 or da.stride(3) != 1 or dx.stride(3) != 1 or tuple(dx.shape) != (B, H, W, Cc):
        raise ValueError(f"stem_act_bwd: da {tuple(da.shape)} (want {want}) / dx {tuple(dx.shape)}")
    if sums is not None:     # a ZEROED contiguous fp64 [B, C, 2] to accumulate into
        if sums.dtype != torch.float64 or tuple(sums.shape) != (B, Cc, 2) or not sums.is_contiguous() or sums.device != x.device:
            raise ValueError(f"stem_act_bwd: sums must be a contiguous zeroed f64 [{B}, {Cc}, 2]")
    else:
        sums = torch.zeros((B, Cc, 2), dtype=torch.float64, device=x.device)
    a = _lib.StemActBwdArgs()
    a.da, a.x, a.dx = da.data_ptr(), x.data_ptr(), dx.data_ptr()
    a.gn_weight, a.gn_bias, a.stats_in, a.sums = gn_weight.data_ptr(), gn_bias.data_ptr(), _stats_ptr(stats_in, B, "stem_act_bwd"), sums.data_ptr()
    a.B, a.H, a.W, a.channels, a.fold, a.phase, a.eps = B, H, W, Cc, int(bool(fold)), 0, float(eps)
    a.da_stride = _strides3(da)
    a.x_stride = _strides3(x)
    a.dx_stride = _strides3(dx)
    with torch.cuda.device(x.device), _Timed("stem_act_bwd"):
        rc = lib.naf_stem_act_bwd(C.byref(a), _stream(x))
    _lib.check(rc, "naf_stem_act_bwd")
    return sums


# ------------------------------------------------------------------------------------------------
def rope_tables(periods: torch.Tensor, Ho: int, Wo: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos/sin tables [Ho, 2, P] and [Wo, 2, P] (fp32) for the module's `periods` buffer [P]."""
    _gpu(periods, "periods")
    lib = _lib.load()
    per = periods.detach().to(torch.float32).contiguous()
    P = per.numel()
    ty = torch.empty((Ho, 2, P), dtype=torch.float32, device=per.device)
    tx = torch.empty((Wo, 2, P), dtype=torch.float32, device=per.device)
    with torch.cuda.device(per.device):
        rc = lib.naf_rope_tables(ty.data_ptr(), tx.data_ptr(), per.data_ptr(), P, int(Ho), int(Wo), _stream(per))
    _lib.check(rc, "naf_rope_tables")
    return ty, tx


def rope_pool(x: torch.Tensor, tab_y: torch.Tensor, tab_x: torch.Tensor, heads: int, lr_size,
              q_layout: str = "head_major", write_q: bool = True) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """x: logical [B, Cq, Ho, Wo] (bf16/fp32, any strides; channels-last is the fast layout).
    Returns q [B, heads, Ho, Wo, Dh] bf16 (RoPE'd queries) and k_lr [B, heads, h, w, Dh] bf16
    (adaptive-avg-pooled RoPE'd keys), both as 5-D strided views with Dh contiguous.
    ``write_q=False``: keys only (q is None) -- for ``xna_forward(..., rope_tables=...)`` which rotates the
    queries as it loads them."""
    _gpu(x, "guidance features")
    lib = _lib.load()
    if x.dtype not in _DT:
        x = x.float()
    B, Cq, Ho, Wo = x.shape
    h, w = int(lr_size[0]), int(lr_size[1])
    if Cq % heads:
        raise ValueError(f"rope_pool: {Cq} channels not divisible by {heads} heads")
    Dh = Cq // heads
    dev = x.device
    if not write_q:
        q = None
    elif q_layout == "head_major":
        q = torch.empty((B, heads, Ho, Wo, Dh), dtype=torch.bfloat16, device=dev)
    elif q_layout == "channels_last":
        q = torch.empty((B, Ho, Wo, heads, Dh), dtype=torch.bfloat16, device=dev).permute(0, 3, 1, 2, 4)
    else:
        raise ValueError(f"unknown q_layout {q_layout!r}")
    k = torch.empty((B, h, w, heads, Dh), dtype=torch.bfloat16, device=dev).permute(0, 3, 1, 2, 4)
    a = RopePoolArgs()
    a.x, a.q, a.k_lr = x.data_ptr(), (q.data_ptr() if q is not None else None), k.data_ptr()
    a.tab_y, a.tab_x = tab_y.data_ptr(), tab_x.data_ptr()
    a.x_dtype = _DT[x.dtype]
    a.B, a.Cq, a.heads, a.Ho, a.Wo, a.h, a.w = B, Cq, heads, Ho, Wo, h, w
    a.x_stride = _strides4(x, (0, 1, 2, 3))
    a.q_stride = _strides4(q, (0, 1, 2, 3)) if q is not None else I64x4(0, 0, 0, 0)
    a.k_stride = _strides4(k, (0, 1, 2, 3))
    if tab_y.shape != (Ho, 2, Dh // 4) or tab_x.shape != (Wo, 2, Dh // 4):
        raise ValueError(f"rope_pool: tables {tuple(tab_y.shape)}/{tuple(tab_x.shape)} do not match Ho={Ho} Wo={Wo} Dh/4={Dh // 4}")
    with torch.cuda.device(dev), _Timed("rope_pool"):
        rc = lib.naf_rope_pool_fwd(C.byref(a), _stream(x))
    _lib.check(rc, "naf_rope_pool_fwd")
    return q, k


def _preshrink_image(image: torch.Tensor, size) -> torch.Tensor:
    _gpu(image, "image")
    if image.dtype not in _DT or image.dim() != 4 or image.shape[1] != 3:
        raise ValueError("preshrink_image: expected a [B, 3, H, W] float32 / bfloat16 image")
    B, _, H, W = image.shape
    Hs, Ws = int(size[0]), int(size[1])
    out = torch.empty((B, 3, Hs, Ws), dtype=torch.float32, device=image.device)
    st = _strides4(image, (0, 1, 2, 3))
    lib = _lib.load()
    with torch.cuda.device(image.device), _Timed("preshrink"):
        rc = lib.naf_preshrink_image(out.data_ptr(), image.data_ptr(), _DT[image.dtype], B, H, W, Hs, Ws, C.byref(st), _stream(image))
    _lib.check(rc, "naf_preshrink_image")
    return out


def preshrink_image_bwd(dout: torch.Tensor, image_like: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adjoint of ``preshrink_image`` with respect to the image (``naf_preshrink_image_bwd``): dout [B, 3, Hs, Ws] (cast to dense fp32)
    -> the gradient of an image of ``image_like``'s shape and dtype (float32 / bfloat16; only those two are read, a meta tensor will do),
    laid out like it when it is dense (``torch.empty_like``).  ``out``: write into this tensor instead, whatever its strides.  Gather form,
    no atomics: bit-reproducible, unlike ATen's scatter."""
    _gpu(dout, "dout")
    if image_like.dtype not in _DT or image_like.dim() != 4 or image_like.shape[1] != 3:
        raise ValueError("preshrink_image_bwd: expected a [B, 3, H, W] float32 / bfloat16 image")
    B, _, H, W = image_like.shape
    if dout.dim() != 4 or dout.shape[0] != B or dout.shape[1] != 3:
        raise ValueError(f"preshrink_image_bwd: gradient {tuple(dout.shape)} does not belong to an image {tuple(image_like.shape)}")
    Hs, Ws = int(dout.shape[2]), int(dout.shape[3])
    if dout.dtype != torch.float32 or not dout.is_contiguous():
        dout = dout.float().contiguous()
    if out is None:
        dimage = torch.empty_like(image_like, device=dout.device)
    else:
        _gpu(out, "out")
        if out.shape != image_like.shape or out.dtype != image_like.dtype:
            raise ValueError(f"preshrink_image_bwd: out is {tuple(out.shape)} {out.dtype}, the image {tuple(image_like.shape)} {image_like.dtype}")
        dimage = out
    st = _strides4(dimage, (0, 1, 2, 3))
    lib = _lib.load()
    with torch.cuda.device(dout.device), _Timed("preshrink_bwd"):
        rc = lib.naf_preshrink_image_bwd(dimage.data_ptr(), dout.data_ptr(), _DT[dimage.dtype], B, H, W, Hs, Ws, C.byref(st), _stream(dout))
    _lib.check(rc, "naf_preshrink_image_bwd")
    return dimage


class PreshrinkFunction(torch.autograd.Function):
    """Differentiable ``preshrink_image``: forward = naf_preshrink_image, backward = naf_preshrink_image_bwd (gradient in the image's dtype)."""

    @staticmethod
    def forward(ctx, image, size):
        ctx.like = torch.empty_like(image, device="meta")     # shape, dtype and layout are all the backward reads
        return _preshrink_image(image, size)

    @staticmethod
    def backward(ctx, dout):
        return preshrink_image_bwd(dout, ctx.like), None


def preshrink_image(image: torch.Tensor, size) -> torch.Tensor:
    """F.interpolate(image, size, mode="bilinear", align_corners=False) of naf.py:39-48 -> fp32 [B, 3, Hs, Ws].  Differentiable with
    respect to the image (``PreshrinkFunction``) when autograd is on and the image requires grad."""
    if torch.is_grad_enabled() and image.requires_grad:
        _gpu(image, "image")
        return PreshrinkFunction.apply(image, size)
    return _preshrink_image(image, size)


def _pool_guidance(x: torch.Tensor, output_size) -> torch.Tensor:
    _gpu(x, "x")
    B, Cc, H, W = x.shape
    Ho, Wo = int(output_size[0]), int(output_size[1])
    xc = x.permute(0, 2, 3, 1)
    if x.dtype != torch.bfloat16 or not xc.is_contiguous() or Cc % 8:
        raise ValueError("pool_guidance: expected a dense channels-last bf16 tensor with C % 8 == 0")
    y = torch.empty((B, Ho, Wo, Cc), dtype=torch.bfloat16, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device), _Timed("pool_guidance"):
        rc = lib.naf_pool_guidance(y.data_ptr(), xc.data_ptr(), B, H, W, Ho, Wo, Cc, _stream(x))
    _lib.check(rc, "naf_pool_guidance")
    return y.permute(0, 3, 1, 2)


def pool_guidance_bwd(dy: torch.Tensor, in_size) -> torch.Tensor:
    """Adjoint of ``pool_guidance`` (``naf_pool_guidance_bwd``): dy logical [B, C, Ho, Wo] (any dtype / strides; cast or copied to dense
    channels-last bf16 only when it is not that already) -> dx, a logical [B, C, H, W] view of a dense channels-last bf16 buffer.
    Gather form, no atomics: bit-reproducible."""
    _gpu(dy, "dy")
    B, Cc, Ho, Wo = dy.shape
    H, W = int(in_size[0]), int(in_size[1])
    if Cc % 8:
        raise ValueError("pool_guidance_bwd: needs C % 8 == 0")
    dc = dy.permute(0, 2, 3, 1)
    if dy.dtype != torch.bfloat16 or not dc.is_contiguous():
        dc = dc.to(torch.bfloat16).contiguous()
    dx = torch.empty((B, H, W, Cc), dtype=torch.bfloat16, device=dy.device)
    lib = _lib.load()
    with torch.cuda.device(dy.device), _Timed("pool_guidance_bwd"):
        rc = lib.naf_pool_guidance_bwd(dx.data_ptr(), dc.data_ptr(), B, H, W, Ho, Wo, Cc, _stream(dy))
    _lib.check(rc, "naf_pool_guidance_bwd")
    return dx.permute(0, 3, 1, 2)


class PoolGuidanceFunction(torch.autograd.Function):
    """Differentiable ``pool_guidance``: forward = naf_pool_guidance, backward = naf_pool_guidance_bwd.  x: logical [B, C, H, W] bf16,
    channels-last; the gradient comes back in the same layout."""

    @staticmethod
    def forward(ctx, x, output_size):
        ctx.size = tuple(x.shape[-2:])
        return _pool_guidance(x, output_size)

    @staticmethod
    def backward(ctx, dy):
        return pool_guidance_bwd(dy, ctx.size), None


def pool_guidance(x: torch.Tensor, output_size) -> torch.Tensor:
    """adaptive_avg_pool2d of the bf16 channels-last guidance [B, C, H, W] (logical) to ``output_size`` (naf.py:34);
    returns a logical [B, C, Ho, Wo] view of a dense channels-last buffer.  Differentiable (``PoolGuidanceFunction``) when autograd is on
    and ``x`` requires grad."""
    if torch.is_grad_enabled() and x.requires_grad:
        _gpu(x, "x")
        return PoolGuidanceFunction.apply(x, output_size)
    return _pool_guidance(x, output_size)


def pack_values(v: torch.Tensor) -> torch.Tensor:
    """[B, C, h, w] (bf16/fp32, any strides) -> dense channels-last bf16 [B, h, w, C]; float16 -> float16, an exact copy."""
    _gpu(v, "lr_features")
    lib = _lib.load()
    if v.dtype not in _DT_VALUES:
        v = v.float()
    B, Cc, h, w = v.shape
    vp = torch.empty((B, h, w, Cc), dtype=torch.float16 if v.dtype == torch.float16 else torch.bfloat16, device=v.device)
    st = _strides4(v, (0, 1, 2, 3))
    with torch.cuda.device(v.device):
        rc = lib.naf_pack_values(vp.data_ptr(), v.data_ptr(), _DT_VALUES[v.dtype], B, Cc, h, w, st, _stream(v))
    _lib.check(rc, "naf_pack_values")
    return vp


# ---- what every attention entry asks of its arguments; ``who`` names the entry in the messages -----------------------------------------
def _rope_table_ptrs(who: str, rope_tables, Ho: int, Wo: int, Dq: int, whole_pairs: bool = False):
    """The two pointers of a ``rope_tables`` pair after checking it against the queries' [.., Ho, Wo, Dq]; ``whole_pairs`` also refuses
    Dq % 4 (the point kernel rotates whole (y, x) pairs itself)."""
    ty, tx = rope_tables
    if (whole_pairs and Dq % 4) or ty.dtype != torch.float32 or tx.dtype != torch.float32 or tuple(ty.shape) != (Ho, 2, Dq // 4) \
            or tuple(tx.shape) != (Wo, 2, Dq // 4) or not (ty.is_contiguous() and tx.is_contiguous()):
        raise ValueError(f"{who}: rope_tables must be the fp32 [Ho,2,Dq/4] / [Wo,2,Dq/4] pair from ops.rope_tables")
    return ty.data_ptr(), tx.data_ptr()


def _check_operands(who: str, operands, *, gpu: bool = True, shape_first: bool = False) -> None:
    """The 5-D operand checks: ``operands`` is (tensor, name, dtypes) triples, ``dtypes`` one of ``_BF16`` / ``_BF16_F16`` below (the
    dtypes the entry reads there and their wording in the message) or None for any.  Per operand, in this order: a ROCm device
    (``gpu``), the dtype (TypeError), 5-D with the last dim contiguous (ValueError) -- ``shape_first`` puts the last in front of the
    dtype, as ``xna_points`` has it."""
    for t, n, dtypes in operands:
        if gpu:
            _gpu(t, n)
        shape_ok = isinstance(t, torch.Tensor) and t.dim() == 5 and t.stride(4) == 1
        if dtypes is not None and (shape_ok or not shape_first) and t.dtype not in dtypes[0]:
            raise TypeError(f"{who}: {n} must be {dtypes[1]}, got {t.dtype}")
        if not shape_ok:
            raise ValueError(f"{who}: {n} must be 5-D [B, heads, H, W, D] with D contiguous")


_BF16 = ((torch.bfloat16,), "bfloat16")
_BF16_F16 = ((torch.bfloat16, torch.float16), "bfloat16 or float16")


def _dense5(H: int, W: int, heads: int, D: int) -> I64x4:
    """Strides of [B, heads, H, W, D] as a view of a dense channels-last [B, H, W, heads * D] buffer: what a shape query assumes."""
    return I64x4(H * W * heads * D, D, W * heads * D, heads * D)


def _fill_geometry(a, q, k, h: int, w: int, ky: int, kx: int, scale) -> None:
    """Geometry, ``scale`` and the q / k strides of any of the attention descriptors (they share these fields).  ``k`` None: a shape
    query without keys, the caller sets ``k_stride``."""
    a.B, a.heads, a.Ho, a.Wo, a.Dq = q.shape
    a.h, a.w, a.ky, a.kx = h, w, ky, kx
    a.scale = float(scale) if scale else 0.0
    a.q_stride = _strides4(q, (0, 1, 2, 3))
    if k is not None:
        a.k_stride = _strides4(k, (0, 1, 2, 3))


def _fill_xna(q, k, v, out, logits, idx_y, idx_x, ky, kx, path, scale, rope_tables=None) -> XnaArgs:
    _, _, h, w, Dv = v.shape
    a = XnaArgs()
    a.q, a.k_lr, a.v_lr, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.logits = logits.data_ptr() if logits is not None else None
    a.idx_y = idx_y.data_ptr() if idx_y is not None else None
    a.idx_x = idx_x.data_ptr() if idx_x is not None else None
    if rope_tables is not None:
        a.rope_tab_y, a.rope_tab_x = _rope_table_ptrs("xna", rope_tables, q.shape[2], q.shape[3], q.shape[4])
    _fill_geometry(a, q, k, h, w, ky, kx, scale)
    a.Dv = Dv
    a.out_dtype = _DT_VALUES[out.dtype]
    a.path = _PATH[path]
    a.v_stride = _strides4(v, (0, 1, 2, 3))
    a.o_stride = _strides4(out, (0, 1, 2, 3))
    return a


def xna_forward(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, kernel_size, *,
                out_dtype: torch.dtype = torch.bfloat16, return_logits: bool = False, path: str = "auto",
                scale: Optional[float] = None, out: Optional[torch.Tensor] = None, rope_tables=None):
    """Cross-scale neighbourhood attention forward.

    ``rope_tables=(tab_y, tab_x)``: ``q`` is the UN-rotated guidance and the kernel applies RoPE while loading
    it (see ``xna_rope_fusable``; raises NafHipError when the shapes do not allow it).

    q [B, heads, Ho, Wo, Dq] bf16, k_lr [B, heads, h, w, Dq] bf16, v_lr [B, heads, h, w, Dv] bf16 --
    5-D strided views with the last dim contiguous.  ``v_lr`` may be float16 together with ``out_dtype=torch.float16``, and only
    together: the values are then read as half, multiplied on the f16 matrix instruction and the output is half (include/naf_hip.h,
    naf_dtype_supported); q, k_lr and the scores stay bf16 / fp32.  Returns ``out`` as a [B, heads, Ho, Wo, Dv] view
    of a dense channels-last [B, Ho, Wo, heads*Dv] buffer (and, with ``return_logits``, the scaled
    pre-softmax scores [B, heads, Ho, Wo, ky*kx] fp32 -- what the reference's return_weights gives).
    ``out``: a caller's buffer to write instead, any strides with Dv contiguous; checked before anything is launched -- ValueError unless
    it is on q's device and has exactly the shape [B, heads, Ho, Wo, Dv].
    """
    if out is not None and q.dim() == 5 and v_lr.dim() == 5:
        # the kernel writes through `out`'s pointer and strides with q's and v_lr's sizes: anything else would be written out of bounds
        want = (*q.shape[:4], v_lr.shape[4])
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != want or out.stride(4) != 1 or out.device != q.device:
            raise ValueError(f"xna_forward: out must be a [B, heads, Ho, Wo, Dv] = {want} buffer on q's device ({q.device}) with Dv contiguous, got "
                             + (f"shape {tuple(out.shape)}, strides {tuple(out.stride())} on {out.device}" if isinstance(out, torch.Tensor) else type(out).__name__))
    half = v_lr.dtype == torch.float16 or out_dtype == torch.float16 or (out is not None and out.dtype == torch.float16)
    _check_operands("xna_forward", ((q, "q", _BF16), (k_lr, "k_lr", _BF16), (v_lr, "v_lr", None if half else _BF16)))
    if half and not (v_lr.dtype == torch.float16 and out_dtype == torch.float16 and (out is None or out.dtype == torch.float16)):
        raise TypeError(f"xna_forward: float16 values go with out_dtype=torch.float16 and only with it "
                        f"(v_lr {v_lr.dtype}, out_dtype {out_dtype}{'' if out is None else f', out {out.dtype}'})")
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, Dq = q.shape
    _, _, h, w, Dv = v_lr.shape
    if k_lr.shape != (B, heads, h, w, Dq):
        raise ValueError(f"xna_forward: k_lr shape {tuple(k_lr.shape)} does not match q/v")
    if out_dtype not in _DT_VALUES:
        raise TypeError(f"xna_forward: out_dtype {out_dtype} not supported (bfloat16 / float32, float16 with float16 values)")
    dev = q.device
    if out is None:
        out = torch.empty((B, Ho, Wo, heads, Dv), dtype=out_dtype, device=dev).permute(0, 3, 1, 2, 4)
    logits = torch.empty((B, heads, Ho, Wo, ky * kx), dtype=torch.float32, device=dev) if return_logits else None
    a = _fill_xna(q, k_lr, v_lr, out, logits, None, None, ky, kx, path, scale, rope_tables)
    sel = lib.naf_xna_select(C.byref(a))
    if sel < 0:
        _lib.check(-sel, "naf_xna_select")
    if sel != _lib.XNA_MFMA:   # the table-driven kernels (MFMA "union" and generic) read the canonical index tables
        iy = device_index_table(Ho, h, ky, dev)
        ix = device_index_table(Wo, w, kx, dev)
        a.idx_y, a.idx_x = iy.data_ptr(), ix.data_ptr()
    with torch.cuda.device(dev), _Timed("xna_" + _PATH_NAME[sel]):
        rc = lib.naf_xna_fwd(C.byref(a), _stream(q))
    _lib.check(rc, "naf_xna_fwd")
    return (out, logits) if return_logits else out


def xna_points(q: torch.Tensor, k_lr: torch.Tensor, v_lr: Optional[torch.Tensor], points: torch.Tensor, kernel_size, *,
               want_logits: bool = True, want_probs: bool = False, scale: Optional[float] = None, rope_tables=None,
               logits: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """The attention of ``xna_forward`` at N query pixels (naf_xna_points): ``points`` int32 [N, 3] of (b, y, x) in output coordinates on q's
    device.  Returns ``(out, logits, probs)``: ``out`` [N, heads * Dv] fp32 feature vectors (None when ``v_lr`` is None: weights only),
    ``logits`` [N, heads, ky*kx] fp32 scaled pre-softmax scores (the rows of ``xna_forward(..., return_logits=True)``'s second result; None
    unless ``want_logits``), ``probs`` their softmax (None unless ``want_probs``).  No dense [B, heads, Ho, Wo, .] tensor is formed.

    q / k_lr / v_lr as ``xna_forward``'s (5-D strided views, last dim contiguous, any strides incl. 0); v_lr bf16 or float16.
    ``rope_tables=(tab_y, tab_x)``: q is the UN-rotated guidance and the kernel rotates the N * heads vectors it reads -- the same bits as
    rotated queries, for every geometry (unlike ``xna_forward``'s rotate-on-load).  Scores and features are bit-identical to the pixel of
    ``xna_forward(..., path="generic", out_dtype=torch.float32, return_logits=True)``.  A point outside [0, B) x [0, Ho) x [0, Wo) gets NaN
    rows; nothing is read for it.  ``logits`` / ``probs`` / ``out``: a caller's dense fp32 buffers of exactly those shapes to write instead
    (giving one asks for that output).  N = 0 launches nothing."""
    who = "xna_points"
    _check_operands(who, ((q, "q", _BF16), (k_lr, "k_lr", _BF16)) + (((v_lr, "v_lr", _BF16_F16),) if v_lr is not None else ()),
                    gpu=False, shape_first=True)
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, Dq = q.shape
    h, w = int(k_lr.shape[2]), int(k_lr.shape[3])
    if tuple(k_lr.shape) != (B, heads, h, w, Dq):
        raise ValueError(f"{who}: k_lr shape {tuple(k_lr.shape)} does not match q {tuple(q.shape)}")
    Dv = 0
    if v_lr is not None:
        Dv = int(v_lr.shape[4])
        if tuple(v_lr.shape) != (B, heads, h, w, Dv):
            raise ValueError(f"{who}: v_lr shape {tuple(v_lr.shape)} does not match k_lr {tuple(k_lr.shape)}")
    elif out is not None:
        raise ValueError(f"{who}: `out` needs the values v_lr")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be [N, 3] of (b, y, x), got "
                         + (f"{tuple(points.shape)}" if isinstance(points, torch.Tensor) else type(points).__name__))
    if points.dtype != torch.int32:
        raise TypeError(f"{who}: points must be int32, got {points.dtype}")
    N = int(points.shape[0])
    want_logits, want_probs = bool(want_logits) or logits is not None, bool(want_probs) or probs is not None
    if not (want_logits or want_probs or v_lr is not None):
        raise ValueError(f"{who}: nothing to compute: no values and neither logits nor probs asked for")
    for buf, n, shape in ((logits, "logits", (N, heads, ky * kx)), (probs, "probs", (N, heads, ky * kx)), (out, "out", (N, heads * Dv))):
        if buf is not None and (not isinstance(buf, torch.Tensor) or buf.dtype != torch.float32 or tuple(buf.shape) != shape
                                or not buf.is_contiguous() or buf.device != q.device):
            raise ValueError(f"{who}: {n} must be a dense float32 {shape} buffer on q's device")
    rope_ptrs = None if rope_tables is None else _rope_table_ptrs(who, rope_tables, Ho, Wo, Dq, whole_pairs=True)
    for t, n in ((q, "q"), (k_lr, "k_lr"), (points, "points")) + (((v_lr, "v_lr"),) if v_lr is not None else ()):
        _gpu(t, n)
        if t.device != q.device:
            raise ValueError(f"{who}: {n} is on {t.device}, q on {q.device}")
    lib = _lib.load()
    dev = q.device
    points = points.contiguous()
    if logits is None and want_logits:
        logits = torch.empty((N, heads, ky * kx), dtype=torch.float32, device=dev)
    if probs is None and want_probs:
        probs = torch.empty((N, heads, ky * kx), dtype=torch.float32, device=dev)
    if out is None and v_lr is not None:
        out = torch.empty((N, heads * Dv), dtype=torch.float32, device=dev)
    if N == 0:
        return out, logits, probs
    iy = device_index_table(Ho, h, ky, dev)
    ix = device_index_table(Wo, w, kx, dev)
    a = _lib.XnaPointsArgs()
    a.q, a.k_lr, a.v_lr, a.points = q.data_ptr(), k_lr.data_ptr(), (v_lr.data_ptr() if v_lr is not None else None), points.data_ptr()
    a.idx_y, a.idx_x = iy.data_ptr(), ix.data_ptr()
    if rope_ptrs is not None:
        a.rope_tab_y, a.rope_tab_x = rope_ptrs
    a.logits = logits.data_ptr() if logits is not None else None
    a.probs = probs.data_ptr() if probs is not None else None
    a.out = out.data_ptr() if out is not None else None
    _fill_geometry(a, q, k_lr, h, w, ky, kx, scale)
    a.N, a.Dv = N, Dv
    a.v_dtype = _DT_VALUES[v_lr.dtype] if v_lr is not None else _lib.NAF_BF16
    if v_lr is not None:
        a.v_stride = _strides4(v_lr, (0, 1, 2, 3))
    with torch.cuda.device(dev), _Timed("xna_points"):
        rc = lib.naf_xna_points(C.byref(a), _stream(q))
    _lib.check(rc, "naf_xna_points")
    return out, logits, probs


def _fill_xna_bwd(q, k, v, dout, dq, dk, dv, ky, kx, scale) -> XnaBwdArgs:
    _, _, h, w, Dv = v.shape
    a = XnaBwdArgs()
    a.q, a.k_lr, a.v_lr, a.dout, a.dq = q.data_ptr(), k.data_ptr(), v.data_ptr(), dout.data_ptr(), dq.data_ptr()
    a.dk_lr, a.dv_lr = dk.data_ptr(), dv.data_ptr()
    _fill_geometry(a, q, k, h, w, ky, kx, scale)
    a.Dv = Dv
    a.v_stride = _strides4(v, (0, 1, 2, 3))
    a.dout_stride, a.dq_stride = _strides4(dout, (0, 1, 2, 3)), _strides4(dq, (0, 1, 2, 3))
    return a


_BWD_PATHS = {"auto": _lib.XNA_AUTO, "mfma": _lib.XNA_MFMA, "rows": _lib.XNA_ROWS, "generic": _lib.XNA_GENERIC}


def _scores_args(dlogits: torch.Tensor, q: torch.Tensor, ky: int, kx: int) -> XnaBwdScoresArgs:
    """naf_xna_bwd_scores_args of a score gradient: fp32 [B, heads, Ho, Wo, ky*kx] with the slot axis contiguous (any other strides)."""
    B, heads, Ho, Wo, _ = q.shape
    if tuple(dlogits.shape) != (B, heads, Ho, Wo, ky * kx):
        raise ValueError(f"xna_backward: dlogits shape {tuple(dlogits.shape)} != {(B, heads, Ho, Wo, ky * kx)}")
    if dlogits.dtype != torch.float32 or dlogits.stride(4) != 1 or dlogits.device != q.device:
        raise TypeError("xna_backward: dlogits must be a float32 tensor on q's device with the slot axis (the last) contiguous")
    s = XnaBwdScoresArgs()
    s.dlogits = dlogits.data_ptr()
    s.dlogits_stride = _strides4(dlogits, (0, 1, 2, 3))
    return s


def _bwd_query_args(q, k_lr, v_lr, kernel_size) -> XnaBwdArgs:
    """naf_xna_bwd_args of a shape / alignment query: nothing is dereferenced, dout and dq are taken as dense channels-last buffers."""
    a = _fill_xna_bwd(q, k_lr, v_lr, q, q, q, q, *_ksize(kernel_size), None)
    B, heads, Ho, Wo, Dq = q.shape
    Dv = v_lr.shape[-1]
    a.dout_stride, a.dq_stride = _dense5(Ho, Wo, heads, Dv), _dense5(Ho, Wo, heads, Dq)
    return a


def _bwd_supported(lib, a: XnaBwdArgs, sa: Optional[XnaBwdScoresArgs]) -> int:
    """The kernel the library picks for ``a`` (with the score gradient ``sa``, or None): the matching ``*_supported`` entry, raising on a refusal."""
    if sa is None:
        sel, entry = lib.naf_xna_bwd_supported(C.byref(a)), "naf_xna_bwd_supported"
    else:
        sel, entry = lib.naf_xna_bwd_scores_supported(C.byref(a), C.byref(sa)), "naf_xna_bwd_scores_supported"
    if sel < 0:
        _lib.check(-sel, entry)
    return sel


def xna_backward_supported(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, kernel_size) -> bool:
    """True when ``xna_backward`` runs the MFMA cell kernel for these shapes (otherwise: the table-driven one)."""
    return _lib.load().naf_xna_bwd_supported(C.byref(_bwd_query_args(q, k_lr, v_lr, kernel_size))) == _lib.XNA_MFMA


def xna_backward_select(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, kernel_size, *, dlogits: Optional[torch.Tensor] = None) -> str:
    """Which kernel ``xna_backward`` runs for these shapes: "mfma" (cell kernel), "rows" (row-streaming matrix-core kernel: the integer ratios
    the cell kernel does not take -- the reference's denoising call, its own training geometry, patch-14 backbones) or "generic" (table-driven scalar kernel).
    ``dlogits``: the score gradient ``xna_backward`` would get (``naf_xna_bwd_scores_supported``: non-integer ratios then run the table-driven kernel)."""
    lib = _lib.load()
    a = _bwd_query_args(q, k_lr, v_lr, kernel_size)
    sa = None if dlogits is None else _scores_args(dlogits, q, a.ky, a.kx)
    return {_lib.XNA_MFMA: "mfma", _lib.XNA_ROWS: "rows"}.get(_bwd_supported(lib, a, sa), "generic")


def xna_backward_chunks(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, kernel_size) -> list:
    """Channel-chunk widths of the launches the cell backward issues for these shapes (``naf_xna_bwd_chunk_plan``): one entry = the
    whole head in one launch, [] = another kernel serves the call.  dQ carries one bf16 rounding per chunk (include/naf_hip.h)."""
    lib = _lib.load()
    a = _bwd_query_args(q, k_lr, v_lr, kernel_size)
    out = (C.c_int32 * 16)()
    n = lib.naf_xna_bwd_chunk_plan(C.byref(a), out, 16)
    if n < 0:
        _lib.check(-n, "naf_xna_bwd_chunk_plan")
    return [int(out[i]) for i in range(min(n, 16))]


def xna_backward(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, dout: torch.Tensor, kernel_size, *,
                 scale: Optional[float] = None, path: str = "auto", dlogits: Optional[torch.Tensor] = None):
    """Gradients of ``xna_forward`` w.r.t. q, k_lr, v_lr given ``dout`` (5-D [B, heads, Ho, Wo, Dv], any strides with
    Dv contiguous; cast to bf16).  Returns (dq bf16 [B,heads,Ho,Wo,Dq] view of a channels-last buffer,
    dk_lr fp32 [B,heads,h,w,Dq] view, dv_lr fp32 [B,heads,h,w,Dv] view).  ``path`` (naf_xna_bwd_args.path): "auto", or insist on "mfma"
    (cell kernels), "rows" (row-streaming matrix-core kernel) or "generic" -- the table-driven scalar kernel, which serves EVERY shape and
    is the independent reference of the parity tests (until 0.4.1 "generic" only withheld the row-streaming kernel's workspace: shapes the
    cell kernels take ran the cell kernel again, and the tests that compared the two compared it with itself).
    ``dlogits`` (C ABI 0.4.3, naf_xna_bwd_scores): the gradient of the scaled scores ``xna_forward(..., return_logits=True)`` returns, fp32
    [B, heads, Ho, Wo, ky*kx] with the slot axis contiguous; it adds scale * dlogits to dS, so it reaches dq and dk_lr (dv_lr does not depend on
    it).  None issues exactly the plain backward."""
    for t, n in ((q, "q"), (k_lr, "k_lr"), (v_lr, "v_lr")):
        _gpu(t, n)
        if t.dtype != torch.bfloat16 or t.dim() != 5 or t.stride(4) != 1:
            raise TypeError(f"xna_backward: {n} must be a bfloat16 5-D [B, heads, H, W, D] view with D contiguous")
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, Dq = q.shape
    _, _, h, w, Dv = v_lr.shape
    if tuple(dout.shape) != (B, heads, Ho, Wo, Dv):
        raise ValueError(f"xna_backward: dout shape {tuple(dout.shape)} != {(B, heads, Ho, Wo, Dv)}")
    if dout.dtype != torch.bfloat16 or dout.stride(4) != 1:
        dout = dout.permute(0, 2, 3, 1, 4).to(torch.bfloat16).contiguous().permute(0, 3, 1, 2, 4)
    dev = q.device
    dq = torch.empty((B, Ho, Wo, heads, Dq), dtype=torch.bfloat16, device=dev).permute(0, 3, 1, 2, 4)
    dk = torch.zeros((B, h, w, heads, Dq), dtype=torch.float32, device=dev)
    dv = torch.zeros((B, h, w, heads, Dv), dtype=torch.float32, device=dev)
    if path not in _BWD_PATHS:
        raise ValueError(f"xna_backward: path must be one of {sorted(_BWD_PATHS)}, got {path!r}")
    a = _fill_xna_bwd(q, k_lr, v_lr, dout, dq, dk, dv, ky, kx, scale)
    a.path = _BWD_PATHS[path]
    sa = None if dlogits is None else _scores_args(dlogits, q, ky, kx)
    sel = _bwd_supported(lib, a, sa)
    if sel in (_lib.XNA_GENERIC, _lib.XNA_ROWS):
        iy = device_index_table(Ho, h, ky, dev)
        ix = device_index_table(Wo, w, kx, dev)
        a.idx_y, a.idx_x = iy.data_ptr(), ix.data_ptr()
    if sel == _lib.XNA_ROWS:    # matrix-core backward of the denoising shapes: per-query softmax statistics live in a workspace
        ws = torch.empty(int(lib.naf_xna_bwd_workspace_bytes(C.byref(a))), dtype=torch.uint8, device=dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    entry = "naf_xna_bwd" if sa is None else "naf_xna_bwd_scores"
    with torch.cuda.device(dev), _Timed("xna_bwd" if sa is None else "xna_bwd_scores"):
        rc = lib.naf_xna_bwd(C.byref(a), _stream(q)) if sa is None else lib.naf_xna_bwd_scores(C.byref(a), C.byref(sa), _stream(q))
    _lib.check(rc, entry)
    return dq, dk.permute(0, 3, 1, 2, 4), dv.permute(0, 3, 1, 2, 4)


def rope_pool_bwd(dq: torch.Tensor, dk: torch.Tensor, tab_y: torch.Tensor, tab_x: torch.Tensor, out_size) -> torch.Tensor:
    """Backward of ``rope_pool``: dq bf16 [B, heads, Ho, Wo, Dh], dk [B, heads, h, w, Dh] (cast to fp32) -> dx, a logical
    [B, heads * Dh, Ho, Wo] view of a channels-last bf16 buffer (``naf_rope_pool_bwd``)."""
    lib = _lib.load()
    _gpu(dq, "dq")
    B, heads, Ho, Wo, Dh = dq.shape
    h, w = dk.shape[2], dk.shape[3]
    if dq.dtype != torch.bfloat16 or dq.stride(4) != 1:
        dq = dq.to(torch.bfloat16).contiguous()
    dk = dk.float()
    if dk.stride(4) != 1:
        dk = dk.contiguous()
    dx = torch.empty((B, Ho, Wo, heads * Dh), dtype=torch.bfloat16, device=dq.device).permute(0, 3, 1, 2)
    a = _lib.RopePoolBwdArgs()
    a.dq, a.dk_lr, a.dx, a.tab_y, a.tab_x = dq.data_ptr(), dk.data_ptr(), dx.data_ptr(), tab_y.data_ptr(), tab_x.data_ptr()
    a.B, a.Cq, a.heads, a.Ho, a.Wo, a.h, a.w = B, heads * Dh, heads, Ho, Wo, h, w
    a.dq_stride = _strides4(dq, (0, 1, 2, 3))
    a.dk_stride = _strides4(dk, (0, 1, 2, 3))
    a.dx_stride = _strides4(dx, (0, 1, 2, 3))
    with torch.cuda.device(dq.device), _Timed("rope_pool_bwd"):
        rc = lib.naf_rope_pool_bwd(C.byref(a), _stream(dq))
    _lib.check(rc, "naf_rope_pool_bwd")
    return dx


class RopePoolFunction(torch.autograd.Function):
    """Differentiable ``rope_pool`` (queries and pooled keys of the guidance): forward = naf_rope_pool_fwd, backward =
    naf_rope_pool_bwd.  x: logical [B, Cq, Ho, Wo] bf16, channels-last."""

    @staticmethod
    def forward(ctx, x, tab_y, tab_x, heads, lr_size):
        q5, k5 = rope_pool(x, tab_y, tab_x, heads, lr_size, q_layout="channels_last")
        ctx.save_for_backward(tab_y, tab_x)
        ctx.size = tuple(x.shape[-2:])
        return q5, k5

    @staticmethod
    def backward(ctx, dq, dk):
        tab_y, tab_x = ctx.saved_tensors
        return rope_pool_bwd(dq, dk, tab_y, tab_x, ctx.size), None, None, None, None


class XnaFunction(torch.autograd.Function):
    """Differentiable ``xna_forward``: forward = naf_xna_fwd, backward = naf_xna_bwd (MFMA or table-driven kernels).  Optional seventh
    argument: True = also return the scaled scores, without a gradient; "differentiable" = also return them as a differentiable output, whose
    gradient the backward hands to naf_xna_bwd_scores (it reaches q and k_lr)."""

    @staticmethod
    def forward(ctx, q, k_lr, v_lr, kernel_size, scale, out_dtype, *rest):
        mode = rest[0] if rest else False
        return_logits = mode == "differentiable" or (not isinstance(mode, str) and bool(mode))
        ctx.nrest = len(rest)
        ctx.differentiable = mode == "differentiable"
        # an unused output's gradient arrives as None instead of zeros: a loss on `out` alone runs the plain backward, one on the scores
        # alone a zero dout
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, k_lr, v_lr)
        ctx.kernel_size, ctx.scale = kernel_size, scale
        if return_logits:
            # return_weights on a gradient-enabled call (attentions.py:64-67 works under autograd): the scaled pre-softmax scores of the
            # very q / k this differentiable step uses.  True: WITHOUT a gradient (notebooks/attention_maps.ipynb reads them for display);
            # "differentiable": with one, as legacy_attention's scores have (attentions.py:16-29) -- losses on the attention maps
            out, logits = xna_forward(q, k_lr, v_lr, kernel_size, out_dtype=out_dtype, path="auto", scale=scale, return_logits=True)
            if not ctx.differentiable:
                ctx.mark_non_differentiable(logits)
            return out, logits
        return xna_forward(q, k_lr, v_lr, kernel_size, out_dtype=out_dtype, path="auto", scale=scale)

    @staticmethod
    def backward(ctx, dout, *rest):
        if not any(ctx.needs_input_grad[:3]):
            return (None,) * (6 + ctx.nrest)
        q, k_lr, v_lr = ctx.saved_tensors
        dlogits = rest[0] if ctx.differentiable and rest else None
        if dout is None and dlogits is None:
            return (None,) * (6 + ctx.nrest)
        if dout is None:
            B, heads, Ho, Wo, _ = q.shape
            dout = torch.zeros((B, heads, Ho, Wo, v_lr.shape[-1]), dtype=torch.bfloat16, device=q.device)
        if dlogits is not None and dlogits.stride(-1) != 1:   # any other strides (0 where a loss reduced over an axis) serve as they are
            dlogits = dlogits.contiguous()
        dq, dk, dv = xna_backward(q, k_lr, v_lr, dout, ctx.kernel_size, scale=ctx.scale,
                                  dlogits=None if dlogits is None else dlogits.float())
        need = ctx.needs_input_grad
        return ((dq if need[0] else None), (dk.to(k_lr.dtype) if need[1] else None), (dv.to(v_lr.dtype) if need[2] else None),
                None, None, None) + (None,) * ctx.nrest


# ---- attention forward with the training objective in its epilogue ---------------------------------
def _check_regress_target(who: str, target, shape, device) -> None:
    """Host-side checks of a regression target against the prediction's [B, C, Ho, Wo] (nothing touches the device)."""
    if not isinstance(target, torch.Tensor):
        raise TypeError(f"{who}: the target must be a tensor, got {type(target).__name__}")
    if target.dtype not in _DT:
        raise TypeError(f"{who}: the target must be float32 or bfloat16, got {target.dtype}")
    if tuple(target.shape) != tuple(shape):
        raise ValueError(f"{who}: target shape {tuple(target.shape)} != prediction shape {tuple(shape)}")
    if target.requires_grad:
        raise ValueError(f"{who}: the target gets no gradient; detach it")
    if target.device != device:
        raise ValueError(f"{who}: the target is on {target.device}, the features on {device}")


def _check_mse_operands(who: str, q, k_lr, v_lr, target) -> None:
    _check_operands(who, ((q, "q", _BF16), (k_lr, "k_lr", _BF16), (v_lr, "v_lr", _BF16)), gpu=False)
    B, heads, Ho, Wo, Dq = q.shape
    _, _, h, w, Dv = v_lr.shape
    if tuple(k_lr.shape) != (B, heads, h, w, Dq) or v_lr.shape[:2] != (B, heads):
        raise ValueError(f"{who}: k_lr shape {tuple(k_lr.shape)} / v_lr shape {tuple(v_lr.shape)} do not match q {tuple(q.shape)}")
    _check_regress_target(who, target, (B, heads * Dv, Ho, Wo), q.device)


def _fill_xna_mse(q, k_lr, v_lr, target, dout, ky, kx, scale) -> "_lib.XnaMSEArgs":
    B, heads, Ho, Wo, _ = q.shape
    Dv = v_lr.shape[-1]
    m = _lib.XnaMSEArgs()
    m.a = _fill_xna(q, k_lr, v_lr, dout if dout is not None else q, None, None, None, ky, kx, "union", scale)
    m.a.out_dtype = _lib.NAF_BF16
    if dout is None:
        m.a.out = None
        m.a.o_stride = _dense5(Ho, Wo, heads, Dv)
    m.target, m.target_dtype = target.data_ptr(), _DT[target.dtype]
    m.target_stride = _strides4(target, (0, 1, 2, 3))
    return m


def xna_mse_supported(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, target: torch.Tensor, kernel_size) -> bool:
    """True when ``xna_mse_forward`` serves these operands (``naf_xna_mse_supported``: the table-driven MFMA kernel's shapes -- Dq = 64,
    Dv % 16 == 0, square odd window 3 .. 15, any ratio >= 1).  Operands of the wrong kind raise as they do there."""
    _check_mse_operands("xna_mse_supported", q, k_lr, v_lr, target)
    ky, kx = _ksize(kernel_size)
    return _lib.load().naf_xna_mse_supported(C.byref(_fill_xna_mse(q, k_lr, v_lr, target, None, ky, kx, None))) == 1


def xna_mse_forward(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, target: torch.Tensor, kernel_size, *,
                    scale: Optional[float] = None, grad: bool = True, out: Optional[torch.Tensor] = None):
    """The training objective of the reference's step (train.py:127-132) from the attention kernel's epilogue:
    ``loss = F.mse_loss(xna_forward(q, k_lr, v_lr).float(), target.float())`` as a 0-dim fp32 tensor, and with ``grad`` its gradient with
    respect to the attention output, ``dout5`` -- a [B, heads, Ho, Wo, Dv] bf16 view of a [B, Ho, Wo, C] buffer that ``xna_backward``
    takes as it is.  The prediction is never written: the kernel subtracts the target from its fp32 accumulators, so ``dout5`` carries
    one bf16 rounding (of (out - target) * 2/N) instead of the two of the composed step.  ``grad=False``: loss only, nothing else is
    written (validation; ``out`` together with ``grad=False`` raises ValueError).  ``target``: float32 / bfloat16, logical [B, heads * Dv, Ho, Wo], any strides (channels-last views are read
    with vector loads).  ``out``: an existing [B, heads, Ho, Wo, Dv] bf16 buffer for ``dout5`` (Dv contiguous).  Two calls on the same
    operands are bit-equal.  Raises NafHipError where ``xna_mse_supported`` says no (no fallback here)."""
    who = "xna_mse_forward"
    _check_mse_operands(who, q, k_lr, v_lr, target)
    if out is not None and not grad:
        raise ValueError(f"{who}: out is the gradient's buffer; with grad=False nothing is written")
    for t, n in ((q, "q"), (k_lr, "k_lr"), (v_lr, "v_lr"), (target, "target")):
        _gpu(t, n)
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, Dq = q.shape
    _, _, h, w, Dv = v_lr.shape
    dev = q.device
    dout = None
    if grad:
        dout = out if out is not None else torch.empty((B, Ho, Wo, heads, Dv), dtype=torch.bfloat16, device=dev).permute(0, 3, 1, 2, 4)
        if tuple(dout.shape) != (B, heads, Ho, Wo, Dv) or dout.dtype != torch.bfloat16 or dout.stride(4) != 1 or dout.device != dev:
            raise ValueError(f"{who}: out must be a bfloat16 [B, heads, Ho, Wo, Dv] buffer on q's device with Dv contiguous")
    m = _fill_xna_mse(q, k_lr, v_lr, target, dout, ky, kx, scale)
    ok = lib.naf_xna_mse_supported(C.byref(m))
    if ok != 1:
        _lib.check(-ok, "naf_xna_mse_supported")
    iy = device_index_table(Ho, h, ky, dev)
    ix = device_index_table(Wo, w, kx, dev)
    m.a.idx_y, m.a.idx_x = iy.data_ptr(), ix.data_ptr()
    ws = torch.empty(int(lib.naf_xna_mse_workspace_bytes(C.byref(m))), dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    m.workspace, m.workspace_bytes, m.loss = ws.data_ptr(), ws.numel(), loss.data_ptr()
    with torch.cuda.device(dev), _Timed("xna_union_mse"):
        rc = lib.naf_xna_mse_fwd(C.byref(m), _stream(q))
    _lib.check(rc, "naf_xna_mse_fwd")
    return loss, dout


def xna_mse_auto(B: int, heads: int, Dq: int, Dv: int, lr_size, out_size, kernel_size, out_dtype, target: torch.Tensor) -> bool:
    """The rule of ``naf(..., regress=..., regress_path="auto")``, from shapes alone (nothing is dereferenced): True where
    ``naf_xna_select`` runs the table-driven MFMA kernel for the plain forward of these shapes (dense channels-last operands) -- the
    fused objective is then the same kernel with another epilogue -- and ``naf_xna_mse_supported`` takes the target."""
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    h, w = int(lr_size[0]), int(lr_size[1])
    Ho, Wo = int(out_size[0]), int(out_size[1])
    if out_dtype not in _DT or target.dtype not in _DT:
        return False
    m = _lib.XnaMSEArgs()
    a = m.a
    a.q = a.k_lr = a.v_lr = a.out = 4096               # shape / alignment query only
    a.B, a.heads, a.Ho, a.Wo, a.h, a.w, a.Dq, a.Dv, a.ky, a.kx = B, heads, Ho, Wo, h, w, Dq, Dv, ky, kx
    a.out_dtype, a.path, a.scale = _DT[out_dtype], _lib.XNA_AUTO, 0.0
    a.q_stride, a.k_stride = _dense5(Ho, Wo, heads, Dq), _dense5(h, w, heads, Dq)
    a.v_stride, a.o_stride = _dense5(h, w, heads, Dv), _dense5(Ho, Wo, heads, Dv)
    if lib.naf_xna_select(C.byref(a)) != _lib.XNA_UNION:
        return False
    a.out_dtype = _lib.NAF_BF16
    m.target, m.target_dtype = target.data_ptr() or 4096, _DT[target.dtype]
    m.target_stride = _strides4(target, (0, 1, 2, 3))
    return lib.naf_xna_mse_supported(C.byref(m)) == 1


class XnaMSEFunction(torch.autograd.Function):
    """``loss = mse(xna(q, k_lr, v_lr), target)`` as one differentiable node: forward = naf_xna_mse_fwd (the attention launch and the
    one-workgroup sum), which leaves the loss's gradient with respect to the attention output in bf16; backward = naf_xna_bwd on that
    buffer as it stands, its three results scaled by the incoming scalar on the device (no host synchronisation; they are smaller than
    dout).  The target gets no gradient."""

    @staticmethod
    def forward(ctx, q, k_lr, v_lr, target, kernel_size, scale):
        loss, dout5 = xna_mse_forward(q, k_lr, v_lr, target, kernel_size, scale=scale, grad=True)
        ctx.save_for_backward(q, k_lr, v_lr, dout5)
        ctx.kernel_size, ctx.scale = kernel_size, scale
        return loss

    @staticmethod
    def backward(ctx, dloss):
        if not any(ctx.needs_input_grad[:3]):
            return (None,) * 6
        q, k_lr, v_lr, dout5 = ctx.saved_tensors
        dq, dk, dv = xna_backward(q, k_lr, v_lr, dout5, ctx.kernel_size, scale=ctx.scale)
        g = dloss.detach().to(torch.float32).reshape(())
        need = ctx.needs_input_grad
        return ((dq.mul_(g) if need[0] else None), (dk.mul_(g).to(k_lr.dtype) if need[1] else None),
                (dv.mul_(g).to(v_lr.dtype) if need[2] else None), None, None, None)


# ---- attention with a linear head folded in ------------------------------------------------------
_HEAD_PATHS = ("auto", "fused", "composed")
_BWD_DV = (32, 64, 96, 128, 192, 256)      # value widths the cell backward serves (naf_xna_bwd)


def head_npad(n_out: int) -> int:
    """Channels of a ``pv5`` row for ``n_out`` head outputs: rounded up to the 16 of an MFMA tile."""
    return (int(n_out) + 15) // 16 * 16


def project_head_values(weight: torch.Tensor, bias: Optional[torch.Tensor], features: torch.Tensor, heads: int, *,
                        dtype: torch.dtype = torch.bfloat16):
    """The low-res half of ``head(naf(features))`` for a linear head: ``PV_g = W[:, g*Dv:(g+1)*Dv] @ V_g`` per attention head ``g``.

    weight [N, C] or [N, C, 1, 1], bias [N] or None, features [B, C, h, w] -> (pv5 [B, heads, h, w, Npad] ``dtype`` with Npad = N rounded
    up to 16 and zero pad channels, bias as fp32 or None).  Pure torch, differentiable (this is where a trainable head's gradient enters
    autograd), works on CPU tensors: an einsum on the low-res grid is host glue, not a hot path."""
    if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight[:, :, 0, 0]
    if weight.dim() != 2:
        raise ValueError(f"project_head_values: weight must be [N, C] or [N, C, 1, 1], got {tuple(weight.shape)}")
    if features.dim() != 4:
        raise ValueError(f"project_head_values: features must be [B, C, h, w], got {tuple(features.shape)}")
    N, Cw = weight.shape
    B, Cc, h, w = features.shape
    if Cw != Cc:
        raise ValueError(f"project_head_values: the head reads {Cw} channels, the features have {Cc}")
    if heads <= 0 or Cc % heads:
        raise ValueError(f"project_head_values: feature channels {Cc} not divisible by {heads} heads")
    if bias is not None and tuple(bias.shape) != (N,):
        raise ValueError(f"project_head_values: bias must be [{N}], got {tuple(bias.shape)}")
    Dv = Cc // heads
    pv = torch.einsum("ngd,bgdhw->bghwn", weight.float().reshape(N, heads, Dv), features.float().reshape(B, heads, Dv, h, w))
    pad = head_npad(N) - N
    if pad:
        pv = torch.nn.functional.pad(pv, (0, pad))
    return pv.to(dtype), (None if bias is None else bias.float())


def _fill_xna_head(q, k, pv, bias, out, n_out, ky, kx, path, scale, rope_tables=None) -> XnaHeadArgs:
    B, heads, Ho, Wo, Dq = q.shape
    h, w = pv.shape[2:4]
    a = XnaHeadArgs()
    a.q, a.k_lr, a.pv_lr, a.out = q.data_ptr(), k.data_ptr(), pv.data_ptr(), out.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    if rope_tables is not None:
        a.rope_tab_y, a.rope_tab_x = _rope_table_ptrs("xna_head", rope_tables, Ho, Wo, Dq)
    _fill_geometry(a, q, k, h, w, ky, kx, scale)
    a.N = int(n_out)
    a.out_dtype = _DT[out.dtype]
    a.path = _lib.XNA_HEAD_FUSED if path == "fused" else _lib.XNA_HEAD_AUTO
    a.pv_stride = _strides4(pv, (0, 1, 2, 3))
    a.o_stride = _strides3(out)
    return a


def _head_route(a, entry: str, q, lr_size, n_out: int, kernel_size, rope_tables, Dv: Optional[int] = None, outer=None) -> str:
    """The answer of ``naf_xna_head_select`` / ``naf_xna_cos_select`` (``entry``) to a shape / alignment query: fills the fresh descriptor
    ``a`` for queries ``q`` with dense channels-last keys, projected values, (``Dv``: the cosine head's) values and output.  ``outer``: the
    struct ``a`` is the first member of, where the entry takes that one (``naf_xna_cos_ce_select``)."""
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    _, heads, Ho, Wo, Dq = q.shape
    h, w = int(lr_size[0]), int(lr_size[1])
    npad, n_out = head_npad(n_out), int(n_out)
    a.q = a.k_lr = a.pv_lr = a.out = ptr = q.data_ptr() or 16      # shape / alignment query only: nothing is dereferenced
    if rope_tables is not None:
        a.rope_tab_y, a.rope_tab_x = rope_tables[0].data_ptr(), rope_tables[1].data_ptr()
    _fill_geometry(a, q, None, h, w, ky, kx, None)
    a.N, a.path = n_out, _lib.XNA_HEAD_AUTO
    a.k_stride = _dense5(h, w, heads, Dq)
    a.pv_stride = I64x4(heads * h * w * npad, h * w * npad, w * npad, npad)
    a.o_stride = I64x3(Ho * Wo * n_out, Wo * n_out, n_out)
    if Dv is not None:
        a.v_lr, a.Dv, a.logit_scale, a.v_stride = ptr, Dv, 1.0, _dense5(h, w, heads, Dv)
    sel = getattr(lib, entry)(C.byref(a if outer is None else outer))
    if sel == -1:
        _lib.check(1, entry)
    return "fused" if sel == _lib.XNA_HEAD_FUSED else "composed"


def xna_head_select(q: torch.Tensor, lr_size, n_out: int, kernel_size, *, out_dtype: torch.dtype = torch.float32, rope_tables=None) -> str:
    """Which route ``xna_head_forward(path="auto")`` takes for these shapes: "fused" (``naf_xna_head_select`` grants the head-summed kernel)
    or "composed" (``xna_forward`` on the projected values, summed over the heads).  ``q``: the 5-D [B, heads, Ho, Wo, Dq] bf16 queries --
    with ``rope_tables`` the un-rotated guidance.  A host-side query: nothing is launched or read.  Invalid arguments raise ValueError."""
    if q.dtype != torch.bfloat16 or q.dim() != 5 or q.stride(4) != 1 or out_dtype not in _DT or not 1 <= int(n_out) <= 256:
        return "composed"
    a = XnaHeadArgs()
    a.out_dtype = _DT[out_dtype]
    return _head_route(a, "naf_xna_head_select", q, lr_size, n_out, kernel_size, rope_tables)


def _check_head_operands(who: str, q, k_lr, pv_lr, bias, kernel_size, n_out, path):
    """What ``xna_head_forward`` and ``xna_head_objective`` ask of their operands; ``who`` names the caller in the messages.
    Returns (ky, kx, B, heads, Ho, Wo, Dq, h, w, npad, n_out)."""
    _check_operands(who, ((q, "q", _BF16), (k_lr, "k_lr", _BF16), (pv_lr, "pv_lr", _BF16)))
    if path not in _HEAD_PATHS:
        raise ValueError(f"{who}: path must be one of {_HEAD_PATHS}, got {path!r}")
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, Dq = q.shape
    h, w, npad = pv_lr.shape[2:]
    n_out = int(n_out)
    if k_lr.shape != (B, heads, h, w, Dq) or pv_lr.shape[:2] != (B, heads):
        raise ValueError(f"{who}: k_lr {tuple(k_lr.shape)} / pv_lr {tuple(pv_lr.shape)} do not match q {tuple(q.shape)}")
    if n_out < 1 or npad != head_npad(n_out):
        raise ValueError(f"{who}: pv_lr holds {npad} channels, n_out = {n_out} needs {head_npad(max(n_out, 1))}")
    if bias is not None:
        _gpu(bias, "bias")
        if bias.dtype != torch.float32 or tuple(bias.shape) != (n_out,) or not bias.is_contiguous():
            raise ValueError(f"{who}: bias must be a contiguous float32 [{n_out}] tensor")
    return ky, kx, B, heads, Ho, Wo, Dq, h, w, npad, n_out


def xna_head_forward(q: torch.Tensor, k_lr: torch.Tensor, pv_lr: torch.Tensor, bias: Optional[torch.Tensor], kernel_size, *,
                     n_out: int, out_dtype: torch.dtype = torch.float32, path: str = "auto", scale: Optional[float] = None,
                     rope_tables=None) -> torch.Tensor:
    """Cross-scale neighbourhood attention with a linear head folded in: ``bias + sum over heads of attention(q, k_lr, pv_lr)``.

    q [B, heads, Ho, Wo, Dq] bf16, k_lr [B, heads, h, w, Dq] bf16, pv_lr [B, heads, h, w, Npad] bf16 from ``project_head_values``
    (5-D strided views, last dim contiguous), bias fp32 [n_out] or None.  Returns the logits as a logical [B, n_out, Ho, Wo] view of a
    dense channels-last [B, Ho, Wo, n_out] buffer of ``out_dtype`` (bfloat16 / float32).
    ``path="auto"``: the head-summed kernel (``naf_xna_head_fwd``) where ``naf_xna_head_select`` grants it, else the composition that
    serves every geometry ``xna_forward`` serves -- ``xna_forward`` on ``pv_lr`` with fp32 output, summed over the head axis, plus bias.
    ``path="fused"`` insists on the kernel and raises where it does not serve the call; ``path="composed"`` insists on the composition.
    ``rope_tables``: as in ``xna_forward`` (q is the un-rotated guidance)."""
    ky, kx, B, heads, Ho, Wo, Dq, h, w, npad, n_out = _check_head_operands("xna_head_forward", q, k_lr, pv_lr, bias, kernel_size, n_out, path)
    if out_dtype not in _DT:
        raise TypeError(f"xna_head_forward: out_dtype {out_dtype} not supported (bfloat16 / float32)")
    lib = _lib.load()
    dev = q.device
    if path != "composed" and (n_out <= 256 or path == "fused"):
        out = torch.empty((B, Ho, Wo, n_out), dtype=out_dtype, device=dev)
        a = _fill_xna_head(q, k_lr, pv_lr, bias, out, n_out, ky, kx, path, scale, rope_tables)
        sel = lib.naf_xna_head_select(C.byref(a))
        if sel == _lib.XNA_HEAD_FUSED:
            with torch.cuda.device(dev), _Timed("xna_head"):
                rc = lib.naf_xna_head_fwd(C.byref(a), _stream(q))
            _lib.check(rc, "naf_xna_head_fwd")
            return out.permute(0, 3, 1, 2)
        if path == "fused" or sel == -1:       # insisted, or arguments no kernel serves
            _lib.check(-sel, "naf_xna_head_select")
        del out
    with _Timed("xna_head_composed"):
        o5 = xna_forward(q, k_lr, pv_lr, (ky, kx), out_dtype=torch.float32, path="auto", scale=scale, rope_tables=rope_tables)
        o = o5.sum(dim=1)[..., :n_out]
        if bias is not None:
            o = o + bias
        return o.to(out_dtype).contiguous().permute(0, 3, 1, 2)


# ---- mask pooling: the attention summed under K masks (region embeddings, prototypes) --------------------------------------------
MASK_POOL_CHUNK = 64          # masks per launch of naf_xna_maskpool_fwd
_MASK_DTYPES = (torch.bool, torch.uint8, torch.bfloat16, torch.float16, torch.float32)
_MASK_REDUCE = ("mean", "sum")


def check_masks(who: str, masks, shape, device) -> None:
    """What every mask-pooling entry asks of ``masks``: a [B, K, Ho, Wo] = ``shape`` tensor (K >= 1; ``shape[1]`` None: any K) of dtype bool, uint8,
    bfloat16, float16 or float32 on ``device`` that carries no gradient.  TypeError / ValueError; nothing touches the device."""
    if not isinstance(masks, torch.Tensor):
        raise TypeError(f"{who}: masks must be a tensor, got {type(masks).__name__}")
    if masks.dtype not in _MASK_DTYPES:
        raise TypeError(f"{who}: masks must be bool, uint8, bfloat16, float16 or float32, got {masks.dtype}")
    want = tuple(shape)
    if masks.dim() != 4 or masks.shape[1] < 1 or any(s is not None and int(m) != int(s) for m, s in zip(masks.shape, want)):
        raise ValueError(f"{who}: masks must be [B, K, Ho, Wo] = ({want[0]}, {'K >= 1' if want[1] is None else want[1]}, {want[2]}, {want[3]}), "
                         f"got {tuple(masks.shape)}")
    if masks.device != device:
        raise ValueError(f"{who}: masks on {masks.device}, the features on {device}")
    if masks.requires_grad:
        raise ValueError(f"{who}: masks carry no gradient (detach them)")


def _mask_operand(masks: torch.Tensor, dx: int) -> Tuple[torch.Tensor, int]:
    """The tensor the kernel reads for ``masks`` and its naf_mask_dtype: bool / uint8 as bytes, bfloat16 as it is, float16 / float32 cast once
    to bfloat16 (a rounding of the mask, documented); a copy where the kernel's vector loads (cells a multiple of 8 pixels wide) would
    not be aligned."""
    if masks.dtype == torch.bool:
        m, dt = masks.view(torch.uint8), _lib.MASK_U8
    elif masks.dtype == torch.uint8:
        m, dt = masks, _lib.MASK_U8
    else:
        m, dt = masks.to(torch.bfloat16), _lib.MASK_BF16
    if m.stride(3) != 1 or (dx % 8 == 0 and (m.data_ptr() % 16 or any(m.stride(i) % 8 for i in range(3)))):
        m = m.contiguous()
    return m, dt


def xna_mask_pool_select(q: torch.Tensor, lr_size, n_masks: int, kernel_size, *, rope_tables=None) -> str:
    """Which route mask pooling takes for these shapes: "fused" (``naf_xna_maskpool_select`` grants the kernel for ``n_masks`` masks per launch,
    at most ``MASK_POOL_CHUNK``) or "composed" (the caller pools the plain forward).  ``q``: the 5-D [B, heads, Ho, Wo, Dq] bf16 queries --
    with ``rope_tables`` the un-rotated guidance.  A host-side query: nothing is launched or read, CPU / meta tensors do.  Invalid
    arguments raise ValueError; the library's reason for "composed" is in ``naf_last_error``."""
    if q.dtype != torch.bfloat16 or q.dim() != 5 or q.stride(4) != 1:
        return "composed"
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    _, heads, Ho, Wo, Dq = q.shape
    h, w = int(lr_size[0]), int(lr_size[1])
    a = _lib.XnaMaskPoolArgs()
    a.q = a.k_lr = a.masks = a.A = a.mass = a.workspace = q.data_ptr() or 16      # shape / alignment query only: nothing is dereferenced
    if rope_tables is not None:
        a.rope_tab_y, a.rope_tab_x = rope_tables[0].data_ptr(), rope_tables[1].data_ptr()
    _fill_geometry(a, q, None, h, w, ky, kx, None)
    a.K, a.path, a.mask_dtype = int(n_masks), _lib.XNA_HEAD_AUTO, _lib.MASK_BF16
    a.k_stride = _dense5(h, w, heads, Dq)
    a.m_stride = I64x4(int(n_masks) * Ho * Wo, Ho * Wo, Wo, 1)
    sel = lib.naf_xna_maskpool_select(C.byref(a))
    if sel == -1:
        _lib.check(1, "naf_xna_maskpool_select")
    return "fused" if sel == _lib.XNA_HEAD_FUSED else "composed"


def xna_mask_pool(q: torch.Tensor, k_lr: torch.Tensor, masks: torch.Tensor, kernel_size, *, scale: Optional[float] = None, rope_tables=None):
    """The attention of ``xna_forward`` summed under K masks, without values (``naf_xna_maskpool_fwd``):

        ``A[b, g, k, j] = sum_px masks[b, k, px] * P_g[px, j]``  fp32 [B, heads, K, h, w],  ``mass[b, k] = masks[b, k].sum()``  fp32 [B, K]

    with ``P_g`` the bf16-rounded softmax weights of head ``g`` -- bit for bit those of ``xna_head_forward``.  q [B, heads, Ho, Wo, Dq] bf16,
    k_lr [B, heads, h, w, Dq] bf16 (5-D strided views, last dim contiguous), masks [B, K, Ho, Wo] bool / uint8 (read as bytes), bfloat16,
    or float16 / float32 (cast once to bfloat16 on the host: a rounding of the mask).  K above ``MASK_POOL_CHUNK`` runs in chunks of at
    most that many masks, concatenated.  No float atomics: two calls give the same bits.  Raises NafHipError where the kernel does not
    serve the geometry (``xna_mask_pool_select``); there is no composed arm at this level.  ``rope_tables``: as in ``xna_forward``."""
    who = "xna_mask_pool"
    _check_operands(who, ((q, "q", _BF16), (k_lr, "k_lr", _BF16)))
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, Dq = q.shape
    h, w = int(k_lr.shape[2]), int(k_lr.shape[3])
    if tuple(k_lr.shape) != (B, heads, h, w, Dq):
        raise ValueError(f"{who}: k_lr shape {tuple(k_lr.shape)} does not match q {tuple(q.shape)}")
    check_masks(who, masks, (B, None, Ho, Wo), q.device)
    lib = _lib.load()
    dev = q.device
    K = int(masks.shape[1])
    A = torch.empty((B, heads, K, h, w), dtype=torch.float32, device=dev)
    mass = torch.empty((B, K), dtype=torch.float32, device=dev)
    if B == 0:
        return A, mass
    rope_ptrs = None if rope_tables is None else _rope_table_ptrs(who, rope_tables, Ho, Wo, Dq)
    ws = None
    for k0 in range(0, K, MASK_POOL_CHUNK):
        kc = min(MASK_POOL_CHUNK, K - k0)
        m, mdt = _mask_operand(masks[:, k0:k0 + kc], Wo // w if w and Wo % w == 0 else 1)
        whole = kc == K
        Ac = A if whole else torch.empty((B, heads, kc, h, w), dtype=torch.float32, device=dev)
        mc = mass if whole else torch.empty((B, kc), dtype=torch.float32, device=dev)
        a = _lib.XnaMaskPoolArgs()
        a.q, a.k_lr, a.masks, a.A, a.mass = q.data_ptr(), k_lr.data_ptr(), m.data_ptr(), Ac.data_ptr(), mc.data_ptr()
        if rope_ptrs is not None:
            a.rope_tab_y, a.rope_tab_x = rope_ptrs
        _fill_geometry(a, q, k_lr, h, w, ky, kx, scale)
        a.K, a.mask_dtype, a.path = kc, mdt, _lib.XNA_HEAD_FUSED
        a.m_stride = _strides4(m, (0, 1, 2, 3))
        need = int(lib.naf_xna_maskpool_workspace_bytes(C.byref(a)))
        if ws is None or ws.numel() < need:
            ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        sel = lib.naf_xna_maskpool_select(C.byref(a))
        if sel != _lib.XNA_HEAD_FUSED:
            _lib.check(-sel, "naf_xna_maskpool_select")
        with torch.cuda.device(dev), _Timed("xna_mask_pool"):
            rc = lib.naf_xna_maskpool_fwd(C.byref(a), _stream(q))
        _lib.check(rc, "naf_xna_maskpool_fwd")
        if not whole:
            A[:, :, k0:k0 + kc] = Ac
            mass[:, k0:k0 + kc] = mc
    return A, mass


def mask_pool_apply(A: torch.Tensor, v_lr: torch.Tensor, mass: Optional[torch.Tensor], reduce: str = "mean") -> torch.Tensor:
    """``pooled[b, k, c] = sum_j A[b, g(c), k, j] * v_lr[b, c, j]`` in fp32 (``naf_maskpool_apply``), divided by ``mass[b, k]`` for
    ``reduce="mean"`` (a mask of zero mass: a row of exact zeros), undivided for ``"sum"``.  A fp32 [B, heads, K, h, w] dense and mass fp32
    [B, K] from ``xna_mask_pool``, v_lr the bf16 feature map [B, C, h, w] (head g owns channels [g*C/heads, (g+1)*C/heads)).  Returns
    fp32 [B, K, C]."""
    who = "mask_pool_apply"
    if reduce not in _MASK_REDUCE:
        raise ValueError(f"{who}: reduce must be one of {_MASK_REDUCE}, got {reduce!r}")
    for t, n in ((A, "A"), (v_lr, "v_lr")) + (((mass, "mass"),) if mass is not None else ()):
        _gpu(t, n)
    if A.dim() != 5 or A.dtype != torch.float32 or not A.is_contiguous():
        raise ValueError(f"{who}: A must be a dense float32 [B, heads, K, h, w] tensor")
    B, heads, K, h, w = A.shape
    if v_lr.dim() != 4 or v_lr.dtype != torch.bfloat16 or v_lr.shape[0] != B or tuple(v_lr.shape[2:]) != (h, w) or v_lr.shape[1] % heads:
        raise ValueError(f"{who}: v_lr must be bfloat16 [B, C, h, w] = ({B}, multiple of {heads}, {h}, {w}), got {tuple(v_lr.shape)} {v_lr.dtype}")
    if reduce == "mean" and (mass is None or mass.dtype != torch.float32 or tuple(mass.shape) != (B, K) or not mass.is_contiguous()):
        raise ValueError(f"{who}: reduce='mean' needs mass as a dense float32 [{B}, {K}] tensor")
    if v_lr.stride(3) != 1 or v_lr.stride(2) != w:
        v_lr = v_lr.contiguous()
    Cc = int(v_lr.shape[1])
    pooled = torch.empty((B, K, Cc), dtype=torch.float32, device=A.device)
    if pooled.numel() == 0:
        return pooled
    lib = _lib.load()
    vs = (C.c_int64 * 2)(int(v_lr.stride(0)), int(v_lr.stride(1)))
    with torch.cuda.device(A.device), _Timed("mask_pool_apply"):
        rc = lib.naf_maskpool_apply(A.data_ptr(), v_lr.data_ptr(), mass.data_ptr() if reduce == "mean" else None, pooled.data_ptr(),
                                    B, heads, K, Cc, h * w, vs, 1 if reduce == "mean" else 0, _stream(A))
    _lib.check(rc, "naf_maskpool_apply")
    return pooled


def mask_pool_from_features(f: torch.Tensor, masks: torch.Tensor, reduce: str = "mean", return_mass: bool = False):
    """Mask pooling as torch ops on a materialised feature map [B, C, Ho, Wo] (any device, CPU included): the composed arm and the
    definition -- ``einsum("bkhw,bchw->bkc", masks.float(), f.float())``, divided by ``mass = masks.float().sum((2, 3))`` for "mean"
    with exact zeros where the mass is zero."""
    if reduce not in _MASK_REDUCE:
        raise ValueError(f"mask pooling: mask_reduce must be one of {_MASK_REDUCE}, got {reduce!r}")
    m = masks.float()
    pooled = torch.einsum("bkhw,bchw->bkc", m, f.float())
    mass = m.sum(dim=(2, 3))
    if reduce == "mean":
        live = (mass != 0)[..., None]
        pooled = torch.where(live, pooled / torch.where(live, mass[..., None], torch.ones_like(mass[..., None])), torch.zeros_like(pooled))
    return (pooled, mass) if return_mass else pooled


def mask_attention_from_scores(scores: torch.Tensor, masks: torch.Tensor, lr_size, kernel_size) -> torch.Tensor:
    """``A[b, g, k, j] = sum_px masks[b, k, px] * softmax(scores)[b, g, px, slot of j]`` as torch ops (any device, CPU included), fp32
    [B, heads, K, h, w]: what ``xna_mask_pool`` computes, from materialised scores [B, heads, Ho, Wo, ky*kx] (``return_weights=True``) and the
    index tables -- any geometry, repeated keys included.  The composed arm of ``return_attention``; rows are processed in chunks so that
    the dense [pixels, keys] weights of a chunk stay below 256 MiB."""
    B, heads, Ho, Wo, kk = scores.shape
    h, w = int(lr_size[0]), int(lr_size[1])
    ky, kx = _ksize(kernel_size)
    dev = scores.device
    iy, ix = axis_index_table(Ho, h, ky).to(dev).long(), axis_index_table(Wo, w, kx).to(dev).long()
    K = masks.shape[1]
    m = masks.float()
    A = torch.zeros((B, heads, K, h * w), dtype=torch.float32, device=dev)
    rows = max(1, min(Ho, (64 << 20) // max(1, B * heads * Wo * h * w)))
    for r0 in range(0, Ho, rows):
        r1 = min(r0 + rows, Ho)
        key = (iy[r0:r1, None, :, None] * w + ix[None, :, None, :]).reshape(1, 1, (r1 - r0) * Wo, kk)
        P = torch.softmax(scores[:, :, r0:r1].float(), dim=-1).reshape(B, heads, (r1 - r0) * Wo, kk)
        dense = torch.zeros((B, heads, (r1 - r0) * Wo, h * w), dtype=torch.float32, device=dev).scatter_add_(3, key.expand_as(P), P)
        A += torch.einsum("bkp,bgpj->bgkj", m[:, :, r0:r1].reshape(B, K, -1), dense)
    return A.view(B, heads, K, h, w)


# ---- ... and a cosine head: scaled cosines between the upsampled feature and N embeddings (open vocabulary, heat maps) -----------
# ---- k-means on the upsampled features: one Lloyd step, assign and accumulate in one launch ---------------------------------------
KMEANS_FUSED_MAX = 64         # clusters naf_xna_kmeans_fwd takes (one launch; above it the step is composed)
KMEANS_MAX = 256              # clusters the composed step takes (the head kernel's uint8 label map)


def project_kmeans_values(centroids: torch.Tensor, features: torch.Tensor, heads: int):
    """The low-res half of the k-means assignment ``argmin_k |f - c_k|^2 = argmax_k (c_k . f - |c_k|^2 / 2)``: a linear head whose weight
    rows are the centroids and whose bias is minus half their squared norm.

    centroids [K, C] or [B, K, C], features [B, C, h, w] -> ``(pv5, bias, mean)``: pv5 bf16 [B, heads, h, w, Kpad] (Kpad = K rounded up to
    16, zero pad channels) as ``project_head_values`` lays it out, bias fp32 [B, K], mean fp32 [B, C].  The per-channel mean ``mu`` of the
    low-res features is subtracted from the features AND the centroids before projecting, and ``bias = -|c - mu|^2 / 2``: the attention
    weights of a head sum to one, so ``(c - mu) . (f - mu) - |c - mu|^2 / 2`` differs from ``c . f - |c|^2 / 2`` by a term without k and
    the argmax is the same, while the magnitudes that are rounded to bf16 shrink.  Pure torch, works on CPU tensors."""
    who = "project_kmeans_values"
    if features.dim() != 4:
        raise ValueError(f"{who}: features must be [B, C, h, w], got {tuple(features.shape)}")
    B, Cc, h, w = features.shape
    if centroids.dim() == 2:
        centroids = centroids[None].expand(B, -1, -1)
    if centroids.dim() != 3 or centroids.shape[0] != B or centroids.shape[2] != Cc or centroids.shape[1] < 1:
        raise ValueError(f"{who}: centroids must be [K, C] or [B, K, C] = ([{B},] K >= 1, {Cc}), got {tuple(centroids.shape)}")
    if heads <= 0 or Cc % heads:
        raise ValueError(f"{who}: feature channels {Cc} not divisible by {heads} heads")
    K, Dv = int(centroids.shape[1]), Cc // heads
    f = features.float()
    mean = f.mean(dim=(2, 3))
    cc = centroids.float() - mean[:, None, :]
    fc = f - mean[:, :, None, None]
    pv = torch.einsum("bkgd,bgdhw->bghwk", cc.reshape(B, K, heads, Dv), fc.reshape(B, heads, Dv, h, w))
    pad = head_npad(K) - K
    if pad:
        pv = torch.nn.functional.pad(pv, (0, pad))
    bias = -0.5 * (cc * cc).sum(dim=2)
    return pv.to(torch.bfloat16), bias.contiguous(), mean


def xna_kmeans_select(q: torch.Tensor, lr_size, k: int, kernel_size, *, rope_tables=None) -> str:
    """Which route a k-means step takes for these shapes: "fused" (``naf_xna_kmeans_select`` grants the one-launch kernel for ``k`` clusters)
    or "composed" (head-kernel labels, then mask pooling under their one-hot masks).  ``q``: the 5-D [B, heads, Ho, Wo, Dq] bf16 queries
    -- with ``rope_tables`` the un-rotated guidance.  A host-side query: nothing is launched or read, CPU / meta tensors do.  Invalid
    arguments raise ValueError; the library's reason for "composed" is in ``naf_last_error``."""
    if q.dtype != torch.bfloat16 or q.dim() != 5 or q.stride(4) != 1:
        return "composed"
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    _, heads, Ho, Wo, Dq = q.shape
    h, w = int(lr_size[0]), int(lr_size[1])
    kpad = head_npad(max(int(k), 1))
    a = _lib.XnaKmeansArgs()
    a.q = a.k_lr = a.pv_lr = a.A = a.mass = a.workspace = q.data_ptr() or 16      # shape / alignment query only: nothing is dereferenced
    if rope_tables is not None:
        a.rope_tab_y, a.rope_tab_x = rope_tables[0].data_ptr(), rope_tables[1].data_ptr()
    _fill_geometry(a, q, None, h, w, ky, kx, None)
    a.K, a.path = int(k), _lib.XNA_HEAD_AUTO
    a.k_stride = _dense5(h, w, heads, Dq)
    a.pv_stride = I64x4(heads * h * w * kpad, h * w * kpad, w * kpad, kpad)
    sel = lib.naf_xna_kmeans_select(C.byref(a))
    if sel == -1:
        _lib.check(1, "naf_xna_kmeans_select")
    return "fused" if sel == _lib.XNA_HEAD_FUSED else "composed"


def xna_kmeans_step(q: torch.Tensor, k_lr: torch.Tensor, pv_lr: torch.Tensor, bias: Optional[torch.Tensor], kernel_size, *,
                    k: Optional[int] = None, want_labels: bool = False, scale: Optional[float] = None, rope_tables=None):
    """One k-means step on the attention of ``xna_forward`` in one launch (``naf_xna_kmeans_fwd``): every pixel is labelled
    ``argmax_k (bias[b, k] + sum over heads and window of P . pv_lr)`` -- the lowest index among equal maxima -- and the attention is summed
    under those labels:

        ``A[b, g, k, j] = sum_px [label(px) = k] * P_g[px, j]``  fp32 [B, heads, K, h, w],  ``mass[b, k]``  fp32 [B, K], an exact count

    q [B, heads, Ho, Wo, Dq] and k_lr [B, heads, h, w, Dq] bf16 as for ``xna_mask_pool``, pv_lr bf16 [B, heads, h, w, Kpad] and bias fp32
    [B, K] (a row per image; any row stride) from ``project_kmeans_values``; bias None needs ``k``.  Returns ``(labels, A, mass)``, labels
    uint8 [B, Ho, Wo] or None (``want_labels``).  Two identities, bit for bit: the labels are ``xna_head_objective(want_labels=True)``'s per
    image, and (A, mass) are ``xna_mask_pool``'s for the bool masks ``labels == k``.  No float atomics: two calls give the same bits.
    Raises NafHipError where the kernel does not serve the request (``xna_kmeans_select``; K above ``KMEANS_FUSED_MAX``): the composition
    of those two operators is the caller's other arm."""
    who = "xna_kmeans_step"
    _check_operands(who, ((q, "q", _BF16), (k_lr, "k_lr", _BF16), (pv_lr, "pv_lr", _BF16)))
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, Dq = q.shape
    h, w, kpad = (int(s) for s in pv_lr.shape[2:])
    if tuple(k_lr.shape) != (B, heads, h, w, Dq) or tuple(pv_lr.shape[:2]) != (B, heads):
        raise ValueError(f"{who}: k_lr {tuple(k_lr.shape)} / pv_lr {tuple(pv_lr.shape)} do not match q {tuple(q.shape)}")
    if bias is not None:
        _gpu(bias, "bias")
        if bias.dtype != torch.float32 or bias.dim() != 2 or bias.shape[0] != B or bias.stride(1) != 1 or (k is not None and int(k) != bias.shape[1]):
            raise ValueError(f"{who}: bias must be a float32 [B, K] = ({B}, {'K' if k is None else int(k)}) tensor with contiguous rows")
        K = int(bias.shape[1])
    elif k is None:
        raise ValueError(f"{who}: without a bias the number of clusters k must be given")
    else:
        K = int(k)
    if K < 1 or kpad != head_npad(K):
        raise ValueError(f"{who}: pv_lr holds {kpad} channels, K = {K} needs {head_npad(max(K, 1))}")
    lib = _lib.load()
    dev = q.device
    A = torch.empty((B, heads, K, h, w), dtype=torch.float32, device=dev)
    mass = torch.empty((B, K), dtype=torch.float32, device=dev)
    labels = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev) if want_labels else None
    if B == 0:
        return labels, A, mass
    a = _lib.XnaKmeansArgs()
    a.q, a.k_lr, a.pv_lr, a.A, a.mass = q.data_ptr(), k_lr.data_ptr(), pv_lr.data_ptr(), A.data_ptr(), mass.data_ptr()
    if bias is not None:
        a.bias, a.bias_stride_b = bias.data_ptr(), (int(bias.stride(0)) if B > 1 else K)
    if labels is not None:
        a.labels, a.labels_stride = labels.data_ptr(), _strides3(labels)
    if rope_tables is not None:
        a.rope_tab_y, a.rope_tab_x = _rope_table_ptrs(who, rope_tables, Ho, Wo, Dq)
    _fill_geometry(a, q, k_lr, h, w, ky, kx, scale)
    a.K, a.path = K, _lib.XNA_HEAD_FUSED
    a.pv_stride = _strides4(pv_lr, (0, 1, 2, 3))
    need = int(lib.naf_xna_kmeans_workspace_bytes(C.byref(a)))
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    sel = lib.naf_xna_kmeans_select(C.byref(a))
    if sel != _lib.XNA_HEAD_FUSED:
        _lib.check(-sel, "naf_xna_kmeans_select")
    with torch.cuda.device(dev), _Timed("xna_kmeans_step"):
        rc = lib.naf_xna_kmeans_fwd(C.byref(a), _stream(q))
    _lib.check(rc, "naf_xna_kmeans_fwd")
    return labels, A, mass


def normalize_embeddings(embeddings: torch.Tensor) -> torch.Tensor:
    """``F.normalize(E.float(), dim=1)`` (eps 1e-12) of an [N, C] or [N, C, 1, 1] embedding matrix: the rows the cosine head projects with."""
    if embeddings.dim() == 4 and tuple(embeddings.shape[2:]) == (1, 1):
        embeddings = embeddings[:, :, 0, 0]
    if embeddings.dim() != 2 or not embeddings.is_floating_point():
        raise ValueError(f"cosine head: embeddings must be a floating-point [N, C] or [N, C, 1, 1] tensor, got {tuple(embeddings.shape)} {embeddings.dtype}")
    return torch.nn.functional.normalize(embeddings.float(), dim=1)


def _check_cos_operands(who: str, q, k_lr, v_lr, embeddings, path):
    _check_operands(who, ((q, "q", None), (k_lr, "k_lr", None), (v_lr, "v_lr", None)))
    if q.dtype != torch.bfloat16 or k_lr.dtype != torch.bfloat16:
        raise TypeError(f"{who}: q and k_lr must be bfloat16, got {q.dtype} / {k_lr.dtype}")
    if path not in _HEAD_PATHS:
        raise ValueError(f"{who}: path must be one of {_HEAD_PATHS}, got {path!r}")
    B, heads, Ho, Wo, Dq = q.shape
    h, w, Dv = v_lr.shape[2:]
    if k_lr.shape != (B, heads, h, w, Dq) or v_lr.shape[:2] != (B, heads):
        raise ValueError(f"{who}: k_lr {tuple(k_lr.shape)} / v_lr {tuple(v_lr.shape)} do not match q {tuple(q.shape)}")
    e = normalize_embeddings(embeddings)
    if e.shape[1] != heads * Dv or e.shape[0] < 1:
        raise ValueError(f"{who}: embeddings {tuple(e.shape)} do not match the {heads} x {Dv} = {heads * Dv} value channels")
    if e.device != q.device:
        raise ValueError(f"{who}: embeddings on {e.device}, q on {q.device}")
    return e, (B, heads, Ho, Wo, Dq, h, w, Dv)


def _fill_xna_cos(q, k, pv, v, out, norms, n_out, ky, kx, path, scale, logit_scale, rope_tables=None) -> "_lib.XnaCosArgs":
    B, heads, Ho, Wo, Dq = q.shape
    h, w, Dv = v.shape[2:]
    a = _lib.XnaCosArgs()
    a.q, a.k_lr, a.pv_lr, a.v_lr, a.out = q.data_ptr(), k.data_ptr(), pv.data_ptr(), v.data_ptr(), out.data_ptr()
    a.norms = norms.data_ptr() if norms is not None else None
    if rope_tables is not None:
        a.rope_tab_y, a.rope_tab_x = _rope_table_ptrs("xna_cos", rope_tables, Ho, Wo, Dq)
    _fill_geometry(a, q, k, h, w, ky, kx, scale)
    a.Dv, a.N = Dv, int(n_out)
    a.path = _lib.XNA_HEAD_FUSED if path == "fused" else _lib.XNA_HEAD_AUTO
    a.logit_scale = float(logit_scale)
    a.pv_stride = _strides4(pv, (0, 1, 2, 3))
    a.v_stride = _strides4(v, (0, 1, 2, 3))
    a.o_stride = _strides3(out)
    if norms is not None:
        a.norms_stride = _strides3(norms)
    return a


def xna_cos_select(q: torch.Tensor, lr_size, Dv: int, n_out: int, kernel_size, *, value_dtype: torch.dtype = torch.bfloat16,
                   rope_tables=None) -> str:
    """Which route ``xna_cos_forward(path="auto")`` takes for these shapes: "fused" (``naf_xna_cos_select`` grants the cosine-head kernel)
    or "composed" (the plain forward, normalised, times the normalised embeddings).  ``q``: the 5-D [B, heads, Ho, Wo, Dq] bf16 queries --
    with ``rope_tables`` the un-rotated guidance; ``Dv``: value channels per head; ``value_dtype``: the features' (the kernel reads
    bfloat16 values).  A host-side query: nothing is launched or read, CPU tensors do.  Invalid arguments raise ValueError."""
    if q.dtype != torch.bfloat16 or q.dim() != 5 or q.stride(4) != 1 or value_dtype != torch.bfloat16 or not 1 <= int(n_out) <= 256 or int(Dv) < 1:
        return "composed"
    return _head_route(_lib.XnaCosArgs(), "naf_xna_cos_select", q, lr_size, n_out, kernel_size, rope_tables, Dv=int(Dv))


def cosine_from_features(f: torch.Tensor, e_hat: torch.Tensor, logit_scale: float = 1.0, return_norms: bool = False):
    """The definition in torch ops: ``logit_scale * einsum("nc,bchw->bnhw", e_hat, F.normalize(f.float(), dim=1))`` for f [B, C, H, W] and
    normalised rows ``e_hat`` [N, C] fp32 (``normalize_embeddings``); with ``return_norms`` also ``f.float().norm(dim=1)``.  A zero feature
    gives exactly 0.  Differentiable; the result is a logical [B, N, H, W] view of a dense channels-last buffer, as the kernel's."""
    ff = f.float().permute(0, 2, 3, 1)
    nrm = ff.norm(dim=3)
    cos = (torch.matmul(ff / nrm.clamp_min(1e-12).unsqueeze(3), e_hat.t()) * float(logit_scale)).permute(0, 3, 1, 2)
    return (cos, nrm) if return_norms else cos


def xna_cos_forward(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, embeddings: torch.Tensor, kernel_size, *,
                    logit_scale: float = 1.0, return_norms: bool = False, path: str = "auto", scale: Optional[float] = None,
                    rope_tables=None):
    """Cross-scale neighbourhood attention with a cosine head folded in: per pixel, ``logit_scale`` times the cosine between the upsampled
    feature ``f = attention(q, k_lr, v_lr)`` (all heads' channels) and each of the N rows of ``embeddings``, without writing ``f``.

    q [B, heads, Ho, Wo, Dq] bf16, k_lr [B, heads, h, w, Dq] bf16, v_lr [B, heads, h, w, Dv] (5-D strided views, last dim contiguous),
    embeddings [N, heads * Dv] (or [N, C, 1, 1]) of any float dtype on the same device.  Returns fp32 ``cos`` as a logical [B, N, Ho, Wo]
    view of a dense channels-last [B, Ho, Wo, N] buffer; with ``return_norms`` also ``||f||_2`` [B, Ho, Wo] fp32 (unclamped).  A pixel whose
    feature is zero gets exactly 0.  Inference only on the fused route (no graph is recorded).
    ``path="auto"``: the kernel (``naf_xna_cos_fwd``: the numerator through ``E^ @ V`` on the low-res grid as in ``xna_head_forward``, the
    norm from ``P . V`` on the matrix cores, squared and dropped) where ``naf_xna_cos_select`` grants it and no gradient is wanted for the
    embeddings, else the composition: ``xna_forward``, ``F.normalize`` and a matrix product as torch ops (``cosine_from_features``;
    differentiable with respect to the embeddings).  ``"fused"`` insists and raises NafHipError where the kernel does not serve the call
    or a gradient is wanted for the embeddings; ``"composed"`` insists on the composition.
    ``rope_tables``: as in ``xna_forward`` (q is the un-rotated guidance)."""
    e_hat, (B, heads, Ho, Wo, Dq, h, w, Dv) = _check_cos_operands("xna_cos_forward", q, k_lr, v_lr, embeddings, path)
    ky, kx = _ksize(kernel_size)
    N = e_hat.shape[0]
    if not math.isfinite(float(logit_scale)):
        raise ValueError(f"xna_cos_forward: logit_scale must be finite, got {logit_scale}")
    lib = _lib.load()
    dev = q.device
    wants_grad = torch.is_grad_enabled() and embeddings.requires_grad
    if path == "fused" and wants_grad:
        raise _lib.NafHipError("xna_cos_forward: the fused cosine kernel is inference-only; the embeddings require a gradient "
                               "(path='composed' is differentiable)")
    if path != "composed" and not wants_grad and (path == "fused" or (v_lr.dtype == torch.bfloat16 and N <= 256)):
        if v_lr.dtype != torch.bfloat16:
            raise _lib.NafHipError(f"xna_cos_forward: the fused kernel needs bfloat16 values, got {v_lr.dtype}")
        with torch.no_grad():
            pv = torch.einsum("ngd,bghwd->bghwn", e_hat.reshape(N, heads, Dv), v_lr.float())
            pad = head_npad(N) - N
            pv5 = (torch.nn.functional.pad(pv, (0, pad)) if pad else pv).to(torch.bfloat16)
            out = torch.empty((B, Ho, Wo, N), dtype=torch.float32, device=dev)
            norms = torch.empty((B, Ho, Wo), dtype=torch.float32, device=dev) if return_norms else None
            a = _fill_xna_cos(q, k_lr, pv5, v_lr, out, norms, N, ky, kx, path, scale, logit_scale, rope_tables)
            sel = lib.naf_xna_cos_select(C.byref(a))
            if sel == _lib.XNA_HEAD_FUSED:
                with torch.cuda.device(dev), _Timed("xna_cos"):
                    rc = lib.naf_xna_cos_fwd(C.byref(a), _stream(q))
                _lib.check(rc, "naf_xna_cos_fwd")
                cos = out.permute(0, 3, 1, 2)
                return (cos, norms) if return_norms else cos
            if path == "fused" or sel == -1:       # insisted, or arguments no kernel serves
                _lib.check(-sel, "naf_xna_cos_select")
            del out, norms, pv5, pv
    with _Timed("xna_cos_composed"):
        with torch.no_grad():
            odt = v_lr.dtype if v_lr.dtype in (torch.bfloat16, torch.float16) else torch.float32
            o5 = xna_forward(q, k_lr, v_lr if v_lr.dtype in (torch.bfloat16, torch.float16) else v_lr.to(torch.bfloat16), (ky, kx),
                             out_dtype=odt, path="auto", scale=scale, rope_tables=rope_tables)
            f = o5.permute(0, 1, 4, 2, 3).reshape(B, heads * Dv, Ho, Wo)
        return cosine_from_features(f, e_hat, logit_scale, return_norms)


# ---- ... and the peak search: where in the upsampled map each embedding matches best, without the N-channel map ------------------
def peaks_from_cosines(cos: torch.Tensor, lr_size) -> Tuple[torch.Tensor, torch.Tensor]:
    """The definition in torch ops: for cos [B, N, Ho, Wo] fp32 and an integer ratio, ``peak`` [B, N, h, w] = the maximum over each cell's
    pixels and ``where`` [B, N, h, w] int32 = the lowest flat index ``y * Wo + x`` among the cell's pixels that attain it
    (``where(cos == peak, index, big).amin``: torch's argmax promises no tie rule on the device)."""
    B, N, Ho, Wo = cos.shape
    h, w = int(lr_size[0]), int(lr_size[1])
    if Ho % h or Wo % w:
        raise ValueError(f"peak search: {Ho}x{Wo} pixels over {h}x{w} cells is not an integer ratio: there are no cells")
    dy, dx = Ho // h, Wo // w
    c = cos.reshape(B, N, h, dy, w, dx)
    peak = c.amax(dim=(3, 5))
    idx = torch.arange(Ho * Wo, dtype=torch.int32, device=cos.device).view(1, 1, h, dy, w, dx)
    big = torch.full((), 2 ** 31 - 1, dtype=torch.int32, device=cos.device)
    where = torch.where(c == peak[:, :, :, None, :, None], idx, big).amin(dim=(3, 5))
    return peak, where


def xna_cos_peaks_select(q: torch.Tensor, lr_size, Dv: int, n_out: int, kernel_size, *, value_dtype: torch.dtype = torch.bfloat16,
                         rope_tables=None) -> str:
    """Which route ``xna_cos_peaks(path="auto")`` takes for these shapes and at most 256 embeddings (more run in chunks of 256): "fused"
    (``naf_xna_cos_peaks_select`` grants the peak epilogue of the cosine kernel) or "composed" (``xna_cos_forward``, then the definition in
    torch ops).  The conventions of ``xna_cos_select``: a host-side query, nothing is launched or read, invalid arguments raise ValueError."""
    if q.dtype != torch.bfloat16 or q.dim() != 5 or q.stride(4) != 1 or value_dtype != torch.bfloat16 or not 1 <= int(n_out) <= 256 or int(Dv) < 1:
        return "composed"
    outer = _lib.XnaCosPeaksArgs()
    h, w, n = int(lr_size[0]), int(lr_size[1]), int(n_out)
    outer.peak = outer.where = q.data_ptr() or 16
    outer.peak_stride = outer.where_stride = I64x3(h * w * n, w * n, n)
    return _head_route(outer.cos, "naf_xna_cos_peaks_select", q, lr_size, n_out, kernel_size, rope_tables, Dv=int(Dv), outer=outer)


def xna_cos_peaks(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, embeddings: torch.Tensor, kernel_size, *,
                  logit_scale: float = 1.0, want_cos: bool = False, path: str = "auto", scale: Optional[float] = None, rope_tables=None):
    """Cell peaks of the scaled cosines: with ``cos`` what ``xna_cos_forward`` returns for the same operands, ``peak[b, n, cy, cx]`` is the
    maximum of ``cos[b, n]`` over the pixels of low-res cell (cy, cx) -- the bits of an element of ``cos`` -- and ``where[b, n, cy, cx]``
    the lowest flat index ``y * Wo + x`` among the cell's pixels that attain it.  Needs an integer ratio (ValueError otherwise: there are
    no cells).  Returns ``(peak [B, N, h, w] fp32, where [B, N, h, w] int32, cos or None)``: the first two are logical views of dense
    channels-last [B, h, w, N] buffers; ``want_cos`` also returns the cosines (then the map is written).  Inference only.
    ``path="auto"``: the kernel (``naf_xna_cos_peaks_fwd``: the maximum over the cell's pixels is taken in the epilogue of the cosine
    kernel, the [B, N, Ho, Wo] map never exists) where ``naf_xna_cos_peaks_select`` grants it, else the composition ``xna_cos_forward`` +
    ``peaks_from_cosines`` (fp16 / fp32 values, windows 13 / 15 with more than 64 embeddings).  More than 256 embeddings run in chunks of
    256.  ``"fused"`` insists and raises NafHipError with the library's reason; ``"composed"`` insists on the composition."""
    e_hat, (B, heads, Ho, Wo, Dq, h, w, Dv) = _check_cos_operands("xna_cos_peaks", q, k_lr, v_lr, embeddings, path)
    ky, kx = _ksize(kernel_size)
    N = e_hat.shape[0]
    if not math.isfinite(float(logit_scale)):
        raise ValueError(f"xna_cos_peaks: logit_scale must be finite, got {logit_scale}")
    if Ho % h or Wo % w:
        raise ValueError(f"xna_cos_peaks: {Ho}x{Wo} pixels over {h}x{w} cells is not an integer ratio: there are no cells")
    if Ho * Wo >= 2 ** 31:
        raise ValueError(f"xna_cos_peaks: {Ho}x{Wo} pixels do not fit an int32 flat index")
    if N > 256:
        parts = [xna_cos_peaks(q, k_lr, v_lr, embeddings[n0:n0 + 256], kernel_size, logit_scale=logit_scale, want_cos=want_cos, path=path, scale=scale,
                               rope_tables=rope_tables) for n0 in range(0, N, 256)]
        return (torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1),
                torch.cat([p[2] for p in parts], dim=1) if want_cos else None)
    lib = _lib.load()
    dev = q.device
    with torch.no_grad():
        if path != "composed" and (path == "fused" or v_lr.dtype == torch.bfloat16):
            if v_lr.dtype != torch.bfloat16:
                raise _lib.NafHipError(f"xna_cos_peaks: the fused kernel needs bfloat16 values, got {v_lr.dtype}")
            pv = torch.einsum("ngd,bghwd->bghwn", e_hat.reshape(N, heads, Dv), v_lr.float())
            pad = head_npad(N) - N
            pv5 = (torch.nn.functional.pad(pv, (0, pad)) if pad else pv).to(torch.bfloat16)
            out = torch.empty((B, Ho, Wo, N), dtype=torch.float32, device=dev) if want_cos else None
            peak = torch.empty((B, h, w, N), dtype=torch.float32, device=dev)
            where = torch.empty((B, h, w, N), dtype=torch.int32, device=dev)
            a = _lib.XnaCosPeaksArgs()
            a.cos = _fill_xna_cos(q, k_lr, pv5, v_lr, out if want_cos else peak, None, N, ky, kx, path, scale, logit_scale, rope_tables)
            if not want_cos:
                a.cos.out = None
            a.peak, a.where = peak.data_ptr(), where.data_ptr()
            a.peak_stride, a.where_stride = _strides3(peak), _strides3(where)
            sel = lib.naf_xna_cos_peaks_select(C.byref(a))
            if sel == _lib.XNA_HEAD_FUSED:
                with torch.cuda.device(dev), _Timed("xna_cos_peaks"):
                    rc = lib.naf_xna_cos_peaks_fwd(C.byref(a), _stream(q))
                _lib.check(rc, "naf_xna_cos_peaks_fwd")
                return peak.permute(0, 3, 1, 2), where.permute(0, 3, 1, 2), (out.permute(0, 3, 1, 2) if want_cos else None)
            if path == "fused" or sel == -1:       # insisted, or arguments no kernel serves
                _lib.check(-sel, "naf_xna_cos_peaks_select")
            del out, peak, where, pv5, pv
        with _Timed("xna_cos_peaks_composed"):
            cos = xna_cos_forward(q, k_lr, v_lr, e_hat, (ky, kx), logit_scale=logit_scale, path="auto", scale=scale, rope_tables=rope_tables)
            peak, where = peaks_from_cosines(cos, (h, w))
            # channels-last, as the kernel's
            peak = peak.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            where = where.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        return peak, where, (cos if want_cos else None)


def peaks_topk(peak: torch.Tensor, where: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ``k`` best cells of every (b, n): the ``h * w`` candidates ``(peak, where)`` ordered by value descending, then by flat index
    ascending (``naf_peaks_topk``: torch promises no tie rule on the device).  One candidate per low-res cell -- a non-maximum suppression
    at the cell grid, not the k best pixels; ``k = 1`` is the global maximum of the cosine map with the lowest flat index among ties.
    ``peak`` fp32 and ``where`` int32, both [B, N, h, w] (``xna_cos_peaks``'s; any strides, channels-last ones are read in place);
    1 <= k <= min(h * w, 64).  Returns ``(values [B, N, k] fp32, index [B, N, k] int32)``."""
    _gpu(peak, "peak")
    _gpu(where, "where")
    if peak.dim() != 4 or peak.shape != where.shape or peak.dtype != torch.float32 or where.dtype != torch.int32:
        raise ValueError(f"peaks_topk: peak must be fp32 and where int32, both [B, N, h, w]; got {tuple(peak.shape)} {peak.dtype} / {tuple(where.shape)} {where.dtype}")
    B, N, h, w = peak.shape
    k = int(k)
    if not 1 <= k <= min(h * w, 64):
        raise ValueError(f"peaks_topk: k must be in 1 .. min(h * w, 64) = {min(h * w, 64)}, got {k}")
    values = torch.empty((B, N, k), dtype=torch.float32, device=peak.device)
    index = torch.empty((B, N, k), dtype=torch.int32, device=peak.device)
    if B == 0 or N == 0:
        return values, index

    def cells(t):   # [B, N, h, w] -> a view [B, h * w, N] with the channel axis contiguous, or a copy that is
        t = t.permute(0, 2, 3, 1)
        if t.stride(3) != 1 or t.stride(1) != w * t.stride(2):
            t = t.contiguous()
        return t, (C.c_int64 * 2)(t.stride(0), t.stride(2))
    pk, ps = cells(peak)
    wh, ws = cells(where)
    lib = _lib.load()
    with torch.cuda.device(peak.device), _Timed("peaks_topk"):
        rc = lib.naf_peaks_topk(pk.data_ptr(), wh.data_ptr(), values.data_ptr(), index.data_ptr(), B, N, h * w, k, ps, ws, _stream(peak))
    _lib.check(rc, "naf_peaks_topk")
    return values, index


def head_dlogits_channels(n_out: int) -> int:
    """Channels of a ``dlogits`` row for ``n_out`` classes: the value width the cell backward serves that holds Npad (``_BWD_DV``)."""
    npad = head_npad(n_out)
    return next((c for c in _BWD_DV if c >= npad), npad)


def _head_values_grad(q, k_lr, pv_lr, g, kernel_size, scale) -> torch.Tensor:
    """fp32 gradient of ``pv_lr`` [B, heads, h, w, Npad] for ONE gradient of the logits ``g`` (bf16 [B, Ho, Wo, Gc], Gc >= Npad a width the
    cell backward serves, zero pad channels): ``pv_lr`` is padded to Gc (the pad channels' gradient is zero), ``g`` is the ``dout`` of every
    head (stride 0), dq / dk are dropped."""
    B, heads, Ho, Wo, _ = q.shape
    npad, gc = pv_lr.shape[-1], g.shape[-1]
    pvp = torch.nn.functional.pad(pv_lr, (0, gc - npad)) if gc != npad else pv_lr
    _, _, dv = xna_backward(q, k_lr, pvp, g.unsqueeze(1).expand(B, heads, Ho, Wo, gc), kernel_size, scale=scale)
    return dv[..., :npad]


class XnaHeadFunction(torch.autograd.Function):
    """Differentiable ``xna_head_forward`` with respect to the head: gradients reach ``pv_lr`` and ``bias`` only (the queries and keys come
    from a frozen upsampler).  ``dPV_g[cell] = sum_px P_g[px, cell] * dOut[px]`` is the ``dv_lr`` of ``naf_xna_bwd`` with ONE ``dout`` shared
    by all heads: the backward hands it over expanded along the head axis (stride 0) and discards dq / dk.  ``q`` holds materialised
    (rotated) queries: the backward kernels have no rotate-on-load."""

    @staticmethod
    def forward(ctx, q, k_lr, pv_lr, bias, kernel_size, n_out, out_dtype, path="auto", scale=None):
        ctx.save_for_backward(q, k_lr, pv_lr)
        ctx.kernel_size, ctx.n_out, ctx.scale, ctx.has_bias = kernel_size, int(n_out), scale, bias is not None
        return xna_head_forward(q, k_lr, pv_lr, bias, kernel_size, n_out=n_out, out_dtype=out_dtype, path=path, scale=scale)

    @staticmethod
    def backward(ctx, dout):
        q, k_lr, pv_lr = ctx.saved_tensors
        need_pv, need_b = ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3]
        N = ctx.n_out
        dpv = dbias = None
        if need_b:
            dbias = dout.float().sum(dim=(0, 2, 3))
        if need_pv:
            B, _, Ho, Wo, _ = q.shape
            g = torch.zeros((B, Ho, Wo, head_dlogits_channels(N)), dtype=torch.bfloat16, device=q.device)
            g[..., :N] = dout.permute(0, 2, 3, 1)
            dpv = _head_values_grad(q, k_lr, pv_lr, g, ctx.kernel_size, ctx.scale).to(pv_lr.dtype)
        return None, None, dpv, dbias, None, None, None, None, None


# ---- ... and a classification objective in its epilogue (cross-entropy / argmax of the probe's logits) -------------------
_REDUCTIONS = ("mean", "sum", "none")


def head_valid_pixels(target: torch.Tensor, ignore_index: int, n_out: int) -> torch.Tensor:
    """Bool map of the pixels the objective counts: ``target != ignore_index`` and ``0 <= target < n_out`` -- what the kernel does not
    ignore.  (``torch.nn.functional.cross_entropy`` raises a device-side assert for a target outside the classes; here it is ignored.)"""
    return (target != int(ignore_index)) & (target >= 0) & (target < int(n_out))


def head_sanitized_target(target: torch.Tensor, ignore_index: int, n_out: int) -> torch.Tensor:
    """``target`` with every ignored pixel (``head_valid_pixels``) set to ``ignore_index``: ``F.cross_entropy(logits, that, ignore_index=...)``
    then has this library's contract for targets outside the classes and torch's arithmetic, without a device-side assert."""
    return torch.where(head_valid_pixels(target, ignore_index, n_out), target, torch.full_like(target, int(ignore_index)))


def head_objective_from_logits(logits: torch.Tensor, target: Optional[torch.Tensor] = None, ignore_index: int = -100, *,
                               want_loss: bool = False, want_labels: bool = False, want_dlogits: bool = False,
                               dlogits_channels: Optional[int] = None):
    """The classification epilogue of ``naf_xna_head_ce_fwd`` as torch ops on materialised logits [B, N, Ho, Wo] (any device, CPU included):
    what ``xna_head_objective`` composes where the kernel does not serve the geometry, with the same contract.  Returns
    ``(loss_map, labels, dlogits)``, each None unless wanted: the per-pixel ``logsumexp(z) - z[t]`` (0 where the pixel is ignored; float64 for
    float64 logits, else float32) [B, Ho, Wo]; ``argmax`` over the classes (uint8 up to 256 classes, else int64); ``softmax(z) - onehot(t)``,
    zero rows for ignored pixels, bf16 channels-last [B, Ho, Wo, dlogits_channels] with zero pad channels.  Ignored: ``t == ignore_index`` or
    ``t`` outside [0, N) (see ``head_valid_pixels``)."""
    B, N, Ho, Wo = logits.shape
    z = logits if logits.dtype == torch.float64 else logits.float()
    if (want_loss or want_dlogits) and target is None:
        raise ValueError("head objective: the loss and the gradient of the logits need a target")
    loss = labels = g = None
    if want_labels:
        labels = z.argmax(dim=1)
        if N <= 256:
            labels = labels.to(torch.uint8)
    if want_loss or want_dlogits:
        valid = head_valid_pixels(target, ignore_index, N)
        tc = torch.where(valid, target, torch.zeros_like(target)).unsqueeze(1)
        lse = torch.logsumexp(z, dim=1)
        if want_loss:
            loss = torch.where(valid, lse - z.gather(1, tc)[:, 0], torch.zeros_like(lse))
        if want_dlogits:
            gc = int(dlogits_channels) if dlogits_channels is not None else head_dlogits_channels(N)
            if gc < N:
                raise ValueError(f"head objective: dlogits_channels {gc} smaller than the {N} classes")
            sm = torch.exp(z - lse.unsqueeze(1)).permute(0, 2, 3, 1)
            sm = sm - torch.nn.functional.one_hot(tc[:, 0], N).to(sm.dtype)
            sm = sm * valid.unsqueeze(-1).to(sm.dtype)
            g = torch.nn.functional.pad(sm, (0, gc - N)).to(torch.bfloat16)
    return loss, labels, g


def reduce_head_loss(loss_map: torch.Tensor, target: torch.Tensor, ignore_index: int, n_out: int, reduction: str) -> torch.Tensor:
    """``reduction`` of the per-pixel loss map as ``F.cross_entropy`` defines it: "none" the map, "sum" its sum, "mean" the sum over the number
    of valid pixels (``head_valid_pixels``, counted on the device without a host synchronisation; no valid pixel: nan, as torch)."""
    if reduction == "none":
        return loss_map
    total = loss_map.sum()
    if reduction == "sum":
        return total
    return total / head_valid_pixels(target, ignore_index, n_out).sum().to(total.dtype)


def _check_target(target: torch.Tensor, shape, device, who: str) -> torch.Tensor:
    if not isinstance(target, torch.Tensor) or target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
        raise TypeError(f"{who}: target must be an integer tensor of class indices, got {getattr(target, 'dtype', type(target).__name__)}")
    if tuple(target.shape) != tuple(shape):
        raise ValueError(f"{who}: target must be [B, Ho, Wo] = {tuple(shape)}, got {tuple(target.shape)}")
    if target.device != device:
        raise ValueError(f"{who}: target is on {target.device}, the features on {device}")
    return target if target.dtype == torch.int64 else target.long()


def _check_confusion(confusion, n_out: int, device, who: str) -> None:
    if not isinstance(confusion, torch.Tensor) or confusion.dtype != torch.int64:
        raise TypeError(f"{who}: confusion must be an int64 tensor, got {getattr(confusion, 'dtype', type(confusion).__name__)}")
    if tuple(confusion.shape) != (int(n_out), int(n_out)) or confusion.stride(1) != 1 or confusion.stride(0) < int(n_out):
        raise ValueError(f"{who}: confusion must be [N, N] = [{int(n_out)}, {int(n_out)}] with contiguous columns, "
                         f"got {tuple(confusion.shape)} with strides {tuple(confusion.stride())}")
    if confusion.device != device:
        raise ValueError(f"{who}: confusion is on {confusion.device}, the features on {device}")


def head_confusion_from_labels(labels: torch.Tensor, target: torch.Tensor, ignore_index: int, n_out: int,
                               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The confusion matrix of ``naf_xna_head_cm_fwd`` as torch ops (any device, CPU included): int64 [N, N], ``cm[t, p]`` = number of
    pixels with target ``t`` and predicted label ``p`` (row = target, column = prediction) over the pixels ``head_valid_pixels`` counts --
    ``target != ignore_index`` and ``0 <= target < n_out``; everything else adds nothing.  ``out`` (int64 [N, N], columns contiguous, any row
    stride): the counts are ADDED to it and it is returned; None: a fresh matrix.  What ``xna_head_objective`` composes where the kernel
    does not serve the geometry, and the definition the tests hold the kernel to.  No host synchronisation: the counts are an
    ``index_add_`` of ones (integer adds, exact in any order) -- ``bincount(t * N + p, minlength=N * N)`` without its size query.  A label
    outside [0, N) (none comes out of an argmax over N classes) is not counted either."""
    N = int(n_out)
    if labels.shape != target.shape:
        raise ValueError(f"head_confusion_from_labels: labels {tuple(labels.shape)} and target {tuple(target.shape)} differ in shape")
    target = target if target.dtype == torch.int64 else target.long()
    pred = labels.long()
    valid = head_valid_pixels(target, ignore_index, N) & (pred >= 0) & (pred < N)
    key = torch.where(valid, target * N + pred, torch.full_like(target, N * N))      # the extra slot takes what is not counted
    counts = torch.zeros(N * N + 1, dtype=torch.int64, device=target.device)
    counts.index_add_(0, key.reshape(-1), torch.ones((), dtype=torch.int64, device=target.device).expand(key.numel()))
    cm = counts[:N * N].view(N, N)
    if out is None:
        return cm
    _check_confusion(out, N, target.device, "head_confusion_from_labels")
    return out.add_(cm)


ConfusionMetrics = collections.namedtuple("ConfusionMetrics", ("accuracy", "iou", "miou", "present"))


def confusion_metrics(cm: torch.Tensor) -> "ConfusionMetrics":
    """Accuracy and intersection-over-union from a confusion matrix [N, N] (row = target, column = prediction), in float64 on the matrix's
    device, without a host synchronisation.  Returns ``ConfusionMetrics(accuracy, iou, miou, present)``:

        accuracy = trace(cm) / sum(cm)                                   (micro: every counted pixel weighs the same)
        iou[c]   = cm[c, c] / (row_c + col_c - cm[c, c]),  0 where that union is 0
        present  = union != 0                                            (bool [N]: the class occurs in the targets or the predictions)
        miou     = mean of iou over the present classes

    A class absent from both targets and predictions is left out of ``miou``; one that is predicted but never a target counts with IoU 0.
    A matrix without counts (every pixel ignored) gives nan for ``accuracy`` and ``miou``, as a 0 / 0 mean is in torch.  These are the
    definitions the reference's ``evaluate()`` gets from ``torchmetrics`` ``Accuracy(task="multiclass")`` (its default, micro) and
    ``JaccardIndex(task="multiclass")`` as far as their documentation goes; ``torchmetrics`` is not a dependency of this project and the
    equivalence has NOT been verified against it."""
    if not isinstance(cm, torch.Tensor) or cm.dim() != 2 or cm.shape[0] != cm.shape[1] or cm.dtype.is_floating_point or cm.dtype == torch.bool:
        raise ValueError(f"confusion_metrics: an integer [N, N] matrix is expected, got {getattr(cm, 'dtype', type(cm).__name__)} "
                         f"{tuple(getattr(cm, 'shape', ()))}")
    c = cm.to(torch.float64)
    diag, total = c.diagonal(), c.sum()
    union = c.sum(dim=1) + c.sum(dim=0) - diag
    present = union != 0
    iou = torch.where(present, diag / torch.where(present, union, torch.ones_like(union)), torch.zeros_like(union))
    return ConfusionMetrics(diag.sum() / total, iou, iou.sum() / present.sum().to(torch.float64), present)


def xna_head_objective(q: torch.Tensor, k_lr: torch.Tensor, pv_lr: torch.Tensor, bias: Optional[torch.Tensor], kernel_size, *,
                       n_out: int, target: Optional[torch.Tensor] = None, ignore_index: int = -100, want_loss: bool = False,
                       want_labels: bool = False, want_dlogits: bool = False, return_logits: bool = False, path: str = "auto",
                       scale: Optional[float] = None, rope_tables=None, confusion: Optional[torch.Tensor] = None):
    """``xna_head_forward`` with the classification objective in the kernel's epilogue (``naf_xna_head_ce_fwd``): one launch gives any of
    the per-pixel cross-entropy, the argmax labels and ``softmax - onehot`` without the [B, N, Ho, Wo] logits ever being written.

    Arguments as ``xna_head_forward``; ``target`` int64 [B, Ho, Wo] (any strides) is needed for the loss and the gradient.  Returns
    ``(loss_map, labels, dlogits, logits)``, each None unless asked for: fp32 [B, Ho, Wo], 0 where the pixel is ignored; uint8 [B, Ho, Wo]
    (int64 beyond 256 classes), the lowest index among equal maxima; bf16 [B, Ho, Wo, Gc] with ``Gc = head_dlogits_channels(n_out)``,
    every channel written (zeros from ``n_out`` up) and NOT divided by the number of valid pixels -- the ``dout`` the attention backward takes
    for all heads at once; fp32 logits as ``xna_head_forward(..., out_dtype=float32)`` returns them (``return_logits``).
    A pixel is ignored when ``target == ignore_index`` OR ``target`` is outside [0, n_out): where ``F.cross_entropy`` raises a device-side
    assert, the pixel contributes nothing.  ``path="auto"`` composes ``xna_head_forward(..., out_dtype=float32)`` with
    ``head_objective_from_logits`` where the kernel does not serve the geometry (same contract); ``path="fused"`` insists and raises.
    ``confusion``: an int64 [n_out, n_out] device tensor (any row stride, columns contiguous) that the call ACCUMULATES into in the same
    launch (``naf_xna_head_cm_fwd``): ``confusion[t, label] += 1`` for every pixel that is not ignored; needs ``target``; the returned
    4-tuple is unchanged and may be all None.  Loss, labels and matrix of one launch are available here together.  The composed route
    counts its labels with ``head_confusion_from_labels``."""
    ky, kx, B, heads, Ho, Wo, Dq, h, w, npad, n_out = _check_head_operands("xna_head_objective", q, k_lr, pv_lr, bias, kernel_size, n_out, path)
    if not (want_loss or want_labels or want_dlogits or return_logits or confusion is not None):
        raise ValueError("xna_head_objective: nothing asked for (want_loss / want_labels / want_dlogits / return_logits / confusion)")
    lib = _lib.load()
    dev = q.device
    if want_loss or want_dlogits:
        if target is None:
            raise ValueError("xna_head_objective: the loss and the gradient of the logits need a target")
    if confusion is not None:
        if target is None:
            raise ValueError("xna_head_objective: a confusion matrix needs a target")
        _check_confusion(confusion, n_out, dev, "xna_head_objective")
    if target is not None:
        target = _check_target(target, (B, Ho, Wo), dev, "xna_head_objective")
    gc = head_dlogits_channels(n_out)
    if path != "composed" and (n_out <= 256 or path == "fused"):
        out = torch.empty((B, Ho, Wo, n_out), dtype=torch.float32, device=dev) if return_logits else None
        loss = torch.empty((B, Ho, Wo), dtype=torch.float32, device=dev) if want_loss else None
        labels = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev) if want_labels else None
        g = torch.empty((B, Ho, Wo, gc), dtype=torch.bfloat16, device=dev) if want_dlogits else None     # the kernel writes every channel
        a = _lib.XnaHeadCEArgs()
        a.head = _fill_xna_head(q, k_lr, pv_lr, bias, out if out is not None else q, n_out, ky, kx, path, scale, rope_tables)
        if out is None:
            a.head.out, a.head.out_dtype = None, _lib.NAF_F32
        a.ignore_index, a.dlogits_channels = int(ignore_index), gc
        for t, ptr, st in ((target if (want_loss or want_dlogits or confusion is not None) else None, "target", "t_stride"), (loss, "loss", "loss_stride"),
                           (labels, "labels", "labels_stride"), (g, "dlogits", "dlogits_stride")):
            if t is not None:
                setattr(a, ptr, t.data_ptr())
                setattr(a, st, _strides3(t))
        if confusion is not None:              # the same epilogue counting into the caller's matrix: an entry point of its own
            m = _lib.XnaHeadCMArgs()
            m.ce, m.confusion, m.cm_stride = a, confusion.data_ptr(), int(confusion.stride(0))
            a, entry, select, fwd = m, "naf_xna_head_cm", lib.naf_xna_head_cm_select, lib.naf_xna_head_cm_fwd
        else:
            entry, select, fwd = "naf_xna_head_ce", lib.naf_xna_head_ce_select, lib.naf_xna_head_ce_fwd
        sel = select(C.byref(a))
        if sel == _lib.XNA_HEAD_FUSED:
            with torch.cuda.device(dev), _Timed("xna_head_ce"):
                rc = fwd(C.byref(a), _stream(q))
            _lib.check(rc, entry + "_fwd")
            return loss, labels, g, (None if out is None else out.permute(0, 3, 1, 2))
        if path == "fused" or sel == -1:       # insisted, or arguments no kernel serves
            _lib.check(-sel, entry + "_select")
        del out, loss, labels, g
    with _Timed("xna_head_ce_composed"):
        logits = xna_head_forward(q, k_lr, pv_lr, bias, (ky, kx), n_out=n_out, out_dtype=torch.float32,
                                  path="auto" if path == "auto" else "composed", scale=scale, rope_tables=rope_tables)
        loss, labels, g = head_objective_from_logits(logits, target, ignore_index, want_loss=want_loss,
                                                     want_labels=want_labels or confusion is not None,
                                                     want_dlogits=want_dlogits, dlogits_channels=gc)
        if confusion is not None:
            head_confusion_from_labels(labels, target, ignore_index, n_out, out=confusion)
        return loss, (labels if want_labels else None), g, (logits if return_logits else None)


class XnaHeadCEFunction(torch.autograd.Function):
    """Differentiable cross-entropy of the head-summed attention's logits, with respect to the head (``pv_lr`` and ``bias`` only, as
    ``XnaHeadFunction``): the forward is ONE launch (``xna_head_objective``) that leaves the loss map and ``g = softmax - onehot`` (bf16,
    the attention backward's width, unnormalised); the backward hands ``g`` to ``xna_backward`` as the ``dout`` of every head (stride 0) and
    scales the low-res result by the incoming gradient and, for "mean", by 1 / number of valid pixels -- the backward is linear in ``g``.
    ``dbias = sum over pixels of g`` times the same.  reduction="none": the incoming gradient is a map, ``g`` is scaled per pixel first.
    Returns the reduced loss, or ``(loss, labels)`` with ``want_labels``.  ``q`` holds materialised (rotated) queries.
    Not here: a head-only backward kernel (dq / dk are computed and dropped), class weights, label smoothing, soft targets."""

    @staticmethod
    def forward(ctx, q, k_lr, pv_lr, bias, target, kernel_size, n_out, ignore_index=-100, reduction="mean", want_labels=False,
                path="auto", scale=None):
        if reduction not in _REDUCTIONS:
            raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
        n_out = int(n_out)
        loss_map, labels, g, _ = xna_head_objective(q, k_lr, pv_lr, bias, kernel_size, n_out=n_out, target=target, ignore_index=ignore_index,
                                                    want_loss=True, want_labels=want_labels, want_dlogits=True, path=path, scale=scale)
        tgt = target if target.dtype == torch.int64 else target.long()
        inv_count = None
        if reduction == "mean":
            inv_count = head_valid_pixels(tgt, ignore_index, n_out).sum().float().reciprocal()
        ctx.save_for_backward(q, k_lr, pv_lr, g, *(() if inv_count is None else (inv_count,)))
        ctx.kernel_size, ctx.n_out, ctx.scale, ctx.has_bias, ctx.reduction = kernel_size, n_out, scale, bias is not None, reduction
        loss = reduce_head_loss(loss_map, tgt, ignore_index, n_out, reduction)
        if want_labels:
            ctx.mark_non_differentiable(labels)
            return loss, labels
        return loss

    @staticmethod
    def backward(ctx, dloss, *rest):
        q, k_lr, pv_lr, g = ctx.saved_tensors[:4]
        need_pv, need_b = ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3]
        N = ctx.n_out
        dpv = dbias = None
        if ctx.reduction == "none":
            g = (g.float() * dloss.unsqueeze(-1)).to(torch.bfloat16)
            factor = None
        else:
            factor = dloss.float() * ctx.saved_tensors[4] if ctx.reduction == "mean" else dloss.float()
        if need_b:
            dbias = g.float().sum(dim=(0, 1, 2))[:N]
            if factor is not None:
                dbias = dbias * factor
        if need_pv:
            dv = _head_values_grad(q, k_lr, pv_lr, g, ctx.kernel_size, ctx.scale)
            if factor is not None:
                dv = dv * factor
            dpv = dv.to(pv_lr.dtype)
        return (None, None, dpv, dbias) + (None,) * 8


# ---- ... or a dense regression objective in that epilogue's place (depth, flow, normals: L1 / MSE / smooth-L1, depth error statistics) ----
_REG_KINDS = ("l1", "mse", "smooth_l1")
HEAD_REG_MAX_N = 32                        # outputs the fused regression epilogue serves (naf_xna_head_reg_select)
DEFAULT_DEPTH_CLAMP = (1e-3, math.inf)


def _f32(v) -> float:
    """``v`` rounded to float32: what the kernel receives in a float field."""
    return C.c_float(float(v)).value


def _check_reg_kind(who: str, kind, beta) -> None:
    if kind not in _REG_KINDS:
        raise ValueError(f"{who}: the loss must be one of {_REG_KINDS}, got {kind!r}")
    if not float(beta) > 0.0:
        raise ValueError(f"{who}: beta must be > 0, got {beta!r}")


def _check_dense_target(who: str, target, shape, device) -> None:
    if not isinstance(target, torch.Tensor) or not target.dtype.is_floating_point:
        raise TypeError(f"{who}: the dense target must be a floating-point tensor, got {getattr(target, 'dtype', type(target).__name__)}")
    if tuple(target.shape) != tuple(shape):
        raise ValueError(f"{who}: the dense target must be [B, N, Ho, Wo] = {tuple(shape)}, got {tuple(target.shape)}")
    if target.device != device:
        raise ValueError(f"{who}: the dense target is on {target.device}, the features on {device}")


def _check_valid_mask(who: str, valid, shape, device) -> None:
    if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{who}: valid must be a bool or uint8 tensor, got {getattr(valid, 'dtype', type(valid).__name__)}")
    if tuple(valid.shape) != tuple(shape):
        raise ValueError(f"{who}: valid must be [B, Ho, Wo] = {tuple(shape)}, got {tuple(valid.shape)}")
    if valid.device != device:
        raise ValueError(f"{who}: valid is on {valid.device}, the features on {device}")


def _check_errors(who: str, errors, device) -> None:
    if not isinstance(errors, torch.Tensor) or errors.dtype != torch.float64:
        raise TypeError(f"{who}: errors must be a float64 [{_lib.HEAD_REG_STATS}] tensor, got {getattr(errors, 'dtype', type(errors).__name__)}")
    if tuple(errors.shape) != (_lib.HEAD_REG_STATS,) or not errors.is_contiguous():
        raise ValueError(f"{who}: errors must be a contiguous [{_lib.HEAD_REG_STATS}] tensor, got {tuple(errors.shape)}")
    if errors.device != device:
        raise ValueError(f"{who}: errors is on {errors.device}, the features on {device}")


def _check_clamp(who: str, clamp) -> Tuple[float, float]:
    lo, hi = (DEFAULT_DEPTH_CLAMP if clamp is None else clamp)
    lo, hi = _f32(lo), _f32(hi)
    if not lo > 0.0 or not hi >= lo:
        raise ValueError(f"{who}: clamp must be (lo, hi) with 0 < lo <= hi, got {clamp!r}")
    return lo, hi


def _regression_terms(r: torch.Tensor, kind: str, beta: float):
    """Elementwise loss and its derivative of the residual ``r``: (l(r), l'(r)), torch's definitions (``sign(0) = 0``)."""
    if kind == "l1":
        return r.abs(), torch.sign(r)
    if kind == "mse":
        return r * r, 2.0 * r
    a = r.abs()
    small = a < beta
    return torch.where(small, 0.5 * r * r / beta, a - 0.5 * beta), torch.where(small, r / beta, torch.sign(r))


def head_regression_from_logits(logits: torch.Tensor, target: torch.Tensor, valid: Optional[torch.Tensor] = None, kind: str = "l1",
                                beta: float = 1.0, *, want_loss: bool = False, want_dlogits: bool = False,
                                dlogits_channels: Optional[int] = None):
    """The regression epilogue of ``naf_xna_head_reg_fwd`` as torch ops on materialised logits [B, N, Ho, Wo] (any device, CPU included):
    what ``xna_head_regression`` composes where the kernel does not serve the call, with the same contract.  ``target`` [B, N, Ho, Wo]
    float, ``valid`` [B, Ho, Wo] bool / uint8 or None (every pixel valid; a pixel is valid for all N channels alike).  Returns
    ``(loss_map, dlogits)``, each None unless wanted: the sum over the channels of the elementwise loss (``kind``: "l1" ``|r|``, "mse"
    ``r * r``, "smooth_l1" torch's with ``beta``; ``r = z - target``) [B, Ho, Wo], 0 where the pixel is not valid -- float64 for float64
    logits, else float32, and differentiable with respect to the logits; and the derivative of that sum with respect to the logits, bf16
    channels-last [B, Ho, Wo, dlogits_channels], zero rows for invalid pixels and zero pad channels.  Values under an invalid pixel (NaN
    included) reach neither."""
    _check_reg_kind("head regression", kind, beta)
    B, N, Ho, Wo = logits.shape
    z = logits if logits.dtype == torch.float64 else logits.float()
    r = z - target.to(z.dtype)
    if valid is not None:
        r = torch.where((valid != 0).unsqueeze(1), r, torch.zeros_like(r))      # l(0) = l'(0) = 0 for the three losses
    loss = g = None
    if want_loss:
        loss = _regression_terms(r, kind, float(beta))[0].sum(dim=1)
    if want_dlogits:
        gc = int(dlogits_channels) if dlogits_channels is not None else head_dlogits_channels(N)
        if gc < N:
            raise ValueError(f"head regression: dlogits_channels {gc} smaller than the {N} outputs")
        d = _regression_terms(r.detach(), kind, float(beta))[1].permute(0, 2, 3, 1)
        g = torch.nn.functional.pad(d, (0, gc - N)).to(torch.bfloat16)
    return loss, g


def reduce_regression_loss(loss_map: torch.Tensor, valid: Optional[torch.Tensor], n_out: int, reduction: str) -> torch.Tensor:
    """``reduction`` of the per-pixel map of channel sums as ``F.l1_loss`` / ``F.mse_loss`` / ``F.smooth_l1_loss`` define it on the selected
    elements: "none" the map, "sum" its sum, "mean" the sum over (number of valid pixels * n_out) -- counted on the device without a host
    synchronisation; no valid pixel: nan, as an empty mean in torch."""
    if reduction == "none":
        return loss_map
    total = loss_map.sum()
    if reduction == "sum":
        return total
    return (total.double() / _regression_count(loss_map, valid, n_out)).to(total.dtype)


def _regression_count(loss_map: torch.Tensor, valid: Optional[torch.Tensor], n_out: int) -> torch.Tensor:
    """Number of selected elements (valid pixels * n_out) as a float64 device scalar: counted in int64, so exact at any batch size."""
    pixels = (valid != 0).sum() if valid is not None else torch.full((), loss_map.numel(), dtype=torch.int64, device=loss_map.device)
    return (pixels * int(n_out)).double()


def head_errors_from_prediction(pred: torch.Tensor, target: torch.Tensor, valid: Optional[torch.Tensor] = None,
                                clamp=None) -> torch.Tensor:
    """The ten error sums of ``naf_xna_head_reg_fwd`` as torch ops in float64 (any device, CPU included): ``pred`` and ``target``
    [B, 1, Ho, Wo] or [B, Ho, Wo], ``valid`` [B, Ho, Wo] bool / uint8 or None, ``clamp=(lo, hi)`` (default (1e-3, inf); the bounds are
    rounded to float32, as the kernel receives them).  With ``p = min(max(pred, lo), hi)`` a pixel is counted when it is valid,
    ``target > 0`` and ``target`` and ``pred`` are finite; with ``d = ln p - ln target`` the result is float64 [10]:
    ``n, sum |p - t|, sum (p - t)^2, sum |p - t| / t, sum (p - t)^2 / t, sum d, sum d^2`` and the numbers of pixels with
    ``max(p / t, t / p)`` below 1.25, 1.25^2, 1.25^3.  ``depth_metrics`` turns them into the usual depth figures."""
    lo, hi = _check_clamp("head_errors_from_prediction", clamp)
    z = (pred[:, 0] if pred.dim() == 4 else pred).double()
    t = (target[:, 0] if target.dim() == 4 else target).double()
    cnt = (t > 0) & torch.isfinite(t) & torch.isfinite(z)
    if valid is not None:
        cnt = cnt & (valid != 0)
    one = torch.ones_like(t)
    p = torch.where(cnt, z.clamp(lo, hi), one)
    t = torch.where(cnt, t, one)
    e, d, ratio = p - t, torch.log(p) - torch.log(t), torch.maximum(p / t, t / p)
    c = cnt.double()
    terms = (c, e.abs(), e * e, e.abs() / t, e * e / t, d, d * d, (ratio < 1.25).double(), (ratio < 1.25 ** 2).double(), (ratio < 1.25 ** 3).double())
    return torch.stack([(x * c).sum() for x in terms])


DepthMetrics = collections.namedtuple("DepthMetrics", ("mae", "rmse", "abs_rel", "sq_rel", "rmse_log", "silog", "d1", "d2", "d3", "n"))


def depth_metrics(acc: torch.Tensor) -> "DepthMetrics":
    """The usual depth-evaluation figures from the ten error sums (``naf(..., errors=acc)``, ``head_errors_from_prediction``), in float64
    on the accumulator's device, without a host synchronisation.  ``DepthMetrics(mae, rmse, abs_rel, sq_rel, rmse_log, silog, d1, d2, d3, n)``:
    means over the ``n`` counted pixels of ``|p - t|``, ``(p - t)^2`` (its root), ``|p - t| / t``, ``(p - t)^2 / t``, ``d^2`` (its root)
    with ``d = ln p - ln t``; ``silog = sqrt(mean d^2 - (mean d)^2)``; ``d1, d2, d3`` the shares of pixels with ``max(p / t, t / p)`` below
    1.25, 1.25^2, 1.25^3.  ``n == 0`` gives nan, as an empty mean does in torch."""
    if not isinstance(acc, torch.Tensor) or tuple(acc.shape) != (_lib.HEAD_REG_STATS,):
        raise ValueError(f"depth_metrics: the [{_lib.HEAD_REG_STATS}] error sums are expected, got "
                         f"{tuple(getattr(acc, 'shape', ())) if isinstance(acc, torch.Tensor) else type(acc).__name__}")
    a = acc.to(torch.float64)
    n = a[0]
    m = a[1:] / n
    var = (m[5] - m[4] * m[4]).clamp_min(0.0)         # rounding can leave a constant ratio's variance below zero; nan stays nan
    return DepthMetrics(m[0], m[1].sqrt(), m[2], m[3], m[5].sqrt(), var.sqrt(), m[6], m[7], m[8], n)


def xna_head_regression(q: torch.Tensor, k_lr: torch.Tensor, pv_lr: torch.Tensor, bias: Optional[torch.Tensor], kernel_size, *,
                        n_out: int, target: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None, kind: str = "l1",
                        beta: float = 1.0, want_loss: bool = False, want_dlogits: bool = False, return_logits: bool = False,
                        errors: Optional[torch.Tensor] = None, clamp=None, path: str = "auto", scale: Optional[float] = None,
                        rope_tables=None):
    """``xna_head_forward`` with a dense regression objective in the kernel's epilogue (``naf_xna_head_reg_fwd``): one launch gives any of
    the per-pixel loss, its gradient with respect to the logits, the logits and the error statistics of depth evaluation, without the
    [B, N, Ho, Wo] logits having to be written.

    Arguments as ``xna_head_forward``; ``target`` [B, n_out, Ho, Wo] float (any strides; other float dtypes are converted with
    ``.float()``), ``valid`` [B, Ho, Wo] bool / uint8 (any strides) or None.  Returns ``(loss_map, dlogits, logits)``, each None unless asked
    for, as ``head_regression_from_logits`` defines them: fp32 [B, Ho, Wo], 0 where invalid; bf16 [B, Ho, Wo, Gc] with
    ``Gc = head_dlogits_channels(n_out)``, every channel written, NOT divided by anything -- the ``dout`` the attention backward takes for
    all heads at once; fp32 logits as ``xna_head_forward(..., out_dtype=float32)`` returns them.  ``errors``: a float64 [10] device tensor
    the call ADDS the ten error sums to (``head_errors_from_prediction``; ``n_out == 1`` only), ``clamp=(lo, hi)`` the bounds of the
    prediction there (default (1e-3, inf)); bit-reproducible, no float atomics.  ``path="auto"`` composes
    ``xna_head_forward(..., out_dtype=float32)`` with ``head_regression_from_logits`` / ``head_errors_from_prediction`` where the kernel
    refuses (n_out > 32, geometry; same contract); ``path="fused"`` insists and raises; ``path="composed"`` is the A/B arm."""
    ky, kx, B, heads, Ho, Wo, Dq, h, w, npad, n_out = _check_head_operands("xna_head_regression", q, k_lr, pv_lr, bias, kernel_size, n_out, path)
    _check_reg_kind("xna_head_regression", kind, beta)
    if not (want_loss or want_dlogits or return_logits or errors is not None):
        raise ValueError("xna_head_regression: nothing asked for (want_loss / want_dlogits / return_logits / errors)")
    dev = q.device
    if (want_loss or want_dlogits or errors is not None) and target is None:
        raise ValueError("xna_head_regression: the loss, its gradient and the error statistics need a target")
    if target is not None:
        _check_dense_target("xna_head_regression", target, (B, n_out, Ho, Wo), dev)
        if target.dtype != torch.float32:
            target = target.float()
    if valid is not None:
        _check_valid_mask("xna_head_regression", valid, (B, Ho, Wo), dev)
        if valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
    lo, hi = _check_clamp("xna_head_regression", clamp)
    if errors is not None:
        if n_out != 1:
            raise ValueError(f"xna_head_regression: the error statistics are defined for one output channel, got n_out = {n_out}")
        _check_errors("xna_head_regression", errors, dev)
    lib = _lib.load()
    gc = head_dlogits_channels(n_out)
    if path != "composed" and (n_out <= 256 or path == "fused"):
        out = torch.empty((B, Ho, Wo, n_out), dtype=torch.float32, device=dev) if return_logits else None
        loss = torch.empty((B, Ho, Wo), dtype=torch.float32, device=dev) if want_loss else None
        g = torch.empty((B, Ho, Wo, gc), dtype=torch.bfloat16, device=dev) if want_dlogits else None     # the kernel writes every channel
        a = _lib.XnaHeadRegArgs()
        a.head = _fill_xna_head(q, k_lr, pv_lr, bias, out if out is not None else q, n_out, ky, kx, path, scale, rope_tables)
        if out is None:
            a.head.out, a.head.out_dtype = None, _lib.NAF_F32
        a.kind, a.beta, a.dlogits_channels, a.clamp_lo, a.clamp_hi = _lib.HEAD_REG_KINDS[kind], float(beta), gc, lo, hi
        if target is not None:
            a.target, a.t_stride = target.data_ptr(), _strides4(target, (0, 1, 2, 3))
        for t, ptr, st in ((valid, "valid", "valid_stride"), (loss, "loss", "loss_stride"), (g, "dlogits", "dlogits_stride")):
            if t is not None:
                setattr(a, ptr, t.data_ptr())
                setattr(a, st, _strides3(t))
        ws = None
        if errors is not None:
            a.errors = errors.data_ptr()
        sel = lib.naf_xna_head_reg_select(C.byref(a))
        if sel == _lib.XNA_HEAD_FUSED:
            if errors is not None:
                nbytes = int(lib.naf_xna_head_reg_workspace_bytes(C.byref(a)))
                ws = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.float64, device=dev)
                a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
            with torch.cuda.device(dev), _Timed("xna_head_reg"):
                rc = lib.naf_xna_head_reg_fwd(C.byref(a), _stream(q))
            _lib.check(rc, "naf_xna_head_reg_fwd")
            return loss, g, (None if out is None else out.permute(0, 3, 1, 2))
        if path == "fused" or sel == -1:       # insisted, or arguments no kernel serves
            _lib.check(-sel, "naf_xna_head_reg_select")
        del out, loss, g
    with _Timed("xna_head_reg_composed"):
        logits = xna_head_forward(q, k_lr, pv_lr, bias, (ky, kx), n_out=n_out, out_dtype=torch.float32,
                                  path="auto" if path == "auto" else "composed", scale=scale, rope_tables=rope_tables)
        loss = g = None
        if want_loss or want_dlogits:
            loss, g = head_regression_from_logits(logits, target, valid, kind, beta, want_loss=want_loss, want_dlogits=want_dlogits,
                                                  dlogits_channels=gc)
        if errors is not None:
            errors.add_(head_errors_from_prediction(logits, target, valid, (lo, hi)))
        return loss, g, (logits if return_logits else None)


class XnaHeadRegFunction(torch.autograd.Function):
    """Differentiable dense regression loss of the head-summed attention's logits, with respect to the head (``pv_lr`` and ``bias`` only, as
    ``XnaHeadCEFunction``): the forward is ONE launch (``xna_head_regression``) that leaves the loss map and its gradient ``g`` (bf16, the
    attention backward's width, unnormalised); the backward hands ``g`` to ``xna_backward`` as the ``dout`` of every head (stride 0) and
    scales the low-res result by the incoming gradient and, for "mean", by 1 / (number of valid pixels * n_out), a device scalar (no host
    synchronisation) -- the backward is linear in ``g``.  ``dbias = sum over pixels of g`` times the same.  reduction="none": the incoming
    gradient is a map, ``g`` is scaled per pixel first and rounded to bf16 a SECOND time (the attention backward reads bf16): exact for an
    incoming map of ones or powers of two, one more 2^-9 relative rounding for a general map -- ``g`` itself is rounded once only in the
    forward and for "mean" / "sum".  Returns the reduced loss, or ``(loss, logits)`` with ``return_logits`` (fp32
    [B, n_out, Ho, Wo], without a gradient).  ``q`` holds materialised (rotated) queries."""

    @staticmethod
    def forward(ctx, q, k_lr, pv_lr, bias, target, valid, kernel_size, n_out, kind="l1", beta=1.0, reduction="mean", return_logits=False,
                path="auto", scale=None):
        if reduction not in _REDUCTIONS:
            raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
        n_out = int(n_out)
        loss_map, g, logits = xna_head_regression(q, k_lr, pv_lr, bias, kernel_size, n_out=n_out, target=target, valid=valid, kind=kind,
                                                  beta=beta, want_loss=True, want_dlogits=True, return_logits=return_logits, path=path,
                                                  scale=scale)
        inv_count = None
        if reduction == "mean":
            inv_count = _regression_count(loss_map, valid, n_out).reciprocal().float()      # exact count, one rounding
        ctx.save_for_backward(q, k_lr, pv_lr, g, *(() if inv_count is None else (inv_count,)))
        ctx.kernel_size, ctx.n_out, ctx.scale, ctx.has_bias, ctx.reduction = kernel_size, n_out, scale, bias is not None, reduction
        loss = reduce_regression_loss(loss_map, valid, n_out, reduction)
        if return_logits:
            ctx.mark_non_differentiable(logits)
            return loss, logits
        return loss

    @staticmethod
    def backward(ctx, dloss, *rest):
        q, k_lr, pv_lr, g = ctx.saved_tensors[:4]
        need_pv, need_b = ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3]
        N = ctx.n_out
        dpv = dbias = None
        if ctx.reduction == "none":
            g = (g.float() * dloss.unsqueeze(-1)).to(torch.bfloat16)
            factor = None
        else:
            factor = dloss.float() * ctx.saved_tensors[4] if ctx.reduction == "mean" else dloss.float()
        if need_b:
            dbias = g.float().sum(dim=(0, 1, 2))[:N]
            if factor is not None:
                dbias = dbias * factor
        if need_pv:
            dv = _head_values_grad(q, k_lr, pv_lr, g, ctx.kernel_size, ctx.scale)
            if factor is not None:
                dv = dv * factor
            dpv = dv.to(pv_lr.dtype)
        return (None, None, dpv, dbias) + (None,) * 10


# ---- ... and the same objective on the cosine head's scaled cosines (cosine classifier, prompt tuning, learnable temperature) ----------
def project_cosine_values(embeddings: torch.Tensor, v_lr: torch.Tensor) -> torch.Tensor:
    """The low-res half of the cosine head: ``PV_g = E^[:, g*Dv:(g+1)*Dv] @ V_g`` with ``E^ = normalize_embeddings(E)`` for v_lr
    [B, heads, h, w, Dv] -> pv5 [B, heads, h, w, Npad] bf16 with zero pad channels.  Pure torch and differentiable: this is where the
    embeddings' gradient enters autograd (``XnaCosCEFunction`` returns the gradient of pv5)."""
    e_hat = normalize_embeddings(embeddings)
    _, heads, _, _, Dv = v_lr.shape
    N = e_hat.shape[0]
    pv = torch.einsum("ngd,bghwd->bghwn", e_hat.reshape(N, heads, Dv), v_lr.float())
    pad = head_npad(N) - N
    return (torch.nn.functional.pad(pv, (0, pad)) if pad else pv).to(torch.bfloat16)


def _check_logit_scale(who: str, logit_scale, device):
    """-> (float for the struct, 1-element fp32 device tensor or None).  A tensor is read by the kernel through a pointer: no host sync."""
    if isinstance(logit_scale, torch.Tensor):
        if logit_scale.numel() != 1 or logit_scale.dtype != torch.float32:
            raise ValueError(f"{who}: a logit_scale tensor must hold one float32 value, got {tuple(logit_scale.shape)} {logit_scale.dtype}")
        if logit_scale.device != device:
            raise ValueError(f"{who}: logit_scale is on {logit_scale.device}, the features on {device}")
        return 1.0, logit_scale.detach()
    if not math.isfinite(float(logit_scale)):
        raise ValueError(f"{who}: logit_scale must be finite, got {logit_scale}")
    return float(logit_scale), None


def xna_cos_ce_select(q: torch.Tensor, lr_size, Dv: int, n_out: int, kernel_size, *, value_dtype: torch.dtype = torch.bfloat16,
                      rope_tables=None) -> str:
    """Which route ``xna_cos_objective(path="auto")`` takes for these shapes: "fused" (``naf_xna_cos_ce_select`` grants the kernel) or
    "composed".  Arguments and conventions as ``xna_cos_select``; a host-side query, CPU / meta tensors do."""
    if q.dtype != torch.bfloat16 or q.dim() != 5 or q.stride(4) != 1 or value_dtype != torch.bfloat16 or not 1 <= int(n_out) <= 256 or int(Dv) < 1:
        return "composed"
    a = _lib.XnaCosCEArgs()
    return _head_route(a.cos, "naf_xna_cos_ce_select", q, lr_size, n_out, kernel_size, rope_tables, Dv=int(Dv), outer=a)


def cosine_objective_from_features(f: torch.Tensor, e_hat: torch.Tensor, logit_scale=1.0, target: Optional[torch.Tensor] = None,
                                   ignore_index: int = -100, *, want_loss: bool = False, want_labels: bool = False,
                                   want_dlogits: bool = False, want_dscale: bool = False, dlogits_channels: Optional[int] = None):
    """The classification epilogue of ``naf_xna_cos_ce_fwd`` as torch ops on a materialised feature map f [B, C, H, W] (any device): what
    ``xna_cos_objective`` composes where the kernel does not serve the call, same contract.  ``e_hat``: normalised rows [N, C] fp32;
    ``logit_scale``: a float or a 1-element tensor.  Returns ``(loss_map, labels, dlogits, dscale)``, each None unless wanted: with
    ``c = cosines``, ``z = s * c`` and ``d = softmax(z) - onehot(t)`` -- ``logsumexp(z) - z[t]`` [B, H, W] fp32; ``argmax z`` (uint8 up to
    256 classes); ``(s / max(||f||, 1e-12)) * d`` bf16 channels-last [B, H, W, dlogits_channels] with zero pad channels; ``sum_n d * c``
    [B, H, W] fp32.  Ignored pixels (``head_valid_pixels``) have loss 0 and zero ``dlogits`` / ``dscale``; a pixel with ``||f|| = 0`` has a zero
    ``dlogits`` row (its exact gradient: every cosine is 0 whatever the embeddings)."""
    ff = f.float().permute(0, 2, 3, 1)
    nrm = ff.norm(dim=3)
    inv = 1.0 / nrm.clamp_min(1e-12)
    c = torch.matmul(ff * inv.unsqueeze(3), e_hat.t())
    s = logit_scale.detach().reshape(()).float() if isinstance(logit_scale, torch.Tensor) else float(logit_scale)
    z = c * s
    N = e_hat.shape[0]
    if (want_loss or want_dlogits or want_dscale) and target is None:
        raise ValueError("cosine objective: the loss and the gradients need a target")
    loss = labels = g = ds = None
    if want_labels:
        labels = z.argmax(dim=3)
        if N <= 256:
            labels = labels.to(torch.uint8)
    if want_loss or want_dlogits or want_dscale:
        valid = head_valid_pixels(target, ignore_index, N)
        tc = torch.where(valid, target, torch.zeros_like(target))
        lse = torch.logsumexp(z, dim=3)
        if want_loss:
            loss = torch.where(valid, lse - z.gather(3, tc.unsqueeze(3))[..., 0], torch.zeros_like(lse))
        if want_dlogits or want_dscale:
            d = (torch.exp(z - lse.unsqueeze(3)) - torch.nn.functional.one_hot(tc, N).to(z.dtype)) * valid.unsqueeze(3).to(z.dtype)
            if want_dscale:
                ds = (d * c).sum(dim=3)
            if want_dlogits:
                gc = int(dlogits_channels) if dlogits_channels is not None else head_dlogits_channels(N)
                if gc < N:
                    raise ValueError(f"cosine objective: dlogits_channels {gc} smaller than the {N} classes")
                gf = torch.where(nrm > 0, inv * s, torch.zeros_like(inv))
                g = torch.nn.functional.pad(d * gf.unsqueeze(3), (0, gc - N)).to(torch.bfloat16)
    return loss, labels, g, ds


def xna_cos_objective(q: torch.Tensor, k_lr: torch.Tensor, v_lr: torch.Tensor, embeddings: torch.Tensor, kernel_size, *,
                      target: Optional[torch.Tensor] = None, ignore_index: int = -100, logit_scale=1.0, want_loss: bool = False,
                      want_labels: bool = False, want_dlogits: bool = False, want_dscale: bool = False, path: str = "auto",
                      scale: Optional[float] = None, rope_tables=None, pv_lr: Optional[torch.Tensor] = None):
    """``xna_cos_forward`` with a classification objective on the scaled cosines in the kernel's epilogue (``naf_xna_cos_ce_fwd``): one launch
    gives any of the per-pixel cross-entropy, the argmax labels and the two gradients, and neither the [B, C, Ho, Wo] features nor the
    [B, N, Ho, Wo] cosines are written.  No graph is recorded here (``XnaCosCEFunction`` is the differentiable form).

    Operands as ``xna_cos_forward``; ``target`` integer [B, Ho, Wo] (any strides; converted to int64), needed for everything but the labels;
    ``logit_scale`` a float or a 1-element fp32 device tensor (read by the kernel through a pointer: no host synchronisation).  Returns
    ``(loss_map, labels, dlogits, dscale)``, each None unless asked for, with ``inv = 1 / max(||f||, 1e-12)``, ``c`` the cosines, ``z = s * c``:
    fp32 [B, Ho, Wo] ``logsumexp(z) - z[t]``, 0 where the pixel is ignored; uint8 [B, Ho, Wo] (int64 beyond 256 embeddings), the lowest index
    among equal maxima, written for ignored pixels too; bf16 [B, Ho, Wo, Gc] ``g' = (s * inv) * (softmax(z) - onehot(t))`` with
    ``Gc = head_dlogits_channels(N)``, every channel written, NOT divided by the number of valid pixels -- the gradient with respect to
    ``E^ . f`` before the division by the norm, i.e. the ``dout`` the attention backward takes for the projected values of all heads at
    once (``_head_values_grad``); fp32 [B, Ho, Wo] ``ds = sum_n (softmax(z) - onehot(t))[n] * c[n]``, whose sum is dloss / ds.  Ignored pixels
    (``target == ignore_index`` or outside [0, N)) have zero ``g'`` and ``ds``; so has, for ``g'``, a pixel whose feature is zero.
    ``pv_lr``: the projected values ``project_cosine_values(embeddings, v_lr)`` when the caller has formed them (with a graph).
    ``path="auto"``: the kernel where ``naf_xna_cos_ce_select`` grants it and the values are bf16, else the composition -- the plain forward and
    ``cosine_objective_from_features`` as torch ops, same contract; ``"fused"`` insists and raises NafHipError; ``"composed"`` insists on the
    composition."""
    e_hat, (B, heads, Ho, Wo, Dq, h, w, Dv) = _check_cos_operands("xna_cos_objective", q, k_lr, v_lr, embeddings, path)
    ky, kx = _ksize(kernel_size)
    N = e_hat.shape[0]
    if not (want_loss or want_labels or want_dlogits or want_dscale):
        raise ValueError("xna_cos_objective: nothing asked for (want_loss / want_labels / want_dlogits / want_dscale)")
    dev = q.device
    ls, ls_t = _check_logit_scale("xna_cos_objective", logit_scale, dev)
    needs_target = want_loss or want_dlogits or want_dscale
    if needs_target and target is None:
        raise ValueError("xna_cos_objective: the loss and the gradients need a target")
    if target is not None:
        target = _check_target(target, (B, Ho, Wo), dev, "xna_cos_objective")
    gc = head_dlogits_channels(N)
    lib = _lib.load()
    with torch.no_grad():
        if path != "composed" and (path == "fused" or (v_lr.dtype == torch.bfloat16 and N <= 256)):
            if v_lr.dtype != torch.bfloat16:
                raise _lib.NafHipError(f"xna_cos_objective: the fused kernel needs bfloat16 values, got {v_lr.dtype}")
            pv5 = pv_lr.detach() if pv_lr is not None else project_cosine_values(embeddings, v_lr)
            if tuple(pv5.shape) != (B, heads, h, w, head_npad(N)) or pv5.dtype != torch.bfloat16:
                raise ValueError(f"xna_cos_objective: pv_lr must be bfloat16 {(B, heads, h, w, head_npad(N))}, got {pv5.dtype} {tuple(pv5.shape)}")
            loss = torch.empty((B, Ho, Wo), dtype=torch.float32, device=dev) if want_loss else None
            labels = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev) if want_labels else None
            g = torch.empty((B, Ho, Wo, gc), dtype=torch.bfloat16, device=dev) if want_dlogits else None     # the kernel writes every channel
            ds = torch.empty((B, Ho, Wo), dtype=torch.float32, device=dev) if want_dscale else None
            a = _lib.XnaCosCEArgs()
            a.cos = _fill_xna_cos(q, k_lr, pv5, v_lr, q, None, N, ky, kx, path, scale, ls, rope_tables)
            a.cos.out = None
            a.cos.o_stride = I64x3(0, 0, 0)
            a.ignore_index, a.dlogits_channels = int(ignore_index), gc
            if ls_t is not None:
                a.logit_scale_ptr = ls_t.data_ptr()
            for t, ptr, st in ((target if needs_target else None, "target", "t_stride"), (loss, "loss", "loss_stride"),
                               (labels, "labels", "labels_stride"), (g, "dlogits", "dlogits_stride"), (ds, "dscale", "dscale_stride")):
                if t is not None:
                    setattr(a, ptr, t.data_ptr())
                    setattr(a, st, _strides3(t))
            sel = lib.naf_xna_cos_ce_select(C.byref(a))
            if sel == _lib.XNA_HEAD_FUSED:
                with torch.cuda.device(dev), _Timed("xna_cos_ce"):
                    rc = lib.naf_xna_cos_ce_fwd(C.byref(a), _stream(q))
                _lib.check(rc, "naf_xna_cos_ce_fwd")
                return loss, labels, g, ds
            if path == "fused" or sel == -1:       # insisted, or arguments no kernel serves
                _lib.check(-sel, "naf_xna_cos_ce_select")
            del loss, labels, g, ds, pv5
        with _Timed("xna_cos_ce_composed"):
            odt = v_lr.dtype if v_lr.dtype in (torch.bfloat16, torch.float16) else torch.float32
            o5 = xna_forward(q, k_lr, v_lr if v_lr.dtype in (torch.bfloat16, torch.float16) else v_lr.to(torch.bfloat16), (ky, kx),
                             out_dtype=odt, path="auto", scale=scale, rope_tables=rope_tables)
            f = o5.permute(0, 1, 4, 2, 3).reshape(B, heads * Dv, Ho, Wo)
            loss, labels, g, ds = cosine_objective_from_features(f, e_hat, ls_t if ls_t is not None else ls, target, ignore_index,
                                                                 want_loss=want_loss, want_labels=want_labels, want_dlogits=want_dlogits,
                                                                 want_dscale=want_dscale, dlogits_channels=gc)
            return loss, labels, g, ds


class XnaCosCEFunction(torch.autograd.Function):
    """Differentiable cross-entropy of the cosine head's scaled cosines, with respect to the projected values ``pv_lr`` (and through them the
    embeddings) and the logit scale -- the queries, keys and values come from a frozen upsampler, as for ``XnaHeadCEFunction``, which this
    mirrors.  The forward is ONE launch (``xna_cos_objective``) that leaves the loss map, ``g'`` (bf16, the attention backward's width,
    unnormalised) and the ``ds`` map; the backward hands ``g'`` to ``xna_backward`` as the ``dout`` of every head (stride 0) and scales the
    low-res result by the incoming gradient and, for "mean", by 1 / number of valid pixels; ``dscale.sum()`` times the same factor is the
    gradient of a ``logit_scale`` tensor.  reduction="none": the incoming gradient is a map, ``g'`` and ``ds`` are scaled per pixel first.
    ``pv_lr = project_cosine_values(embeddings, v_lr)`` is formed by the caller WITH the graph on: autograd carries its gradient to the
    embeddings through the low-res product and the normalisation.  ``embeddings`` itself gets no gradient from this function (the
    composed route needs its values).  Returns the reduced loss, or ``(loss, labels)`` with ``want_labels``.  ``q`` holds materialised (rotated)
    queries.  Not here: a gradient for q, k_lr or v_lr, class weights, label smoothing, soft targets."""

    @staticmethod
    def forward(ctx, q, k_lr, pv_lr, v_lr, embeddings, logit_scale, target, kernel_size, ignore_index=-100, reduction="mean",
                want_labels=False, path="auto", scale=None):
        if reduction not in _REDUCTIONS:
            raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
        scale_grad = isinstance(logit_scale, torch.Tensor) and ctx.needs_input_grad[5]
        loss_map, labels, g, ds = xna_cos_objective(q, k_lr, v_lr, embeddings.detach(), kernel_size, target=target, ignore_index=ignore_index,
                                                    logit_scale=logit_scale, want_loss=True, want_labels=want_labels, want_dlogits=True,
                                                    want_dscale=scale_grad, path=path, scale=scale, pv_lr=pv_lr)
        n_out = embeddings.shape[0]
        tgt = target if target.dtype == torch.int64 else target.long()
        saved = [q, k_lr, pv_lr, g]
        ctx.has_ds = ds is not None
        if ds is not None:
            saved.append(ds)
        if reduction == "mean":
            saved.append(head_valid_pixels(tgt, ignore_index, n_out).sum().float().reciprocal())
        ctx.save_for_backward(*saved)
        ctx.kernel_size, ctx.scale, ctx.reduction = kernel_size, scale, reduction
        ctx.ls_shape = tuple(logit_scale.shape) if isinstance(logit_scale, torch.Tensor) else None
        loss = reduce_head_loss(loss_map, tgt, ignore_index, n_out, reduction)
        if want_labels:
            ctx.mark_non_differentiable(labels)
            return loss, labels
        return loss

    @staticmethod
    def backward(ctx, dloss, *rest):
        q, k_lr, pv_lr, g = ctx.saved_tensors[:4]
        ds = ctx.saved_tensors[4] if ctx.has_ds else None
        dpv = dls = None
        if ctx.reduction == "none":
            g = (g.float() * dloss.unsqueeze(-1)).to(torch.bfloat16)
            factor = None
        else:
            factor = dloss.float() * ctx.saved_tensors[-1] if ctx.reduction == "mean" else dloss.float()
        if ds is not None:
            dls = ((ds * dloss).sum() if factor is None else ds.sum() * factor).reshape(ctx.ls_shape)
        if ctx.needs_input_grad[2]:
            dv = _head_values_grad(q, k_lr, pv_lr, g, ctx.kernel_size, ctx.scale)
            if factor is not None:
                dv = dv * factor
            dpv = dv.to(pv_lr.dtype)
        return (None, None, dpv, None, None, dls) + (None,) * 7


def xna_rope_fusable(q: torch.Tensor, lr_size, Dv: int, kernel_size, rope_tables, out_dtype=torch.bfloat16,
                     path: str = "auto") -> bool:
    """True when ``xna_forward(q, ..., rope_tables=...)`` can rotate the queries on load for these shapes (MFMA path,
    Wo/w a multiple of 16).  ``q``: the un-rotated guidance as a 5-D [B, heads, Ho, Wo, Dq] bf16 view."""
    if q.dtype != torch.bfloat16 or q.dim() != 5 or q.stride(4) != 1 or out_dtype not in _DT_VALUES:
        return False
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, Dq = q.shape
    h, w = int(lr_size[0]), int(lr_size[1])
    a = XnaArgs()
    a.q = a.k_lr = a.v_lr = a.out = q.data_ptr()      # shape / alignment query only: nothing is dereferenced
    a.rope_tab_y, a.rope_tab_x = rope_tables[0].data_ptr(), rope_tables[1].data_ptr()
    _fill_geometry(a, q, None, h, w, ky, kx, None)
    a.Dv, a.out_dtype, a.path = int(Dv), _DT_VALUES[out_dtype], _PATH[path]
    a.k_stride, a.v_stride, a.o_stride = _dense5(h, w, heads, Dq), _dense5(h, w, heads, Dv), _dense5(Ho, Wo, heads, Dv)
    return lib.naf_xna_select(C.byref(a)) == _lib.XNA_MFMA


def xna_select(q, k_lr, v_lr, kernel_size, out_dtype=torch.bfloat16, return_logits=False, path="auto") -> str:
    """Name of the kernel ``xna_forward`` would dispatch to ('mfma' / 'generic') -- for tests / bench."""
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, Dq = q.shape
    Dv = v_lr.shape[-1]
    out = torch.empty((1, 1, 1, heads, Dv), dtype=out_dtype, device=q.device).permute(0, 3, 1, 2, 4)
    fake = torch.empty((1,), dtype=torch.float32, device=q.device) if return_logits else None
    a = _fill_xna(q, k_lr, v_lr, out, fake, None, None, ky, kx, path, None)
    a.o_stride = _dense5(Ho, Wo, heads, Dv)
    sel = lib.naf_xna_select(C.byref(a))
    if sel < 0:
        _lib.check(-sel, "naf_xna_select")
    return _PATH_NAME[sel]


def xna_union_plan(q, k_lr, v_lr, kernel_size) -> Optional[Dict[str, int]]:
    """The workgroup plan of the table-driven MFMA kernel for these operands (``naf_xna_union_plan``), or None where it does not serve
    them: slots per window row ``wt``, output rows ``ry`` and pixels ``seg`` per workgroup, the staged rectangle ``hub`` x ``wub``, value
    channels per workgroup ``dvt``, LDS bytes ``lds`` -- for tools and tests."""
    lib = _lib.load()
    ky, kx = _ksize(kernel_size)
    B, heads, Ho, Wo, _ = q.shape
    Dv = v_lr.shape[-1]
    a = _fill_xna(q, k_lr, v_lr, q, None, None, None, ky, kx, "auto", None)
    a.out_dtype = _lib.NAF_BF16
    a.o_stride = _dense5(Ho, Wo, heads, Dv)
    out = (C.c_int32 * 7)()
    if lib.naf_xna_union_plan(C.byref(a), out) != 1:
        return None
    return dict(zip(("wt", "ry", "seg", "hub", "wub", "dvt", "lds"), (int(x) for x in out)))


# ------------------------------------------------------------------------------------------------
class _AuxPool:
    """The ``naf_forward_aux`` objects (a second stream and the fork / join events) this host LENDS to ``naf_forward_ex``.  The
    library owns none (C ABI 0.4.0): one per (host thread, device, caller stream), so concurrent forwards never share fork / join
    events and a hipGraph capture pulls in a stream nothing else uses.  The sixteen most recently used are kept; a bundle that is
    lent out at the moment (``lease``: inside a ``naf_forward_ex`` call of some thread) is never the one that is destroyed."""
    LIMIT = 16

    def __init__(self):
        self._by_key: Dict[tuple, list] = {}      # key -> [ForwardAux, leases outstanding]
        self._lock = threading.Lock()

    def _entry(self, device_index: int, stream_handle: int) -> list:      # caller holds the lock
        key = (threading.get_ident(), device_index, stream_handle)
        ent = self._by_key.pop(key, None)
        if ent is None:
            lib = _lib.load()
            idle = [k for k, e in self._by_key.items() if e[1] == 0]
            while len(self._by_key) >= self.LIMIT and idle:
                old = self._by_key.pop(idle.pop(0))                         # least recently used idle one (dicts keep insertion order)
                lib.naf_forward_aux_destroy(C.byref(old[0]))                # work already queued on a destroyed stream still completes
            aux = _lib.ForwardAux()
            with torch.cuda.device(device_index):
                _lib.check(lib.naf_forward_aux_create(C.byref(aux)), "naf_forward_aux_create")
            ent = [aux, 0]
        self._by_key[key] = ent
        return ent

    def get(self, device_index: int, stream_handle: int) -> "_lib.ForwardAux":
        with self._lock:
            return self._entry(device_index, stream_handle)[0]

    @contextlib.contextmanager
    def lease(self, device_index: int, stream_handle: int):
        """The bundle of (this thread, device, stream) for the duration of one foreign call."""
        with self._lock:
            ent = self._entry(device_index, stream_handle)
            ent[1] += 1
        try:
            yield ent[0]
        finally:
            with self._lock:
                ent[1] -= 1

    def clear(self) -> None:
        with self._lock:
            lib = _lib.load()
            for k in [k for k, e in self._by_key.items() if e[1] == 0]:
                lib.naf_forward_aux_destroy(C.byref(self._by_key.pop(k)[0]))


AUX_POOL = _AuxPool()


def forward_aux(device, stream=None) -> "_lib.ForwardAux":
    """The second-stream bundle ``ForwardPlan.run`` lends to the library for forwards issued by this thread on ``stream`` (default:
    the current one) of ``device``.  Call it BEFORE a hipGraph capture on that stream so that nothing is created while capturing."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    st = stream if stream is not None else torch.cuda.current_stream(idx)
    return AUX_POOL.get(idx, int(st.cuda_stream))


class ForwardPlan:
    """Argument block of ``naf_forward`` (the whole forward in ONE foreign call) for fixed parameters and shapes.
    Built once per (parameter versions, shapes); ``run`` only swaps the image / features / output pointers."""

    def __init__(self, branches, nlayer: int, gn_eps: float, tabs, image: torch.Tensor, features: torch.Tensor,
                 heads: int, ksize: int, out_dtype: torch.dtype, scale: Optional[float], output_size=None, heads_rope: int = 0):
        lib = _lib.load()
        B, _, H, W = image.shape
        Ho, Wo = (int(output_size[0]), int(output_size[1])) if output_size is not None else (H, W)
        _, Cc, h, w = features.shape
        a = ForwardArgs()
        a.tab_y, a.tab_x = tabs[0].data_ptr(), tabs[1].data_ptr()
        a.nlayer = nlayer
        a.image_dtype, a.feat_dtype, a.out_dtype = _DT[image.dtype], _DT_VALUES[features.dtype], _DT_VALUES[out_dtype]     # float16: both or neither
        a.B, a.H, a.W, a.h, a.w, a.C, a.heads, a.ksize = B, H, W, h, w, Cc, heads, ksize
        a.Ho, a.Wo = Ho, Wo
        a.heads_rope = int(heads_rope)
        a.gn_eps = float(gn_eps)
        a.scale = float(scale) if scale else 0.0
        self._keep = [tabs]
        for br, (w0, b0, k0, kb, layers) in enumerate(branches):
            sb = a.branch[br]
            sb.conv0_weight, sb.conv0_bias, sb.conv0_ksize, sb.ksize = w0.data_ptr(), b0.data_ptr(), k0, kb
            self._keep += [w0, b0]
            for l, (gw, gb, wp, cb) in enumerate(layers):
                sb.gn_weight[l], sb.gn_bias[l] = gw.data_ptr(), gb.data_ptr()
                sb.conv_weight_packed[l], sb.conv_bias[l] = wp.data_ptr(), cb.data_ptr()
                self._keep += [gw, gb, wp, cb]
        a.image_stride = _strides4(image, (0, 1, 2, 3))
        a.feat_stride = _strides4(features, (0, 1, 2, 3))
        # shape / alignment query with placeholder pointers (nothing is dereferenced)
        a.image, a.features, a.out = image.data_ptr(), features.data_ptr(), image.data_ptr() & ~0xFF
        self.supported = lib.naf_forward_supported(C.byref(a)) == 1
        self.args, self.lib = a, lib
        self.out_dtype, self.shape_out = out_dtype, (B, Ho, Wo, Cc)
        self.ws_bytes = int(lib.naf_forward_workspace_bytes(C.byref(a))) if self.supported else 0
        # a forward that runs on ONE stream never touches the fourth activation buffer (C ABI 0.4.2: a quarter of the workspace at 1024^2)
        self.ws_bytes_one = int(lib.naf_forward_workspace_bytes_ex(C.byref(a), _lib.FWD_ONE_STREAM)) if self.supported else 0
        self._planned = {}
        self.key = (tuple(image.shape), tuple(image.stride()), image.dtype, tuple(features.shape), tuple(features.stride()), features.dtype,
                    (Ho, Wo))

    WS_POOL_BYTES = 8 << 30
    streams = 0            # 0: the library's plan (naf_forward_streams), 1: one stream, 2: two whenever possible
    conv0_exact = False    # NAF_FWD_CONV0_EXACT: exact fp32 products in the 3x3 first convolution (default: 16 mantissa bits)

    def planned_streams(self) -> int:
        """How many streams ``run`` will use (2 = the branches side by side on the lent stream)."""
        st = int(self.streams)
        if st not in self._planned:          # a pure function of the geometry and the flag: asked once
            flags = {0: 0, 1: _lib.FWD_ONE_STREAM, 2: _lib.FWD_TWO_STREAMS}[st]
            self._planned[st] = int(self.lib.naf_forward_streams(C.byref(self.args), flags))
        return self._planned[st]

    def release_workspaces(self, keep_stream: Optional[int] = None) -> None:
        """Drop the plan's scratch buffers (all of them, or all but the one of raw stream handle ``keep_stream``).  Safe once
        the work queued on those streams has been synchronised with; a captured graph keeps its own workspace alive itself."""
        pool = self.__dict__.get("_ws_by_stream", {})
        for k in [k for k in pool if keep_stream is None or k[1] != keep_stream]:
            del pool[k]
        if keep_stream is None:
            self._ws = None

    def view(self, which: str) -> torch.Tensor:
        """A tensor VIEW of an intermediate of the last ``run`` inside its workspace (naf_forward_workspace_view): ``"guidance"`` bf16
        [B, Ho, Wo, 256] (un-rotated), ``"keys"`` bf16 [B, h, w, 256], ``"values"`` bf16 [B, h, w, C].  Valid until the next run on
        that workspace; synchronise with the stream of the run before reading it on another one."""
        ws = self.__dict__.get("_ws")
        if ws is None:
            raise RuntimeError("ForwardPlan.view: no forward has run on this plan (or its workspace was released)")
        a = self.args
        code = {"guidance": 0, "keys": 1, "values": 2}[which]
        off, nbytes = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self.lib.naf_forward_workspace_view(C.byref(a), code, C.byref(off), C.byref(nbytes)), "naf_forward_workspace_view")
        B, Ho, Wo, _ = self.shape_out
        shape = {"guidance": (B, Ho, Wo, 256), "keys": (B, a.h, a.w, 256), "values": (B, a.h, a.w, a.C)}[which]
        dt = torch.float16 if (which == "values" and a.feat_dtype == _lib.NAF_F16) else torch.bfloat16     # half features are packed as half
        return ws[off.value: off.value + nbytes.value].view(dt).view(shape)

    def release_stream(self, device_index: int, stream_handle: int) -> None:
        """Drop the scratch buffer of ONE (device, raw stream handle) -- a throw-away stream's -- once its work has been synchronised with."""
        ws = self.__dict__.get("_ws_by_stream", {}).pop((device_index, stream_handle), None)
        if ws is not None and self.__dict__.get("_ws") is ws:
            self._ws = None

    def run(self, image: torch.Tensor, features: torch.Tensor, events=None, return_logits: bool = False, phase_events=None):
        a = self.args
        dev = image.device
        # the workspace belongs to the plan (one allocation per geometry, not per call) -- one per (device, stream) the plan has
        # been run on (round 3: forwards of one module on two streams no longer share scratch; the four most recent are kept).
        # Host-side state (the argument struct) is still per plan: calls from several THREADS need a module each.
        # Memory: a workspace is ~1 GB at 1024^2 and several GB at 2048^2, so the pool is bounded in BYTES too (WS_POOL_BYTES,
        # default 8 GiB: at least the current stream's workspace always stays); ``release_workspaces()`` drops all of them.
        skey = (dev.index, int(torch.cuda.current_stream(dev).cuda_stream))
        pool = self.__dict__.setdefault("_ws_by_stream", {})
        one = self.planned_streams() == 1       # then the call is made with NAF_FWD_ONE_STREAM and the smaller workspace is enough
        need = self.ws_bytes_one if one else self.ws_bytes
        ws = pool.pop(skey, None)
        if ws is not None and ws.numel() < need:
            ws = None
        if ws is None:
            while pool and (len(pool) >= 4 or (len(pool) + 1) * self.ws_bytes > self.WS_POOL_BYTES):
                pool.pop(next(iter(pool)))     # least recently used (dicts keep insertion order)
            ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        pool[skey] = ws
        self._ws = ws                           # the one the last call used (GraphedForward keeps it alive)
        out = torch.empty(self.shape_out, dtype=self.out_dtype, device=dev)
        a.image, a.features, a.out = image.data_ptr(), features.data_ptr(), out.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        a.events[0] = events[0].cuda_event if events else None
        a.events[1] = events[1].cuda_event if events else None
        for i in range(8):     # naf_forward_args.phase_events: hipEvent_t handles at the phase boundaries of the one call
            e = phase_events[i] if (phase_events and i < len(phase_events)) else None    # None entries are skipped by the library
            a.phase_events[i] = e.cuda_event if e is not None else None
        logits = None
        if return_logits:
            logits = torch.empty((self.shape_out[0], a.heads, self.shape_out[1], self.shape_out[2], a.ksize * a.ksize),
                                 dtype=torch.float32, device=dev)
        a.logits = logits.data_ptr() if logits is not None else None
        flags = (_lib.FWD_CONV0_EXACT if self.conv0_exact else 0) | (_lib.FWD_ONE_STREAM if one else {0: 0, 2: _lib.FWD_TWO_STREAMS}[int(self.streams)])
        with torch.cuda.device(dev):
            if one:
                rc = self.lib.naf_forward_ex(C.byref(a), None, flags, _stream(image))
            else:
                with AUX_POOL.lease(skey[0], skey[1]) as aux:
                    rc = self.lib.naf_forward_ex(C.byref(a), C.byref(aux), flags, _stream(image))
        _lib.check(rc, "naf_forward_ex")
        out = out.permute(0, 3, 1, 2)
        return (out, logits) if return_logits else out


# ---- label propagation for video evaluation (evaluation/eval_video_seg.py:499-561) -----------------------------------------------
class FrameFeatures:
    """One frame's features as ``propagate_labels`` consumes them: ``data`` is the dense channels-last bf16 buffer ``[h, w, C]`` and
    ``inv_norm`` the fp32 ``[h, w]`` map of ``1 / max(||x||, 1e-12)`` (``F.normalize``'s eps).  Built by ``pack_frame``; a caller keeps one
    per frame of its queue, so that a frame is packed once however many targets it serves as context for."""
    __slots__ = ("data", "inv_norm")

    def __init__(self, data: torch.Tensor, inv_norm: torch.Tensor):
        self.data, self.inv_norm = data, inv_norm

    @property
    def shape(self):
        """(C, h, w)"""
        return (int(self.data.shape[2]), int(self.data.shape[0]), int(self.data.shape[1]))

    @property
    def device(self):
        return self.data.device


def _frame_chw(x, name: str):
    """(C, h, w) of a frame given as a [C, h, w] / [1, C, h, w] tensor or as FrameFeatures; ValueError on anything else."""
    if isinstance(x, FrameFeatures):
        return x.shape
    if not torch.is_tensor(x):
        raise ValueError(f"naf_amd: `{name}` must be a tensor or FrameFeatures, got {type(x).__name__}")
    if x.dim() == 4 and x.shape[0] == 1:
        shape = x.shape[1:]
    elif x.dim() == 3:
        shape = x.shape
    else:
        raise ValueError(f"naf_amd: `{name}` must be [C, h, w] or [1, C, h, w], got {tuple(x.shape)}")
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"naf_amd: `{name}` must be bfloat16 or float32 features, got {x.dtype}")
    C_, h, w = (int(v) for v in shape)
    if h < 1 or w < 1:
        raise ValueError(f"naf_amd: `{name}` has an empty grid {h} x {w}")
    if C_ % 32 != 0 or not 32 <= C_ <= 1024:
        raise ValueError(f"naf_amd: `{name}` has C = {C_} channels; label propagation serves C % 32 == 0 and 32 <= C <= 1024")
    return C_, h, w


def pack_frame(feats, name: str = "feats") -> FrameFeatures:
    """Pack one frame's features ``[C, h, w]`` or ``[1, C, h, w]`` (bf16 or fp32, any strides) for ``propagate_labels``.

    fp32 features are rounded to bf16 ONCE, as they are (they are not normalised first): the kernel multiplies the raw bf16 dot products by
    the inverse norms computed here from those same bf16 values.  When ``feats`` is already a dense channels-last bf16 view -- what
    ``naf(...)`` returns -- the buffer is used as it is, without a copy."""
    if isinstance(feats, FrameFeatures):
        return feats
    C_, h, w = _frame_chw(feats, name)
    _gpu(feats, name)
    x = (feats[0] if feats.dim() == 4 else feats).detach()
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)
    hwc = x.permute(1, 2, 0)
    if not hwc.is_contiguous():
        hwc = hwc.contiguous()
    if hwc.data_ptr() % 16:
        hwc = hwc.clone()
    inv = torch.empty((h, w), dtype=torch.float32, device=hwc.device)
    with torch.cuda.device(hwc.device):
        rc = _lib.load().naf_feature_inv_norm(hwc.data_ptr(), inv.data_ptr(), h, w, C_, _stream(hwc))
    _lib.check(rc, "naf_feature_inv_norm")
    return FrameFeatures(hwc, inv)


def propagate_labels(target, context, segs, radius: int = 12, topk: int = 5, temperature: float = 0.1) -> torch.Tensor:
    """Propagate the context frames' label maps to the target frame: the reference's ``label_propagation`` after feature extraction
    (evaluation/eval_video_seg.py:499-561), with the affinity matrix never materialised.

    ``target`` and each element of ``context`` are ``[C, h, w]`` / ``[1, C, h, w]`` features (bf16, or fp32 that is rounded to bf16 once) or
    ``FrameFeatures`` from ``pack_frame``; ``context`` may also be one stacked ``[n, C, h, w]`` tensor.  ``segs`` is ``[n, K, h, w]`` or a
    list of ``[1, K, h, w]`` / ``[K, h, w]`` soft label maps, one per context frame.  For every target pixel the candidates are the pixels
    of every context frame within ``radius`` in both directions (window clipped at the borders); the ``topk``-th largest cosine similarity
    is the threshold, every candidate at or above it is kept -- ties at the threshold are ALL kept -- and the output is the
    ``exp(s / temperature)``-weighted mean of the kept candidates' labels.  Returns ``[1, K, h, w]`` fp32, detached (not differentiable).

    Served: C % 32 == 0 and 32 <= C <= 1024, 1 <= K <= 64, 1 <= topk <= 16, 1 <= radius <= 15, 1 <= n <= 16.  ``radius=0`` is the
    reference's dense case and is not served.  Anything else raises ``ValueError``; there is no torch fallback."""
    who = "propagate_labels"
    if torch.is_tensor(context):
        if context.dim() != 4:
            raise ValueError(f"naf_amd.{who}: a `context` tensor must be stacked frames [n, C, h, w], got {tuple(context.shape)}")
        frames = list(context.unbind(0))
    elif isinstance(context, FrameFeatures):
        frames = [context]
    elif isinstance(context, (list, tuple)):
        frames = list(context)
    else:
        raise ValueError(f"naf_amd.{who}: `context` must be a list of frames or a stacked tensor, got {type(context).__name__}")
    n = len(frames)
    if not 1 <= n <= _lib.PROPAGATE_MAX_FRAMES:
        raise ValueError(f"naf_amd.{who}: n = {n} context frames; served: 1 <= n <= {_lib.PROPAGATE_MAX_FRAMES}")
    C_, h, w = _frame_chw(target, "target")
    for i, f in enumerate(frames):
        if _frame_chw(f, f"context[{i}]") != (C_, h, w):
            raise ValueError(f"naf_amd.{who}: context[{i}] is (C, h, w) = {_frame_chw(f, 'context')}, the target is {(C_, h, w)}")
    if torch.is_tensor(segs):
        if segs.dim() != 4:
            raise ValueError(f"naf_amd.{who}: a `segs` tensor must be [n, K, h, w], got {tuple(segs.shape)}")
        seg_list = [segs]
    elif isinstance(segs, (list, tuple)) and all(torch.is_tensor(s) for s in segs):
        for i, s in enumerate(segs):
            if not (s.dim() == 3 or (s.dim() == 4 and s.shape[0] == 1)):
                raise ValueError(f"naf_amd.{who}: segs[{i}] must be [K, h, w] or [1, K, h, w], got {tuple(s.shape)}")
        seg_list = [s if s.dim() == 4 else s[None] for s in segs]
    else:
        raise ValueError(f"naf_amd.{who}: `segs` must be an [n, K, h, w] tensor or a list of label maps")
    if sum(int(s.shape[0]) for s in seg_list) != n:
        raise ValueError(f"naf_amd.{who}: {sum(int(s.shape[0]) for s in seg_list)} label maps for n = {n} context frames")
    K = int(seg_list[0].shape[1])
    for s in seg_list:
        if not s.is_floating_point():
            raise ValueError(f"naf_amd.{who}: `segs` must be floating-point soft label maps (one-hot for the first frame), got {s.dtype}")
        if tuple(s.shape[1:]) != (K, h, w):
            raise ValueError(f"naf_amd.{who}: a label map is (K, h, w) = {tuple(s.shape[1:])}, expected {(K, h, w)}")
    a = _lib.PropagateArgs()
    a.n, a.C, a.h, a.w, a.K = n, C_, h, w, K
    try:
        a.radius, a.topk, a.temperature = int(radius), int(topk), float(temperature)
    except (TypeError, OverflowError) as e:
        raise ValueError(f"naf_amd.{who}: radius, topk and temperature must be numbers: {e}") from e
    lib = _lib.load()
    if lib.naf_propagate_select(C.byref(a)) != 0:            # host only: the limits live in one place, the library
        raise ValueError(f"naf_amd.{who}: {_lib.last_error()}")

    tensors = [t.data if isinstance(t, FrameFeatures) else t for t in [target, *frames]] + seg_list
    for t in tensors:
        _gpu(t, "features and segs")
    dev = tensors[0].device
    if any(t.device != dev for t in tensors):
        raise ValueError(f"naf_amd.{who}: target, context and segs must live on one device")
    tgt = pack_frame(target, "target")
    ctx = [pack_frame(f, f"context[{i}]") for i, f in enumerate(frames)]
    sg = (seg_list[0] if len(seg_list) == 1 else torch.cat(seg_list, 0)).detach()
    sg = sg.to(torch.float32).permute(0, 2, 3, 1).contiguous()           # [n, h, w, K]: one kept candidate's labels are contiguous
    out = torch.empty((1, K, h, w), dtype=torch.float32, device=dev)
    a.target, a.target_inv = tgt.data.data_ptr(), tgt.inv_norm.data_ptr()
    for i, f in enumerate(ctx):
        a.context[i], a.context_inv[i] = f.data.data_ptr(), f.inv_norm.data_ptr()
    a.segs, a.out = sg.data_ptr(), out.data_ptr()
    with torch.cuda.device(dev), _Timed("propagate"):
        rc = lib.naf_propagate_fwd(C.byref(a), _stream(out))
    _lib.check(rc, "naf_propagate_fwd")
    return out


def propagate_plan(n: int, C_: int, h: int, w: int, K: int, radius: int = 12, topk: int = 5, temperature: float = 0.1) -> Dict[str, int]:
    """What ``propagate_labels`` launches for these sizes (``naf_propagate_plan``, host only): ``ksmax`` the kernel instantiation's query
    fragments, ``nkb`` the 16-key blocks per halo row, ``nbuf`` 2 for the double-buffered key stream and 1 for the single buffer, ``lds``
    the launch's LDS bytes.  ``ValueError`` outside the served range, as ``propagate_labels`` raises it."""
    a = _lib.PropagateArgs()
    a.n, a.C, a.h, a.w, a.K, a.radius, a.topk, a.temperature = int(n), int(C_), int(h), int(w), int(K), int(radius), int(topk), float(temperature)
    out = (C.c_int32 * 4)()
    if _lib.load().naf_propagate_plan(C.byref(a), out) != 0:
        raise ValueError(f"naf_amd.propagate_plan: {_lib.last_error()}")
    return dict(zip(("ksmax", "nkb", "nbuf", "lds"), (int(v) for v in out)))


# ---- DAVIS J and F measures (evaluation/eval_video_seg.py:145-269) --------------------------------------------------------------------
DavisJF = collections.namedtuple("DavisJF", ("J", "F", "counts"))


def _davis_bound(bound_th, H: int, W: int, who: str):
    """(r2, half_width) = (floor(bound_pix^2), floor(bound_pix)) with bound_pix as eval_video_seg.py:183 forms it; host only."""
    try:
        th = float(bound_th)
    except (TypeError, ValueError) as e:
        raise ValueError(f"naf_amd.{who}: bound_th must be a number: {e}") from e
    if not math.isfinite(th):
        raise ValueError(f"naf_amd.{who}: bound_th must be finite, got {th}")
    bound_pix = th if th >= 1 else float(math.ceil(th * math.sqrt(float(H * H + W * W))))
    half = int(math.floor(min(max(bound_pix, -1.0), 40000.0)))
    if half < 0 or half > _lib.DAVIS_MAX_HALF_WIDTH:          # not served: the library words the refusal; r2 stays inside int32
        return (0, -1) if half < 0 else (half * half, half)
    return int(math.floor(bound_pix * bound_pix)), half


def davis_jf(annotation: torch.Tensor, segmentation: torch.Tensor, num_objects: Optional[int] = None, bound_th: float = 0.008) -> "DavisJF":
    """The DAVIS region similarity J and boundary measure F of every (object, frame) of two label-map sequences, in one kernel launch: the
    reference's ``davis_db_eval_iou`` and ``davis_db_eval_boundary`` (evaluation/eval_video_seg.py:145-248) without PNG files, one-hot
    float64 arrays or per-frame distance transforms on the host.

    ``annotation`` and ``segmentation`` are ``[T, H, W]`` (or ``[H, W]``: one frame) label maps on one ROCm device, ``torch.uint8`` (read as
    they are; a view that is not dense is copied once) or ``torch.int64`` (converted once on the device).  Label 0 is background, labels
    ``1 .. N`` are objects.  Returns ``DavisJF(J, F, counts)``: ``J`` and ``F`` float64 ``[N, T]``, ``counts`` int64 ``[N, T, 6]`` holding
    ``inters, union, n_seg, n_gt, seg_hits, gt_hits``; all on the inputs' device, detached.  With ``g = (annotation[t] == o)`` and
    ``s = (segmentation[t] == o)``:

        J = inters / union = |g & s| / |g | s|, and 1 where the union is empty
        the boundary map of a mask is where its 3 x 3 Sobel pair is non-zero, the border reflected without repeating the edge
        n_seg, n_gt   boundary pixels of s and of g;   seg_hits   boundary pixels of s with a boundary pixel of g within bound_pix (gt_hits: the converse)
        P = seg_hits / (n_seg + 1e-10), R = gt_hits / (n_gt + 1e-10), F = 2 P R / (P + R), and 0 where P + R == 0
        bound_pix = bound_th if bound_th >= 1 else ceil(bound_th * sqrt(H^2 + W^2))        (8 at 480 x 854 with the default)

    Against an EMPTY boundary the hit counts are 0 here.  The reference's distance transform of a map without a boundary pixel returns
    arbitrary small distances there and so counts spurious hits, but that count is then multiplied by the other side's ``0 / 1e-10``: ``F`` is
    identical to the reference's in every case, only the raw ``seg_hits`` / ``gt_hits`` of those cases differ.

    ``num_objects=None`` takes N = ``annotation.max()`` -- ONE host synchronisation -- and raises ``ValueError`` when ``segmentation`` holds a
    higher label (the reference skips such a sequence: "an index higher than the number of objects", eval_video_seg.py:282-284) or when
    ``annotation`` has no object.  With ``num_objects=N`` nothing synchronises: labels above N in either map belong to no object, and an
    object missing from ``segmentation`` has an empty mask there (the reference's zero padding, eval_video_seg.py:285-287).  There are no
    void pixels (the reference passes none, :322); dropping the first and last frame (:318) is the caller's slice.

    Served: 1 <= N <= 32, H, W >= 2, T >= 1, 1 <= floor(bound_pix) <= 32.  Anything else raises ``ValueError``; there is no torch fallback."""
    who = "davis_jf"
    for name, t in (("annotation", annotation), ("segmentation", segmentation)):
        if not torch.is_tensor(t):
            raise ValueError(f"naf_amd.{who}: `{name}` must be a tensor, got {type(t).__name__}")
        if t.dtype not in (torch.uint8, torch.int64):
            raise ValueError(f"naf_amd.{who}: `{name}` must be a torch.uint8 or torch.int64 label map, got {t.dtype}")
        if t.dim() not in (2, 3):
            raise ValueError(f"naf_amd.{who}: `{name}` must be [T, H, W] or [H, W], got {tuple(t.shape)}")
    if tuple(annotation.shape) != tuple(segmentation.shape):
        raise ValueError(f"naf_amd.{who}: annotation {tuple(annotation.shape)} and segmentation {tuple(segmentation.shape)} must have one shape")
    T, H, W = (1, *annotation.shape) if annotation.dim() == 2 else annotation.shape
    T, H, W = int(T), int(H), int(W)
    if num_objects is not None and (isinstance(num_objects, bool) or not isinstance(num_objects, int)):
        raise ValueError(f"naf_amd.{who}: num_objects must be an int or None, got {num_objects!r}")
    if num_objects is not None and not -(1 << 31) <= num_objects < (1 << 31):
        raise ValueError(f"naf_amd.{who}: num_objects = {num_objects} is not served: 1 <= N <= {_lib.DAVIS_MAX_OBJECTS}")
    a = _lib.DavisJFArgs()
    a.T, a.H, a.W = T, H, W
    a.r2, a.half_width = _davis_bound(bound_th, H, W, who)
    a.N = 1 if num_objects is None else num_objects
    lib = _lib.load()
    if lib.naf_davis_jf_select(C.byref(a)) != 0:               # host only: the limits live in one place, the library
        raise ValueError(f"naf_amd.{who}: {_lib.last_error()}")

    _gpu(annotation, "annotation")
    _gpu(segmentation, "segmentation")
    dev = annotation.device
    if segmentation.device != dev:
        raise ValueError(f"naf_amd.{who}: annotation and segmentation must live on one device")
    with torch.cuda.device(dev):
        maps = []
        for t in (annotation, segmentation):
            x = t.detach()
            x = x[None] if x.dim() == 2 else x
            if x.dtype != torch.uint8:
                x = x.clamp(0, 255).to(torch.uint8)            # above N (<= 32) is "no object" either way
            maps.append(x if x.is_contiguous() else x.contiguous())
        if num_objects is None:
            top = torch.stack([annotation.max(), segmentation.max()]).tolist()      # the one synchronisation
            if top[0] < 1:
                raise ValueError(f"naf_amd.{who}: annotation holds no object (its largest label is {top[0]})")
            if top[1] > top[0]:
                raise ValueError(f"naf_amd.{who}: segmentation holds label {top[1]}, an index higher than the number of objects in the "
                                 f"annotation ({top[0]}); the reference skips such a sequence (eval_video_seg.py:282-284)")
            a.N = int(min(top[0], (1 << 31) - 1))
            if lib.naf_davis_jf_select(C.byref(a)) != 0:
                raise ValueError(f"naf_amd.{who}: {_lib.last_error()}")
        N = int(a.N)
        counts = torch.zeros((N, T, 6), dtype=torch.int64, device=dev)
        a.annotation, a.segmentation, a.counts = maps[0].data_ptr(), maps[1].data_ptr(), counts.data_ptr()
        with _Timed("davis_jf"):
            rc = lib.naf_davis_jf(C.byref(a), _stream(counts))
        _lib.check(rc, "naf_davis_jf")
        c = counts.to(torch.float64)
        inters, union, n_seg, n_gt, seg_hits, gt_hits = c.unbind(-1)
        one, zero = torch.ones_like(union), torch.zeros_like(union)
        J = torch.where(union == 0, one, inters / torch.where(union == 0, one, union))
        P, Rc = seg_hits / (n_seg + 1e-10), gt_hits / (n_gt + 1e-10)
        den = P + Rc
        F = torch.where(den == 0, zero, 2 * P * Rc / torch.where(den == 0, one, den))
    return DavisJF(J, F, counts)


def davis_statistics(per_frame_values: torch.Tensor):
    """Mean, recall and decay of per-frame values, the reference's ``davis_db_statistics`` (evaluation/eval_video_seg.py:251-269), for
    every object at once: ``per_frame_values`` is ``[N, T]`` (or ``[T]``), e.g. ``davis_jf(...).J``.  Returns ``(mean, recall, decay)``, each
    float64 ``[N]`` (0-dim for a ``[T]`` input) on the input's device -- plain torch operations, no kernel, no synchronisation:

        mean = nanmean(v),   recall = mean(v > 0.5),   decay = nanmean(first bin) - nanmean(fourth bin)

    with the four bins ``v[ids[i] : ids[i + 1] + 1]``, ``ids = round(linspace(1, T, 5) + 1e-10) - 1`` -- the reference's edges, overlapping
    by one frame as they do there (T = 68: 0, 17, 34, 50, 67).  The reference casts the edges to uint8, which wraps beyond 256 frames:
    ``T > 256`` raises ``ValueError`` instead."""
    who = "davis_statistics"
    v = per_frame_values
    if not torch.is_tensor(v) or v.dim() not in (1, 2) or not v.is_floating_point():
        raise ValueError(f"naf_amd.{who}: a floating-point [N, T] or [T] tensor is expected, got "
                         f"{getattr(v, 'dtype', type(v).__name__)} {tuple(getattr(v, 'shape', ()))}")
    T = int(v.shape[-1])
    if T < 1:
        raise ValueError(f"naf_amd.{who}: no frames (T = 0)")
    if T > 256:
        raise ValueError(f"naf_amd.{who}: T = {T} frames; the reference's uint8 bin edges wrap beyond 256 frames, so T <= 256 is served")
    v = v.detach().to(torch.float64)
    step = (T - 1) / 4
    ids = [int(round(x + 1e-10)) - 1 for x in [1 + i * step for i in range(4)] + [float(T)]]
    mean = torch.nanmean(v, dim=-1)
    recall = (v > 0.5).to(torch.float64).mean(dim=-1)
    decay = torch.nanmean(v[..., ids[0]:ids[1] + 1], dim=-1) - torch.nanmean(v[..., ids[3]:ids[4] + 1], dim=-1)
    return mean, recall, decay


# ---- a propagated frame's label map, and the tracker around it (evaluation/eval_video_seg.py:389-457, 611-643) ---------------------------
def nearest_index_table(n_in: int, n_out: int) -> torch.Tensor:
    """[n_out] int32 CPU tensor: the source index Pillow's ``Image.resize(size, 0)`` (nearest) reads for every output index along an axis
    of ``n_in`` pixels resized to ``n_out`` (host function of the library, no GPU and no Pillow needed).  With ``s = n_in / n_out`` in
    doubles: ``xo = 0.5 * s``; ``idx[x] = min(int(xo), n_in - 1)``; ``xo += s``.  The accumulation is the definition: the closed form
    ``floor((2x + 1) n_in / (2 n_out))`` differs from it, and so does ``F.interpolate(mode="nearest")``, which reads ``floor(x * s)``."""
    for name, v in (("n_in", n_in), ("n_out", n_out)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v < (1 << 31):
            raise ValueError(f"naf_amd.nearest_index_table: {name} must be an int of at least 1, got {v!r}")
    out = torch.empty((n_out,), dtype=torch.int32)
    rc = _lib.load().naf_nearest_resize_table(C.cast(out.data_ptr(), C.POINTER(C.c_int32)), n_in, n_out)
    _lib.check(rc, "naf_nearest_resize_table")
    return out


_nearest_cache = {}


def device_nearest_table(n_in: int, n_out: int, device) -> torch.Tensor:
    key = (int(n_in), int(n_out), str(device))
    t = _nearest_cache.get(key)
    if t is None:
        if len(_nearest_cache) > 64:
            _nearest_cache.clear()
        t = nearest_index_table(int(n_in), int(n_out)).to(device)
        _nearest_cache[key] = t
    return t


def _size2(size, who: str, name: str) -> Tuple[int, int]:
    try:
        a, b = size
    except (TypeError, ValueError) as e:
        raise ValueError(f"naf_amd.{who}: `{name}` must be a pair (rows, columns), got {size!r}") from e
    for v in (a, b):
        if isinstance(v, bool) or not isinstance(v, int) or not -(1 << 31) <= v < (1 << 31):
            raise ValueError(f"naf_amd.{who}: `{name}` must be a pair of ints, got {size!r}")
    return a, b


def masks_to_labels(seg: torch.Tensor, mid_size, out_size, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The label map the reference writes to disk for a propagated frame (evaluation/eval_video_seg.py:444-457), from the soft masks
    ``propagate_labels`` returns, in two kernel launches and without a host synchronisation.

    ``seg`` is ``[1, K, h, w]`` or ``[K, h, w]`` fp32 on a ROCm device, any strides (it is read as it is).  Returns ``torch.uint8``
    ``[out_h, out_w]`` on that device.  Line for line:

        u = F.interpolate(seg, size=mid_size, mode="bilinear", align_corners=False)     ATen's fp32 arithmetic, never written to memory
        norm_mask: per channel, with mx / mn over the mid grid: (u - mn) / (mx - mn) where mx > 0, unchanged where not;
                   mx > 0 and mx == mn is 0 / 0, the channel is NaN everywhere -- as in the reference
        label = torch.max(u, dim=0) indices: the first maximum, a NaN above every number (the CPU's rule)
        Image.resize((out_w, out_h), 0): output pixel (y, x) reads mid pixel (ty[y], tx[x]), ty / tx = nearest_index_table(mid, out)

    In the reference ``mid_size = (h * ps // ups_factor, w * ps // ups_factor)`` and ``out_size`` is the frame's own size.  ``out=`` is a
    ``torch.uint8`` view ``[out_h, out_w]`` on the same device whose columns are adjacent (``stride(1) == 1``, any row stride of at
    least ``out_w``), e.g. row ``t`` of a ``[T, H, W]`` sequence buffer for ``davis_jf``: it is written in place and returned, nothing outside
    it is touched.  NaN inputs are unspecified.

    Served: 1 <= K <= 64, every size 1 .. 16384.  Anything else raises ``ValueError``; there is no torch fallback."""
    who = "masks_to_labels"
    if not torch.is_tensor(seg):
        raise ValueError(f"naf_amd.{who}: `seg` must be a tensor, got {type(seg).__name__}")
    if seg.dim() == 4 and seg.shape[0] == 1:
        s3 = seg[0]
    elif seg.dim() == 3:
        s3 = seg
    else:
        raise ValueError(f"naf_amd.{who}: `seg` must be [1, K, h, w] or [K, h, w], got {tuple(seg.shape)}")
    if seg.dtype != torch.float32:
        raise ValueError(f"naf_amd.{who}: `seg` must be float32 soft masks (what propagate_labels returns), got {seg.dtype}")
    (mh, mw), (oh, ow) = _size2(mid_size, who, "mid_size"), _size2(out_size, who, "out_size")
    a = _lib.MaskLabelsArgs()
    a.K, a.h, a.w = (int(v) for v in s3.shape)
    a.mid_h, a.mid_w, a.out_h, a.out_w = mh, mw, oh, ow
    lib = _lib.load()
    if lib.naf_mask_labels_select(C.byref(a)) != 0:            # host only: the limits live in one place, the library
        raise ValueError(f"naf_amd.{who}: {_lib.last_error()}")
    _gpu(seg, "seg")
    dev = seg.device
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (oh, ow):
            raise ValueError(f"naf_amd.{who}: `out` must be a torch.uint8 tensor of shape {(oh, ow)}, got "
                             f"{getattr(out, 'dtype', type(out).__name__)} {tuple(getattr(out, 'shape', ()))}")
        if out.device != dev:
            raise ValueError(f"naf_amd.{who}: `out` is on {out.device}, `seg` on {dev}")
        if (ow > 1 and out.stride(1) != 1) or (oh > 1 and out.stride(0) < ow):
            raise ValueError(f"naf_amd.{who}: `out` must have adjacent columns and rows that do not overlap, got strides {tuple(out.stride())}")
    with torch.cuda.device(dev):
        s3 = s3.detach()
        res = out if out is not None else torch.empty((oh, ow), dtype=torch.uint8, device=dev)
        ty, tx = device_nearest_table(mh, oh, dev), device_nearest_table(mw, ow, dev)
        ws = torch.empty((_lib.MASK_LABELS_WORKSPACE_BYTES // 4,), dtype=torch.float32, device=dev)
        a.seg, a.tab_y, a.tab_x, a.out, a.workspace = s3.data_ptr(), ty.data_ptr(), tx.data_ptr(), res.data_ptr(), ws.data_ptr()
        a.workspace_bytes = _lib.MASK_LABELS_WORKSPACE_BYTES
        a.seg_stride = _strides3(s3)
        a.out_stride = int(res.stride(0)) if oh > 1 else ow
        with _Timed("mask_labels"):
            rc = lib.naf_mask_labels(C.byref(a), _stream(res))
        _lib.check(rc, "naf_mask_labels")
    return res


def labels_to_masks(labels: torch.Tensor, size, num_classes: Optional[int] = None) -> torch.Tensor:
    """The first frame's one-hot masks: the reference's ``read_seg`` + ``to_one_hot`` (evaluation/eval_video_seg.py:638-643, 611-623).
    ``labels`` is a ``[H, W]`` ``torch.uint8`` or ``torch.int64`` label map on the device; it is resized to ``size = (h, w)`` as Pillow's
    nearest resize reads it (``nearest_index_table``) and expanded to fp32 ``[1, K, h, w]``.  ``num_classes=None`` takes
    ``K = labels.max() + 1`` -- ONE host synchronisation, as in the reference; with ``num_classes=K`` nothing synchronises and a label outside
    ``0 .. K - 1`` belongs to no channel.  (The reference takes the maximum AFTER the resize; an object the resize drops is an all-zero
    channel here, which wins nowhere: ties go to a lower channel.)  Plain torch indexing on the labels' device; no kernel."""
    who = "labels_to_masks"
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"naf_amd.{who}: `labels` must be a [H, W] torch.uint8 or torch.int64 label map, got "
                         f"{getattr(labels, 'dtype', type(labels).__name__)} {tuple(getattr(labels, 'shape', ()))}")
    h, w = _size2(size, who, "size")
    H, W = (int(v) for v in labels.shape)
    if min(h, w, H, W) < 1:
        raise ValueError(f"naf_amd.{who}: sizes must be at least 1, got {H} x {W} -> {h} x {w}")
    if num_classes is not None and (isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1):
        raise ValueError(f"naf_amd.{who}: num_classes must be a positive int or None, got {num_classes!r}")
    dev = labels.device
    ty, tx = device_nearest_table(H, h, dev).long(), device_nearest_table(W, w, dev).long()
    small = labels.detach()[ty][:, tx].long()
    K = int(labels.max()) + 1 if num_classes is None else num_classes        # None: the one synchronisation (to_one_hot, :617)
    if K < 1:
        raise ValueError(f"naf_amd.{who}: labels.max() = {K - 1}: no class")
    return (small[None] == torch.arange(K, device=dev)[:, None, None]).to(torch.float32)[None]


class VideoTracker:
    """The per-sequence loop of the reference's ``eval_video_tracking_davis`` (evaluation/eval_video_seg.py:389-441) on the device.

        trk = VideoTracker(first_feats, first_labels, ps=16, ups_factor=8, n_last_frames=7, radius=12, topk=5, temperature=0.1)
        pred[t] = trk.step(feats_t)               # or trk.step(feats_t, out=pred[t]): uint8 [H0, W0] on the device

    ``first_feats`` and every ``feats_t`` are what ``naf(...)`` returns (``[C, h, w]`` / ``[1, C, h, w]``) or ``FrameFeatures``;
    ``first_labels`` is frame 0's annotation ``[H0, W0]`` (uint8 or int64).  The first mask is ``labels_to_masks(first_labels, (h, w),
    num_classes)``, the label maps are ``masks_to_labels(seg, (h * ps // ups_factor, w * ps // ups_factor), (H0, W0))``.  The tracker keeps the
    packed first frame and a queue of at most ``n_last_frames`` pairs (packed features, the soft masks ``propagate_labels`` returned: BEFORE
    the upsample and the normalisation, as :440-441 stores them); a step propagates from ``[first] + queue`` in that order, pushes its
    result and returns its label map.  A step makes no host synchronisation (the constructor makes one when ``num_classes`` is None).  The
    bilinear feature resize of :407 / :532 stays the caller's; a frame whose grid differs from the first frame's raises ``ValueError``."""

    def __init__(self, first_feats, first_labels: torch.Tensor, ps: int = 16, ups_factor: int = 8, n_last_frames: int = 7, radius: int = 12,
                 topk: int = 5, temperature: float = 0.1, num_classes: Optional[int] = None):
        who = "VideoTracker"
        for name, v, lo in (("ps", ps, 1), ("ups_factor", ups_factor, 1), ("n_last_frames", n_last_frames, 0)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"naf_amd.{who}: {name} must be an int of at least {lo}, got {v!r}")
        if n_last_frames + 1 > _lib.PROPAGATE_MAX_FRAMES:
            raise ValueError(f"naf_amd.{who}: n_last_frames = {n_last_frames}; the first frame and the queue are at most "
                             f"{_lib.PROPAGATE_MAX_FRAMES} context frames")
        self._first = pack_frame(first_feats, "first_feats")
        self._grid = self._first.shape
        _, h, w = self._grid
        if not torch.is_tensor(first_labels) or first_labels.dim() != 2:
            raise ValueError(f"naf_amd.{who}: `first_labels` must be a [H0, W0] label map")
        if first_labels.device != self._first.device:
            raise ValueError(f"naf_amd.{who}: first_labels is on {first_labels.device}, the features on {self._first.device}")
        self.out_size = (int(first_labels.shape[0]), int(first_labels.shape[1]))
        self.mid_size = (h * ps // ups_factor, w * ps // ups_factor)
        self._first_seg = labels_to_masks(first_labels, (h, w), num_classes)
        self._prop = dict(radius=radius, topk=topk, temperature=temperature)
        self._n_last = n_last_frames
        self._queue = collections.deque()
        a = _lib.MaskLabelsArgs()                                # refuse a geometry no step could serve now, not at the first step
        a.K, a.h, a.w = int(self._first_seg.shape[1]), h, w
        (a.mid_h, a.mid_w), (a.out_h, a.out_w) = self.mid_size, self.out_size
        if _lib.load().naf_mask_labels_select(C.byref(a)) != 0:
            raise ValueError(f"naf_amd.{who}: {_lib.last_error()}")
        for n_in, n_out in zip(self.mid_size, self.out_size):    # the resize tables go to the device now, so that no step uploads one
            device_nearest_table(n_in, n_out, self._first.device)

    @property
    def context_feats(self) -> tuple:
        """The frames the next step propagates from, first frame first (``FrameFeatures``)."""
        return (self._first, *(f for f, _ in self._queue))

    @property
    def context_segs(self) -> tuple:
        """Their soft masks ``[1, K, h, w]``, in the same order."""
        return (self._first_seg, *(s for _, s in self._queue))

    def step(self, feats, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if _frame_chw(feats, "feats") != self._grid:
            raise ValueError(f"naf_amd.VideoTracker: the frame is (C, h, w) = {_frame_chw(feats, 'feats')}, the first frame {self._grid}; "
                             "resize the features to the first frame's grid (eval_video_seg.py:532)")
        tgt = pack_frame(feats, "feats")
        seg = propagate_labels(tgt, list(self.context_feats), list(self.context_segs), **self._prop)
        if self._n_last > 0:
            if len(self._queue) == self._n_last:
                self._queue.popleft()
            self._queue.append((tgt, seg))
        return masks_to_labels(seg, self.mid_size, self.out_size, out=out)


# ---- frame preparation: the resizes and normalisations in front of the model (eval_video_seg.py:577-597, train.py:115-126) ---------------
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # the upsampler's statistics everywhere in the reference
_PREP_MODE = {None: _lib.PREP_NONE, "bilinear": _lib.PREP_BILINEAR, "bicubic": _lib.PREP_BICUBIC}


class PrepView:
    """One derived image of ``prepare_views``: first resize, normalise, second resize, store -- every step optional.

        size, mode   the first resize, to ``size = (h, w)`` with ``mode`` ``"bilinear"`` / ``"bicubic"`` (``align_corners=False``, no
                     antialiasing); ``size=None`` keeps the source's size, ``mode=None`` is no resize (the sizes must then be equal)
        mean, std    three values each: ``(v - mean) / std`` per channel; both ``None``: the step is skipped
        then         ``((h, w), mode)``: the second resize, of the normalised image; ``None``: none
        dtype        ``torch.float32`` or ``torch.bfloat16`` of the result
        out          an existing ``[B, 3, h, w]`` tensor of that dtype (any strides) to write instead of a new one
    """
    __slots__ = ("size", "mode", "mean", "std", "then", "dtype", "out")

    def __init__(self, size=None, mode=None, mean=None, std=None, then=None, dtype=torch.float32, out=None):
        self.size, self.mode, self.mean, self.std, self.then, self.dtype, self.out = size, mode, mean, std, then, dtype, out

    def __repr__(self):
        return (f"PrepView(size={self.size!r}, mode={self.mode!r}, mean={self.mean!r}, std={self.std!r}, then={self.then!r}, "
                f"dtype={self.dtype}, out={'given' if self.out is not None else None})")


def _prep_mode(mode, who: str) -> int:
    if not (mode is None or isinstance(mode, str)) or mode not in _PREP_MODE:
        raise ValueError(f"naf_amd.{who}: a resize mode is 'bilinear', 'bicubic' or None, got {mode!r}")
    return _PREP_MODE[mode]


def _prep_stats(v, who: str, name: str):
    try:
        vals = [float(x) for x in (v.tolist() if torch.is_tensor(v) else v)]
    except (TypeError, ValueError) as e:
        raise ValueError(f"naf_amd.{who}: `{name}` must be three numbers, got {v!r}") from e
    if len(vals) != 3:
        raise ValueError(f"naf_amd.{who}: `{name}` must be three numbers (one per channel), got {len(vals)}")
    return vals


def prepare_views(src: torch.Tensor, views, hflip: bool = False):
    """Every resized, normalised image the reference's callers derive from one decoded frame or batch, in ONE kernel launch: no
    intermediate image, no host synchronisation, and the frame may stay the uint8 it was decoded as.

    ``src`` is ``torch.uint8`` ``[H, W, 3]`` / ``[B, H, W, 3]`` (its value is ``u / 255``, ``ToTensor``), or ``torch.float32`` /
    ``torch.bfloat16`` ``[3, H, W]`` / ``[B, 3, H, W]``, with any strides (a crop, a channels-last tensor), on a ROCm device.  ``views`` is a
    sequence of 1 .. 4 ``PrepView``; ``hflip=True`` mirrors the source's columns first.  Returns a list with one ``[B, 3, h, w]`` tensor per view
    (dense unless the view names ``out=``).  The arithmetic is ATen's device arithmetic in fp32, every operation rounded on its own, stated
    in include/naf_hip.h (naf_image_prep): the second resize reads the normalised first-stage image as if it had been stored in fp32.

    Served: every size 1 .. 16384, fewer than 2^31 output pixels per view.  A CPU tensor raises ``RuntimeError``; anything else not served
    raises ``ValueError`` with the library's message.  There is no torch fallback."""
    who = "prepare_views"
    if not torch.is_tensor(src):
        raise ValueError(f"naf_amd.{who}: `src` must be a tensor, got {type(src).__name__}")
    if src.dtype == torch.uint8:
        if src.dim() not in (3, 4) or src.shape[-1] != 3:
            raise ValueError(f"naf_amd.{who}: a uint8 `src` must be [H, W, 3] or [B, H, W, 3] (3 channels last), got {tuple(src.shape)}")
        s4 = src if src.dim() == 4 else src[None]
        s4 = s4.permute(0, 3, 1, 2)
        dt = _lib.IMAGE_PREP_U8
    elif src.dtype in _DT:
        if src.dim() not in (3, 4) or src.shape[-3] != 3:
            raise ValueError(f"naf_amd.{who}: a {src.dtype} `src` must be [3, H, W] or [B, 3, H, W] (3 channels), got {tuple(src.shape)}")
        s4 = src if src.dim() == 4 else src[None]
        dt = _DT[src.dtype]
    else:
        raise ValueError(f"naf_amd.{who}: `src` must be uint8, float32 or bfloat16, got {src.dtype}")
    try:
        views = list(views)
    except TypeError as e:
        raise ValueError(f"naf_amd.{who}: `views` must be a sequence of PrepView") from e
    if any(not isinstance(v, PrepView) for v in views):
        raise ValueError(f"naf_amd.{who}: `views` must be a sequence of PrepView")
    a = _lib.ImagePrepArgs()
    a.src_dtype, a.hflip, a.n_views = dt, int(bool(hflip)), len(views)
    a.B, a.H, a.W = int(s4.shape[0]), int(s4.shape[2]), int(s4.shape[3])
    shapes = []
    for i, v in enumerate(views[:_lib.IMAGE_PREP_MAX_VIEWS]):
        q = a.view[i]
        if v.dtype not in _DT:
            raise ValueError(f"naf_amd.{who}: view {i}: dtype must be torch.float32 or torch.bfloat16, got {v.dtype}")
        q.out_dtype = _DT[v.dtype]
        q.mode1 = _prep_mode(v.mode, who)
        q.h1, q.w1 = (a.H, a.W) if v.size is None else _size2(v.size, who, "size")
        if v.then is None:
            q.h2, q.w2, q.mode2 = q.h1, q.w1, _lib.PREP_NONE
        else:
            try:
                size2, mode2 = v.then
            except (TypeError, ValueError) as e:
                raise ValueError(f"naf_amd.{who}: view {i}: `then` must be ((h, w), mode), got {v.then!r}") from e
            (q.h2, q.w2), q.mode2 = _size2(size2, who, "then"), _prep_mode(mode2, who)
        if (v.mean is None) != (v.std is None):
            raise ValueError(f"naf_amd.{who}: view {i}: give both `mean` and `std`, or neither")
        if v.mean is not None:
            q.normalise = 1
            q.mean = (C.c_float * 3)(*_prep_stats(v.mean, who, "mean"))       # rounded to fp32 here, once
            q.std = (C.c_float * 3)(*_prep_stats(v.std, who, "std"))
        shapes.append((a.B, 3, int(q.h2), int(q.w2)))
    lib = _lib.load()
    if lib.naf_image_prep_select(C.byref(a)) != 0:              # host only: the limits live in one place, the library
        raise ValueError(f"naf_amd.{who}: {_lib.last_error()}")
    _gpu(src, "src")
    dev = src.device
    for i, (v, shape) in enumerate(zip(views, shapes)):
        if v.out is None:
            continue
        if not torch.is_tensor(v.out) or v.out.dtype != v.dtype or tuple(v.out.shape) != shape:
            raise ValueError(f"naf_amd.{who}: view {i}: `out` must be a {v.dtype} tensor of shape {shape}, got "
                             f"{getattr(v.out, 'dtype', type(v.out).__name__)} {tuple(getattr(v.out, 'shape', ()))}")
        if v.out.device != dev:
            raise ValueError(f"naf_amd.{who}: view {i}: `out` is on {v.out.device}, `src` on {dev}")
    with torch.cuda.device(dev):
        s4 = s4.detach()
        a.src = s4.data_ptr()
        a.src_stride = _strides4(s4, (0, 1, 2, 3))
        res = []
        for i, (v, shape) in enumerate(zip(views, shapes)):
            t = v.out.detach() if v.out is not None else torch.empty(shape, dtype=v.dtype, device=dev)
            a.view[i].out = t.data_ptr()
            a.view[i].out_stride = _strides4(t, (0, 1, 2, 3))
            res.append(v.out if v.out is not None else t)
        with _Timed("image_prep"):
            rc = lib.naf_image_prep(C.byref(a), _stream(s4))
        _lib.check(rc, "naf_image_prep")
    return res


def lr_image_size(H: int, W: int, factor: float, ps: int) -> Tuple[int, int]:
    """The size of the training step's low-res pass: the reference's ``round_to_nearest_multiple(v * factor, ps)`` per axis
    (utils/training.py:24-25, 44-46), with Python's ``round`` (halves go to the even multiple)."""
    return ps * round(H * factor / ps), ps * round(W * factor / ps)


def davis_frame_views(frame_hw, ps: int, ups_factor: int, backbone_mean, backbone_std):
    """The two images ``extract_feature`` derives from a decoded DAVIS frame (evaluation/eval_video_seg.py:579-595), as views for
    ``prepare_views``.  Returns ``(views, lr_grid, hr_size)``: the frame goes bilinearly to ``(H // ps * ps, W // ps * ps)``; ``views[0]`` is that
    image with the backbone's statistics; ``views[1]`` is it with the upsampler's (ImageNet) statistics, then bicubically at
    ``hr_size = lr_grid * ups_factor``, ``lr_grid = (H // ps, W // ps)`` being the backbone's feature grid."""
    H, W = _size2(frame_hw, "davis_frame_views", "frame_hw")
    lr_grid = (H // ps, W // ps)
    first = (lr_grid[0] * ps, lr_grid[1] * ps)
    hr_size = (lr_grid[0] * ups_factor, lr_grid[1] * ups_factor)
    views = [PrepView(first, "bilinear", backbone_mean, backbone_std),
             PrepView(first, "bilinear", IMAGENET_MEAN, IMAGENET_STD, then=(hr_size, "bicubic"))]
    return views, lr_grid, hr_size


def training_views(img_size, hr_grid, lr_image_size, backbone_mean, backbone_std):
    """The three images a training step derives from a batch (train.py:115-126, utils/training.py:47), as views for ``prepare_views``: the
    batch bilinearly at ``img_size`` with the backbone's statistics; that image's bilinear shrink to ``lr_image_size`` (``lr_image_size()`` of
    this module, or the configured ``lr_img_size``) for the low-res pass; the batch at ``img_size`` with the upsampler's (ImageNet) statistics,
    then bilinearly at ``[min(224, 4 * v) for v in hr_grid]``, ``hr_grid`` being the backbone's feature grid at ``img_size``."""
    who = "training_views"
    size = (img_size, img_size) if isinstance(img_size, int) and not isinstance(img_size, bool) else _size2(img_size, who, "img_size")
    lr = (lr_image_size, lr_image_size) if isinstance(lr_image_size, int) and not isinstance(lr_image_size, bool) else \
        _size2(lr_image_size, who, "lr_image_size")
    gh, gw = _size2(hr_grid, who, "hr_grid")
    ups = (min(224, 4 * gh), min(224, 4 * gw))
    return [PrepView(size, "bilinear", backbone_mean, backbone_std),
            PrepView(size, "bilinear", backbone_mean, backbone_std, then=(lr, "bilinear")),
            PrepView(size, "bilinear", IMAGENET_MEAN, IMAGENET_STD, then=(ups, "bilinear"))]


def probing_views(backbone_mean, backbone_std):
    """The two normalisations of the probing loops (evaluation/eval_seg_probing.py:97-98, 162-165), no resize: the backbone's image and the
    upsampler's.  The horizontal flip of the training loop is ``prepare_views(..., hflip=True)``."""
    return [PrepView(mean=backbone_mean, std=backbone_std), PrepView(mean=IMAGENET_MEAN, std=IMAGENET_STD)]


# ---- denoising objective (denoising.py:61-177) ------------------------------------------------------------------------------------
def _denoise_check(who: str, pred, target) -> None:
    """Host-only checks, before any device work: TypeError for non-tensors and dtypes the kernel does not read, ValueError for shapes."""
    for name, t in (("pred", pred), ("target", target)):
        if not torch.is_tensor(t):
            raise TypeError(f"naf_amd.{who}: `{name}` must be a tensor, got {type(t).__name__}")
        if t.dtype not in _DT:
            raise TypeError(f"naf_amd.{who}: `{name}` must be a float32 or bfloat16 tensor, got {t.dtype}")
    if pred.dim() != 4 or tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"naf_amd.{who}: pred and target must be [B, C, H, W] of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if min(pred.shape) < 1:
        raise ValueError(f"naf_amd.{who}: empty input {tuple(pred.shape)}")
    if target.requires_grad:
        raise ValueError(f"naf_amd.{who}: `target` requires grad; the objective is differentiable with respect to `pred` only")


def _denoise_weights(who: str, l1_weight, l2_weight, ssim_weight) -> Tuple[float, float, float]:
    try:
        w = (float(l1_weight), float(l2_weight), float(ssim_weight))
    except (TypeError, ValueError) as e:
        raise ValueError(f"naf_amd.{who}: the weights must be numbers: {e}") from e
    if not all(v >= 0.0 for v in w):
        raise ValueError(f"naf_amd.{who}: l1_weight, l2_weight and ssim_weight must not be negative, got {w}")
    return w


def denoise_objective(pred: torch.Tensor, target: torch.Tensor, weights=(1.0, 1.0, 0.1), *, grad: bool = False, metrics: bool = False,
                      clamp: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """naf_denoise_objective: the tile launch plus the finishing launch.  Returns ``(out, grad_map)``: ``out`` is the entry's fp32 ``[8]``
    result vector (include/naf_hip.h: loss mode ``mean|p-t|, mean (p-t)^2, mean S, l1, l2, ssim, total, 0``; metrics mode ``psnr, ssim,
    mse, 0...``) and ``grad_map`` the gradient of ``total`` with respect to ``pred`` when ``grad`` is set -- in ``pred``'s dtype, with
    ``pred``'s strides when ``pred`` is dense in either memory format and contiguous otherwise -- else ``None``.  Nothing here is recorded
    by autograd."""
    who = "denoise_objective"
    _denoise_check(who, pred, target)
    w = _denoise_weights(who, *weights)
    if metrics and grad:
        raise ValueError(f"naf_amd.{who}: the metrics are forward only")
    _gpu(pred, "pred")
    _gpu(target, "target")
    if pred.device != target.device:
        raise ValueError(f"naf_amd.{who}: pred is on {pred.device}, target on {target.device}")
    pred, target = pred.detach(), target.detach()
    dev = pred.device
    lib = _lib.load()
    a = _lib.DenoiseArgs()
    a.B, a.C, a.H, a.W = (int(v) for v in pred.shape)
    a.mode = _lib.DENOISE_METRICS if metrics else _lib.DENOISE_LOSS
    a.clamp = int(bool(clamp))
    a.pred_dtype, a.target_dtype = _DT[pred.dtype], _DT[target.dtype]
    a.l1_weight, a.l2_weight, a.ssim_weight = w
    a.pred_stride, a.target_stride = _strides4(pred, (0, 1, 2, 3)), _strides4(target, (0, 1, 2, 3))
    nbytes = int(lib.naf_denoise_workspace_bytes(C.byref(a)))
    if nbytes == 0:
        raise ValueError(f"naf_amd.{who}: {tuple(pred.shape)} is not a valid shape")
    out = torch.empty(8, dtype=torch.float32, device=dev)
    workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    gmap = torch.empty_like(pred) if grad else None            # preserve_format: pred's strides when dense, contiguous otherwise
    a.pred, a.target, a.out = pred.data_ptr(), target.data_ptr(), out.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
    if gmap is not None:
        a.grad, a.grad_dtype, a.grad_stride = gmap.data_ptr(), _DT[gmap.dtype], _strides4(gmap, (0, 1, 2, 3))
    with torch.cuda.device(dev), _Timed("denoise_metrics" if metrics else "denoise_loss"):
        rc = lib.naf_denoise_objective(C.byref(a), _stream(out))
    _lib.check(rc, "naf_denoise_objective")
    return out, gmap


class DenoiseLossFunction(torch.autograd.Function):
    """``total`` of the denoising loss: the forward writes the gradient map in the same launch, the backward scales it."""

    @staticmethod
    def forward(ctx, pred, target, w1, w2, w3):
        out, gmap = denoise_objective(pred, target, (w1, w2, w3), grad=ctx.needs_input_grad[0])
        if gmap is not None:
            ctx.save_for_backward(gmap)
        ctx.mark_non_differentiable(out)
        return out[6], out

    @staticmethod
    def backward(ctx, g_total, _g_out):
        (gmap,) = ctx.saved_tensors
        return gmap * g_total, None, None, None, None


def denoising_loss(pred: torch.Tensor, target: torch.Tensor, l1_weight: float = 1.0, l2_weight: float = 1.0,
                   ssim_weight: float = 0.1) -> Dict[str, torch.Tensor]:
    """The reference's ``DenoisingLoss.forward`` (denoising.py:161-177) in one kernel launch plus a finishing launch: the dict
    ``{"l1", "l2", "ssim", "total"}`` of 0-dim fp32 device tensors, each term already multiplied by its weight, a key present only where
    its weight is > 0, ``total`` their sum.  ``ssim`` is ``ssim_weight * (1 - mean S)`` over zero-padded 3 x 3 windows.

    Only ``total`` carries a gradient, and only to ``pred``: the three terms are detached (the reference's loop only logs them).  The
    gradient map is written by the forward launch when ``pred`` requires grad; ``backward`` multiplies it by the incoming scalar.
    ``pred`` and ``target`` are ``[B, C, H, W]``, fp32 or bf16 independently, any strides; all arithmetic is fp32.  A ``target`` that
    requires grad raises ``ValueError``; CPU tensors raise ``RuntimeError`` (no fallback)."""
    who = "denoising_loss"
    _denoise_check(who, pred, target)
    w = _denoise_weights(who, l1_weight, l2_weight, ssim_weight)
    _gpu(pred, "pred")
    _gpu(target, "target")
    if not any(v > 0.0 for v in w):
        return {"total": torch.zeros((), dtype=torch.float32, device=pred.device)}
    if pred.requires_grad and torch.is_grad_enabled():
        total, out = DenoiseLossFunction.apply(pred, target, *w)
    else:
        out, _ = denoise_objective(pred, target, w)
        total = out[6]
    losses = {name: out[3 + i] for i, name in enumerate(("l1", "l2", "ssim")) if w[i] > 0.0}
    losses["total"] = total
    return losses


class DenoisingLoss(torch.nn.Module):
    """Drop-in for the reference's ``DenoisingLoss`` (denoising.py:129-177): same constructor and call, served by ``denoising_loss``."""

    def __init__(self, l1_weight=1.0, l2_weight=1.0, ssim_weight=0.1):
        super().__init__()
        self.l1_weight = l1_weight
        self.l2_weight = l2_weight
        self.ssim_weight = ssim_weight

    def forward(self, pred, target):
        return denoising_loss(pred, target, self.l1_weight, self.l2_weight, self.ssim_weight)


def denoising_metrics(pred: torch.Tensor, target: torch.Tensor, clamp: bool = False) -> Dict[str, torch.Tensor]:
    """The reference's ``MetricsCalculator.calculate_batch_metrics`` (denoising.py:64-126): ``{"psnr", "ssim"}`` as 0-dim fp32 device
    tensors -- PSNR in dB (``+inf`` for identical inputs), SSIM through the zero-padded 11 x 11 Gaussian window.  ``clamp=True`` folds the
    ``torch.clamp(pred, 0, 1)`` in front of it (denoising.py:302).  No host synchronisation happens here; ``.item()`` is the caller's."""
    who = "denoising_metrics"
    _denoise_check(who, pred, target)
    out, _ = denoise_objective(pred, target, (0.0, 0.0, 0.0), metrics=True, clamp=clamp)
    return {"psnr": out[0], "ssim": out[1]}


# ---- feature PCA for display (include/naf_hip.h, "feature PCA for display") ----------------------------------------------------------
def _pca_map_shape(x, who: str, name: str = "map"):
    """(C, H, W) of one feature map given as [C, H, W] or [1, C, H, W]; TypeError / ValueError before any device work."""
    if not torch.is_tensor(x):
        raise TypeError(f"naf_amd.{who}: `{name}` must be a tensor, got {type(x).__name__}")
    if x.dtype not in _DT:
        raise TypeError(f"naf_amd.{who}: `{name}` must be a float32 or bfloat16 tensor, got {x.dtype}")
    if x.dim() == 4:
        if x.shape[0] != 1:
            raise ValueError(f"naf_amd.{who}: `{name}` has B = {x.shape[0]}; like the reference's pca(), one map at a time (B = 1)")
        shape = x.shape[1:]
    elif x.dim() == 3:
        shape = x.shape
    else:
        raise ValueError(f"naf_amd.{who}: `{name}` must be [C, H, W] or [1, C, H, W], got {tuple(x.shape)}")
    C_, H, W = (int(v) for v in shape)
    if H < 1 or W < 1:
        raise ValueError(f"naf_amd.{who}: `{name}` has an empty grid {H} x {W}")
    if C_ % 32 != 0 or not 32 <= C_ <= _lib.PCA_MAX_C:
        raise ValueError(f"naf_amd.{who}: `{name}` has C = {C_} channels; served: C % 32 == 0 and 32 <= C <= {_lib.PCA_MAX_C}")
    return C_, H, W


def _pca_rows(x: torch.Tensor, who: str, name: str = "map"):
    """The map as the kernels read it: ``(hwc, C, H, W, ld)`` with ``hwc`` a bf16 [H, W, C] tensor whose pixels are rows of C contiguous
    values at one constant stride ``ld``.  A bf16 channels-last view -- what ``naf(...)`` returns -- is used as it is, without a copy;
    anything else (fp32, NCHW) is converted ONCE to a dense bf16 channels-last buffer (fp32 values are rounded to bf16 once, as
    ``pack_frame`` documents)."""
    C_, H, W = _pca_map_shape(x, who, name)
    _gpu(x, name)
    x = (x[0] if x.dim() == 4 else x).detach()
    hwc = x.permute(1, 2, 0)
    ld = int(hwc.stride(1)) if W > 1 else (int(hwc.stride(0)) if H > 1 else C_)
    as_is = (x.dtype == torch.bfloat16 and hwc.stride(2) == 1 and ld >= C_ and ld % 8 == 0 and (W == 1 or hwc.stride(1) == ld)
             and (H == 1 or hwc.stride(0) == W * ld) and hwc.data_ptr() % 16 == 0)
    if not as_is:
        hwc = hwc.to(torch.bfloat16).contiguous()
        if hwc.data_ptr() % 16:
            hwc = hwc.clone()
        ld = C_
    return hwc, C_, H, W, ld


def feature_moments_plan(P: int, C_: int) -> Tuple[int, int]:
    """``(nsplit, slab_pixels)`` of naf_feature_moments for P pixels of C channels (host only)."""
    a = _lib.FeatureMomentsArgs()
    a.P, a.C, a.ld = int(P), int(C_), int(C_)
    ns, slab = C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.load().naf_feature_moments_plan(C.byref(a), C.byref(ns), C.byref(slab)), "naf_feature_moments_plan")
    return int(ns.value), int(slab.value)


def feature_moments(map: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """naf_feature_moments: ``(gram fp64 [C, C], sum fp64 [C], P)`` of one map ``[1, C, H, W]`` or ``[C, H, W]`` -- ``gram[i, j]`` the sum
    over the P = H W pixels of ``x[i] x[j]``, exactly symmetric, and the channel sums, of the map's bf16 values (see ``_pca_rows`` for what
    is copied).  Summation contract: include/naf_hip.h.  Two launches, no atomics: a second call gives the same bits."""
    who = "feature_moments"
    hwc, C_, H, W, ld = _pca_rows(map, who)
    dev = hwc.device
    lib = _lib.load()
    a = _lib.FeatureMomentsArgs()
    a.P, a.ld, a.C = H * W, ld, C_
    nbytes = int(lib.naf_feature_moments_workspace_bytes(C.byref(a)))
    if nbytes == 0:
        raise ValueError(f"naf_amd.{who}: {(C_, H, W)} is not a served shape")
    gram = torch.empty((C_, C_), dtype=torch.float64, device=dev)
    total = torch.empty(C_, dtype=torch.float64, device=dev)
    workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    a.x, a.gram, a.sum = hwc.data_ptr(), gram.data_ptr(), total.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
    with torch.cuda.device(dev), _Timed("feature_moments"):
        rc = lib.naf_feature_moments(C.byref(a), _stream(hwc))
    _lib.check(rc, "naf_feature_moments")
    return gram, total, H * W


def _minmax_workspace(lib, P: int, dev) -> Tuple[torch.Tensor, int]:
    q = _lib.PcaProjectArgs()
    q.P = P
    nbytes = int(lib.naf_pca_project_workspace_bytes(C.byref(q)))
    return torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=dev), nbytes


def pca_project(map: torch.Tensor, V: torch.Tensor, b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """naf_pca_project: ``(raw, minmax)`` with ``raw[0, r, y, x] = b[r] + sum_c map[0, c, y, x] V[c, r]`` in fp32 -- a logical
    ``[1, n, H, W]`` view of the dense ``[P][n]`` buffer the kernel writes -- and ``minmax`` fp32 ``[2, n]``, the exact minima and maxima
    of ``raw`` per component.  ``V`` is fp32 ``[C, n]``, ``b`` fp32 ``[n]``, 1 <= n <= 8, on the map's device."""
    who = "pca_project"
    C_, H, W = _pca_map_shape(map, who)
    for name, t in (("V", V), ("b", b)):
        if not torch.is_tensor(t):
            raise TypeError(f"naf_amd.{who}: `{name}` must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"naf_amd.{who}: `{name}` must be float32, got {t.dtype}")
    if V.dim() != 2 or V.shape[0] != C_ or not 1 <= V.shape[1] <= _lib.PCA_MAX_COMPONENTS:
        raise ValueError(f"naf_amd.{who}: `V` must be [C = {C_}, n] with 1 <= n <= {_lib.PCA_MAX_COMPONENTS}, got {tuple(V.shape)}")
    n = int(V.shape[1])
    if tuple(b.shape) != (n,):
        raise ValueError(f"naf_amd.{who}: `b` must be [{n}], got {tuple(b.shape)}")
    hwc, C_, H, W, ld = _pca_rows(map, who)
    dev = hwc.device
    _gpu(V, "V")
    _gpu(b, "b")
    if V.device != dev or b.device != dev:
        raise ValueError(f"naf_amd.{who}: map is on {dev}, V on {V.device}, b on {b.device}")
    V, b = V.detach().contiguous(), b.detach().contiguous()
    lib = _lib.load()
    y = torch.empty((1, H, W, n), dtype=torch.float32, device=dev)
    minmax = torch.empty((2, n), dtype=torch.float32, device=dev)
    workspace, nbytes = _minmax_workspace(lib, H * W, dev)
    a = _lib.PcaProjectArgs()
    a.x, a.V, a.b, a.y, a.minmax = hwc.data_ptr(), V.data_ptr(), b.data_ptr(), y.data_ptr(), minmax.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
    a.P, a.ld, a.C, a.n = H * W, ld, C_, n
    with torch.cuda.device(dev), _Timed("pca_project"):
        rc = lib.naf_pca_project(C.byref(a), _stream(hwc))
    _lib.check(rc, "naf_pca_project")
    return y.permute(0, 3, 1, 2), minmax                   # strides (P n, 1, W n, n): the batch stride of the dense buffer


def pca_minmax(raw: torch.Tensor) -> torch.Tensor:
    """naf_pca_minmax: fp32 ``[B, 2, n]``, the minima and maxima per image and component of an fp32 projection ``[B, n, H, W]`` (or
    ``[n, H, W]``: then ``[2, n]``).  A channels-last view whose pixels lie at one constant stride -- ``pca_project``'s result, or the head
    kernel's ``[B, Ho, Wo, Npad]`` logits -- is read in place; any other layout is copied to channels-last once."""
    who = "pca_minmax"
    if not torch.is_tensor(raw):
        raise TypeError(f"naf_amd.{who}: `raw` must be a tensor, got {type(raw).__name__}")
    if raw.dtype != torch.float32:
        raise TypeError(f"naf_amd.{who}: `raw` must be float32, got {raw.dtype}")
    if raw.dim() not in (3, 4) or min(raw.shape) < 1:
        raise ValueError(f"naf_amd.{who}: `raw` must be a non-empty [B, n, H, W] or [n, H, W], got {tuple(raw.shape)}")
    x = raw.detach() if raw.dim() == 4 else raw.detach().unsqueeze(0)
    B, n, H, W = (int(v) for v in x.shape)
    if n > _lib.PCA_MAX_COMPONENTS:
        raise ValueError(f"naf_amd.{who}: n = {n} components; served: 1 <= n <= {_lib.PCA_MAX_COMPONENTS}")
    _gpu(x, "raw")
    ld = int(x.stride(3)) if W > 1 else (int(x.stride(2)) if H > 1 else n)
    if not (x.stride(1) == 1 and ld >= n and (W == 1 or x.stride(3) == ld) and (H == 1 or x.stride(2) == W * ld) and x.data_ptr() % 4 == 0):
        x = x.contiguous(memory_format=torch.channels_last)
        if x.stride(1) != 1:                               # n = 1 or a 1 x 1 grid: torch reports such a tensor dense either way
            x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        ld = n
    dev = x.device
    lib = _lib.load()
    out = torch.empty((B, 2, n), dtype=torch.float32, device=dev)
    workspace, nbytes = _minmax_workspace(lib, H * W, dev)
    with torch.cuda.device(dev), _Timed("pca_minmax"):
        for i in range(B):
            a = _lib.PcaMinmaxArgs()
            a.y, a.minmax = x[i].data_ptr(), out[i].data_ptr()
            a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
            a.P, a.ld, a.n = H * W, ld, n
            _lib.check(lib.naf_pca_minmax(C.byref(a), _stream(x)), "naf_pca_minmax")
    return out if raw.dim() == 4 else out[0]
