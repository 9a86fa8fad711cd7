"""fp64 restatements of the two adjoints the training call needs when the guidance image is larger than the output
(train.py:126-127 feeds an image 4x the output): the adjoint of ``F.adaptive_avg_pool2d`` (naf.py:34, naf_pool_guidance_bwd) and of the
bilinear pre-shrink ``F.interpolate(mode="bilinear", align_corners=False)`` with respect to the image (naf.py:39-48,
naf_preshrink_image_bwd).  Each returns, next to the gradient, the per-element quantities the tests' error bounds are stated in: the
number of terms and the sum of their magnitudes.

Both adjoints factor over the two axes, so each is two small matrices: ``d_in = A_h^T . d_out . A_w`` per (sample, channel) plane.

The bilinear weights are computed in fp32 exactly as resize.hip states them (and as ATen's device kernel does): the coordinate
``scale * (dst + 0.5) - 0.5`` carries a rounding error of about ``extent * 2^-24``, which lands in the weights undiminished -- a restatement
with fp64 coordinates would differ from the kernel by that much, far more than the accumulation error the tests bound.  Everything after the
weights is fp64.  The shapes the tests use live here so that the CPU and the GPU tests cannot drift apart."""
import numpy as np
import torch

# (H, W) -> (Ho, Wo), C; all with B = 2
POOL_SHAPES = [((8, 12), (4, 6), 32),        # divisible, area 4
               ((16, 16), (4, 4), 256),      # the training ratio
               ((7, 10), (3, 4), 40),        # overlapping windows, C / 8 not a power of two
               ((5, 5), (5, 5), 8),          # identity
               ((3, 4), (7, 9), 32),         # output larger than the image: many windows per pixel
               ((9, 8), (3, 8), 32)]         # one axis pooled only
POOL_BATCH = 2

# name -> (B, H, W), (Hs, Ws)
RESIZE_CASES = {"a": ((2, 20, 24), (5, 6)),
                "b": ((1, 9, 31), (9, 7)),           # scale 1 on one axis
                "c": ((1, 17, 17), (16, 16))}        # scale between 1 and 2, border clamp


# ---- adaptive average pooling ---------------------------------------------------------------------------------------------------
def pool_window(i, n_in, n_out):
    """[start, end) of output index i, as torch: floor(i * in / out), ceil((i + 1) * in / out)."""
    return (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)


def pool_windows_of(p, n_in, n_out):
    """Closed form: the output indices whose window holds input index p, first and last (inclusive)."""
    return (p * n_out) // n_in, -((-(p + 1) * n_out) // n_in) - 1


def pool_axis(n_in, n_out):
    """[n_in, n_out] fp64: 1 / window length where output i's window holds input p (by the closed form), and the window count per input."""
    A = torch.zeros(n_in, n_out, dtype=torch.float64)
    for p in range(n_in):
        lo, hi = pool_windows_of(p, n_in, n_out)
        for i in range(lo, hi + 1):
            s, e = pool_window(i, n_in, n_out)
            A[p, i] = 1.0 / (e - s)
    return A, (A > 0).sum(1)


def pool_adjoint(dy, in_size):
    """dy [B, C, Ho, Wo] (any float dtype) -> (dx fp64 [B, C, H, W], n int [H, W] windows per pixel, mag fp64 = sum_j |dy_j| / area_j)."""
    H, W = in_size
    Ho, Wo = dy.shape[-2:]
    Ah, nh = pool_axis(H, Ho)
    Aw, nw = pool_axis(W, Wo)
    d = dy.double()
    dx = torch.einsum("yi,bcij,xj->bcyx", Ah, d, Aw)
    mag = torch.einsum("yi,bcij,xj->bcyx", Ah, d.abs(), Aw)
    return dx, nh[:, None] * nw[None, :], mag


# ---- bilinear resize ------------------------------------------------------------------------------------------------------------
def bilinear_taps(n_in, n_out):
    """The forward's fp32 source coordinates of one axis (resize.hip): per output index the two neighbours p0, p1 = min(p0 + 1, in - 1) and their
    weights l0 = 1 - l1, l1 = src - p0, src = max(0, scale * (dst + 0.5) - 0.5), scale = in / out; every operation rounded to fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    f = np.maximum(scale * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0.0))
    assert f.dtype == np.float32
    p0 = f.astype(np.int32)
    p1 = np.minimum(p0 + 1, n_in - 1)
    l1 = f - p0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    return p0, p1, l0, l1


def bilinear_axis(n_in, n_out):
    """[n_out, n_in] fp64 weight matrix of one axis from the fp32 taps (p0 and p1 may coincide on the last row: the weights add), the number of
    taps that land on each input index, and a 0/1 matrix of the input indices within one of an output's taps."""
    p0, p1, l0, l1 = bilinear_taps(n_in, n_out)
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    near = torch.zeros(n_out, n_in, dtype=torch.float64)
    cnt = torch.zeros(n_in, dtype=torch.int64)
    for o in range(n_out):
        M[o, p0[o]] += float(l0[o])
        M[o, p1[o]] += float(l1[o])
        cnt[p0[o]] += 1
        cnt[p1[o]] += 1
        near[o, max(int(p0[o]) - 1, 0):min(int(p1[o]) + 2, n_in)] = 1.0
    return M, cnt, near


def resize_adjoint(dout, in_size):
    """dout [B, 3, Hs, Ws] -> (dimage fp64 [B, 3, H, W], T int [H, W] terms per element, mag fp64 = sum of |term|,
    near fp64 = sum of |g| over the output pixels with a tap within one row and one column of the element)."""
    H, W = in_size
    Hs, Ws = dout.shape[-2:]
    Mh, ch, nh = bilinear_axis(H, Hs)
    Mw, cw, nw = bilinear_axis(W, Ws)
    g = dout.double()
    d = torch.einsum("iy,bcij,jx->bcyx", Mh, g, Mw)
    mag = torch.einsum("iy,bcij,jx->bcyx", Mh, g.abs(), Mw)      # the weights are >= 0
    near = torch.einsum("iy,bcij,jx->bcyx", nh, g.abs(), nw)
    return d, ch[:, None] * cw[None, :], mag, near


def bilinear_scan_offsets(n_in, n_out):
    """Offsets o - floor(p * out / in) of every (output o, input p) pair with a tap of o on p: what a gather kernel's candidate scan must cover."""
    p0, p1, _, _ = bilinear_taps(n_in, n_out)
    off = set()
    for o in range(n_out):
        for p in (int(p0[o]), int(p1[o])):
            off.add(o - (p * n_out) // n_in)
    return off
