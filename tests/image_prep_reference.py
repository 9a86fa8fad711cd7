"""The yardstick of the frame-preparation tests (``naf_amd.prepare_views`` / naf_image_prep): three restatements of a view -- first resize,
normalise, second resize, store -- and the bounds that relate them.  No GPU and no library: numpy and torch on the host (``torch_composition``
runs on whatever device it is given).

``literal32``  the semantics of include/naf_hip.h, operation by operation in numpy float32 (every numpy operation on float32 arrays is one
               correctly rounded fp32 operation; nothing is fused).  The kernel is asked for these BITS.
``exact``      the same taps and the same fp32 coordinates (``real``, ``t``), everything after them in fp64: the weights from ``t``, the blends,
               the source divide, the normalisation.  Alongside each value it carries the abs-sum S of the chain that produced it:
               ``sum |w| |v|`` through a resize, ``(S + |mean|) / |std|`` through the normalisation, ``sum |w2| S`` through the second resize
               (and the cubic weights' own error, ``wterm``, below).
``torch_composition``  the reference's own calls: ``ToTensor``'s divide on the host, ``F.interpolate(align_corners=False)``, a tensor subtract and a
               tensor divide, ``F.interpolate`` again (evaluation/eval_video_seg.py:578-595, train.py:115-126).

**The blend bound** is ``r * 2**-24 * S``: r fp32 roundings of relative error 2**-24 each on the longest path from a source value to the
result, each charged against the abs-sum of what it rounds.  r is COUNTED from ``literal32`` (``roundings``), not tuned:

    source   uint8: the divide by 255                                                        1      (fp32 / bf16 sources: 0)
    bilinear l0 = 1 - l1 (l1 is shared with ``exact``), w * v, the row sum; the same three over the rows          6
    bicubic  a weight is 2 roundings of its argument (u = 1 - t, u + 1) and 6 operations of c2 (c1: 1 + 5);
             then w * v and three additions of the row pass; the same twelve over the four row results           24
    none                                                                                     0
    normalise  the subtract and the divide                                                   2

so uint8 -> bilinear -> normalise -> bicubic is r = 1 + 6 + 2 + 24 = 33.  A bf16 store adds one rounding of relative error 2**-8.

**The cubic weights' term.**  ``r * 2**-24 * S`` charges a weight's roundings against |w| |v|.  That holds for a bilinear weight, which is one
operation whose rounding is relative to the weight itself.  A cubic weight is a chain of six -- c2(2) = ((-0.75 * 2 + 3.75) * 2 - 6) * 2 + 3
passes through 4.5 on its way to 0 -- and its roundings are relative to those intermediates, not to the result: a weight near 0 carries an
absolute error of up to 30 x 2**-24.  With ``r * 2**-24 * S`` alone the bound is not one: 2 x 2 -> bicubic 9 x 9, where clamped taps repeat one
pixel under weights that cancel, has |literal32 - exact| = 21.3 x 2**-24 against 24 x 2**-24 x S = 15.1 x 2**-24 (two restatements, no kernel
involved).  So ``exact`` also carries ``wterm``: with e the running error bound of each cubic weight (``_running_c1`` / ``_running_c2``: every
operation's result in magnitude, carried through the multiplications after it, plus the rounding of the argument; between 2 and 32),
``sum |wy| e_x S_in + sum e_y |wx| S_in`` per bicubic stage, carried through the normalisation (1 / |std|) and a second stage's ``sum |w2|`` like an
error.  ``blend_bound = 2**-24 * (r * S + wterm)``; wterm is 0 for a view without a bicubic resize, and the r of a bicubic stage still counts
the weights' roundings, so the bound errs on the wide side there.  Measured on the cases (tests/test_image_prep_cpu.py prints them):
|literal32 - exact| is at most 0.26 of the bound on fp32 views (0.93 where the view is the normalisation alone, r = 2).

**The coordinate term** stands between the stated semantics and torch, as DESIGN 4.1h's tau does: ATen rounds the source coordinate once
more or once less (a fused multiply-add on the device; another expression, partly in other precision, in its CPU kernels).  Per axis that
moves ``src`` by at most two ulps at n_in, ``eps = 2**-22 * n_in``; a resize is continuous in ``src`` with slope at most ``kappa * g``, g the
steepest adjacent difference of that stage's input and kappa = 1 (bilinear) or 4 (bicubic: with P the partial sums of the weights'
derivatives, |sum w' v| <= sum |P| g <= (0.75 + 2.1 + 0.75) g).  The first stage's term is carried through the normalisation (1 / min |std|) and
through the second stage's ``sum |w2|``; the second stage's own term is added.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
F32 = np.float32
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BACKBONE_MEAN, BACKBONE_STD = (0.5, 0.45, 0.4), (0.5, 0.26, 0.27)          # some backbone's statistics: not ImageNet's, not all different
R_SOURCE_U8, R_NORMALISE = 1, 2
R_RESIZE = {None: 0, "bilinear": 6, "bicubic": 24}
KAPPA = {None: 0.0, "bilinear": 1.0, "bicubic": 4.0}


# ---- a view as plain data -------------------------------------------------------------------------------------------------------------------
def view_spec(v, H, W):
    """(size1, mode1, mean, std, size2, mode2, dtype) of a ``naf_amd.PrepView`` (or of an object with its attributes) on an H x W source."""
    size1 = (H, W) if v.size is None else tuple(int(s) for s in v.size)
    if v.then is None:
        size2, mode2 = size1, None
    else:
        size2, mode2 = tuple(int(s) for s in v.then[0]), v.then[1]
    mean = None if v.mean is None else tuple(float(F32(m)) for m in v.mean)      # rounded to fp32 once, as the host does
    std = None if v.std is None else tuple(float(F32(s)) for s in v.std)
    return size1, v.mode, mean, std, size2, mode2, v.dtype


def roundings(src_dtype, spec):
    _, mode1, mean, _, _, mode2, _ = spec
    return (R_SOURCE_U8 if src_dtype == torch.uint8 else 0) + R_RESIZE[mode1] + (R_NORMALISE if mean is not None else 0) + R_RESIZE[mode2]


# ---- the source ---------------------------------------------------------------------------------------------------------------------------
def _source_u8_or_float(src, hflip):
    """[B, 3, H, W] numpy array of the source as stored (uint8, or float32 with bf16 widened), columns mirrored when ``hflip``."""
    if src.dtype == torch.uint8:
        a = src.cpu().numpy()
        a = (a if a.ndim == 4 else a[None]).transpose(0, 3, 1, 2)
    else:
        a = src.cpu().float().numpy()
        a = a if a.ndim == 4 else a[None]
    return np.ascontiguousarray(a[..., ::-1] if hflip else a)


# ---- one axis: taps, fp32 weights, fp64 weights from the same fp32 t ----------------------------------------------------------------------------
def _c1(x, one, k125, k225):
    return (((k125 * x) - k225) * x) * x + one


def _c2(x, k075, k375, k6, k3):
    return ((((k075 * x) - k375) * x) + k6) * x - k3


def _running_c1(x):
    """Bound, in units of 2**-24, of the absolute error of c1 evaluated in fp32 at x in [0, 1]: every operation's result in magnitude, carried
    through the multiplications that follow it, plus the rounding of the argument (|c1'| <= 1.35)."""
    p1 = 1.25 * x
    p2 = p1 - 2.25
    p3 = p2 * x
    p4 = p3 * x
    e = ((np.abs(p1) + np.abs(p2)) * x + np.abs(p3)) * x + np.abs(p4) + np.abs(p4 + 1.0)
    return e + 1.35


def _running_c2(x):
    """The same for c2 at x in [1, 2] (|c2'| <= 0.75; the argument is rounded twice, each time by at most 2**-24 x)."""
    p1 = -0.75 * x
    p2 = p1 + 3.75
    p3 = p2 * x
    p4 = p3 - 6.0
    p5 = p4 * x
    e = (((np.abs(p1) + np.abs(p2)) * x + np.abs(p3) + np.abs(p4)) * x + np.abs(p5)) + np.abs(p5 + 3.0)
    return e + 2 * 0.75 * x


def axis(n_in, n_out, mode):
    """(idx [n_out, n] int64, w32 [n_out, n] float32, w64 [n_out, n] float64, werr [n_out, n] float64) of resizing n_in -> n_out; n = 1
    (none), 2 or 4.  ``werr`` is the cubic weights' absolute error in units of 2**-24 (module docstring); 0 for the other modes."""
    if mode is None:
        assert n_in == n_out, "mode none requires equal sizes"
        idx = np.arange(n_out, dtype=np.int64)[:, None]
        return idx, np.ones((n_out, 1), F32), np.ones((n_out, 1), np.float64), np.zeros((n_out, 1), np.float64)
    scale = F32(n_in) / F32(n_out)
    dst = np.arange(n_out, dtype=F32)
    real = (scale * (dst + F32(0.5))) - F32(0.5)
    assert real.dtype == F32
    if mode == "bilinear":
        src = np.maximum(real, F32(0))
        i0 = src.astype(np.int32)
        i1 = np.minimum(i0 + 1, n_in - 1)
        l1 = src - i0.astype(F32)
        l0 = F32(1) - l1
        t = l1.astype(np.float64)
        w64 = np.stack([1.0 - t, t], 1)
        return np.stack([i0, i1], 1).astype(np.int64), np.stack([l0, l1], 1).astype(F32), w64, np.zeros_like(w64)
    assert mode == "bicubic", mode
    fl = np.floor(real)
    t = real - fl
    u = F32(1) - t
    i = fl.astype(np.int64)
    idx = np.clip(np.stack([i - 1, i, i + 1, i + 2], 1), 0, n_in - 1)
    k32 = dict(one=F32(1), k125=F32(1.25), k225=F32(2.25))
    q32 = dict(k075=F32(-0.75), k375=F32(-3.75), k6=F32(-6), k3=F32(-3))
    w32 = np.stack([_c2(t + F32(1), **q32), _c1(t, **k32), _c1(u, **k32), _c2(u + F32(1), **q32)], 1)
    assert w32.dtype == F32
    t64 = t.astype(np.float64)
    k64, q64 = dict(one=1.0, k125=1.25, k225=2.25), dict(k075=-0.75, k375=-3.75, k6=-6.0, k3=-3.0)
    w64 = np.stack([_c2(t64 + 1.0, **q64), _c1(t64, **k64), _c1(1.0 - t64, **k64), _c2(2.0 - t64, **q64)], 1)
    werr = np.stack([_running_c2(t64 + 1.0), _running_c1(t64), _running_c1(1.0 - t64), _running_c2(2.0 - t64)], 1)
    return idx, w32, w64, werr


def blend(img, iy, wy, ix, wx):
    """Rows first: ((v0 wx0 + v1 wx1) + v2 wx2) + v3 wx3 left to right, then the same form with wy over the row results.  ``img`` and the
    weights are of ONE dtype (float32: every operation is one fp32 rounding)."""
    assert img.dtype == wy.dtype == wx.dtype
    acc = None
    for j in range(iy.shape[1]):
        rows = img[:, :, iy[:, j], :]
        r = None
        for i in range(ix.shape[1]):
            term = wx[:, i][None, None, None, :] * rows[:, :, :, ix[:, i]]
            r = term if r is None else r + term
        term = wy[:, j][None, None, :, None] * r
        acc = term if acc is None else acc + term
    assert acc.dtype == img.dtype
    return acc


def _store(a32, dtype):
    return torch.from_numpy(np.ascontiguousarray(a32)).to(dtype)            # bf16: round to nearest even


# ---- literal32 -----------------------------------------------------------------------------------------------------------------------------
def literal32(src, spec, hflip=False):
    """The view as include/naf_hip.h states it, in numpy float32.  Returns a torch tensor [B, 3, h, w] of the view's dtype."""
    size1, mode1, mean, std, size2, mode2, dtype = spec
    a = _source_u8_or_float(src, hflip)
    v = a.astype(F32) / F32(255) if a.dtype == np.uint8 else a.astype(F32)
    H, W = v.shape[2:]
    if mode1 is not None:
        (iy, wy, _, _), (ix, wx, _, _) = axis(H, size1[0], mode1), axis(W, size1[1], mode1)
        v = blend(v, iy, wy, ix, wx)
    else:
        assert (H, W) == size1
    if mean is not None:
        v = (v - np.array(mean, F32)[None, :, None, None]) / np.array(std, F32)[None, :, None, None]
    if mode2 is not None:
        (iy, wy, _, _), (ix, wx, _, _) = axis(size1[0], size2[0], mode2), axis(size1[1], size2[1], mode2)
        v = blend(v, iy, wy, ix, wx)
    else:
        assert size1 == size2
    assert v.dtype == F32
    return _store(v, dtype)


# ---- exact ---------------------------------------------------------------------------------------------------------------------------------
def _steepest(v):
    g = 0.0
    if v.shape[2] > 1:
        g = max(g, float(np.abs(np.diff(v, axis=2)).max()))
    if v.shape[3] > 1:
        g = max(g, float(np.abs(np.diff(v, axis=3)).max()))
    return g


def exact(src, spec, hflip=False):
    """(value, S, coord, wterm): the fp64 value [B, 3, h, w], the abs-sum of its chain, the coordinate term and the cubic weights' term (arrays
    or 0.0), all float64; the last in units of 2**-24."""
    size1, mode1, mean, std, size2, mode2, _ = spec
    a = _source_u8_or_float(src, hflip)
    v = a.astype(np.float64) / 255.0 if a.dtype == np.uint8 else a.astype(np.float64)
    S = np.abs(v)
    H, W = v.shape[2:]
    coord, wterm = 0.0, 0.0
    if mode1 is not None:
        coord = KAPPA[mode1] * _steepest(v) * (2.0 ** -22) * (H + W)
        (iy, _, wy, ey), (ix, _, wx, ex) = axis(H, size1[0], mode1), axis(W, size1[1], mode1)
        wterm = blend(S, iy, np.abs(wy), ix, ex) + blend(S, iy, ey, ix, np.abs(wx))
        v, S = blend(v, iy, wy, ix, wx), blend(S, iy, np.abs(wy), ix, np.abs(wx))
    if mean is not None:
        m, s = np.array(mean, np.float64)[None, :, None, None], np.array(std, np.float64)[None, :, None, None]
        v, S = (v - m) / s, (S + np.abs(m)) / np.abs(s)
        coord, wterm = coord / float(np.abs(s).min()), wterm / np.abs(s)
    if mode2 is not None:
        c2 = KAPPA[mode2] * _steepest(v) * (2.0 ** -22) * (size1[0] + size1[1])
        (iy, _, wy, ey), (ix, _, wx, ex) = axis(size1[0], size2[0], mode2), axis(size1[1], size2[1], mode2)
        L2 = np.abs(wy).sum(1)[None, None, :, None] * np.abs(wx).sum(1)[None, None, None, :]
        carried = blend(np.broadcast_to(wterm, S.shape).astype(np.float64), iy, np.abs(wy), ix, np.abs(wx))
        wterm = carried + blend(S, iy, np.abs(wy), ix, ex) + blend(S, iy, ey, ix, np.abs(wx))
        v, S = blend(v, iy, wy, ix, wx), blend(S, iy, np.abs(wy), ix, np.abs(wx))
        coord = coord * L2 + c2
    return v, S, coord, wterm


def blend_bound(src_dtype, spec, S, wterm):
    """r * 2**-24 * S, plus the cubic weights' own error (0 for a view without a bicubic resize)."""
    return roundings(src_dtype, spec) * U * S + U * wterm


def store_term(dtype, magnitude, sides=1):
    """What the store adds between a stored result and an unrounded one (``sides=1``) or another stored one (``sides=2``)."""
    return sides * 2.0 ** -8 * magnitude if dtype == torch.bfloat16 else 0.0     # 8 significant bits: half a spacing is 2^-8 relative


# ---- the reference's own calls ---------------------------------------------------------------------------------------------------------------
def torch_composition(src, spec, hflip=False, device="cpu"):
    size1, mode1, mean, std, size2, mode2, dtype = spec
    if src.dtype == torch.uint8:
        x = src.cpu()
        x = (x if x.dim() == 4 else x[None]).permute(0, 3, 1, 2).contiguous().float().div(255)     # ToTensor, on the host
    else:
        x = src.cpu().float()
        x = x if x.dim() == 4 else x[None]
    x = x.to(device)
    if hflip:
        x = torch.flip(x, dims=[-1])
    if mode1 is not None:
        x = F.interpolate(x, size=list(size1), mode=mode1, align_corners=False)
    if mean is not None:
        m = torch.tensor(mean, dtype=torch.float32, device=device).view(1, 3, 1, 1)
        s = torch.tensor(std, dtype=torch.float32, device=device).view(1, 3, 1, 1)
        x = (x - m) / s
    if mode2 is not None:
        x = F.interpolate(x, size=list(size2), mode=mode2, align_corners=False)
    return x.to(dtype)


# ---- the cases of the GPU tests (and of the CPU tests that hold the yardstick against itself) ------------------------------------------------
def _u8(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _f32(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 1.5 - 0.25


def _views(name):
    from naf_amd import PrepView, davis_frame_views, training_views
    if name == "small":                       # 1. non-integer ratios, up and down on different axes
        return [PrepView((12, 10), "bilinear", BACKBONE_MEAN, BACKBONE_STD, then=((5, 14), "bicubic"))]
    if name == "davis":                       # 2. the two views at ups_factor 8, and the upsampler's at ups_factor 1: one call of 3
        v8, grid, hr8 = davis_frame_views((480, 854), 16, 8, BACKBONE_MEAN, BACKBONE_STD)
        v1, _, hr1 = davis_frame_views((480, 854), 16, 1, BACKBONE_MEAN, BACKBONE_STD)
        assert grid == (30, 53) and hr8 == (240, 424) and hr1 == (30, 53)
        return [v8[0], v8[1], v1[1]]
    if name == "training":                    # 3. 56 x 56, its 28 x 28 shrink, hr_grid 4 -> 16 x 16, and a plain upsampler view
        return training_views(56, (4, 4), 28, BACKBONE_MEAN, BACKBONE_STD) + [PrepView(mean=IMAGENET_MEAN, std=IMAGENET_STD)]
    if name == "one_pixel":                   # 4. every tap clamped
        return [PrepView((4, 6), "bilinear"), PrepView((4, 6), "bicubic"), PrepView(then=((4, 6), "bicubic"), mean=BACKBONE_MEAN, std=BACKBONE_STD)]
    if name == "two_by_two":
        return [PrepView((9, 9), "bicubic")]
    if name == "skipping":                    # taps skip pixels down (37 -> 14), crowd up (53 -> 70)
        return [PrepView((14, 70), "bicubic"), PrepView((14, 70), "bilinear", then=((37, 53), "bicubic"))]
    if name in ("batch_bf16", "bf16_source"):  # 5. B = 3, bf16 outputs (and a bf16 source)
        return [PrepView((11, 13), "bilinear", BACKBONE_MEAN, BACKBONE_STD, dtype=torch.bfloat16),
                PrepView((11, 13), "bicubic", IMAGENET_MEAN, IMAGENET_STD, then=((16, 9), "bilinear"), dtype=torch.bfloat16),
                PrepView(dtype=torch.bfloat16)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def source(name):
    """The case's source tensor on the host (never modified)."""
    if name == "small":
        return _u8((1, 7, 9, 3), 1)
    if name == "davis":
        return _u8((480, 854, 3), 2)
    if name == "training":
        return _f32((2, 3, 64, 64), 3)
    if name == "one_pixel":
        return _f32((3, 1, 1), 4)
    if name == "two_by_two":
        return _f32((1, 3, 2, 2), 5)
    if name == "skipping":
        return _u8((37, 53, 3), 6)
    if name == "batch_bf16":
        return _f32((5, 3, 10, 17), 7)[::2]                      # three different images, a batch stride of two images
    if name == "bf16_source":
        return _f32((3, 3, 10, 17), 8).to(torch.bfloat16)
    raise KeyError(name)


CASES = ("small", "davis", "training", "one_pixel", "two_by_two", "skipping", "batch_bf16", "bf16_source")


def views(name):
    return _views(name)


def specs(name, src=None):
    src = source(name) if src is None else src
    H, W = (src.shape[-3], src.shape[-2]) if src.dtype == torch.uint8 else (src.shape[-2], src.shape[-1])
    return [view_spec(v, int(H), int(W)) for v in _views(name)]


@functools.lru_cache(maxsize=None)
def reference(name, hflip=False):
    """Per view of the case: (literal32 tensor, exact value, S, coord, wterm), computed once and shared; callers do not modify them."""
    src = source(name)
    return [(literal32(src, sp, hflip),) + exact(src, sp, hflip) for sp in specs(name)]


def check_against_exact(got, src_dtype, spec, value, S, wterm, extra=0.0, sides=1):
    """max of |got - value| / bound over the view (must be <= 1), bound = blend bound + extra (+ the store's rounding)."""
    bound = blend_bound(src_dtype, spec, S, wterm) + extra
    bound = bound + store_term(spec[-1], np.abs(value) + bound, sides)
    err = np.abs(got.detach().cpu().double().numpy() - value)
    tiny = np.finfo(np.float64).tiny
    return float((err / np.maximum(bound, tiny)).max()), float(err.max()), float(np.max(bound))
