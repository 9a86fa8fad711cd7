"""The yardstick of the label-map tests: a restatement of what the reference does with a propagated frame before it scores it
(evaluation/eval_video_seg.py:444-457, ``norm_mask`` :488-496) and with the first frame's annotation (``read_seg`` :638-643, ``to_one_hot``
:611-623).  The reference's module imports hydra and cv2 and cannot run here, so the semantics are written down twice:

  ``literal``   the lines as written: ``F.interpolate(..., mode="bilinear", align_corners=False)`` in fp32 on the CPU (:444-450), the
                ``norm_mask`` loop (:488-496), ``torch.max(dim=0)`` (:453), and the PIL nearest resize (:457) as a gather through the index
                table Pillow's resize reads (``pil_table``; held against Pillow itself by tests/test_label_map_cpu.py)
  ``exact``     the same arithmetic in fp64 throughout, which also returns, per output pixel, the winner's margin over the runner-up

A pixel is UNDECIDED when 0 < margin <= tau, with g the largest difference of two adjacent pixels of ``seg`` and R the smallest range
(max - min) of a channel that is normalised:

    tau = 6 * (2^-21 * max(h, w) * g + 2^-21 * max|seg|) / R

The first term is a one-rounding difference in the source coordinate (whether ``scale * (dst + 0.5) - 0.5`` contracts to an FMA is left open;
fp32 against fp64 scale) times the steepest slope, the second a few ulps in the blend, both carried through the subtract and the divide by
the range.  An fp32 implementation must equal ``exact`` on every decided pixel.  Exact ties (margin 0), a channel without a positive value
(left as it is) and the NaN rule (a positive constant channel is 0 / 0 = NaN everywhere and ``torch.max`` returns the first NaN) are decided.
The share of undecided pixels is capped at ``MAX_UNDECIDED_SHARE`` per case: a condition on the inputs, asserted by the CPU test from this
module alone.

``emulate`` is the library's two-pass arithmetic on the host: fp32, the kernel's order of operations, every operation rounded on its own.

This module is a helper (no tests in it); the cases the GPU test runs are defined here so that the CPU test can check their condition.
"""
import functools

import torch
import torch.nn.functional as F

MAX_UNDECIDED_SHARE = 0.005

# (K, (h, w), mid, out, input construction)
CASES = [
    (3, (9, 11), (15, 19), (13, 23), "smooth"),        # ps 14 / factor 8: non-integer scale; shrink in y, grow in x
    (4, (30, 53), (60, 106), (67, 119), "smooth"),     # exact x2; several workgroups both ways; widths no multiple of 64
    (4, (30, 53), (480, 848), (480, 854), "smooth"),   # the reference's default geometry (ps 16, ups_factor 1), x16
    (1, (5, 7), (5, 7), (5, 7), "smooth"),             # K = 1, scale 1 everywhere
    (64, (12, 20), (21, 35), (40, 33), "blurred"),     # the K limit: a blurred one-hot map, every channel's range near 1
    (2, (1, 1), (3, 3), (2, 2), "constant"),           # every channel a positive constant: NaN everywhere, the lowest channel wins
    (2, (9, 11), (18, 22), (13, 23), "identical"),     # two identical channels: label 0 everywhere
    (3, (9, 11), (18, 22), (13, 23), "zero-among-disjoint"),   # an all-zero channel between two channels with disjoint supports
    (4, (9, 11), (18, 22), (13, 23), "one-constant"),  # channel 2 a positive constant among ordinary ones: NaN, it wins everywhere
    (4, (9, 11), (18, 22), (13, 23), "two-constant"),  # channels 1 and 3 positive constants: the lower wins
]
CASE_IDS = ["K%d-%dx%d-%dx%d-%dx%d-%s" % (c[0], *c[1], *c[2], *c[3], c[4]) for c in CASES]
# every (n_in, n_out) pair the cases resize with (mid -> out, both axes) -- tests/golden/pil_nearest_tables.npz holds them
CASE_PAIRS = sorted({(c[2][i], c[3][i]) for c in CASES for i in (0, 1)})
DAVIS_PAIRS = [(976, 854), (544, 480), (424, 854), (848, 854), (1952, 854), (1088, 480)]
# the tracker case: T frames, C channels, grid, ps, ups_factor, out, n_last_frames, classes
TRACKER = dict(T=5, C=32, grid=(9, 13), ps=14, ups_factor=8, out=(13, 23), n_last_frames=2, K=3, radius=12, topk=5, temperature=0.1)
TRACKER_PAIRS = [(13, 9), (23, 13), (15, 13), (22, 23)]      # first labels -> grid, mid -> out
FIXTURE_PAIRS = sorted(set(CASE_PAIRS) | set(DAVIS_PAIRS) | set(TRACKER_PAIRS))


# ---- Pillow's nearest resize ------------------------------------------------------------------------------------------------------------
def pil_table(n_in, n_out):
    """The source index Image.resize(size, 0) reads for each output index: the affine nearest filter steps xo in doubles."""
    s = float(n_in) / n_out
    xo = 0.5 * s
    idx = []
    for _ in range(n_out):
        idx.append(min(int(xo), n_in - 1))
        xo += s
    return idx


def closed_form_table(n_in, n_out):
    """floor((2x + 1) n_in / (2 n_out)) in integers: NOT what Pillow reads (it differs at 64 columns of 976 -> 854)."""
    return [((2 * x + 1) * n_in) // (2 * n_out) for x in range(n_out)]


def resize_nearest(label_map, out_size):
    """:457 / :641 as a gather: a [H, W] map resized to out_size = (rows, columns)."""
    ty = torch.tensor(pil_table(label_map.shape[0], out_size[0]))
    tx = torch.tensor(pil_table(label_map.shape[1], out_size[1]))
    return label_map[ty][:, tx]


def one_hot_first_frame(labels, size, num_classes=None):
    """read_seg + to_one_hot (:638-643, :611-623): fp32 [1, K, h, w]."""
    small = resize_nearest(labels, size).long()
    K = int(small.max()) + 1 if num_classes is None else num_classes
    return F.one_hot(small, K).permute(2, 0, 1)[None].float()


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _smooth(K, h, w, seed):
    """Smooth soft masks: the softmax over K of 3 x a bicubic-upsampled randn at 1/6 resolution."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(1, K, max(2, -(-h // 6)), max(2, -(-w // 6)), generator=g)
    return torch.softmax(3.0 * F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False), dim=1)[0].float().contiguous()


def make_case(case, seed=0):
    """fp32 seg [K, h, w] of a case."""
    K, (h, w), _, _, kind = case
    if kind == "smooth":
        return _smooth(K, h, w, seed)
    if kind == "blurred":
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        coarse = (yy * 4 // h) * 16 + (xx * 16 // w)                      # 4 x 16 blocks: all 64 labels present
        assert K == 64 and int(coarse.max()) == 63
        onehot = F.one_hot(coarse, K).permute(2, 0, 1)[:, None].float()
        k1 = torch.tensor([0.15, 0.7, 0.15])
        blur = F.conv2d(F.pad(onehot, (1, 1, 1, 1), mode="replicate"), (k1[:, None] * k1[None, :])[None, None])
        # neighbouring blocks mirror each other, and a mirror pair ties to the last bit halfway between them: a little noise per channel
        # and pixel decides those pixels one way or the other and leaves every range near 1
        return (blur[:, 0] + 0.1 * torch.rand(K, h, w, generator=torch.Generator().manual_seed(seed))).contiguous()
    if kind == "constant":
        # powers of two: l0 * c + l1 * c = c * fl(l0 + l1) = c at any weights, so the upsampled channel is exactly constant
        return torch.tensor([0.5, 0.25]).reshape(2, 1, 1).expand(K, h, w).contiguous()
    base = _smooth(4, h, w, seed + 10)
    if kind == "identical":
        return torch.stack([base[0], base[0]])
    if kind == "zero-among-disjoint":
        left = torch.zeros(h, w)
        right = torch.zeros(h, w)
        left[1:6, 0:4] = base[0, 1:6, 0:4]
        right[3:8, 6:11] = base[1, 3:8, 6:11]
        return torch.stack([left, torch.zeros(h, w), right])
    if kind == "one-constant":
        seg = base.clone()
        seg[2] = 0.5                                                      # a power of two: x2 weights (1/4, 3/4) keep it exactly constant
        return seg
    if kind == "two-constant":
        seg = base.clone()
        seg[1] = 0.25
        seg[3] = 0.5
        return seg
    raise ValueError(kind)


# ---- the two forms ----------------------------------------------------------------------------------------------------------------------
def literal(seg, mid, out):
    """:444-457 as written, fp32 on the CPU.  seg [K, h, w] -> uint8 [out_h, out_w]."""
    u = F.interpolate(seg[None].clone(), size=list(mid), mode="bilinear", align_corners=False, recompute_scale_factor=False)[0]
    for c in range(u.shape[0]):                                           # norm_mask
        m = u[c]
        if m.max() > 0:
            m = m - m.min()
            m = m / m.max()
            u[c] = m
    _, lab = torch.max(u, dim=0)
    return resize_nearest(lab.to(torch.uint8), out)


def _axis(n_in, n_out, dtype):
    """Source indices and weights of one axis, align_corners = False, in `dtype`, every operation rounded on its own."""
    scale = torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    src = (scale * (torch.arange(n_out, dtype=dtype) + 0.5) - 0.5).clamp_min(0)
    i0 = src.to(torch.int64).clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = src - i0.to(dtype)
    return i0, i1, 1 - l1, l1


def _upsample(seg, mid, dtype):
    """h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11) over the mid grid, in `dtype`."""
    s = seg.to(dtype)
    y0, y1, h0, h1 = _axis(s.shape[1], mid[0], dtype)
    x0, x1, w0, w1 = _axis(s.shape[2], mid[1], dtype)
    top = w0 * s[:, y0][:, :, x0] + w1 * s[:, y0][:, :, x1]
    bot = w0 * s[:, y1][:, :, x0] + w1 * s[:, y1][:, :, x1]
    return h0[:, None] * top + h1[:, None] * bot


def _normalised(u):
    """norm_mask on [K, H, W] in u's dtype; also the smallest range of a normalised channel (1 when none is)."""
    n = u.clone()
    R = None
    for c in range(u.shape[0]):
        mx, mn = u[c].max(), u[c].min()
        if mx > 0:
            n[c] = (u[c] - mn) / (mx - mn)                                # mx == mn: 0 / 0 = NaN everywhere
            if mx > mn:
                R = float(mx - mn) if R is None else min(R, float(mx - mn))
    return n, (1.0 if R is None else R)


def _first_max(n):
    """torch.max(dim=0) indices on the CPU: the first maximum, a NaN above every number."""
    return torch.max(n, dim=0)[1]


def exact(seg, mid, out):
    """fp64 throughout.  Returns (labels uint8 [out_h, out_w], margin fp64 [out_h, out_w], tau)."""
    u = _upsample(seg, mid, torch.float64)
    n, R = _normalised(u)
    lab = _first_max(n)
    K = n.shape[0]
    nan = torch.isnan(n).any(0)
    if K == 1:
        margin = torch.full(lab.shape, float("inf"), dtype=torch.float64)
    else:
        top2 = torch.topk(torch.nan_to_num(n, nan=0.0), 2, dim=0).values
        margin = top2[0] - top2[1]
        margin[nan] = float("inf")                                        # the NaN rule decides, whatever the numbers beside it
    h, w = seg.shape[1:]
    g = 0.0
    if h > 1:
        g = max(g, float((seg[:, 1:] - seg[:, :-1]).abs().max()))
    if w > 1:
        g = max(g, float((seg[:, :, 1:] - seg[:, :, :-1]).abs().max()))
    tau = 6.0 * (2.0 ** -21 * max(h, w) * g + 2.0 ** -21 * float(seg.abs().max())) / R
    ty, tx = torch.tensor(pil_table(mid[0], out[0])), torch.tensor(pil_table(mid[1], out[1]))
    return lab.to(torch.uint8)[ty][:, tx], margin[ty][:, tx], tau


def undecided(margin, tau):
    return (margin > 0) & (margin <= tau)


def emulate(seg, mid, out):
    """The library's two passes on the host in fp32: pass 1 the minimum and maximum of the upsampled value over the mid grid; pass 2, per
    OUTPUT pixel, the K values at its source mid pixel, (u - sub) / den with (sub, den) = (mn, mx - mn) where mx > 0 and (0, 1) where not,
    the first maximum with a NaN above every number."""
    u = _upsample(seg.float(), mid, torch.float32)
    mx, mn = u.amax((1, 2)), u.amin((1, 2))
    pos = mx > 0
    sub = torch.where(pos, mn, torch.zeros_like(mn))
    den = torch.where(pos, mx - mn, torch.ones_like(mn))
    ty, tx = torch.tensor(pil_table(mid[0], out[0])), torch.tensor(pil_table(mid[1], out[1]))
    v = (u[:, ty][:, :, tx] - sub[:, None, None]) / den[:, None, None]
    return _first_max(v).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def reference(case_index, seed=0):
    """(seg, labels, margin, tau) of CASES[case_index] from ``exact``, computed once per process and shared; callers must not modify it."""
    case = CASES[case_index]
    seg = make_case(case, seed)
    return (seg, *exact(seg, case[2], case[3]))


# ---- the tracker case -------------------------------------------------------------------------------------------------------------------
def tracker_inputs(seed=0):
    """(frames: T bf16 [C, h, w] tensors, first_labels uint8 [H0, W0]) of the TRACKER case."""
    t = TRACKER
    g = torch.Generator().manual_seed(seed)
    h, w = t["grid"]
    base = torch.randn(t["C"], h, w, generator=g)
    frames = [(base + 0.6 * torch.randn(t["C"], h, w, generator=g)).to(torch.bfloat16) for _ in range(t["T"])]   # a scene that persists
    H0, W0 = t["out"]
    yy, xx = torch.meshgrid(torch.arange(H0), torch.arange(W0), indexing="ij")
    labels = torch.zeros(H0, W0, dtype=torch.uint8)
    labels[(yy - 4) ** 2 + (xx - 6) ** 2 <= 9] = 1
    labels[(yy - 8).abs() + (xx - 16).abs() <= 4] = 2
    return frames, labels
