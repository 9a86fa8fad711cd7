"""The yardstick of the denoising-objective tests: a restatement of the reference's ``DenoisingLoss`` (denoising.py:129-177) and
``MetricsCalculator`` (denoising.py:61-126), written as torch ops that run in any floating dtype on the values as given.

  in fp64   the reference every test compares against: the loss terms, the per-pixel SSIM maps, the gradient of ``total`` by autograd,
            the metrics with the reference's fp32 window values widened
  in fp32   the composition of torch ops that ``naf_amd.DenoisingLoss`` / ``denoising_metrics`` replace.  Its own deviation from the
            fp64 form on the same inputs (``E_map`` for an SSIM map, ``E_g`` for the gradient) is the unit the GPU tests' bounds are
            stated in: sigma = e - mu^2 cancels against C2 = 9e-4, so the error of ANY fp32 evaluation depends on the input, and
            is measured rather than guessed

``analytic_grad`` is the closed form of the gradient the kernel evaluates (include/naf_hip.h); tests/test_denoise_cpu.py holds it
against autograd.  tests/golden/denoise_objective.npz (tools/make_denoise_golden.py) holds the reference's own classes' results on one
input pair; the CPU test holds this restatement against it.

This module is a helper (no tests in it); the cases the GPU tests run are defined here so that the CPU tests can use them too.
"""
import functools
import math

import torch
import torch.nn.functional as F

# (B, C, H, W)
CASES = [
    (2, 3, 37, 45),    # several tiles both ways, no multiple of a tile
    (2, 3, 64, 64),    # exact tile multiples
    (1, 2, 33, 130),   # wide
    (3, 1, 70, 3),     # narrower than a tile
    (1, 3, 5, 9),      # smaller than the 11-window
    (1, 3, 2, 70),     # smaller than the 11-window in one direction
    (1, 1, 1, 1),
]
CASE_IDS = ["%dx%dx%dx%d" % c for c in CASES]
WEIGHTS = [(1.0, 1.0, 0.1), (1.0, 5.0, 0.2), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)]
GOLDEN_SHAPE = (2, 3, 20, 24)
GOLDEN_WEIGHTS = (1.0, 5.0, 0.2)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def make_inputs(shape, clamped=False, seed=0):
    """Image-like fp32 (pred, target): target is a smooth pattern in [0, 1] with a flat patch of zeros and a flat patch of ones (the SSIM
    denominators' worst case); pred is target plus sigma = 0.1 noise, equal to target exactly on a patch in the upper right corner, and
    clamped to [0, 1] in the clamped variant (the unclamped one leaves [0, 1])."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W)
    y = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1) / max(H, 8)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W) / max(W, 8)
    b = torch.arange(B, dtype=torch.float64).view(B, 1, 1, 1)
    c = torch.arange(C, dtype=torch.float64).view(1, C, 1, 1)
    target = 0.5 + 0.25 * torch.sin(2 * math.pi * (1.3 * y + 0.21 * c + 0.1 * b)) + 0.25 * torch.cos(2 * math.pi * (1.7 * x - 0.13 * c))
    ph, pw = max(1, H // 4), max(1, W // 4)
    target[:, :, H // 8:H // 8 + ph, W // 8:W // 8 + pw] = 0.0
    target[:, :, H // 2:H // 2 + ph, W // 2:W // 2 + pw] = 1.0
    target = target.clamp(0.0, 1.0).float()
    pred = target + 0.1 * torch.randn(shape, generator=g)
    eh, ew = max(1, H // 5), max(1, W // 5)
    pred[:, :, :eh, W - ew:] = target[:, :, :eh, W - ew:]
    if clamped:
        pred = pred.clamp(0.0, 1.0)
    return pred.contiguous(), target.contiguous()


# ---- DenoisingLoss (denoising.py:142-177), in the dtype of its inputs ---------------------------------------------------------------
def ssim_map_loss(pred, target):
    """The per-pixel map whose mean ``ssim_loss`` subtracts from 1: zero-padded 3 x 3 means, divisor always 9."""
    mu1 = F.avg_pool2d(pred, 3, 1, 1)
    mu2 = F.avg_pool2d(target, 3, 1, 1)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.avg_pool2d(pred * pred, 3, 1, 1) - mu1_sq
    sigma2_sq = F.avg_pool2d(target * target, 3, 1, 1) - mu2_sq
    sigma12 = F.avg_pool2d(pred * target, 3, 1, 1) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def loss_terms(pred, target, weights):
    """``DenoisingLoss(*weights)(pred, target)``: the dict of weighted terms and ``total``, a key present only where its weight is > 0."""
    w1, w2, w3 = weights
    losses = {}
    if w1 > 0:
        losses["l1"] = (pred - target).abs().mean() * w1
    if w2 > 0:
        losses["l2"] = (pred - target).pow(2).mean() * w2
    if w3 > 0:
        losses["ssim"] = (1 - ssim_map_loss(pred, target).mean()) * w3
    losses["total"] = sum(losses.values())
    return losses


def loss_and_grad(pred, target, weights, dtype=torch.float64):
    """(dict of detached terms, SSIM map, gradient of total with respect to pred), all evaluated in ``dtype`` on the values as given."""
    p = pred.detach().to(dtype).requires_grad_(True)
    t = target.detach().to(dtype)
    losses = loss_terms(p, t, weights)
    if torch.is_tensor(losses["total"]) and losses["total"].requires_grad:
        (grad,) = torch.autograd.grad(losses["total"], p)
    else:
        grad = torch.zeros_like(p)
    with torch.no_grad():
        smap = ssim_map_loss(p, t)
    return {k: (v.detach() if torch.is_tensor(v) else torch.tensor(float(v), dtype=dtype)) for k, v in losses.items()}, smap.detach(), grad


def _box(x):
    return F.avg_pool2d(x, 3, 1, 1)


def analytic_grad(pred, target, weights, dtype=torch.float64):
    """The closed form of d total / d pred the kernel evaluates: box is its own adjoint under zero padding, sign(0) = 0."""
    w1, w2, w3 = weights
    p, t = pred.detach().to(dtype), target.detach().to(dtype)
    mu1, mu2 = _box(p), _box(t)
    s1, s2, s12 = _box(p * p) - mu1 * mu1, _box(t * t) - mu2 * mu2, _box(p * t) - mu1 * mu2
    n1, n2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    d1, d2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    S = n1 * n2 / (d1 * d2)
    a = 2 * mu2 * (n2 - n1) / (d1 * d2) - 2 * mu1 * S * (1 / d1 - 1 / d2)
    b = -S / d2
    c = 2 * n1 / (d1 * d2)
    return (w1 * torch.sign(p - t) + 2 * w2 * (p - t) - w3 * (_box(a) + 2 * p * _box(b) + t * _box(c))) / p.numel()


# ---- MetricsCalculator (denoising.py:64-126) ------------------------------------------------------------------------------------
def gaussian_window(window_size=11):
    """``create_window``'s 2-D window as the reference builds it, in fp32: [11, 11]."""
    gaussian = torch.exp(-torch.arange(window_size, dtype=torch.float32).sub(window_size // 2).pow(2) / (2 * (window_size / 6) ** 2))
    gaussian = gaussian / gaussian.sum()
    _1d = gaussian.unsqueeze(1)
    return _1d.mm(_1d.t()).float()


def ssim_map_metrics(pred, target):
    """``calculate_ssim``'s per-pixel map: zero-padded 11 x 11 Gaussian means; the fp32 window values are widened to the inputs' dtype."""
    channel = pred.size(1)
    window = gaussian_window().to(pred.dtype).expand(channel, 1, 11, 11).contiguous()
    conv = lambda v: F.conv2d(v, window, padding=5, groups=channel)  # noqa: E731
    mu1, mu2 = conv(pred), conv(target)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(pred * pred) - mu1_sq
    sigma2_sq = conv(target * target) - mu2_sq
    sigma12 = conv(pred * target) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def metrics(pred, target, clamp=False, dtype=torch.float64):
    """({"psnr", "ssim"} as Python floats, SSIM map), evaluated in ``dtype``; ``clamp`` is the torch.clamp(pred, 0, 1) of denoising.py:302."""
    p, t = pred.detach().to(dtype), target.detach().to(dtype)
    if clamp:
        p = p.clamp(0, 1)
    mse = float((p - t).pow(2).mean())
    psnr = float("inf") if mse == 0 else 20 * math.log10(1.0 / math.sqrt(mse))
    smap = ssim_map_metrics(p, t)
    return {"psnr": psnr, "ssim": float(smap.mean())}, smap


# ---- shared, computed once per process; callers must not modify what they get -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(case_index, clamped):
    return make_inputs(CASES[case_index], clamped=clamped)


@functools.lru_cache(maxsize=None)
def loss_reference(case_index, clamped, weight_index):
    """fp64 terms and gradient of a case, and the fp32 torch composition's own deviations E_map and E_g from them."""
    pred, target = inputs(case_index, clamped)
    w = WEIGHTS[weight_index]
    terms64, map64, grad64 = loss_and_grad(pred, target, w, torch.float64)
    _, map32, grad32 = loss_and_grad(pred, target, w, torch.float32)
    return {"terms": {k: float(v) for k, v in terms64.items()}, "grad": grad64,
            "E_map": float((map32.double() - map64).abs().max()), "E_g": float((grad32.double() - grad64).abs().max())}


@functools.lru_cache(maxsize=None)
def metrics_reference(case_index, clamped, clamp):
    pred, target = inputs(case_index, clamped)
    m64, map64 = metrics(pred, target, clamp, torch.float64)
    _, map32 = metrics(pred, target, clamp, torch.float32)
    return {"metrics": m64, "E_map": float((map32.double() - map64).abs().max())}
