"""The yardstick of the label propagation tests: a restatement of the reference's ``label_propagation`` after feature extraction
(evaluation/eval_video_seg.py:499-561, with ``restrict_neighborhood`` as the mask), evaluated in fp64 on the SAME bf16 inputs the kernel
receives.  The reference's own function cannot run here (it calls ``.cuda()`` and its module imports hydra, cv2 and pandas), so there
is no golden fixture; instead the semantics are written down twice, independently, and the CPU tests hold the two forms together:

  ``dense``     as the reference writes it: normalise, one matmul per context frame, exp, multiply by the [h*w, h*w] neighbourhood mask,
                topk along the source axis, ``aff[aff < tk_val_min] = 0``, normalise, matmul with the label maps
  ``windowed``  per target pixel: gather the clipped window of every frame, threshold at the topk-th largest score (all candidates when
                there are fewer than topk), keep every candidate at or above it, weighted mean with the exponent shifted by the maximum

``windowed`` also reports, per pixel, whether it is AMBIGUOUS: some candidate's score lies within 0 < |s - threshold| < 4 * C * 2^-24
of the threshold, so that a kernel whose scores carry the contract's error (C + 8) * 2^-24 may legitimately keep a different set.  An
exact tie is not ambiguous: both sides keep it.

This module is a helper (no tests in it); the cases the GPU test runs are defined here so that the CPU test can check their condition.
"""
import functools

import torch

# (n, C, h, w, radius, topk, K, duplicate frame 0 as frame 1)
CASES = [
    (1, 32, 9, 13, 1, 5, 3, False),       # one tile row, fewer candidates than topk in the corners (4 < 5)
    (2, 64, 19, 27, 2, 5, 4, False),      # h, w no multiple of the tile, several tiles both ways
    (3, 64, 19, 27, 12, 5, 11, False),    # a window larger than the image on both sides; K no multiple of 4
    (2, 384, 19, 27, 3, 1, 2, False),     # topk = 1, channel chunking
    (2, 64, 19, 27, 2, 5, 4, True),       # exact ties: "exactly k" and "all ties" differ
    (8, 128, 37, 41, 12, 5, 7, False),    # the reference's own n / radius / topk over several tiles in both directions
]
CASE_IDS = ["n%d-C%d-%dx%d-r%d-k%d-K%d%s" % (c[:7] + ("-dup" if c[7] else "",)) for c in CASES]
TEMPERATURE = 0.1
MAX_AMBIGUOUS_SHARE = 0.03


def ambiguity_margin(C):
    return 4.0 * C * 2.0 ** -24


def make_case(case, seed=0):
    """bf16 target [C, h, w], list of n bf16 context frames, fp32 segs [n, K, h, w] (positive, summing to one over K)."""
    n, C, h, w, _, _, K, dup = case
    g = torch.Generator().manual_seed(seed)
    target = torch.randn(C, h, w, generator=g).to(torch.bfloat16)
    context = [torch.randn(C, h, w, generator=g).to(torch.bfloat16) for _ in range(n)]
    if dup:
        context[1] = context[0].clone()
    segs = torch.rand(n, K, h, w, generator=g) + 0.05
    segs = (segs / segs.sum(1, keepdim=True)).float()
    return target, context, segs


def _normalized(x):
    """F.normalize(x, dim=channel, p=2, eps=1e-12) in fp64 on the values as given."""
    x = x.double()
    return x / x.pow(2).sum(0, keepdim=True).sqrt().clamp_min(1e-12)


def neighbourhood_mask(h, w, radius):
    """restrict_neighborhood: mask[p, q] = 1 when target pixel p and source pixel q are within `radius` in both directions."""
    ii, jj = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    return ((ii[:, None] - ii[None, :]).abs() <= radius) & ((jj[:, None] - jj[None, :]).abs() <= radius)


def dense(target, context, segs, radius, topk, temperature=TEMPERATURE):
    """eval_video_seg.py:539-560 line by line, in fp64.  Returns [1, K, h, w]."""
    C, h, w = target.shape
    n, K = segs.shape[:2]
    feat_tar = _normalized(target).reshape(C, h * w).T                                    # (h w) c
    feat_sources = torch.stack([_normalized(f).reshape(C, h * w) for f in context])      # n x c x (h w)
    aff = torch.exp(torch.bmm(feat_tar.unsqueeze(0).repeat(n, 1, 1), feat_sources) / temperature)
    aff = aff * neighbourhood_mask(h, w, radius).double().unsqueeze(0)
    aff = aff.transpose(2, 1).reshape(-1, h * w)                                          # n*h*w (keys) x h*w (queries)
    tk_val, _ = torch.topk(aff, dim=0, k=topk)
    tk_val_min, _ = torch.min(tk_val, dim=0)
    aff[aff < tk_val_min] = 0
    aff = aff / torch.sum(aff, keepdim=True, dim=0)
    sg = segs.double().reshape(n, K, -1).transpose(2, 1).reshape(-1, K).T                # K x n*h*w
    return torch.mm(sg, aff).reshape(1, K, h, w)


def windowed(target, context, segs, radius, topk, temperature=TEMPERATURE):
    """The per-pixel form.  Returns (out [1, K, h, w] fp64, ambiguous [h, w] bool, kept [h, w] int: the size of each kept set)."""
    C, h, w = target.shape
    n, K = segs.shape[:2]
    q = _normalized(target)
    ctx = torch.stack([_normalized(f) for f in context])                                  # n x C x h x w
    sg = segs.double()
    out = torch.zeros(1, K, h, w, dtype=torch.float64)
    ambiguous = torch.zeros(h, w, dtype=torch.bool)
    kept_n = torch.zeros(h, w, dtype=torch.int64)
    margin = ambiguity_margin(C)
    for i in range(h):
        i0, i1 = max(0, i - radius), min(h, i + radius + 1)
        for j in range(w):
            j0, j1 = max(0, j - radius), min(w, j + radius + 1)
            s = torch.einsum("c,ncyx->nyx", q[:, i, j], ctx[:, :, i0:i1, j0:j1]).reshape(-1)
            lab = sg[:, :, i0:i1, j0:j1].permute(0, 2, 3, 1).reshape(-1, K)
            if s.numel() >= topk:
                theta = torch.topk(s, topk).values[-1]
                d = (s - theta).abs()
                ambiguous[i, j] = bool(((d > 0) & (d < margin)).any())
                keep = s >= theta
            else:
                keep = torch.ones_like(s, dtype=torch.bool)
            wgt = torch.exp((s[keep] - s.max()) / temperature)
            out[0, :, i, j] = (wgt[:, None] * lab[keep]).sum(0) / wgt.sum()
            kept_n[i, j] = int(keep.sum())
    return out, ambiguous, kept_n


@functools.lru_cache(maxsize=None)
def reference(case_index, seed=0):
    """(inputs, windowed result) of CASES[case_index], computed once per process and shared; callers must not modify it."""
    case = CASES[case_index]
    inputs = make_case(case, seed)
    return inputs, windowed(*inputs, radius=case[4], topk=case[5])
