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
``CASES`` are random (gaussian) features at C <= 384; ``LIMIT_CASES`` reach the limits of the served range, from C = 416 on with LATTICE
features whose scores are exact (``lattice_features``), because the ambiguity margin grows with C and gaussian features would make 4 - 47 %
of the pixels ambiguous there.  ``windowed_with_defect`` restates what a subtly wrong kernel would compute, for the sensitivity tests.
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
    tk_val, _ = torch.topk(aff, dim=0, k=min(topk, aff.shape[0]))                         # (the reference raises where n*h*w < topk)
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


# ---- the limits of the served range ------------------------------------------------------------------------------------
# (n, C, h, w, radius, topk, K, features).  Which kernel instantiation (KSMAX), how many 16-key blocks per halo row (nkb) and which key
# stream (nbuf 2 double-buffered, nbuf 1 single) a case launches is the library's decision; tests/test_propagate_cpu.py reads it from
# naf_propagate_plan and asserts that CASES and LIMIT_CASES together reach every instantiation and both streams.
LIMIT_CASES = [
    (2, 160, 11, 21, 2, 5, 3, "gauss"),          # KSMAX 8, partly filled (5 chunks)
    (2, 256, 16, 32, 3, 5, 4, "gauss"),          # KSMAX 8 full; h, w exact tile multiples
    (2, 544, 9, 17, 1, 3, 2, "gauss"),           # KSMAX 24 partly filled; one column in a second tile
    (2, 416, 9, 19, 2, 7, 2, "lattice"),         # KSMAX 16 partly filled
    (2, 512, 8, 16, 4, 16, 5, "lattice"),        # KSMAX 16 full; topk 16 (no +inf slot); exactly one tile; kept sets above 16
    (2, 768, 10, 18, 15, 5, 64, "lattice"),      # KSMAX 24 full, single buffer, 3 key blocks, K 64
    (2, 800, 9, 19, 9, 5, 3, "lattice"),         # KSMAX 32 partly filled, double buffer
    (2, 1024, 9, 19, 1, 5, 64, "lattice"),       # KSMAX 32, single buffer with 2 key blocks
    (2, 1024, 11, 21, 9, 5, 3, "lattice"),       # KSMAX 32, single buffer with 3 key blocks
    (3, 1024, 17, 33, 15, 16, 64, "lattice"),    # every limit but n at once; tiles both ways; the frame changes inside the single buffer
    (16, 32, 9, 17, 2, 16, 1, "lattice"),        # n 16, K 1, kept sets far above the 16 list slots
    (1, 64, 1, 1, 1, 5, 2, "lattice"),           # grids thinner than a tile; fewer candidates than topk
    (2, 64, 1, 40, 3, 5, 2, "lattice"),
    (2, 64, 20, 1, 3, 5, 2, "lattice"),
]
LIMIT_IDS = ["n%d-C%d-%dx%d-r%d-k%d-K%d-%s" % c for c in LIMIT_CASES]


def lattice_m(C):
    """The largest power of four <= C: 16, 64, 256 or 1024 over the served channel counts."""
    m = 1
    while 4 * m <= C:
        m *= 4
    return m


def lattice_features(C, h, w, generator):
    """bf16 [C, h, w]: every pixel has exactly m = lattice_m(C) channels at +-1, at random positions, and 0 elsewhere.  Then ||x|| = sqrt(m)
    is a power of two and the fp32 sum of squares is exact, so 1 / ||x|| is exact; dot products are integers of magnitude <= m <= 1024, exact
    in the matrix cores' fp32 in whatever order they are added; and every score is EXACTLY dot / m, in the kernel and in the fp64 reference
    alike.  Distinct scores differ by >= 1 / 1024, far above the ambiguity margin 4 * C * 2^-24 <= 2.5e-4: no pixel is ambiguous, and exact
    ties are plentiful."""
    m = lattice_m(C)
    live = torch.rand(h, w, C, generator=generator).argsort(-1)[..., :m]
    sign = (torch.randint(0, 2, (h, w, m), generator=generator) * 2 - 1).float()
    x = torch.zeros(h, w, C).scatter_(-1, live, sign)
    return x.permute(2, 0, 1).contiguous().to(torch.bfloat16)


def make_labels(n, K, h, w, generator):
    """fp32 segs [n, K, h, w], positive; summing to one over K as make_case's -- except for K = 1, where that normalisation would make them
    constant 1 and every output 1 whatever the kernel keeps: K = 1 label maps stay unnormalised, uniform in [0.05, 1.05]."""
    segs = torch.rand(n, K, h, w, generator=generator) + 0.05
    return (segs if K == 1 else segs / segs.sum(1, keepdim=True)).float()


def make_limit_case(case, seed=0):
    """As make_case, for a LIMIT_CASES entry."""
    n, C, h, w, _, _, K, features = case
    g = torch.Generator().manual_seed(seed)
    if features == "gauss":
        target = torch.randn(C, h, w, generator=g).to(torch.bfloat16)
        context = [torch.randn(C, h, w, generator=g).to(torch.bfloat16) for _ in range(n)]
    else:
        assert features == "lattice"
        target = lattice_features(C, h, w, g)
        context = [lattice_features(C, h, w, g) for _ in range(n)]
    return target, context, make_labels(n, K, h, w, g)


@functools.lru_cache(maxsize=None)
def limit_reference(case_index, seed=0):
    """(inputs, windowed result) of LIMIT_CASES[case_index], computed once per process and shared; callers must not modify it."""
    case = LIMIT_CASES[case_index]
    inputs = make_limit_case(case, seed)
    return inputs, windowed(*inputs, radius=case[4], topk=case[5])


def gpu_bound(C, kept_max, segs_max, temperature=TEMPERATURE):
    """The bound of the GPU tests on a non-ambiguous pixel, no constant fitted: 2 * (delta_s / T + 2^-20 + kept_max * 2^-24) * max|segs| with
    delta_s = (C + 8) * 2^-24 (tests/test_gpu_propagate.py derives the first two terms).  The third covers the fp32 additions of the kept terms
    into the numerator and the denominator, kept_max - 1 roundings of relative size 2^-24 each on sums of positive terms: the "handful" the
    2^-20 absorbs in CASES is not a handful where ties keep dozens of candidates.  kept_max is the reference's own largest kept set."""
    return 2.0 * ((C + 8) * 2.0 ** -24 / temperature + 2.0 ** -20 + kept_max * 2.0 ** -24) * segs_max


# ---- planted defects: what a subtly wrong kernel would compute ------------------------------------------------------------
DEFECTS = ("exactly_topk", "cut_at_16", "drop_last_chunk", "stale_row0")


def windowed_with_defect(defect, target, context, segs, radius, topk, temperature=TEMPERATURE):
    """``windowed`` with one planted defect; returns out [1, K, h, w] only.  The CPU tests assert that each moves the output by more than
    the GPU bound on the limit cases, i.e. that those cases would catch a kernel with that defect.
      exactly_topk     keeps exactly topk candidates (the first in scan order among ties at the threshold) instead of all ties
      cut_at_16        the kept set is cut at the kernel's 16 list slots (the first 16 in scan order: frame, row, column)
      drop_last_chunk  the target's last 32-channel chunk is left out of the dot product; the norms are those of the whole vector
                       (a query fragment that never reached the matrix cores)
      stale_row0       the FEATURES of image row 0 of context frame f >= 1 are those of frame f - 1 (a key buffer not reloaded when the frame
                       changes); the inverse norms and the labels are frame f's own"""
    assert defect in DEFECTS
    C, h, w = target.shape
    n, K = segs.shape[:2]
    q = _normalized(target)
    if defect == "drop_last_chunk":
        q[C - 32:] = 0
    ctx = torch.stack([_normalized(f) for f in context])
    if defect == "stale_row0":
        raw = torch.stack([f.double() for f in context])
        inv = 1.0 / raw.pow(2).sum(1, keepdim=True).sqrt().clamp_min(1e-12)
        stale = raw.clone()
        stale[1:, :, 0, :] = raw[:-1, :, 0, :]
        ctx = stale * inv
    sg = segs.double()
    out = torch.zeros(1, K, h, w, dtype=torch.float64)
    for i in range(h):
        i0, i1 = max(0, i - radius), min(h, i + radius + 1)
        for j in range(w):
            j0, j1 = max(0, j - radius), min(w, j + radius + 1)
            s = torch.einsum("c,ncyx->nyx", q[:, i, j], ctx[:, :, i0:i1, j0:j1]).reshape(-1)
            lab = sg[:, :, i0:i1, j0:j1].permute(0, 2, 3, 1).reshape(-1, K)
            keep = torch.ones_like(s, dtype=torch.bool)
            if s.numel() >= topk:
                keep = s >= torch.topk(s, topk).values[-1]
                if defect == "exactly_topk":
                    keep = torch.zeros_like(keep)
                    keep[torch.sort(s, descending=True, stable=True).indices[:topk]] = True
            if defect == "cut_at_16":
                keep = keep & (keep.cumsum(0) <= 16)
            wgt = torch.exp((s[keep] - s.max()) / temperature)
            out[0, :, i, j] = (wgt[:, None] * lab[keep]).sum(0) / wgt.sum()
    return out
