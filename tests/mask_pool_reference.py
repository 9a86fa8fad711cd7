"""fp64 restatement of mask pooling and the exact pixel census of its kernels (tests/test_mask_pool_cpu.py without a device,
tests/test_gpu_mask_pool.py on one).  Plain helper module: no test in it.

    A[b, g, k, j]   = sum_px M[b, k, px] * P_g[px, j]            abs_sum[b, g, k, j] = sum_px |M[b, k, px]| * P_g[px, j]
    mass[b, k]      = sum_px M[b, k, px]
    pooled[b, k, c] = sum_j A[b, g(c), k, j] * V[b, c, j]        pooled_abs[b, k, c] = sum_j abs_sum[b, g(c), k, j] * |V[b, c, j]|

P is the oracle's softmax over the window of ``input_statistics._tables`` (the index tables of ``attention_reference``); P >= 0, so no
cancellation hides in A beyond the mask's own signs, which abs_sum carries.

Bounds.  The kernel rounds the normalised P to bf16 (one rounding per weight, U = 2^-8) and multiplies by the mask on the matrix cores
in fp32; byte masks are exact operands (n = 1), soft masks are rounded to bf16 once more (n = 2).  The per-cell sums and the gather add
at most a few hundred fp32 terms: 2^-22 * abs_sum, the allowance ``head_bound`` makes for its fp32 head sum.  The contraction with V is
fp32 over h*w terms of bf16-exact values: the bound of A propagated through |V| plus h*w * 2^-24 * pooled_abs.

Census.  With q = 0 every score is 0, every softmax weight is the bf16 value p nearest 1 / NSLOT, and with 0 / 1 masks A / p is the number
of masked pixels whose window holds key j: an integer of at most Ho * Wo <= 2^16 (``census_is_exact``), p has 8 significant bits, so every partial sum of the kernel is exact in fp32 in any order and the comparison is ``torch.equal``.  ``census_counts``
restates the count from the cell geometry alone (clamped windows, no tables, no attention) and can plant the defects the kernel could
have: a window shifted by one, x and y swapped, the clamp dropped, a pad pixel counted, a pad slot leaked.
"""
import numpy as np
import torch

import input_statistics as S
from oracle import naf_oracle as O


def window_indicators(q, k, ksz):
    """(Wy [Ho, h], Wx [Wo, w]) bool: key row / column inside the window of query row / column, from the oracle's index tables."""
    iy, ix = S._tables(q, k, ksz)
    out = []
    for tab, n in ((iy, k.shape[-2]), (ix, k.shape[-1])):
        assert (np.diff(np.sort(tab, axis=1), axis=1) > 0).all(), "a window that repeats a key: not a geometry of these tests"
        ind = torch.zeros(tab.shape[0], n, dtype=torch.bool)
        ind[torch.arange(tab.shape[0])[:, None], torch.from_numpy(np.ascontiguousarray(tab))] = True
        out.append(ind)
    return out


def dense_weights(q, k, ksz, heads, r0, r1):
    """P [B, heads, (r1 - r0) * Wo, h * w] fp64 of the query rows [r0, r1): the softmax over the window, zero outside it."""
    Wy, Wx = window_indicators(q, k, ksz)
    qh, kh = S._heads(q[:, :, r0:r1], heads), S._heads(k, heads)          # b n R Wo d / b n h w d
    B, n, R, Wo, D = qh.shape
    s = torch.einsum("bnpd,bnjd->bnpj", qh.reshape(B, n, R * Wo, D), kh.reshape(B, n, -1, D)) * D ** -0.5
    win = (Wy[r0:r1, None, :, None] & Wx[None, :, None, :]).reshape(R * Wo, -1)
    s = s.masked_fill(~win, float("-inf"))
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    return e / e.sum(dim=-1, keepdim=True)


def mask_pool_reference(q, k, masks, ksz, heads, v=None, rows_per_chunk=8):
    """fp64 dict: A, abs_sum [B, heads, K, h, w], mass [B, K] and, with ``v`` [B, C, h, w], pooled (the SUM) and pooled_abs [B, K, C].
    q [B, Cq, Ho, Wo], k [B, Cq, h, w], masks [B, K, Ho, Wo] (any dtype: read as float64)."""
    B, _, Ho, Wo = q.shape
    h, w = k.shape[-2:]
    m = masks.double()
    K = m.shape[1]
    A = torch.zeros(B, heads, K, h * w, dtype=torch.float64)
    absA = torch.zeros_like(A)
    for r0 in range(0, Ho, rows_per_chunk):
        r1 = min(r0 + rows_per_chunk, Ho)
        P = dense_weights(q, k, ksz, heads, r0, r1)
        mc = m[:, :, r0:r1].reshape(B, K, -1)
        A += torch.einsum("bkp,bnpj->bnkj", mc, P)
        absA += torch.einsum("bkp,bnpj->bnkj", mc.abs(), P)
    r = dict(A=A.view(B, heads, K, h, w), abs_sum=absA.view(B, heads, K, h, w), mass=m.sum(dim=(2, 3)))
    if v is not None:
        C = v.shape[1]
        v5 = v.double().view(B, heads, C // heads, h * w)
        r["pooled"] = torch.einsum("bnkj,bndj->bknd", A, v5).reshape(B, K, C)
        r["pooled_abs"] = torch.einsum("bnkj,bndj->bknd", absA, v5.abs()).reshape(B, K, C)
    return r


def a_bound(abs_sum, soft):
    """Per-element bound of A: ``soft`` masks are rounded to bf16 on their way to the matrix cores (n = 2), byte masks are exact (n = 1)."""
    return S.bf16_bound(2 if soft else 1, abs_sum) + 2.0 ** -22 * abs_sum


def pooled_bound(pooled_abs, hw, soft):
    """... propagated through |V| (bf16-exact values), plus the fp32 contraction over the h * w keys."""
    return a_bound(pooled_abs, soft) + hw * S.F32 * pooled_abs


def mean_of(pooled, mass):
    """pooled / mass with exact zeros where the mass is zero (fp64)."""
    live = (mass != 0)[..., None]
    return torch.where(live, pooled / torch.where(live, mass[..., None], torch.ones_like(mass[..., None])), torch.zeros_like(pooled))


# ---- masks ---------------------------------------------------------------------------------------------------------------------
def binary_masks(B, K, Ho, Wo, seed, density=0.3):
    """bool [B, K, Ho, Wo]: hash-noise masks of the given density; mask K - 1 (when K > 1) is empty."""
    m = O.hash_normal((B, K, Ho, Wo), seed) > float(np.sqrt(2.0) * _erfinv(1.0 - 2.0 * density))
    if K > 1:
        m[:, K - 1] = False
    return m


def _erfinv(x):
    # Winitzki's approximation: the density of a test mask needs two digits, not fifteen
    a = 0.147
    ln = np.log(1.0 - x * x)
    t = 2.0 / (np.pi * a) + ln / 2.0
    return float(np.sign(x) * np.sqrt(np.sqrt(t * t - ln / a) - t))


def soft_masks(B, K, Ho, Wo, seed):
    """fp32 [B, K, Ho, Wo] in [0, 1], NOT bf16-representable (the host's cast to bf16 is the documented rounding), zero on about half of
    the pixels; mask K - 1 (when K > 1) is empty."""
    x = O.hash_normal((B, K, Ho, Wo), seed)
    m = torch.clamp(x * 0.37 + 0.11, 0.0, 1.0)
    if K > 1:
        m[:, K - 1] = 0.0
    return m


def census_masks(B, K, h, w, dy, dx):
    """bool [B, K, h * dy, w * dx] of the census: corners, edges, a single cell, a single pixel, the whole image, cell-aligned and not,
    cycled over the K masks and shifted per batch so that no two are alike."""
    Ho, Wo = h * dy, w * dx
    m = torch.zeros(B, K, Ho, Wo, dtype=torch.bool)
    for b in range(B):
        for k in range(K):
            kind, t = (k + b) % 9, (k // 9 + b) % 3
            if kind == 0:
                m[b, k] = True
            elif kind == 1:
                m[b, k, :dy + t, :dx + 2 * t] = True                      # top-left corner, one cell and a bit
            elif kind == 2:
                m[b, k, Ho - dy - t:, Wo - 3 - t:] = True                 # bottom-right corner, not cell-aligned
            elif kind == 3:
                m[b, k, :1 + t, :] = True                                 # top edge
            elif kind == 4:
                m[b, k, :, Wo - 1 - t:] = True                            # right edge
            elif kind == 5:
                cy, cx = (h // 2 + t) % h, (w // 2 + k) % w
                m[b, k, cy * dy:(cy + 1) * dy, cx * dx:(cx + 1) * dx] = True   # one cell
            elif kind == 6:
                m[b, k, (7 * k + 3 * t) % Ho, (11 * k + 5) % Wo] = True    # one pixel
            elif kind == 7:
                m[b, k, Ho - 1, :] = True                                 # bottom edge
                m[b, k, :, 0] = True                                      # and left edge
            else:
                m[b, k, dy // 2::dy, dx - 1::dx] = True                   # the last pixel of a row of every cell
    return m


# ---- census ----------------------------------------------------------------------------------------------------------------------
DEFECTS = ("shift", "swap", "no_clamp", "pad_pixel", "pad_slot")


def census_p(ksz):
    """The bf16 value every softmax weight takes with q = 0: 1 / NSLOT rounded to bf16 (fp32 tensor scalar)."""
    return torch.tensor(1.0 / (ksz * ksz), dtype=torch.float32).to(torch.bfloat16).to(torch.float32)


def census_is_exact(ksz, Ho, Wo):
    """True when (a) the bf16 rounding of 1 / NSLOT does not depend on the last bits of the hardware's reciprocal (it is the same for
    every fp32 within 4 ulp of 1 / NSLOT) and (b) p times any count up to the largest possible one is exact in fp32.  Away from the border a
    key lies in the windows of window^2 cells, but the clamp piles the windows of all border cells onto the same keys (on an 8 x 10 grid with
    a 7 x 7 window, key (3, 3) is in every cell's window), so the only bound is the image: Ho * Wo pixels.  p has 8 significant bits, so a
    count of at most 2^16 gives a product of at most 24 bits; the fp32 partial sums of the kernel are integers times p below that, exact in any order."""
    n = ksz * ksz
    x = np.float32(1.0) / np.float32(n)
    near = [x]
    for _ in range(4):
        near = [np.nextafter(near[0], np.float32(0)), *near, np.nextafter(near[-1], np.float32(1))]
    r = {float(torch.tensor(float(y), dtype=torch.float32).to(torch.bfloat16)) for y in near}
    cmax = Ho * Wo
    p = float(census_p(ksz))
    exact = all(float(np.float32(p) * np.float32(c)) == p * c and float(np.float32(p * c) / np.float32(p)) == c for c in (cmax, cmax - 1, cmax // 2 + 1, 1))
    return len(r) == 1 and cmax <= 2 ** 16 and exact


def census_counts(masks, h, w, ksz, defect=None):
    """int64 [B, K, h, w]: for every key j the number of masked pixels whose cell's clamped window holds j -- from the cell geometry
    alone.  ``defect``: one of DEFECTS planted into the count (what a wrong kernel would produce)."""
    B, K, Ho, Wo = masks.shape
    dy, dx = Ho // h, Wo // w
    r = ksz // 2
    mi = masks.to(torch.int64)
    cnt = torch.zeros(B, K, h, w, dtype=torch.int64)
    for cy in range(h):
        for cx in range(w):
            cell = mi[:, :, cy * dy:(cy + 1) * dy, cx * dx:(cx + 1) * dx]
            n = cell.sum(dim=(2, 3))
            if defect == "pad_pixel":       # the idle lanes of a partial row tile repeat the row's last pixel: counted once each
                n = n + ((-dx) % 16) * cell[:, :, :, -1].sum(dim=2)
            y0, x0 = min(max(cy - r, 0), h - ksz), min(max(cx - r, 0), w - ksz)
            if defect == "shift":
                x0 = min(max(cx - r + 1, 0), w - ksz)
            elif defect == "swap":          # the cell's coordinates swapped when the window is placed
                y0, x0 = min(max(cx - r, 0), h - ksz), min(max(cy - r, 0), w - ksz)
            elif defect == "no_clamp":
                y0, x0 = cy - r, cx - r
            ya, yb, xa, xb = max(y0, 0), min(y0 + ksz, h), max(x0, 0), min(x0 + ksz, w)
            cnt[:, :, ya:yb, xa:xb] += n[:, :, None, None]
            if defect == "pad_slot" and y0 + ksz < h:      # slot NSLOT = (row ksz, column 0) of the window reaches a real key
                cnt[:, :, y0 + ksz, x0] += n
    return cnt
