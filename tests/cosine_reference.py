"""The yardstick of the cosine-head tests (``naf(..., head=E, cosine=True)``, ``ops.xna_cos_forward``, naf_xna_cos_fwd): the definition
restated in fp64 on the kernel's bf16 inputs, and the per-element bounds the results are held to.  Nothing in the bounds is measured.

1. ``reference``.  With E^ = F.normalize(E.float(), dim=1) (then fp64), P_g the softmax weights of head g over the pixel's k x k window of
   low-res cells (integer ratio: every pixel of a cell shares the cell's clamped window, oracle/naf_oracle.py ``lowres_window_table``),
       f[c]   = sum_s P_g(c)[s] v[c, s]                         the upsampled feature, C = heads * Dv channels
       cos[n] = logit_scale * (E^[n] . f) / max(||f||_2, 1e-12),   norms = ||f||_2
   tests/test_cosine_head_cpu.py holds it against F.cosine_similarity on the oracle's attention.

2. The kernel's rounding points (naf_amd/csrc/xna_cos_kernel.h), and what each costs:
   a. IMPLIED FEATURE.  The denominator is formed from P rounded once to bf16 after normalisation (pf = (bf16_t)(s * inv)), fp32
      accumulation, nothing stored: per channel |f~[c] - f[c]| <= delta[c] = 1.25 * 2^-8 * sum_s P[s] |v[c, s]|, the existing bound of the
      matrix-core forward (tests/input_statistics.bf16_bound, n = 1) WITHOUT a store term.  So | ||f~|| - ||f|| | <= ||delta||_2.
   b. NUMERATOR.  num = sum_g sum_s P_g[s] PV_g[n, s] with PV_g = E^[n, g] . v_g formed in fp32 on the low-res grid and rounded once to
      bf16, and the same P rounded once to bf16:
          delta_num = 2 * 2^-9 * A_pv + 2^-24 * ((Dv + 2) * A_ev + (K * heads + 2) * A_pv)
      A_pv = sum_g sum_s P |PV|, A_ev = sum_g sum_s P sum_d |E^[n, d]| |v[d, s]|; the second part is the fp32 chain: the Dv-term dot product
      behind PV (its error moves the value that is rounded) and the K * heads-term accumulation of the matrix cores and the head sum.
   c. COSINE.  cos~ = ls * (num + e) / ||f~|| with |e| <= delta_num and ||f~|| within ||delta||_2 of ||f||:
          |cos~ - cos| <= |ls| * (delta_num / ||f|| + |cos / ls| * ||delta||_2 / ||f||) + (C / 2 + 6) * 2^-24 * |cos|
      the last term: the C-term fp32 chain of the sum of squares (halved by the root), the reduction across four lanes, sqrt, max, the
      divide and two multiplications.  Where ||f|| = 0 the bound is 0: the result must be exactly 0.
   d. NORMS.  |norms~ - ||f||| <= ||delta||_2 + (C / 2 + 2) * 2^-24 * ||f||.

3. ``composed_bound``: the same for the composition (the plain forward stored in bf16, normalised and multiplied in fp32 torch ops):
   per channel delta_c[c] = bf16_bound(1, A_f[c], stored=|f[c]|) (P rounded, one bf16 store); numerator error <= sum_c |E^[n, c]| delta_c[c]
   + C * 2^-24 * sum_c |E^[n, c]| |f[c]|; the denominator as in c with delta_c; the fp32 feature path (fp32 features: no store) drops
   the store term.  fused against composed is held to the sum of the two bounds.

``emulate`` is the kernel's arithmetic on the host (fp64 between the documented rounding points) with one planted defect per keyword;
tests/test_cosine_head_cpu.py states the input on which each defect leaves the bound.

This module is a helper (no tests in it); the cases the GPU tests run are defined here so that the CPU tests can use them too.
"""
import os
import sys

import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402

DQ = 64          # head dim of the cell kernels
F32 = S.F32
EPS = 1e-12

# name -> (B, heads, Dv, (h, w), (dy, dx) pixels per cell, window, N)
CASES = {
    "a_c128_k7_n21": (1, 4, 32, (8, 8), (16, 16), 7, 21),          # 16-pixel cells: the whole cell in one round
    "b_whole_grid_n1": (2, 2, 32, (7, 7), (2, 16), 7, 1),           # window = whole grid, two images, one embedding
    "c_dv192_n151": (1, 4, 192, (9, 10), (16, 16), 5, 151),         # C 768: three value chunks per head; ten channel tiles
    "d_dv256_n256": (1, 4, 256, (8, 8), (16, 16), 7, 256),          # C 1024: four chunks; sixteen channel tiles (one tile per wave)
    "e_patch14_n21": (1, 4, 48, (6, 7), (14, 14), 5, 21),           # partial row tiles; Dv 48: a chunk of three channel tiles
    "f_rows30_n151": (1, 4, 32, (5, 5), (3, 30), 3, 151),           # 30-pixel rows: a full and a 14-pixel tile
    "g_k9_n256": (1, 4, 32, (11, 12), (2, 16), 9, 256),             # window 9, sixteen channel tiles
    "h_three_heads_n1": (1, 3, 64, (8, 8), (2, 16), 7, 1),          # three heads, one whole chunk
    "i_k11_n40": (1, 2, 64, (12, 13), (2, 16), 11, 40),             # window 11, four channel tiles
    "j_k13_n21": (1, 1, 64, (14, 13), (1, 16), 13, 21),             # window 13, one head, one-row cells (seven dead waves)
    "k_k15_n40": (1, 2, 32, (16, 15), (1, 16), 15, 40),             # window 15 (one tile per wave), four channel tiles
    "l_two_rounds_n21": (1, 4, 32, (7, 8), (32, 16), 7, 21),        # 32 tiles per cell: two rounds per workgroup
}
# what the kernel's dispatch distinguishes (naf_amd/csrc/xna_cos_kernel.h): channel tiles per N, value chunks of 64 channels
NCT_OF = lambda n: 2 if n <= 32 else 4 if n <= 64 else 10 if n <= 160 else 16
WINDOWS = (3, 5, 7, 9, 11, 13, 15)


def make_inputs(name, seed=5100, zero_block=None, const_v=False, geom=None, chan_offset=0.0):
    """q [B, heads*64, Ho, Wo], k [B, heads*64, h, w], v [B, C, h, w] fp32 tensors holding bf16 values, E [N, C] fp32.
    ``zero_block`` = (y0, y1, x0, x1): the features of those low-res cells are zero.  ``const_v``: every cell holds the same vector.
    ``geom``: a geometry in the form of a CASES entry, used in place of CASES[name] (tests/layout_contract.py: COS_GEOMS).
    ``chan_offset``: every value channel gets an offset of its own, hash_normal((1, C, 1, 1), seed) times this, before the bf16 rounding,
    so that a head, a channel or an image read from the wrong place shows."""
    B, heads, Dv, (h, w), (dy, dx), ks, N = CASES[name] if geom is None else geom
    C = heads * Dv
    q = S.bf16r(O.hash_normal((B, heads * DQ, h * dy, w * dx), seed + 1))
    k = S.bf16r(O.hash_normal((B, heads * DQ, h, w), seed + 2))
    off = O.hash_normal((1, C, 1, 1), seed) * chan_offset if chan_offset else 0.0
    v = S.bf16r(O.hash_normal((B, C, h, w), seed + 3) + off + (0.5 if const_v else 0.0))
    if const_v:
        v = v[:, :, :1, :1].expand(B, C, h, w).contiguous()
    if zero_block is not None:
        y0, y1, x0, x1 = zero_block
        v[:, :, y0:y1, x0:x1] = 0.0
    E = O.hash_normal((N, C), seed + 4) * 3.0
    return q, k, v, E


def sees_only(zero_block, h, w, ks):
    """[h, w] bool: the cells whose clamped ks x ks window lies inside ``zero_block`` = (y0, y1, x0, x1)."""
    y0, y1, x0, x1 = zero_block
    m = torch.zeros(h, w, dtype=torch.bool)
    for cy in range(h):
        for cx in range(w):
            wy, wx = min(max(cy - ks // 2, 0), h - ks), min(max(cx - ks // 2, 0), w - ks)
            m[cy, cx] = wy >= y0 and wy + ks <= y1 and wx >= x0 and wx + ks <= x1
    return m


def _cells(q, k, v, ks, heads, fn, scale=None):
    """Runs ``fn(cy, cx, P [B, heads, dy*dx, K] fp64, window slices)`` for every low-res cell of an integer-ratio geometry."""
    B, Cq, Ho, Wo = q.shape
    h, w = v.shape[-2:]
    dy, dx = Ho // h, Wo // w
    assert Ho == dy * h and Wo == dx * w and h >= ks and w >= ks
    Dq = Cq // heads
    sc = Dq ** -0.5 if scale is None else scale
    qh = q.double().view(B, heads, Dq, h, dy, w, dx)
    kh = k.double().view(B, heads, Dq, h, w)
    for cy in range(h):
        for cx in range(w):
            wy, wx = min(max(cy - ks // 2, 0), h - ks), min(max(cx - ks // 2, 0), w - ks)
            kw = kh[:, :, :, wy:wy + ks, wx:wx + ks].reshape(B, heads, Dq, ks * ks)
            qc = qh[:, :, :, cy, :, cx, :].reshape(B, heads, Dq, dy * dx)
            P = torch.softmax(torch.einsum("bgdp,bgdk->bgpk", qc, kw) * sc, dim=-1)
            fn(cy, cx, P, (slice(wy, wy + ks), slice(wx, wx + ks)))


def _e_hat(E):
    return F.normalize(E.float(), dim=1).double()


def reference(q, k, v, E, ks, heads, logit_scale=1.0):
    """fp64 dict: cos [B, N, Ho, Wo], norms [B, Ho, Wo], f and a_f = sum_s P |v| [B, C, Ho, Wo], a_pv and a_ev [B, N, Ho, Wo]
    (module docstring, 2b), plus the sizes the bounds need."""
    B, C, h, w = v.shape
    Ho, Wo = q.shape[-2:]
    dy, dx = Ho // h, Wo // w
    Dv = C // heads
    eh = _e_hat(E)
    N = eh.shape[0]
    vh = v.double().view(B, heads, Dv, h, w)
    eg = eh.view(N, heads, Dv)
    pv = torch.einsum("ngd,bgdhw->bgnhw", eg, vh)
    aev = torch.einsum("ngd,bgdhw->bgnhw", eg.abs(), vh.abs())
    f = torch.zeros(B, heads, Dv, h, dy, w, dx, dtype=torch.float64)
    a_f = torch.zeros_like(f)
    num = torch.zeros(B, N, h, dy, w, dx, dtype=torch.float64)
    a_pv, a_ev = torch.zeros_like(num), torch.zeros_like(num)

    def cell(cy, cx, P, win):
        K = P.shape[-1]
        vw = vh[:, :, :, win[0], win[1]].reshape(B, heads, Dv, K)
        f[:, :, :, cy, :, cx, :] = torch.einsum("bgpk,bgdk->bgdp", P, vw).view(B, heads, Dv, dy, dx)
        a_f[:, :, :, cy, :, cx, :] = torch.einsum("bgpk,bgdk->bgdp", P, vw.abs()).view(B, heads, Dv, dy, dx)
        pw = pv[:, :, :, win[0], win[1]].reshape(B, heads, N, K)
        aw = aev[:, :, :, win[0], win[1]].reshape(B, heads, N, K)
        num[:, :, cy, :, cx, :] = torch.einsum("bgpk,bgnk->bnp", P, pw).view(B, N, dy, dx)
        a_pv[:, :, cy, :, cx, :] = torch.einsum("bgpk,bgnk->bnp", P, pw.abs()).view(B, N, dy, dx)
        a_ev[:, :, cy, :, cx, :] = torch.einsum("bgpk,bgnk->bnp", P, aw).view(B, N, dy, dx)

    _cells(q, k, v, ks, heads, cell)
    f, a_f = f.view(B, C, Ho, Wo), a_f.view(B, C, Ho, Wo)
    num, a_pv, a_ev = num.view(B, N, Ho, Wo), a_pv.view(B, N, Ho, Wo), a_ev.view(B, N, Ho, Wo)
    norms = f.norm(dim=1)
    cos = logit_scale * num / norms.clamp_min(EPS).unsqueeze(1)
    return {"cos": cos, "norms": norms, "f": f, "a_f": a_f, "a_pv": a_pv, "a_ev": a_ev, "e_hat": eh,
            "ls": float(logit_scale), "heads": heads, "Dv": Dv, "C": C, "K": ks * ks}


def cosine_from_features64(f, E, logit_scale=1.0):
    """The definition on a given feature map, fp64: (cos [B, N, H, W], norms [B, H, W])."""
    f = f.double()
    nrm = f.norm(dim=1)
    return logit_scale * torch.einsum("nc,bchw->bnhw", _e_hat(E), f / nrm.clamp_min(EPS).unsqueeze(1)), nrm


def feature_delta(r):
    """2a: ||delta||_2 per pixel [B, Ho, Wo] of the kernel's implied feature."""
    return S.bf16_bound(1, r["a_f"]).pow(2).sum(dim=1).sqrt()


def _over_norm(x, nrm):
    """x / ||f|| where ||f|| > 0, 0 where ||f|| = 0 (the result must be exact there)."""
    n = nrm if x.dim() == nrm.dim() else nrm.unsqueeze(1)
    return torch.where(n > 0, x / n.clamp_min(1e-300), torch.zeros_like(x))


def bound(r):
    """2c: per-element bound [B, N, Ho, Wo] on |cos~ - cos| of the fused kernel."""
    ls, cosu = abs(r["ls"]), (r["cos"] / r["ls"]).abs() if r["ls"] != 0 else r["cos"].abs()
    dnum = 2.0 * 2.0 ** -9 * r["a_pv"] + F32 * ((r["Dv"] + 2) * r["a_ev"] + (r["K"] * r["heads"] + 2) * r["a_pv"])
    d2 = feature_delta(r)
    return ls * (_over_norm(dnum, r["norms"]) + cosu * _over_norm(d2, r["norms"]).unsqueeze(1)) + (r["C"] / 2 + 6) * F32 * r["cos"].abs()


def norms_bound(r):
    """2d."""
    return feature_delta(r) + (r["C"] / 2 + 2) * F32 * r["norms"]


def composed_bound(r, stored_bf16=True):
    """3: per-element bound on the composition's cosines ((bound [B, N, Ho, Wo], norms bound [B, Ho, Wo]))."""
    ls, cosu = abs(r["ls"]), (r["cos"] / r["ls"]).abs() if r["ls"] != 0 else r["cos"].abs()
    dc = S.bf16_bound(1, r["a_f"], r["f"].abs() if stored_bf16 else None)
    ea = r["e_hat"].abs()
    dnum = torch.einsum("nc,bchw->bnhw", ea, dc) + r["C"] * F32 * torch.einsum("nc,bchw->bnhw", ea, r["f"].abs())
    d2 = dc.pow(2).sum(dim=1).sqrt()
    b = ls * (_over_norm(dnum, r["norms"]) + cosu * _over_norm(d2, r["norms"]).unsqueeze(1)) + (r["C"] / 2 + 6) * F32 * r["cos"].abs()
    return b, d2 + (r["C"] / 2 + 2) * F32 * r["norms"]


def check(got, ref, bnd, what):
    """Every element, none left out, NaN counts as a miss; the message names the worst one."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(torch.nan_to_num(ratio, nan=float("inf")).max())
    print(f"{what}: max err {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e}, worst err / bound {worst:.3f}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the bound (worst err / bound {worst:.3f})"
    return worst


def outside(got, ref, bnd):
    """Number of elements outside the bound (NaN included)."""
    return int((~((got.double() - ref).abs() <= bnd)).sum())


def _r16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def emulate(q, k, v, E, ks, heads, logit_scale=1.0, *, norm_per_head=False, drop_head=None, raw_embeddings=False, clamp_squared=False,
            zero_nan=False):
    """The kernel's arithmetic on the host: P rounded to bf16 after normalisation, PV = bf16(E^ . v), everything else fp64, then the
    epilogue ``ls * (num * (1 / max(sqrt(ssq), 1e-12)))``.  -> (cos [B, N, Ho, Wo], norms [B, Ho, Wo]).  One planted defect per keyword:
    the norm taken per head (each head's numerator divided by that head's norm); head ``drop_head``'s channels missing from the norm;
    E not normalised; the clamp applied to the squared norm (1 / sqrt(max(ssq, 1e-12))); 0 / 0 at a zero feature."""
    B, C, h, w = v.shape
    Ho, Wo = q.shape[-2:]
    dy, dx = Ho // h, Wo // w
    Dv = C // heads
    eh = E.double() if raw_embeddings else _e_hat(E)
    N = eh.shape[0]
    vh = v.double().view(B, heads, Dv, h, w)
    pv = _r16(torch.einsum("ngd,bgdhw->bgnhw", eh.view(N, heads, Dv).float(), vh.float()))
    numg = torch.zeros(B, heads, N, h, dy, w, dx, dtype=torch.float64)
    ssqg = torch.zeros(B, heads, h, dy, w, dx, dtype=torch.float64)

    def cell(cy, cx, P, win):
        K = P.shape[-1]
        Pr = _r16(P)
        vw = vh[:, :, :, win[0], win[1]].reshape(B, heads, Dv, K)
        fg = torch.einsum("bgpk,bgdk->bgdp", Pr, vw)
        ssqg[:, :, cy, :, cx, :] = fg.pow(2).sum(dim=2).view(B, heads, dy, dx)
        pw = pv[:, :, :, win[0], win[1]].reshape(B, heads, N, K)
        numg[:, :, :, cy, :, cx, :] = torch.einsum("bgpk,bgnk->bgnp", Pr, pw).view(B, heads, N, dy, dx)

    _cells(q, k, v, ks, heads, cell)
    numg, ssqg = numg.view(B, heads, N, Ho, Wo), ssqg.view(B, heads, Ho, Wo)
    keep = [g for g in range(heads) if g != drop_head]
    ssq = ssqg[:, keep].sum(dim=1)
    nrm = ssq.sqrt()
    inv = 1.0 / (ssq.clamp_min(EPS).sqrt() if clamp_squared else nrm.clamp_min(EPS))
    if zero_nan:
        inv = 1.0 / nrm
    if norm_per_head:
        cos = logit_scale * (numg / ssqg.sqrt().clamp_min(EPS).unsqueeze(2)).sum(dim=1)
    else:
        cos = logit_scale * (numg.sum(dim=1) * inv.unsqueeze(1))
    return cos, nrm
