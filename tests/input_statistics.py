"""Input families, abs-sum references and rounding emulations for the scale-aware parity tests
(tests/test_gpu_input_statistics.py on the device, tests/test_input_statistics_cpu.py without one).  Plain helper module: no test in it.

Why abs-sums.  The attention kernels round the softmax weights P (forward, dV) and the score gradients dS (dQ, dK) to bf16 before the
matrix-core contractions; everything else is fp32.  One rounding to bf16 moves a number by at most U = 2^-8 of itself (8 significand
bits, round to nearest), so a contraction sum_j w_j x_j with n roundings per weight is off by at most n * U * sum_j |w_j| |x_j| -- per
element, and equivariant under any scaling of the inputs.  ``sum_j |w_j||x_j|`` is the "abs-sum" computed here in fp64 from the oracle.
A result stored as bf16 adds U * |result|.  The tests assert SLACK = 1.25 times that; the quarter covers the fp32 accumulation order
and the hardware exp2 / rcp (a few 2^-24 per term against 2^-8).

Ranges (everything far from overflow / underflow of bf16 and fp32, both of which reach 2^-126 .. 2^127):
  * hash_normal is bounded: |x| <= 2 sqrt(3) = 3.47 (sum of four uniforms), granularity 2.6e-5.
  * values / gradients: unit 3.5; channel offsets x8: 32; outliers x60: 208; x2^10: 3.6e3; x2^-10: 2.6e-8 .. 3.4e-3; dout x1e-4: 2.6e-9 ..
    3.5e-4.  The largest product any backward forms is |dout||v||k| * window < 3.6e3 * 3.5 * 64 * 3.5 * 225 < 2^30.
  * scores: scale * q.k with |q|, |k| <= 4 * 3.47 (peaked) or 3.47 + 6 * 3.47 (key offset): |s| < 1600 in the worst case and about 80
    in these tensors; the kernels subtract the row maximum, so exp2 underflows to zero (never overflows), which the bound covers: a
    weight below 2^-126 contributes less than 2^-126 * |v| to the abs-sum and to the error alike.
  * images: |x| <= 255 (raw), 1000 * 3.47 for the single hot pixel.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

U = 2.0 ** -8          # unit roundoff of bf16
SLACK = 1.25           # asserted multiple of every derived bf16 bound
F32 = 2.0 ** -24       # unit roundoff of fp32


def bf16r(x):
    return x.to(torch.bfloat16).to(torch.float32)


# ---- input families ----------------------------------------------------------------------------------------------------------
VALUE_FAMILIES = ("unit", "chan_offset", "outlier", "small", "big", "smooth")
GRAD_FAMILIES = VALUE_FAMILIES + ("tiny",)
LOGIT_FAMILIES = ("unit", "peaked", "flat", "key_offset")
OUTLIER_PERIOD = 23    # one position in 23 (4.3 %) is an outlier token


def outlier_mask(h, w):
    """[h, w] bool: the positions whose tokens are scaled x60 in the ``outlier`` family -- (7 i + 3) mod 23 == 0 over the row-major index."""
    idx = torch.arange(h * w, dtype=torch.int64)
    return (((idx * 7 + 3) % OUTLIER_PERIOD) == 0).view(h, w)


def _smooth(shape, seed):
    """Spatially smooth unit-scale field: hash_normal on a grid four times coarser, bilinearly interpolated in fp64 (align_corners)."""
    B, C, h, w = shape
    coarse = O.hash_normal((B, C, (h + 3) // 4 + 1, (w + 3) // 4 + 1), seed).double()
    return F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True).float()


def make_values(shape, family, seed):
    """bf16-representable fp32 [B, C, h, w] of the value / gradient family ``family`` (GRAD_FAMILIES)."""
    B, C, h, w = shape
    x = O.hash_normal(shape, seed)
    if family == "unit":
        pass
    elif family == "chan_offset":
        x = x + 8.0 * O.hash_normal((1, C, 1, 1), seed + 7001)
    elif family == "outlier":
        x = torch.where(outlier_mask(h, w).view(1, 1, h, w), x * 60.0, x)
    elif family == "small":
        x = x * 2.0 ** -10
    elif family == "big":
        x = x * 2.0 ** 10
    elif family == "smooth":
        x = _smooth(shape, seed)
    elif family == "tiny":
        x = x * 1e-4
    else:
        raise ValueError(family)
    return bf16r(x)


def make_qk(q_shape, k_shape, family, seed, heads):
    """bf16-representable (q [B, Cq, Ho, Wo], k [B, Cq, h, w]) of the logit family ``family``.  Heads wider than 64 are scaled by
    (64 / Dq)^(1/4) each so that the unit family has unit-variance scores at every head width (as tests/test_gpu_parity.py does)."""
    Cq = q_shape[1]
    s = (64.0 / (Cq // heads)) ** 0.25
    q = O.hash_normal(q_shape, seed) * s
    k = O.hash_normal(k_shape, seed + 1) * s
    if family == "unit":
        pass
    elif family == "peaked":
        q, k = q * 4.0, k * 4.0
    elif family == "flat":
        q, k = q * 0.05, k * 0.05
    elif family == "key_offset":
        k = k + 6.0 * s * O.hash_normal((1, Cq, 1, 1), seed + 7002)
    else:
        raise ValueError(family)
    return bf16r(q), bf16r(k)


# the nine forward families: (value family, logit family)
FORWARD_FAMILIES = [("unit", "unit"), ("chan_offset", "unit"), ("outlier", "unit"), ("small", "unit"), ("big", "unit"), ("smooth", "unit"),
                    ("unit", "peaked"), ("unit", "key_offset"), ("unit", "flat")]
# a short list for the cases that exist for their geometry (other windows, other kernels of the same rounding structure)
FORWARD_FAMILIES_SHORT = [("outlier", "peaked"), ("chan_offset", "key_offset"), ("big", "flat")]
# backward: (value family, gradient family, logit family)
BACKWARD_FAMILIES = [("unit", "unit", "unit"), ("unit", "unit", "peaked"), ("unit", "unit", "key_offset"), ("chan_offset", "unit", "unit"),
                     ("outlier", "outlier", "unit"), ("unit", "tiny", "flat"), ("big", "small", "unit")]
BACKWARD_FAMILIES_SHORT = [("chan_offset", "outlier", "peaked"), ("unit", "tiny", "key_offset")]


IMAGE_FAMILIES = ("unit", "natural_norm", "natural_01", "natural_255", "const", "zero", "const_ripple", "half_black", "hot_pixel")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def natural_image(B, H, W, seed):
    """An image that looks like one, in [0, 1]: three octaves of smooth noise shared by the colour channels (luminance), a weaker
    per-channel octave (chroma), a rectangle with hard edges and a little pixel noise, through a logistic curve."""
    def octave(c, div, s):
        coarse = O.hash_normal((B, c, max(2, H // div + 1), max(2, W // div + 1)), s).double()
        return F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    lum = octave(1, 32, seed) + 0.5 * octave(1, 8, seed + 1) + 0.25 * octave(1, 2, seed + 2)
    x = lum + 0.4 * octave(3, 16, seed + 3) + 0.05 * O.hash_normal((B, 3, H, W), seed + 4).double()
    x[:, :, H // 4: H // 2, W // 3: 2 * W // 3] += 1.5
    return torch.sigmoid(1.5 * x).float()


def make_image(B, H, W, family, seed):
    """fp32 [B, 3, H, W] of the image family ``family`` (IMAGE_FAMILIES)."""
    if family == "unit":
        return O.hash_normal((B, 3, H, W), seed)
    if family in ("natural_norm", "natural_01", "natural_255", "half_black"):
        x = natural_image(B, H, W, seed)
        if family == "natural_norm":
            return (x - torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
        if family == "natural_255":
            return torch.round(x * 255.0)
        if family == "half_black":
            x[:, :, :, : W // 2] = 0.0
        return x
    if family == "const":
        return torch.full((B, 3, H, W), 0.5)
    if family == "zero":
        return torch.zeros((B, 3, H, W))
    if family == "const_ripple":
        return 0.5 + 0.004 * O.hash_normal((B, 3, H, W), seed) / 3.47
    if family == "hot_pixel":
        x = O.hash_normal((B, 3, H, W), seed)
        x[:, :, H // 3, W // 2] *= 1000.0
        return x
    raise ValueError(family)


# ---- attention: fp64 reference, abs-sums and rounding emulation ------------------------------------------------------------------
def _tables(q, k, ksz):
    ky, kx = (ksz, ksz) if isinstance(ksz, int) else ksz
    return O.axis_index_table(q.shape[-2], k.shape[-2], ky), O.axis_index_table(q.shape[-1], k.shape[-1], kx)


def attention_reference(q, k, v, ksz, heads):
    """(out, abs_sum) in fp64, [B, C, Ho, Wo] each: the oracle's attention and ``sum_j P_j |v_j|`` -- ONE call of O.xna_tables on the
    values and their absolute values side by side (the weights do not depend on them)."""
    B, C, h, w = v.shape
    Dv = C // heads
    v5 = v.double().view(B, heads, Dv, h, w)
    both = torch.cat([v5, v5.abs()], dim=2).reshape(B, 2 * C, h, w)
    iy, ix = _tables(q, k, ksz)
    o = O.xna_tables(q.double(), k.double(), both, iy, ix, heads).view(B, heads, 2 * Dv, *q.shape[-2:])
    return o[:, :, :Dv].reshape(B, C, *q.shape[-2:]), o[:, :, Dv:].reshape(B, C, *q.shape[-2:])


def _heads(t, heads):
    B, C, H, W = t.shape
    return t.double().view(B, heads, C // heads, H, W).permute(0, 1, 3, 4, 2)          # b n H W d


def _gather(th, yy, ix):
    """th [B, n, h, w, D] -> [B, n, R, Wo, ky*kx, D] for the query rows whose key rows are yy [R, ky]."""
    g = th[:, :, yy][:, :, :, :, ix]                                                     # b n R ky Wo kx d
    B, n, R, ky, Wo, kx, D = g.shape
    return g.permute(0, 1, 2, 4, 3, 5, 6).reshape(B, n, R, Wo, ky * kx, D)


def _r16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def attention_emulated(q, k, v, ksz, heads, round_p="normalised", scale_mul=1.0, drop_dims=0, out_bf16=False, rows_per_chunk=8):
    """The fp64 oracle with the kernels' documented rounding point: P is rounded to bf16 before the PV product
    (``round_p="normalised"``: xna_mfma_kernel.h / xna_slide_kernel.h / xna_union_kernel.h / xna_head_kernel.h round P / sum;
    ``"unnormalised"``: xna_rows.hip rounds exp(s - max) and divides the fp32 accumulator by the unrounded sum; None: no rounding).
    ``scale_mul`` and ``drop_dims`` are the two planted defects of the sensitivity check: the softmax scale times ``scale_mul`` and the
    last ``drop_dims`` query dims of every head left out of the scores."""
    iy, ix = _tables(q, k, ksz)
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    if drop_dims:
        qh = qh.clone()
        qh[..., -drop_dims:] = 0.0
    scale = qh.shape[-1] ** -0.5 * scale_mul
    B, n, Ho, Wo, _ = qh.shape
    out = torch.empty(B, n, Ho, Wo, vh.shape[-1], dtype=torch.float64)
    iyt, ixt = torch.from_numpy(np.ascontiguousarray(iy)), torch.from_numpy(np.ascontiguousarray(ix))
    for r0 in range(0, Ho, rows_per_chunk):
        yy = iyt[r0:r0 + rows_per_chunk]
        kg, vg = _gather(kh, yy, ixt), _gather(vh, yy, ixt)
        s = torch.einsum("bnrwd,bnrwkd->bnrwk", qh[:, :, r0:r0 + rows_per_chunk], kg) * scale
        e = torch.exp(s - s.amax(dim=-1, keepdim=True))
        den = e.sum(dim=-1, keepdim=True)
        if round_p == "normalised":
            o = torch.einsum("bnrwk,bnrwkd->bnrwd", _r16(e / den), vg)
        elif round_p == "unnormalised":
            o = torch.einsum("bnrwk,bnrwkd->bnrwd", _r16(e), vg) / den
        else:
            o = torch.einsum("bnrwk,bnrwkd->bnrwd", e / den, vg)
        out[:, :, r0:r0 + rows_per_chunk] = o
    out = out.permute(0, 1, 4, 2, 3).reshape(B, -1, Ho, Wo)
    return _r16(out) if out_bf16 else out


def backward_reference(q, k, v, dout, ksz, heads, chunks=None, emulate=False, scale_mul=1.0, drop_dims=0, rows_per_chunk=8):
    """The attention backward written out in fp64 (P = softmax(scale q.k), dP = dout.v, dS = scale P (dP - sum_j P dP)):
        dq_i = sum_j dS_ij k_j,   dk_j = sum_i dS_ij q_i,   dv_j = sum_i P_ij dout_i
    with the abs-sums the bounds are built from.  ``chunks``: the widths of the value-channel chunks a chunked launch plan runs (None:
    one chunk).  Every chunk is a complete backward of its channel slice -- its own dP, its own delta, its own dS_c -- and dS = sum_c
    dS_c, so a chunked kernel rounds each dS_c separately (xna_bwd2_kernel.h:451): the abs-sums are sum_c |dS_c|.
    Returns a dict of fp64 tensors in NCHW:
      dq, dk, dv              the gradients (``emulate``: with P and every dS_c rounded to bf16 before the contractions and dq
                              rounded to bf16 once per chunk on the running sum, naf_hip.h "NUMERICS OF A CHUNKED CALL")
      a_dq, a_dk, a_dv        sum_c sum_j |dS_c,ij||k_j|,  sum_c sum_i |dS_c,ij||q_i|,  sum_i P_ij |dout_i|
      dq_store                sum over the chunks of |running sum of dq after the chunk|: the bf16 stores of dq
      u_dq, u_dk              the abs-sums with dS replaced by scale P (|dout|.|v| + sum_j P |dout|.|v|): what bounds fp32 arithmetic, in
                              which dP - delta is a difference of two rounded numbers
      m_dq, m_dk              the abs-sums with |dS_ij| replaced by |dS_ij| + P_ij sum_l |dS_il|: what a RELATIVE error of the weights P moves dS by
                              (delta is a convex combination, dS_ij = scale P_ij sum_l P_il (dP_ij - dP_il), so such an error does not uncancel)
      L                       (a float) the largest scale * sum_d |q_d||k_d| over the (query, key) pairs of the windows
      nacc                    (an int) the largest number of (query, slot) pairs that add into one key
    ``scale_mul`` / ``drop_dims``: the planted defects of the sensitivity check."""
    iy, ix = _tables(q, k, ksz)
    qh, kh, vh, gh = _heads(q, heads), _heads(k, heads), _heads(v, heads), _heads(dout, heads)
    qs = qh
    if drop_dims:
        qs = qh.clone()
        qs[..., -drop_dims:] = 0.0
    B, n, Ho, Wo, Dq = qh.shape
    h, w, Dv = kh.shape[2], kh.shape[3], vh.shape[-1]
    chunks = [Dv] if not chunks else list(chunks)
    assert sum(chunks) == Dv
    scale = Dq ** -0.5 * scale_mul
    iyt, ixt = torch.from_numpy(np.ascontiguousarray(iy)), torch.from_numpy(np.ascontiguousarray(ix))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    dq, a_dq, u_dq, dq_store = z(B, n, Ho, Wo, Dq), z(B, n, Ho, Wo, Dq), z(B, n, Ho, Wo, Dq), z(B, n, Ho, Wo, Dq)
    dk, a_dk, u_dk = z(B, n, h * w, Dq), z(B, n, h * w, Dq), z(B, n, h * w, Dq)
    m_dq, m_dk, hits = z(B, n, Ho, Wo, Dq), z(B, n, h * w, Dq), torch.zeros(h * w, dtype=torch.int64)
    dv, a_dv = z(B, n, h * w, Dv), z(B, n, h * w, Dv)
    rnd = _r16 if emulate else (lambda t: t)
    L = 0.0

    def scatter(dst, wts, rows):          # dst[b, n, key, :] += sum over (r, w, slot -> key) of wts[b, n, r, w, slot] * rows[b, n, r, w, :]
        contrib = wts.unsqueeze(-1) * rows.unsqueeze(-2)                                 # b n R Wo kk D
        dst.index_add_(2, lin.reshape(-1), contrib.reshape(B, n, -1, rows.shape[-1]))

    for r0 in range(0, Ho, rows_per_chunk):
        sl = slice(r0, r0 + rows_per_chunk)
        yy = iyt[sl]
        lin = (yy[:, None, :, None] * w + ixt[None, :, None, :]).reshape(yy.shape[0], Wo, -1)     # [R, Wo, kk] key index of every slot
        hits += torch.bincount(lin.reshape(-1), minlength=h * w)
        kg, vg = _gather(kh, yy, ixt), _gather(vh, yy, ixt)
        P = torch.softmax(torch.einsum("bnrwd,bnrwkd->bnrwk", qs[:, :, sl], kg) * scale, dim=-1)
        L = max(L, float(torch.einsum("bnrwd,bnrwkd->bnrwk", qh[:, :, sl].abs(), kg.abs()).max()) * Dq ** -0.5)
        g = gh[:, :, sl]
        scatter(dv, rnd(P), g)
        scatter(a_dv, P, g.abs())
        c0 = 0
        run = z(*dq[:, :, sl].shape)
        for cw in chunks:
            cs = slice(c0, c0 + cw)
            c0 += cw
            dP = torch.einsum("bnrwc,bnrwkc->bnrwk", g[..., cs], vg[..., cs])
            dS = scale * P * (dP - (P * dP).sum(dim=-1, keepdim=True))
            aP = torch.einsum("bnrwc,bnrwkc->bnrwk", g[..., cs].abs(), vg[..., cs].abs())
            uS = scale * P * (aP + (P * aP).sum(dim=-1, keepdim=True))
            mS = dS.abs() + P * dS.abs().sum(dim=-1, keepdim=True)
            run = run + torch.einsum("bnrwk,bnrwkd->bnrwd", rnd(dS), kg)
            if emulate:
                run = _r16(run)
            dq_store[:, :, sl] += run.abs()
            a_dq[:, :, sl] += torch.einsum("bnrwk,bnrwkd->bnrwd", dS.abs(), kg.abs())
            u_dq[:, :, sl] += torch.einsum("bnrwk,bnrwkd->bnrwd", uS, kg.abs())
            scatter(dk, rnd(dS), qh[:, :, sl])
            scatter(a_dk, dS.abs(), qh[:, :, sl].abs())
            scatter(u_dk, uS, qh[:, :, sl].abs())
            m_dq[:, :, sl] += torch.einsum("bnrwk,bnrwkd->bnrwd", mS, kg.abs())
            scatter(m_dk, mS, qh[:, :, sl].abs())
        dq[:, :, sl] = run
    hi = lambda t: t.permute(0, 1, 4, 2, 3).reshape(B, -1, Ho, Wo)
    lo = lambda t: t.view(B, n, h, w, -1).permute(0, 1, 4, 2, 3).reshape(B, -1, h, w)
    return dict(dq=hi(dq), a_dq=hi(a_dq), u_dq=hi(u_dq), dq_store=hi(dq_store), dk=lo(dk), a_dk=lo(a_dk), u_dk=lo(u_dk), dv=lo(dv), a_dv=lo(a_dv), L=L,
                m_dq=hi(m_dq), m_dk=lo(m_dk), nacc=int(hits.max()), chunk=max(chunks))


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def bf16_bound(n, abs_sum, stored=None):
    """SLACK * (n * U * abs_sum + U * stored): ``n`` bf16 roundings per weight of the contraction, ``stored`` = |ref| summed over the bf16
    stores of the result (None: the result is stored in fp32)."""
    b = n * U * abs_sum
    if stored is not None:
        b = b + U * stored
    return SLACK * b


def score_abs_max(q, k, ksz, heads, rows_per_chunk=8):
    """L = the largest scale * sum_d |q_d||k_d| over the (query, key) pairs of the windows."""
    iy, ix = _tables(q, k, ksz)
    qh, kh = _heads(q, heads).abs(), _heads(k, heads).abs()
    iyt, ixt = torch.from_numpy(np.ascontiguousarray(iy)), torch.from_numpy(np.ascontiguousarray(ix))
    L = 0.0
    for r0 in range(0, qh.shape[2], rows_per_chunk):
        kg = _gather(kh, iyt[r0:r0 + rows_per_chunk], ixt)
        L = max(L, float(torch.einsum("bnrwd,bnrwkd->bnrwk", qh[:, :, r0:r0 + rows_per_chunk], kg).max()))
    return L * qh.shape[-1] ** -0.5


def fp32_weight_factor(L, Dq, kk):
    """Relative error of a softmax weight computed in fp32 throughout (the table-driven scalar kernels, xna_generic.hip): a score of Dq fp32
    multiply-adds is off by at most (Dq + 3) * 2^-24 * L with L = scale * sum_d |q_d||k_d| (the standard bound of an fp32 dot product; the
    largest over the window pairs), the weight by twice that (numerator and denominator), plus exp2 / rcp (a few ulp) and the kk-term
    sum: 2^-24 * (2 (Dq + 3) L + 2 kk + 16)."""
    return F32 * (2.0 * (Dq + 3) * L + 2.0 * kk + 16.0)


def fp32_score_factor(q, k, heads, ksz):
    kk = ksz * ksz if isinstance(ksz, int) else ksz[0] * ksz[1]
    return fp32_weight_factor(score_abs_max(q, k, ksz, heads), q.shape[1] // heads, kk)


def cancellation_factor(Dv, kk):
    """The fp32 term of dS = scale P (dP - delta), relative to the uncancelled sums u_dq / u_dk = contractions of
    scale P (|dout|.|v| + sum_l P_l |dout|.|v|_l): dP is a Dv-term fp32 sum, off by at most Dv * 2^-24 * |dout|.|v|; delta = sum_l P_l dP_l
    inherits that and adds its own kk-term sum and the few ulp by which the stored weights miss sum P = 1: (Dv + kk + 4) * 2^-24 *
    sum_l P_l |dout|.|v|_l.  Both under one factor: (Dv + kk + 8) * 2^-24.  Nothing of the scores' own error is in it: a relative error of
    P does not uncancel (m_dq / m_dk of backward_reference)."""
    return F32 * (Dv + kk + 8.0)


def backward_bounds(r, q, k, heads, ksz, path):
    """{"dq", "dk", "dv"} -> per-element bound for the backward ``path`` from backward_reference's dict ``r``.
    bf16 paths (anything but "generic"): P and dS are rounded to bf16 once, n = 1: 1.25 * 2^-8 * (abs-sum + stored).  On top of it dq and dk
    carry cancellation_factor * (u_dq, u_dk) -- and only that.  dP and delta are fp32 numbers and dS is scale P times their DIFFERENCE
    (xna_bwd2_kernel.h:396 / :451, xna_rows_bwd.hip:369 / :426): where the softmax is peaked, P -> one-hot and delta -> dP of the dominant
    key, the exact dS of that key is orders of magnitude below 2^-24 |dP| and no bound relative to |dS| holds for fp32 arithmetic.  Where
    nothing cancels the term is (Dv + kk + 8) * 2^-24 / 2^-8 of the bf16 term times u / a: a few per cent.  dv has no difference in it.
    "generic" (fp32 throughout, n = 0): the weights' relative error (fp32_weight_factor) on m_dq / m_dk / a_dv, the cancellation term, and
    the fp32 accumulation of kk (dq) or ``nacc`` (dk, dv: atomics) terms; dq is stored as bf16."""
    kk = ksz * ksz if isinstance(ksz, int) else ksz[0] * ksz[1]
    Dq = q.shape[1] // heads
    cc = cancellation_factor(r["chunk"], kk)
    fq, fk = cc * r["u_dq"], cc * r["u_dk"]
    if path == "generic":
        ep = fp32_weight_factor(r["L"], Dq, kk)
        return {"dq": ep * r["m_dq"] + fq + kk * F32 * r["a_dq"] + SLACK * U * r["dq_store"],
                "dk": ep * r["m_dk"] + fk + r["nacc"] * F32 * r["a_dk"], "dv": (ep + r["nacc"] * F32) * r["a_dv"], "fp32_dq": fq, "fp32_dk": fk}
    return {"dq": bf16_bound(1, r["a_dq"], r["dq_store"]) + fq, "dk": bf16_bound(1, r["a_dk"]) + fk, "dv": bf16_bound(1, r["a_dv"]),
            "fp32_dq": fq, "fp32_dk": fk}


def worst_ratio(err, abs_sum):
    """max err / abs_sum over the elements with a non-zero abs-sum (and the error where it is zero must be zero: asserted by the bound)."""
    m = abs_sum > 0
    return float((err[m] / abs_sum[m]).max()) if bool(m.any()) else 0.0


def check(err, bound, what):
    """Every element, none left out; the message names the worst one."""
    bad = err > bound
    if bool(bad.any()):
        r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        i = int(r.argmax())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements over the bound; worst err / bound {float(r.flatten()[i]):.3f} "
                             f"at {np.unravel_index(i, tuple(err.shape))} (err {float(err.flatten()[i]):.3e}, bound {float(bound.flatten()[i]):.3e})")


# ---- the cases of the device test (here so that the CPU companion sweeps the same geometries without importing that module) ----
# (id, path, sub-kernel, heads, Dq, (h, w), (Ho, Wo), window, C, families)
FWD_CASES = [
    ("cell-k7", "mfma", "cell", 4, 64, (9, 10), (36, 40), 7, 256, FORWARD_FAMILIES),             # 4 x 4 cells: generic tile loop
    ("cell-k3-ragged", "mfma", "cell", 4, 64, (6, 5), (18, 25), 3, 128, FORWARD_FAMILIES_SHORT),  # 15-query cells
    ("cell-k9-patch14", "mfma", "cell", 2, 64, (9, 9), (18, 126), 9, 128, FORWARD_FAMILIES_SHORT),  # partial row tiles
    ("cell-k15", "mfma", "cell", 2, 64, (15, 16), (30, 64), 15, 128, FORWARD_FAMILIES_SHORT),
    ("sliding-k7", "mfma", "sliding", 4, 64, (9, 10), (18, 160), 7, 256, FORWARD_FAMILIES),
    ("sliding-k9", "mfma", "sliding", 2, 64, (9, 10), (9, 160), 9, 128, FORWARD_FAMILIES_SHORT),
    ("sliding-k15", "mfma", "sliding", 2, 64, (15, 16), (15, 256), 15, 128, FORWARD_FAMILIES_SHORT),
    ("union-k7", "union", None, 4, 64, (9, 10), (23, 27), 7, 256, FORWARD_FAMILIES),              # ratio 2.56 x 2.7
    ("union-k3", "union", None, 4, 64, (9, 10), (23, 27), 3, 64, FORWARD_FAMILIES_SHORT),
    ("union-k9-ratio1", "union", None, 4, 64, (12, 14), (12, 14), 9, 256, FORWARD_FAMILIES_SHORT),
    ("union-k15", "union", None, 2, 64, (15, 16), (33, 35), 15, 128, FORWARD_FAMILIES_SHORT),
    ("rows-k7", "rows", None, 1, 96, (16, 18), (16, 18), 7, 3, FORWARD_FAMILIES),                 # the denoising call's shape class
    ("rows-k15", "rows", None, 1, 96, (16, 18), (16, 18), 15, 3, FORWARD_FAMILIES_SHORT),          # fifteen rows folded in by the online softmax
    ("rows-k3-noninteger", "rows", None, 2, 128, (9, 10), (23, 27), 3, 10, FORWARD_FAMILIES_SHORT),
    ("rows-k9", "rows", None, 1, 192, (10, 14), (50, 70), 9, 64, FORWARD_FAMILIES_SHORT),          # 5 x 5 cells, four channel tiles
    ("generic-k7", "generic", None, 4, 64, (9, 10), (23, 27), 7, 256, FORWARD_FAMILIES),
    ("generic-k9-cells", "generic", None, 2, 64, (9, 10), (36, 40), 9, 128, FORWARD_FAMILIES_SHORT),
    ("generic-k15", "generic", None, 1, 96, (16, 18), (16, 18), 15, 3, FORWARD_FAMILIES_SHORT),
    ("generic-k3", "generic", None, 4, 64, (9, 10), (23, 27), 3, 64, FORWARD_FAMILIES_SHORT),
]


def sliding_runs(ksz, lr, out_sz, out_dtype, logits=False):
    """xna_mfma.hip:94 restated: the sliding-window kernel takes an MFMA-path call when the window is 7 x 7 or larger, the plan has no staged
    stores, the cell rows are whole row tiles and no scores are asked for.  Staged stores exist for bf16 output only (xna_mfma_kernel.h:923),
    so the answer is known for fp32 output, for windows from 11 x 11 and wherever another condition fails; None = depends on the plan.  The device
    test checks the answer against the names of the kernels that actually ran."""
    dy, dx = out_sz[0] // lr[0], out_sz[1] // lr[1]
    if ksz < 7 or logits or dx % 16 or dy * dx // 16 > 1024:
        return False
    if ksz >= 11:
        return True                      # xna_mfma.hip:90: windows of 11 x 11 and up have no staged plan, whatever the output type
    return True if out_dtype == torch.float32 else None


def forward_inputs(case, fam):
    _, path, sub, heads, Dq, lr, out_sz, ksz, C, _ = case
    seed = 1000 + 7 * ksz + out_sz[1]
    q, k = make_qk((1, heads * Dq, *out_sz), (1, heads * Dq, *lr), fam[1], seed, heads)
    return q, k, make_values((1, C, *lr), fam[0], seed + 2)


def forward_bound(case, q, k, ref, a, out_dtype):
    _, path, _, heads, _, _, _, ksz, _, _ = case
    stored = ref.abs() if out_dtype == torch.bfloat16 else None
    if path == "generic":
        c = fp32_score_factor(q, k, heads, ksz)
        return c * a + (SLACK * U * stored if stored is not None else 0.0), c
    return bf16_bound(1, a, stored), U


# (id, path, heads, Dq, (h, w), (Ho, Wo), window, C, chunk count, families)
BWD_CASES = [
    ("cell", "mfma", 2, 64, (7, 8), (14, 128), 5, 64, 1, BACKWARD_FAMILIES),
    ("cell-k9", "mfma", 2, 64, (9, 10), (9, 160), 9, 128, 1, BACKWARD_FAMILIES_SHORT),
    ("cell-partial-tiles", "mfma", 2, 64, (7, 8), (14, 112), 7, 128, 1, BACKWARD_FAMILIES_SHORT),       # 14 of a tile's 16 lanes hold a query
    ("cell-chunked-k13", "mfma", 1, 64, (13, 14), (13, 224), 13, 128, 2, BACKWARD_FAMILIES_SHORT),      # chunks 64 + 64
    ("rows-ratio1", "rows", 1, 96, (12, 20), (12, 20), 5, 3, 0, BACKWARD_FAMILIES),
    ("rows-cells", "rows", 2, 64, (9, 11), (27, 44), 7, 64, 0, BACKWARD_FAMILIES_SHORT),                # ratio (3, 4): fragment path
    ("generic", "generic", 2, 64, (7, 8), (28, 32), 5, 64, 0, BACKWARD_FAMILIES),
    ("generic-noninteger", "generic", 2, 64, (5, 7), (23, 30), 3, 32, 0, BACKWARD_FAMILIES_SHORT),
]


def backward_inputs(case, fam):
    _, path, heads, Dq, lr, out_sz, ksz, C, _, _ = case
    seed = 2000 + 7 * ksz + out_sz[1]
    q, k = make_qk((1, heads * Dq, *out_sz), (1, heads * Dq, *lr), fam[2], seed, heads)
    return q, k, make_values((1, C, *lr), fam[0], seed + 2), make_values((1, C, *out_sz), fam[1], seed + 3)



# ---- stem ------------------------------------------------------------------------------------------------------------------------
def conv_reflect64(x, w, b):
    pad = w.shape[-1] // 2
    x = x.double()
    if pad:
        x = F.pad(x, (pad,) * 4, mode="reflect")
    return F.conv2d(x, w.double(), None if b is None else b.double())


def conv0_reference(img, w, b):
    """(ref, abs_sum) fp64: the first convolution and ``sum |x||w| + |bias|``."""
    return conv_reflect64(img, w, b), conv_reflect64(img.abs(), w.abs(), b.abs())


def conv0_bound(ref, abs_sum, ks, width):
    """include/naf_hip.h (naf_stem_conv0_fwd): the 3x3 layer of the default width carries its products to 16 mantissa bits -- within
    2^-15 * sum|x||w| of the fp32 convolution; the 1x1 layer and the general widths (stem_generic.hip:103, an fmaf chain) are fp32:
    (taps + 2) * 2^-24 * sum|x||w|.  Then ONE rounding to bf16 of ref + e: U * (|ref| + e)."""
    c = 2.0 ** -15 + (3 * ks * ks + 2) * F32 if (ks == 3 and width == 128) else (3 * ks * ks + 2) * F32
    return (1.0 + U) * c * abs_sum + U * ref.abs()


def group_sums(y, groups=8):
    """fp64 [B, groups, 2]: sum and sum of squares per GroupNorm group of y [B, C, H, W]."""
    B = y.shape[0]
    g = y.double().reshape(B, groups, -1)
    return torch.stack([g.sum(-1), (g * g).sum(-1)], dim=-1)


def group_sums_bound(ref, bound, groups=8):
    """GroupNorm sums of a tensor that is within ``bound`` of ``ref`` elementwise: |sum y - sum r| <= sum bound and |sum y^2 - sum r^2| <= sum
    bound (2|r| + bound); plus the fp32 partial sums of the producing workgroup (at most 256 sequential adds before the fp64 atomics):
    2^-16 of sum|r| and of sum r^2.  Relative to sum|y| and sum y^2, no absolute constant."""
    B = ref.shape[0]
    r, b = ref.double().reshape(B, groups, -1), bound.double().reshape(B, groups, -1)
    s1 = b.sum(-1) + 2.0 ** -16 * (r.abs() + b).sum(-1)
    s2 = (b * (2.0 * r.abs() + b)).sum(-1) + 2.0 ** -16 * ((r.abs() + b) ** 2).sum(-1)
    return torch.stack([s1, s2], dim=-1)


def layer_reference(x, gw, gb, w, b, eps=1e-5):
    """One GroupNorm -> SiLU -> conv layer on the bf16 activation x with bf16 weights w, in fp64, WITHOUT rounding SiLU(GN(x)): returns
    (ref, abs_sum = sum |w||a| ).  The kernel rounds a to bf16 once before the matrix cores (n = 1) and stores bf16."""
    a = F.silu(F.group_norm(x.double(), 8, gw.double(), gb.double(), eps))
    return conv_reflect64(a, w, b), conv_reflect64(a.abs(), w.abs(), None)


def conv_stem_bf16(image, p):
    """The oracle's conv stem with the HIP stem's roundings: every stored activation bf16, SiLU(GN(x)) rounded to bf16 before its
    convolution, the 128 -> 128 weights bf16 (ops.pack_conv_weight); fp32 arithmetic otherwise."""
    outs = []
    for pre in ("image_encoder.encoder", "image_encoder.sem_encoder"):
        x = bf16r(O._conv_reflect(image, p[f"{pre}.0.weight"], p[f"{pre}.0.bias"]))
        blk = 1
        while f"{pre}.{blk}.conv1.weight" in p:
            for j in (1, 2):
                a = bf16r(F.silu(F.group_norm(x, 8, p[f"{pre}.{blk}.norm{j}.weight"], p[f"{pre}.{blk}.norm{j}.bias"], eps=1e-5)))
                x = bf16r(O._conv_reflect(a, bf16r(p[f"{pre}.{blk}.conv{j}.weight"]), p[f"{pre}.{blk}.conv{j}.bias"]))
            blk += 1
        outs.append(x)
    return torch.cat(outs, dim=1)


def model_reference(p, image, feats, size, ksz, heads_attn=4, heads_rope=4, emulate=False):
    """(out, abs_sum) fp64 of the whole forward from the oracle's fp32 guidance; ``emulate``: the bf16 stem (conv_stem_bf16), bf16 pooled
    guidance, bf16 q / k / v and P rounded to bf16 -- the HIP pipeline's rounding points with exact arithmetic between them."""
    size = (int(size[0]), int(size[1]))
    if not emulate:
        x = O.image_encoder(image, size, p, heads_rope)
        k = O.key_pool(x, feats.shape[-2:])
        return attention_reference(x, k, feats, ksz, heads_attn)
    g = conv_stem_bf16(image, p)
    if g.shape[-2:] != size:
        g = bf16r(F.adaptive_avg_pool2d(g, size))
    xr = O.rope(g, p["image_encoder.rope.periods"], heads_rope)
    q, k = bf16r(xr), bf16r(O.key_pool(xr, feats.shape[-2:]))
    return attention_emulated(q, k, bf16r(feats), ksz, heads_attn), None


STEM_MEAN, STEM_MAX, STEM_HOT_REL = 8e-3, 1.5e-1, 1e-2


def stem_bound(ref, family):
    """(mean, max) error allowed for the whole stem: tests/test_gpu_parity.py::test_stem_whole_matches_oracle's mean <= 8e-3 / max <= 1.5e-1
    (GroupNorm makes the stem's output O(1) whatever the image's scale, so these constants carry over to every family) -- and for the
    hot pixel, whose outputs reach |ref| ~ 140 next to it, the same plus 1e-2 of the mean / max |ref|.  Both are statistics of the whole
    tensor, as the existing bound is: the bf16 emulation's largest error (0.93) is not at the largest |ref|."""
    rel = STEM_HOT_REL if family == "hot_pixel" else 0.0
    return STEM_MEAN + rel * float(ref.abs().mean()), STEM_MAX + rel * float(ref.abs().max())


def model_case():
    """(params, image, features) of the whole-model cases: a natural-like ImageNet-normalised 64 x 128 image and 8 x 8 x 128 features with
    per-channel offsets (x8) plus outlier tokens (x60), bf16-representable."""
    p = O.make_params(seed=11)
    img = make_image(1, 64, 128, "natural_norm", 95)
    ft = bf16r(make_values((1, 128, 8, 8), "chan_offset", 96) + make_values((1, 128, 8, 8), "outlier", 97))
    return p, img, ft


def model_bound(abs_sum):
    """SURVEY 8c's whole-forward bound with its relative term on the abs-sum instead of |ref|: 2e-2 + 1e-2 * sum_j P_j |v_j|."""
    return 2e-2 + 1e-2 * abs_sum


# ---- head ------------------------------------------------------------------------------------------------------------------------
HEAD_GEOM = (1, 8, 8, 8, 16, 7, 4)         # B, h, w, dy, dx, window, heads: 8 x 8 -> 64 x 128, row tiles, what the fused kernel serves
HEAD_CASES = {
    # name: (N, projected-value family, multiplier of PV (a power of two), bias offset, dominant class or None)
    "offset": (21, "chan_offset", 1.0, 0.0, None),
    "outlier": (21, "outlier", 1.0, 0.0, None),
    "logits50": (21, "unit", 16.0, 0.0, None),             # logits of magnitude ~50
    "bias40": (21, "unit", 16.0, 40.0, None),              # + 40 on every class bias: loss, g and labels are invariant
    "dominant": (19, "unit", 1.0, 0.0, 3),                 # class 3 carries + 30
}


def make_head_inputs(name, geom=HEAD_GEOM, seed=2300):
    """(q, k, pv [B, heads, h, w, Npad] with zero pad channels, pvn = its NCHW head-major form, bias [N]) -- all bf16-representable but
    the fp32 bias."""
    N, fam, mul, boff, dom = HEAD_CASES[name]
    B, h, w, dy, dx, ksz, heads = geom
    npad = (N + 15) // 16 * 16
    q, k = make_qk((B, 64 * heads, h * dy, w * dx), (B, 64 * heads, h, w), "unit", seed, heads)
    vals = make_values((B, heads * N, h, w), fam, seed + 2) * mul
    pv = torch.zeros(B, heads, h, w, npad)
    pv[..., :N] = vals.view(B, heads, N, h, w).permute(0, 1, 3, 4, 2)
    bias = O.hash_normal((N,), seed + 3) + boff
    if dom is not None:
        bias[dom] += 30.0
    return q, k, pv, pv.permute(0, 1, 4, 2, 3).reshape(B, heads * npad, h, w), bias


def head_reference64(q, k, pvn, ksz, heads, N, bias):
    """(ref [B, N, Ho, Wo], abs_sum = sum_g sum_j P_g,j |PV_g,j|) in fp64: the head-summed attention on the projected values plus bias."""
    B, _, Ho, Wo = q.shape
    o, a = attention_reference(q, k, pvn, ksz, heads)
    ref = o.view(B, heads, -1, Ho, Wo).sum(1)[:, :N] + bias.double().view(1, N, 1, 1)
    return ref, a.view(B, heads, -1, Ho, Wo).sum(1)[:, :N]


def head_bound(ref, abs_sum, out_bf16=False):
    """xna_head_kernel.h:287 rounds each head's normalised P to bf16 (n = 1 against the head-summed abs-sum); the heads and the bias add
    in fp32 (a 2^-22 |ref| allowance: the accumulators hold bias + partial sums of magnitude <= |bias| + abs_sum)."""
    b = bf16_bound(1, abs_sum, ref.abs() if out_bf16 else None)
    return b + 2.0 ** -22 * (ref.abs() + abs_sum)


def share_determined(ref, bound):
    """Share of the pixels whose top-2 margin in ref [B, N, H, W] exceeds 2 * bound [B, H, W]: where the argmax is fixed by the oracle alone."""
    top = ref.double().topk(2, dim=1).values
    det = (top[:, 0] - top[:, 1]) > 2.0 * bound
    return det, float(det.double().mean())


def profile_line(path, family, ratio, derived, of_bound):
    return f"{path:<34s} {str(family):<44s} worst err/abs_sum {ratio:.3e}   derived {derived:.3e}   worst err/bound {of_bound:.3f}"


def worst_of_bound(err, bound):
    m = bound > 0
    return float((err[m] / bound[m]).max()) if bool(m.any()) else 0.0


assert math.isclose(U, 0.00390625)
