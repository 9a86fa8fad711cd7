"""The training side of the conv stem restated in fp64, the input families it is tested on and the per-element bounds the HIP kernels are
held to (tests/test_gpu_stem_backward.py on the device, tests/test_stem_backward_cpu.py without one).  Plain helper module: no test in it.

Layout: activations and their gradients are [B, H, W, C] (channels last, as the kernels store them), weights [oc, ic, k, k], images
[B, 3, H, W].  Every function returns fp64 and, next to each result, its ABS-SUM: the same contraction with absolute values
(tests/input_statistics.py explains why: a rounding of relative size u inside a sum moves it by at most u * abs-sum, per element and
equivariant under scaling of the inputs).  U = 2^-8 (bf16), F32 = 2^-24, SLACK = 1.25 are input_statistics' (``S.``).

Rounding points, read from the sources (naf_amd/csrc):

  SiLU(GroupNorm) backward, stem_act_bwd_kernel<1 / 2> (stem_bwd.hip:100-288), dx = rstd (gamma dz - m1 - xhat m2), dz = da silu'(z)
    gn_vectors (stem_bwd.hip:44-60)  mean and rstd in fp64 from the {sum, sum^2} the caller passes, then rounded to fp32: sc = gamma * rstd,
              sh = beta - mean * gamma * rstd, rs = rstd, rm = -mean * rstd -- two to three fp32 roundings each.  z = fmaf(x, sc, sh) (:142)
              and xhat = fmaf(x, rs, rm) (:145) are therefore off by |dz_| <= 4 F32 zabs, zabs = (|x| + |mean|) rstd |gamma| + |beta|, and
              |dxhat_| <= 3 F32 xhabs, xhabs = (|x| + |mean|) rstd: ABSOLUTE in the uncancelled magnitudes (a group whose mean is far above
              its standard deviation loses that many bits of xhat).
    sigmoidf_fast (:62)  rcp(1 + exp2(-z log2 e)): the product z * log2 e is rounded (relative 2^-24 of a number of size 1.44 |z|, i.e. a
              relative |z| 2^-24 of the exponential, twice with the constant's own rounding), v_exp_f32 and v_rcp_f32 are 1 ulp each:
              s is relative (2 |z| + 4) F32.  silu'(z) = s (1 + z (1 - s)) (:144: one subtraction, one fmaf, two products): within
              (2 |z| + 8) F32 G of exact, G = s (1 + |z| (1 - s)) (for z > 10 the subtraction 1 - s is exact and inherits 2 ulp of s, times
              |z|: covered by 2 |z| F32 G since G >= s ~ 1).  Where exp2 overflows (z < -88) rcp(inf) = 0 and the exact value is below
              2^-126 (1 + |z|); denormal results are flushed: an absolute floor TINY (1 + |z|) per unit of |da|.  |silu''| <= 1/2, so the
              error of z adds |da| dz_ / 2.
    fold (:164-178, :203, :216, :261, :267)  the adjoint of the reflect padding adds up to four bf16 values in fp32: 3 F32 fold(|da|).
              Together  E_dz = fold(|da|) (F32 ((2 |z| + 11) G + 2 zabs) + TINY (1 + |z|)).
    sums (:147-148, :272-286)  a thread adds its pixels' dz and dz * xhat in fp32 -- rows_per_block * ceil(W / nplanes) of them, nplanes =
              256 / tpp pixel planes (act_common :290-308, restated in ``act_bwd_chain``) --, one thread adds the nplanes partial sums in fp32
              (:283), the workgroups meet in fp64 atomics (:285).  A sum of n fp32 terms in ANY order is within (n - 1) F32 sum |terms|:
              dS1 <= chain F32 sum |dz| + sum E_dz,  dS2 <= (chain + 2) F32 sum |dz xhat| + sum (E_dz |xhat| + |dz| dxhat_),  chain = pixels per
              thread + nplanes.  These are d beta and d gamma per sample.
    means (:107-112)  m1, m2 = sum_c gamma_c S[c] / N in fp64, rounded to fp32 once: dm <= sum_c |gamma_c| dS[c] / N + F32 |m|.
    dx (:150)  rs * (gam * dz - m1 - xh * m2): four fp32 roundings of the uncancelled terms, then ONE bf16 store:
              |err| <= 1.25 * 2^-8 |ref| + (1 + 2^-8) rstd (|gamma| E_dz + dm1 + |xhat| dm2 + |m2| dxhat_ + 4 F32 (|gamma dz| + |m1| + |xhat m2|)).
  weight gradient, dW[oc, ic, ty, tx] = sum_px dy[px, oc] a_pad[px + tap, ic]
    stem_wgrad_kernel (stem_wgrad.hip:128-131), stem_wgrad2_kernel (silu8, :336-350), stem_wgradg_kernel (stem_generic_bwd.hip:131-132): with
              stats_in the loader computes a = z * rcp(1 + exp2(-z log2 e)) in fp32 from the same affine vectors (|da_| <= F32 (4.4 zabs +
              (2 |z| + 6) |a|) + TINY: |silu'| <= 1.1) and rounds it to bf16 ONCE: n = 1 against sum |dy| |a|.  Plain mode (stats_in == NULL):
              both operands are the caller's bf16, products of bf16 are exact in fp32.
    accumulation  v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16 into fp32 registers over the workgroup's pixels, then fp32 atomics
              (stem_wgrad.hip:212, :546; stem_generic_bwd.hip:179).  Any order of an n-term fp32 sum: (n - 1) F32 abs-sum with n = B H W.
    d bias    sum_px dy: fp32 per-thread sums, an LDS reduction, atomics (stem_wgrad.hip:113-114, :184-195, :521-531): B H W F32 sum |dy|.
  first convolution
    stem_conv0_wgrad_kernel (stem_bwd.hip:382-392, C < 32: the launcher's condition at :555) an fmaf chain in fp32: B H W F32 abs-sum.
    stem_conv0_wgrad_mfma_kernel (:505-513) splits every fp32 image value v into bf16 hi + bf16 lo: hi = bf16(v) is within U |v| = 2^-8 |v| (round to
              nearest, 8 significand bits), r = v - hi is exact in fp32, and lo = bf16(r) misses r by at most U |r| <= 2^-16 |v|: 2^-16 sum |dy| |image|
              on top of the accumulation; a bf16 image has lo = 0.
    stem_conv0_dgrad_kernel (stem_generic_bwd.hip:250-283) one thread, one fmaf chain over (row pairs) x (column pairs) x C: at most 5 x 5 pairs
              (three taps plus two mirrored ones per axis, H = 3 or W = 3): 25 C F32.
  RoPE + key pooling adjoint, rope_pool_bwd_kernel (rope_pool.hip:443-510): G = dq + sum_cells dk / npix (1 / npix: a division, the product of
              the two axes' weights and up to four fmaf: 9 roundings), then the rotation by the negative angle (:504-505: a product, an fmaf)
              from the fp32 cos / sin TABLES the caller passes -- the reference takes the same tables --: 12 F32 (|G1| |c| + |G2| |s|), ONE
              bf16 store.
  composed layer (naf_amd/model.py:287-301): stem_conv_plain stores the data gradient in bf16 once (stem_generic.hip:110 and the hand-scheduled
              kernels alike) after an fp32 matrix-core sum of k k C products of bf16 numbers: e = 1.25 * 2^-8 |da| + k k C F32 sum |w| |g|.  The
              SiLU / GroupNorm backward is linear in da: its own bound evaluated at |da| + e, plus the image of e under it.

No constant here is measured: every factor is one of the counts above.  The worst err / abs_sum and the worst share of each bound that the
kernels use on an MI355X are recorded in profiles/stem_backward_statistics.txt (NAF_STEM_BWD_PROFILE=<file> appends the lines).
"""
import math

import torch
import torch.nn.functional as F

import input_statistics as S
from oracle import naf_oracle as O

U, F32, SLACK = S.U, S.F32, S.SLACK
TINY = 2.0 ** -125
GROUPS = 8
FAMILIES = ("iid", "correlated", "chan_offset", "outlier", "from_stem")
OUTLIER_PERIOD = 97     # one pixel in 97 carries 100 x the scale: the group's standard deviation rises to ~10, xhat of those pixels to ~35


def r16(t):
    return t.to(torch.bfloat16).to(torch.float64)


# ---- GroupNorm statistics as the kernels receive and use them ---------------------------------------------------------------------
def group_totals(x):
    """fp64 [B, 8, 2]: {sum, sum of squares} per (sample, GroupNorm group) of x [B, H, W, C] -- what the forward kernels accumulate."""
    B, C = x.shape[0], x.shape[-1]
    xd = x.double().reshape(B, -1, GROUPS, C // GROUPS)
    return torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], dim=-1)


def gn_mean_rstd(x, eps, totals=None):
    """fp64 ([B, 1, 1, C] mean, rstd) from the {sum, sum^2} totals exactly as gn_vectors forms them (stem_bwd.hip:47-53)."""
    B, H, W, C = x.shape
    t = group_totals(x) if totals is None else totals.double()
    n = float(H * W * (C // GROUPS))
    mean = t[..., 0] / n
    var = (t[..., 1] / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    ex = lambda v: v.repeat_interleave(C // GROUPS, dim=1).view(B, 1, 1, C)
    return ex(mean), ex(rstd)


def act_forward(x, gamma, beta, eps, totals=None):
    """a = SiLU(GroupNorm(x)) in fp64 with the intermediates the bounds need: dict a, z, xh, s, zabs, xhabs, rstd, mean, da_ (the fp32 error
    of a before its bf16 rounding)."""
    xd = x.double()
    mean, rstd = gn_mean_rstd(x, eps, totals)
    g, b = gamma.double().view(1, 1, 1, -1), beta.double().view(1, 1, 1, -1)
    xh = (xd - mean) * rstd
    z = xh * g + b
    s = torch.sigmoid(z)
    xhabs = (xd.abs() + mean.abs()) * rstd
    zabs = xhabs * g.abs() + b.abs()
    a = z * s
    return dict(a=a, z=z, xh=xh, s=s, zabs=zabs, xhabs=xhabs, rstd=rstd, mean=mean,
                da_=F32 * (4.4 * zabs + (2.0 * z.abs() + 6.0) * a.abs()) + TINY)


def fold_adjoint(d, skip=None):
    """Adjoint of reflect padding by one pixel: [B, H + 2, W + 2, C] -> [B, H, W, C]; padded row -1 adds onto row 1, padded row H onto row
    H - 2, the same for columns.  ``skip=(py, px)``: that element of the padded domain is left out (a planted defect)."""
    if skip is not None:
        d = d.clone()
        d[:, skip[0], skip[1]] = 0
    r = d[:, 1:-1].clone()
    r[:, 1] += d[:, 0]
    r[:, -2] += d[:, -1]
    c = r[:, :, 1:-1].clone()
    c[:, :, 1] += r[:, :, 0]
    c[:, :, -2] += r[:, :, -1]
    return c


def _group_mean(t):
    """mean over (pixels, channels of a group) of t [B, H, W, C], expanded back to [B, 1, 1, C]."""
    B, H, W, C = t.shape
    m = t.reshape(B, H * W, GROUPS, C // GROUPS).mean((1, 3))
    return m.repeat_interleave(C // GROUPS, dim=1).view(B, 1, 1, C)


def act_bwd_chain(H, W, C, cu_count=256):
    """act_common (stem_bwd.hip:290-308) restated: the number of fp32 additions behind one element of the sums = a thread's pixels
    (rows_per_block rows, every nplanes-th pixel) + the nplanes partial sums."""
    tpp = 1
    while tpp * 8 < C:
        tpp <<= 1
    nplanes = 256 // tpp
    rows = max(1, -(-H // (cu_count * 8)))
    return rows * -(-W // nplanes) + nplanes


def act_bwd_reference(x, da, gamma, beta, eps, fold, totals=None, extra=None):
    """SiLU(GroupNorm(x)) backward in fp64.  da [B, H, W, C], or [B, H + 2, W + 2, C] with ``fold``.  Returns a dict:
      dx [B, H, W, C];  sums [B, C, 2] = per sample {d beta, d gamma} (the kernel's layout);  dgamma, dbeta [C]
      the tensors the bounds are built from (act_bwd_bounds).  ``extra`` [B, H, W, C] >= 0: an error of da (after the fold) that the caller
      wants carried through (the composed layer)."""
    f = act_forward(x, gamma, beta, eps, totals)
    g = gamma.double().view(1, 1, 1, -1)
    dad = da.double()
    d, ad = (fold_adjoint(dad), fold_adjoint(dad.abs())) if fold else (dad, dad.abs())
    if extra is not None:
        ad = ad + extra
    z, s, xh, rstd = f["z"], f["s"], f["xh"], f["rstd"]
    gp = s * (1.0 + z * (1.0 - s))
    G = s * (1.0 + z.abs() * (1.0 - s))
    dz, adz = d * gp, ad * gp.abs()
    m1, m2 = _group_mean(g * dz), _group_mean(g * dz * xh)
    dx = rstd * (g * dz - m1 - xh * m2)
    sums = torch.stack([dz.sum((1, 2)), (dz * xh).sum((1, 2))], dim=-1)
    return dict(dx=dx, sums=sums, dbeta=sums[..., 0].sum(0), dgamma=sums[..., 1].sum(0), f=f, g=g, ad=ad, adz=adz, dz=dz, G=G, m1=m1, m2=m2)


def act_bwd_linear_image(r, e):
    """What an error ``e`` >= 0 of da (after the fold) can move dx by: rstd (|gamma| |silu'| e + mean(...) + |xhat| mean(... |xhat|))."""
    f, g = r["f"], r["g"].abs()
    gp = (r["f"]["s"] * (1.0 + f["z"] * (1.0 - f["s"]))).abs()
    t = g * gp * e
    return f["rstd"] * (t + _group_mean(t) + f["xh"].abs() * _group_mean(t * f["xh"].abs()))


def act_bwd_bounds(r, chain):
    """{"dx", "sums"} -> per-element bounds of the module docstring from act_bwd_reference's dict; ``chain`` = act_bwd_chain(...)."""
    f, g = r["f"], r["g"].abs()
    z, xh, rstd = f["z"], f["xh"].abs(), f["rstd"]
    e_dz = r["ad"] * (F32 * ((2.0 * z.abs() + 11.0) * r["G"] + 2.0 * f["zabs"]) + TINY * (1.0 + z.abs()))
    dxh = 3.0 * F32 * f["xhabs"]
    ds1 = chain * F32 * r["adz"].sum((1, 2)) + e_dz.sum((1, 2))                                           # [B, C]
    ds2 = (chain + 2) * F32 * (r["adz"] * xh).sum((1, 2)) + (e_dz * xh + r["adz"] * dxh).sum((1, 2))
    B, H, W, C = z.shape
    n = float(H * W * (C // GROUPS))
    gsum = lambda t: (g.view(1, C) * t).reshape(B, GROUPS, C // GROUPS).sum(-1).repeat_interleave(C // GROUPS, dim=1).view(B, 1, 1, C) / n
    dm1, dm2 = gsum(ds1) + F32 * r["m1"].abs(), gsum(ds2) + F32 * r["m2"].abs()
    fp = rstd * (g * e_dz + dm1 + xh * dm2 + r["m2"].abs() * dxh + 4.0 * F32 * ((g * r["dz"]).abs() + r["m1"].abs() + (xh * r["m2"]).abs()))
    return {"dx": SLACK * U * r["dx"].abs() + (1.0 + U) * fp, "sums": torch.stack([ds1, ds2], dim=-1), "fp32_dx": fp}


def act_bwd_abs_sum(r):
    """The uncancelled magnitude of dx: rstd (|gamma dz| + |m1| + |xhat m2|) -- what the profile's err / abs_sum is relative to."""
    return r["f"]["rstd"] * ((r["g"] * r["dz"]).abs() + r["m1"].abs() + (r["f"]["xh"] * r["m2"]).abs())


def act_bwd_emulated(x, da, gamma, beta, eps, fold, m1_scale=1.0, wrong_group=False, skip=None):
    """The kernel's arithmetic on the host: fp32 throughout from gn_vectors' fp32 affine vectors, fp32 sums (torch's order), the means rounded
    to fp32, dx rounded to bf16.  Planted defects: ``m1_scale`` multiplies mean(dxhat); ``wrong_group``: the LAST channel of every group reads
    the next group's two means (what one pair of means per 8-channel chunk would do at widths 48 and 240); ``skip``: see fold_adjoint.
    Returns (dx fp64 [B, H, W, C], sums fp64 [B, C, 2])."""
    B, H, W, C = x.shape
    mean, rstd = gn_mean_rstd(x, eps)
    gm = gamma.float().view(1, 1, 1, C)
    rs = rstd.float()
    sc, sh = gm * rs, beta.float().view(1, 1, 1, C) - mean.float() * gm * rs
    rm = -mean.float() * rs
    xf = x.float()
    d = fold_adjoint(da.float(), skip) if fold else da.float()
    z = xf * sc + sh
    s = torch.sigmoid(z)
    dz = d * (s * (z * (1.0 - s) + 1.0))
    xh = xf * rs + rm
    sums = torch.stack([dz.sum((1, 2)), (dz * xh).sum((1, 2))], dim=-1).double()
    n = float(H * W * (C // GROUPS))
    gs = (gamma.double().view(1, C, 1) * sums).reshape(B, GROUPS, C // GROUPS, 2).sum(2) / n         # [B, 8, 2]
    m = gs.float().repeat_interleave(C // GROUPS, dim=1)                                               # [B, C, 2]
    if wrong_group:
        last = torch.arange(C) % (C // GROUPS) == C // GROUPS - 1
        nxt = gs.float().roll(-1, dims=1).repeat_interleave(C // GROUPS, dim=1)
        m = torch.where(last.view(1, C, 1), nxt, m)
    m1, m2 = m[..., 0].view(B, 1, 1, C) * m1_scale, m[..., 1].view(B, 1, 1, C)
    return r16(rs * (gm * dz - m1 - xh * m2)), sums


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------
def reflect_pad_nhwc(a, pad):
    return F.pad(a.permute(0, 3, 1, 2), (pad,) * 4, mode="reflect").permute(0, 2, 3, 1) if pad else a


def wgrad_reference(dy, a, k, shift_tap=None, dtype=torch.float64):
    """(dW [oc, ic, k, k], abs-sum, d bias [oc], its abs-sum) of y = conv_k(reflect_pad(a)): dW[oc, ic, ty, tx] = sum dy[b, y, x, oc]
    a_pad[b, y + ty, x + tx, ic].  ``shift_tap=(ty, tx)``: that tap reads its pixels shifted by one column (a planted defect)."""
    B, H, W, C = a.shape
    dyd, ad = dy.to(dtype), a.to(dtype)
    ap = reflect_pad_nhwc(ad, k // 2)
    dw = torch.empty(dy.shape[-1], C, k, k, dtype=dtype)
    aw = torch.empty_like(dw)
    dy2, ady2 = dyd.reshape(-1, dy.shape[-1]), dyd.abs().reshape(-1, dy.shape[-1])
    for ty in range(k):
        for tx in range(k):
            win = ap[:, ty:ty + H, tx:tx + W]
            if shift_tap == (ty, tx):                          # the neighbouring tap's pixels (k = 3), the row rotated by one (k = 1: no border to read)
                win = ap[:, ty:ty + H, (tx + 1 if tx < 2 else tx - 1):][:, :, :W] if k == 3 else win.roll(-1, dims=2)
            w2 = win.reshape(-1, C)
            dw[:, :, ty, tx] = dy2.t() @ w2
            aw[:, :, ty, tx] = ady2.t() @ w2.abs()
    return dw, aw, dy2.sum(0), ady2.sum(0)


def wgrad_bounds(dy, aw, a_db, k, f=None):
    """Per-element bounds of (dW, d bias).  ``f`` = act_forward's dict: the loader computed a (one bf16 rounding of a plus its fp32 error);
    None: plain mode, the fp32 accumulation only."""
    B, H, W, _ = dy.shape
    n = B * H * W
    acc = n * F32 * aw
    if f is None:
        return acc, n * F32 * a_db
    _, e, _, _ = wgrad_reference(dy.double().abs(), f["da_"], k)
    return S.bf16_bound(1, aw) + (1.0 + U) * e + acc, n * F32 * a_db


def wgrad_emulated(dy, x, gamma, beta, eps, k, shift_tap=None):
    """fp32 SiLU(GroupNorm(x)) rounded to bf16, the contraction in fp32."""
    mean, rstd = gn_mean_rstd(x, eps)
    gm = gamma.float().view(1, 1, 1, -1)
    sc = gm * rstd.float()
    sh = beta.float().view(1, 1, 1, -1) - mean.float() * sc
    z = x.float() * sc + sh
    a = S.bf16r(z * torch.sigmoid(z))
    dw, _, db, _ = wgrad_reference(dy.float(), a, k, shift_tap, dtype=torch.float32)
    return dw.double(), db.double()


# ---- first convolution ------------------------------------------------------------------------------------------------------------------
def conv0_grads_reference(dy, image, weight):
    """Gradients of y = conv_k(reflect_pad(image)) + bias, image [B, 3, H, W], weight [C, 3, k, k], dy [B, H, W, C]: dict dw [C, 3, k, k], db [C],
    dimage [B, 3, H, W] and the abs-sums a_dw, a_db, a_dimage."""
    k = weight.shape[-1]
    im = image.double().permute(0, 2, 3, 1)                                  # [B, H, W, 3]
    dw, a_dw, db, a_db = wgrad_reference(dy, im, k)

    def adjoint(g, w):
        B, H, W, C = g.shape
        out = torch.zeros(B, H + k - 1, W + k - 1, 3, dtype=torch.float64)
        for ty in range(k):
            for tx in range(k):
                out[:, ty:ty + H, tx:tx + W] += g @ w[:, :, ty, tx]
        return (fold_adjoint(out) if k == 3 else out).permute(0, 3, 1, 2)
    return dict(dw=dw, a_dw=a_dw, db=db, a_db=a_db, dimage=adjoint(dy.double(), weight.double()), a_dimage=adjoint(dy.double().abs(), weight.double().abs()))


def conv0_bounds(r, dy, image_is_fp32, mfma):
    B, H, W, C = dy.shape
    n = B * H * W
    split = 2.0 ** -16 if (mfma and image_is_fp32) else 0.0
    return {"dw": (n * F32 + split) * r["a_dw"], "db": n * F32 * r["a_db"], "dimage": 25 * C * F32 * r["a_dimage"]}


def conv0_grads_emulated(dy, image, weight, mfma):
    """The first convolution's gradients with the kernels' arithmetic on the host: fp32 sums (torch's order); ``mfma``: the image as bf16 hi + bf16 lo,
    two contractions (stem_bwd.hip:508-523).  Returns fp64 (dw, db, dimage)."""
    k = weight.shape[-1]
    im = image.float().permute(0, 2, 3, 1)
    if mfma:
        hi = S.bf16r(im)
        lo = S.bf16r(im - hi)
        d1, _, db, _ = wgrad_reference(dy, hi, k, dtype=torch.float32)
        d2, _, _, _ = wgrad_reference(dy, lo, k, dtype=torch.float32)
        dw = d1 + d2
    else:
        dw, _, db, _ = wgrad_reference(dy, im, k, dtype=torch.float32)
    B, H, W, C = dy.shape
    out = torch.zeros(B, H + k - 1, W + k - 1, 3)
    for ty in range(k):
        for tx in range(k):
            out[:, ty:ty + H, tx:tx + W] += dy.float() @ weight.float()[:, :, ty, tx]
    dimage = (fold_adjoint(out) if k == 3 else out).permute(0, 3, 1, 2)
    return dw.double(), db.double(), dimage.double()


# ---- RoPE + adaptive key pooling, adjoint -------------------------------------------------------------------------------------------------
def rope_tables64(periods, H, W):
    """fp64 ([H, 2, P], [W, 2, P]) cos / sin tables of the oracle's angles (naf_oracle.rope_angles), the layout of ops.rope_tables."""
    per = periods.double()
    ay = 2 * math.pi * (2.0 * (torch.arange(0.5, H, dtype=torch.float64) / H) - 1.0)[:, None] / per[None]
    ax = 2 * math.pi * (2.0 * (torch.arange(0.5, W, dtype=torch.float64) / W) - 1.0)[:, None] / per[None]
    return torch.stack([ay.cos(), ay.sin()], 1), torch.stack([ax.cos(), ax.sin()], 1)


def rope_pool_bwd_reference(dq, dk, tab_y, tab_x, dtype=torch.float64):
    """dx = R^T (dq + sum over the cells whose window holds the pixel of dk / npix), fp64.  dq [B, heads, H, W, D], dk [B, heads, h, w, D],
    tables as ops.rope_tables returns them.  Returns (dx [B, heads * D, H, W], abs-sum).  ``dtype=torch.float32``: the host emulation's arithmetic."""
    B, n, H, W, D = dq.shape
    h, w = dk.shape[2], dk.shape[3]
    P = D // 4

    def spread(L, m):                       # [L, m]: 1 / window size where cell i's window [floor(i L / m), ceil((i + 1) L / m)) holds the position
        M = torch.zeros(L, m, dtype=dtype)
        for i in range(m):
            s, e = (i * L) // m, -((-(i + 1) * L) // m)
            M[s:e, i] = 1.0 / (e - s)
        return M
    My, Mx = spread(H, h), spread(W, w)
    up = lambda t: torch.einsum("yi,bnijd,xj->bnyxd", My, t, Mx)
    ty, tx = tab_y.to(dtype), tab_x.to(dtype)
    c = torch.cat([ty[:, None, 0].expand(H, W, P), tx[None, :, 0].expand(H, W, P)], -1)     # [H, W, D / 2]
    s = torch.cat([ty[:, None, 1].expand(H, W, P), tx[None, :, 1].expand(H, W, P)], -1)

    def rot(G, c_, s_, sign):
        g1, g2 = G[..., : D // 2], G[..., D // 2:]
        return torch.cat([g1 * c_ + g2 * s_, g2 * c_ + sign * g1 * s_], -1)
    G, A = dq.to(dtype) + up(dk.to(dtype)), dq.to(dtype).abs() + up(dk.to(dtype).abs())
    nchw = lambda t: t.permute(0, 1, 4, 2, 3).reshape(B, n * D, H, W)
    return nchw(rot(G, c, s, -1.0)), nchw(rot(A, c.abs(), s.abs(), 1.0))


def rope_pool_bwd_bound(ref, a):
    return SLACK * U * ref.abs() + 12.0 * F32 * a


# ---- composed layer ---------------------------------------------------------------------------------------------------------------------
def layer_dgrad_reference(g, weight, dtype=torch.float64):
    """The data gradient of y = conv_k(reflect_pad(a)) on the PADDED domain (k = 3: [B, H + 2, W + 2, C], before the fold) or on the image (k = 1),
    with its abs-sum: da[p + tap, ic] += g[p, oc] w[oc, ic, tap]."""
    k = weight.shape[-1]
    B, H, W, C = g.shape
    gd, wd = g.to(dtype), weight.to(dtype)
    out, ab = (torch.zeros(B, H + k - 1, W + k - 1, C, dtype=dtype) for _ in range(2))
    for ty in range(k):
        for tx in range(k):
            out[:, ty:ty + H, tx:tx + W] += gd @ wd[:, :, ty, tx]
            ab[:, ty:ty + H, tx:tx + W] += gd.abs() @ wd[:, :, ty, tx].abs()
    return out, ab


def layer_emulated(x, g, gamma, beta, eps, weight):
    """The composed layer on the host: the data gradient summed in fp32 and stored as bf16, then act_bwd_emulated on it."""
    k = weight.shape[-1]
    da = S.bf16r(layer_dgrad_reference(g, weight, torch.float32)[0])
    return act_bwd_emulated(x, da, gamma, beta, eps, k == 3)[0]


def layer_reference(x, g, gamma, beta, eps, weight, chain):
    """One layer of _HipStem.backward: dx of conv_k(reflect_pad(SiLU(GN(x)))) for the output gradient g, and its per-element bound = the
    convolution's (one bf16 store e of da, the fp32 sum) carried through the activation backward, plus that kernel's own bound at |da| + e."""
    k = weight.shape[-1]
    da, ab = layer_dgrad_reference(g, weight)
    e = SLACK * U * da.abs() + k * k * x.shape[-1] * F32 * ab
    ef = fold_adjoint(e) if k == 3 else e
    r = act_bwd_reference(x, da, gamma, beta, eps, fold=(k == 3), extra=ef)
    b = act_bwd_bounds(r, chain)
    return r, b["dx"] + (1.0 + U) * act_bwd_linear_image(r, ef)


# ---- input families -----------------------------------------------------------------------------------------------------------------------
def outlier_pixels(H, W):
    idx = torch.arange(H * W, dtype=torch.int64)
    return (((idx * 7 + 3) % OUTLIER_PERIOD) == 0).view(1, H, W, 1)


def make_affine(C, seed, family="iid"):
    gamma, beta = 1.0 + 0.3 * O.hash_normal((C,), seed + 11), 0.2 * O.hash_normal((C,), seed + 12)
    if family == "outlier":
        gamma = torch.where(torch.arange(C) % 5 == 0, gamma * 4.0, gamma)        # z of the outlier pixels passes -88: exp2 overflows in sigmoidf_fast
    return gamma, beta


def make_x(family, B, H, W, C, seed):
    """bf16-representable fp32 layer input [B, H, W, C] of the family (not ``from_stem``: that one is computed from an image)."""
    x = O.hash_normal((B, H, W, C), seed)
    if family in ("iid", "correlated"):
        x = x * 1.5 - 0.3
    elif family == "chan_offset":
        # per-channel means up to +-8 (x 3.47), per-group scales 2^-3 .. 2^3; groups 2 and 5: every channel near +30, |mean| ~ 30 standard deviations
        off = 8.0 * O.hash_normal((C,), seed + 1) / 3.47
        grp = torch.arange(C) // (C // GROUPS)
        off = torch.where((grp == 2) | (grp == 5), 30.0 + 0.25 * off, off)
        scale = 2.0 ** (grp % 7 - 3).float()
        x = (x + off) * scale
    elif family == "outlier":
        x = torch.where(outlier_pixels(H, W), x * 100.0, x)
    else:
        raise ValueError(family)
    return S.bf16r(x)


def make_grad(family, x, fold, seed):
    """bf16-representable incoming gradient for x [B, H, W, C]: [B, H, W, C], or on the reflect-padded domain with ``fold``."""
    B, H, W, C = x.shape
    xp = reflect_pad_nhwc(x, 1) if fold else x
    n = O.hash_normal(tuple(xp.shape), seed + 5)
    if family == "iid":
        d = n
    elif family in ("correlated", "from_stem"):
        sd = xp.std().clamp_min(1e-6)
        d = 0.5 + 0.5 * (xp - xp.mean()) / sd + n                       # a mean and a correlation with x: both GroupNorm means are O(1)
    elif family == "chan_offset":
        d = n + 0.5 * O.hash_normal((C,), seed + 6)
    elif family == "outlier":
        hp, wp = xp.shape[1], xp.shape[2]
        d = torch.where(outlier_pixels(hp, wp), n * 100.0, n)
    else:
        raise ValueError(family)
    return S.bf16r(d)


def from_stem_case(C, B, H, W, image_family, seed):
    """(image fp32 [B, 3, H, W], conv0 weight [C, 3, 3, 3], bias [C]): x of the ``from_stem`` family is bf16(conv0(image))."""
    img = S.make_image(B, H, W, image_family, seed)
    return img, O.hash_normal((C, 3, 3, 3), seed + 1, 1.0 / math.sqrt(27.0)), O.hash_normal((C,), seed + 2, 0.1)


def from_stem_x_host(img, w, b):
    """The host's stand-in for the HIP stem's first layer (the CPU companion test): fp64 convolution, one bf16 rounding."""
    return S.bf16r(S.conv_reflect64(img, w, b).permute(0, 2, 3, 1).float())


# ---- the exact pixel census ---------------------------------------------------------------------------------------------------------------
def census_bits(n):
    return max(1, int(n).bit_length())


def census_dy(B, H, W, C):
    """Pass (a): dy[b, y, x, oc] = bit (oc mod nbits) of (1 + the pixel's index over the batch); with a == 1 every dW[oc, ic, tap] and d bias[oc]
    is the number of pixels whose index has that bit.  Returns (dy fp32 0 / 1, counts int64 [C], nbits)."""
    n = B * H * W
    nbits = census_bits(n)
    assert nbits <= C, "every bit of the pixel index needs an output channel"
    idx = torch.arange(1, n + 1, dtype=torch.int64).view(B, H, W, 1)
    bit = (torch.arange(C) % nbits).view(1, 1, 1, C)
    dy = ((idx >> bit) & 1)
    return dy.float(), dy.reshape(-1, C).sum(0), nbits


def census_decode(diff, nbits, shape):
    """diff = got - expected of pass (a), int64 [oc, ic, k, k] -> a sentence naming the pixel whose contribution was lost (-) or doubled (+):
    the output channels that are off spell the bits of 1 + its index; the input channels and taps that are off name the 16-byte piece."""
    B, H, W = shape
    bad = diff != 0
    if not bool(bad.any()):
        return "nothing lost"
    kk = diff.shape[2] * diff.shape[3]
    cols = bad.sum(0).flatten()                                             # wrong output channels per (ic, tap) column
    col = int(cols.argmax())
    centre = (col // kk) * kk + kk // 2                                     # the same input channel through the centre tap, where that one is off too
    if int(cols[centre]) == int(cols[col]):
        col = centre
    ic, t = col // kk, col % kk
    ty, tx = t // diff.shape[3], t % diff.shape[3]
    d = diff[:, ic, ty, tx]
    code = 0
    for j in range(nbits):
        if bool((d[torch.arange(diff.shape[0]) % nbits == j] != 0).any()):
            code |= 1 << j
    p = code - 1
    b, y, x = p // (H * W), (p % (H * W)) // W, p % W
    r = diff.shape[2] // 2
    ics = sorted({int(i) // 8 for i in bad.any(0).flatten(1).any(1).nonzero().flatten()})
    ocs = sorted({int(i) // 8 for i in bad.flatten(1).any(1).nonzero().flatten()})
    taps = sorted({(int(i) // diff.shape[3], int(i) % diff.shape[3]) for i in bad.any(0).any(0).flatten().nonzero().flatten()})
    return (f"{'lost' if int(d.sum()) < 0 else 'doubled'}: dy pixel index {p} = (b {b}, y {y}, x {x}) [the bits that the wrong output channels spell] times a pixel "
            f"(b {b}, y {y + ty - r}, x {x + tx - r}) through tap ({ty}, {tx}), "
            f"8-channel pieces: input {ics} output {ocs}, taps {taps}, largest |diff| {int(diff.abs().max())}")


def census_a(B, H, W, C):
    """Pass (b): a[b, y, x, ic] = bit ((ic / 2) mod nbits) of the column index (even ic) or of the row index (odd ic), dy == 1: every tap of every
    input channel counts ITS OWN shifted, reflected pixels.  Returns a fp32 0 / 1 [B, H, W, C]."""
    ic = torch.arange(C)
    bx, by = (ic // 2) % census_bits(W - 1), (ic // 2) % census_bits(H - 1)
    col = (torch.arange(W).view(1, 1, W, 1) >> bx.view(1, 1, 1, C)) & 1
    row = (torch.arange(H).view(1, H, 1, 1) >> by.view(1, 1, 1, C)) & 1
    return torch.where((ic % 2 == 0).view(1, 1, 1, C), col.expand(B, H, W, C), row.expand(B, H, W, C)).float()


def census_a_counts(a, k):
    """int64 [ic, k, k]: sum over pixels of a_pad[p + tap, ic] (the same for every output channel when dy == 1)."""
    B, H, W, C = a.shape
    dw, _, _, _ = wgrad_reference(torch.ones(B, H, W, 1), a, k)
    return dw[0].round().long()


def wgrad_plan(k, B, H, W, cu):
    """naf_launch_stem_wgrad / stem_wgrad2_launch (stem_wgrad.hip:552-599) restated for the 128-channel kernels: dict kernel ("simple" /
    "pipelined"), why (the simple kernel's condition), nseg, spb (segments per workgroup), nranges, cut (a range starts inside an image row),
    last (pixels of a row's last segment)."""
    nseg = -(-W // 32)
    why = "W<32" if W < 32 else ("Wmod32in1..3" if 1 <= W % 32 <= 3 else ("H<2" if H < 2 else None))
    plan = dict(kernel="simple" if why else "pipelined", why=why, nseg=nseg, last=W - 32 * (nseg - 1), B=B, H=H)
    if why is not None:
        rows = max(1, -(-H // max(1, cu // (k * B))))                      # the simple kernel: rows per workgroup, and whether the last band is cut short
        plan.update(rows=rows, partial=rows > 1 and H % rows != 0)
    if why is None:
        total = H * nseg
        blocks = max(1, cu // (k * B))
        spb = max(1, -(-total // blocks))
        nranges = -(-total // spb)
        plan.update(spb=spb, nranges=nranges, cut=any((r * spb) % nseg for r in range(1, nranges)))
    return plan


WGRAD_CLASSES = {
    "simple: W < 32": lambda p: p["why"] == "W<32",
    "simple: W mod 32 in 1..3": lambda p: p["why"] == "Wmod32in1..3",
    "simple: H < 2": lambda p: p["why"] == "H<2",
    "simple: several rows per workgroup, last band partial": lambda p: p["kernel"] == "simple" and p["partial"],
    "pipelined: one segment per workgroup": lambda p: p["kernel"] == "pipelined" and p["spb"] == 1,
    "pipelined: odd segments per workgroup": lambda p: p["kernel"] == "pipelined" and p["spb"] > 1 and p["spb"] % 2 == 1,
    "pipelined: even segments per workgroup": lambda p: p["kernel"] == "pipelined" and p["spb"] % 2 == 0,
    "pipelined: range cut inside a row": lambda p: p["kernel"] == "pipelined" and p["cut"] and p["nranges"] >= 3,
    "pipelined: last segment of 4 pixels": lambda p: p["kernel"] == "pipelined" and p["last"] == 4,
    "pipelined: last segment of 31 pixels": lambda p: p["kernel"] == "pipelined" and p["last"] == 31,
    "pipelined: H = 2": lambda p: p["kernel"] == "pipelined" and p["H"] == 2,
    "pipelined: batch 2": lambda p: p["kernel"] == "pipelined" and p["B"] == 2,
    "pipelined: batch 3": lambda p: p["kernel"] == "pipelined" and p["B"] == 3,
}
# (k, B, H, W) of the census at width 128: every class above on a 256-CU device (asserted from the device's own count by the GPU test);
# at most 19 200 pixels per sample
WGRAD_CENSUS_SHAPES = [(3, 1, 20, 24), (1, 2, 9, 33), (3, 1, 7, 67), (1, 1, 1, 64), (3, 3, 41, 24), (3, 2, 90, 35),
                       (3, 1, 2, 32), (1, 1, 2, 32), (3, 1, 40, 36), (1, 1, 40, 36), (3, 1, 64, 100), (3, 1, 50, 95), (1, 1, 50, 95),
                       (3, 2, 90, 95), (1, 2, 90, 95), (3, 3, 31, 64), (1, 3, 31, 64), (3, 1, 173, 77), (1, 1, 173, 77), (3, 1, 200, 96), (1, 1, 200, 96),
                       (1, 2, 60, 128), (3, 1, 120, 159)]


PIXEL_CAP = 30000


def wgrad_class_reachable(name, cu):
    """Whether ANY (k, B, H, W) below the pixel cap reaches the class on a device of ``cu`` CUs (a grid of widths around the segment boundaries, every
    height up to 300): tells a class the device cannot reach from a gap in WGRAD_CENSUS_SHAPES."""
    cond = WGRAD_CLASSES[name]
    for k in (1, 3):
        for B in (1, 2, 3):
            for W in (8, 24, 32, 33, 35, 36, 63, 64, 67, 95, 96, 100, 128, 159, 160, 191, 224):
                for H in range(1, 301):
                    if H * W <= PIXEL_CAP and cond(wgrad_plan(k, B, H, W, cu)):
                        return True
    return False


def wgradg_plan(k, B, H, C, cu):
    """naf_launch_stem_wgrad_generic (stem_generic_bwd.hip:196-205) restated: (rows per workgroup, number of bands)."""
    bands = max(1, (2 * cu) // (k * k * ((C + 127) // 128) * B))
    rows = max(1, -(-H // bands))
    return rows, -(-H // rows)


def profile_line(kernel, family, ratio, of_bound):
    return f"{kernel:<44s} {str(family):<28s} worst err/abs_sum {ratio:.3e}   worst err/bound {of_bound:.3f}"
