"""The forward conv stem on inputs for which every fp32 partial sum is exactly representable: the input constructions, their exact references, host
emulations with planted defects and restatements of the launchers' plans (tests/test_gpu_stem_forward.py on the device, tests/test_stem_forward_cpu.py
without one).  Plain helper module: no test in it.

Layout: activations are [B, H, W, C] (channels last, as the kernels store them), layer weights [oc, ic, k, k], images [B, 3, H, W], conv0 weights
[C, 3, k, k].  References are fp64; a case keeps them as fp32 once they are shown to survive ``.float().double()``.

Rounding points, read from the sources (naf_amd/csrc):

  GroupNorm vectors  stem_rows_kernel.h:134-145, stem_conv1x1.hip:185-197, stem_generic.hip:158-168 (and gn_vectors of stem_bwd.hip): the 16 copies of
              ``stats_in`` are added in fp64 (naf_gn_sums, naf_common.h:190-197), mean = s1 / n, var = max(s2 / n - mean^2, 0), rstd = (float)(1 /
              sqrt(var + (double)eps)), scale = gamma * rstd, shift = beta - (float)mean * gamma * rstd, all fp32.  The 128-wide kernels multiply both by
              (float)log2(e) (stem_rows_kernel.h:174-175, stem_conv1x1.hip:196-197); the general widths do not.
  activation  z = fmaf(x, scale, shift) (stem_rows_sched.inc, stem_rows_kernel.h:225, stem_generic.hip:195-196) or x * scale + shift on float pairs
              (stem_conv1x1.hip:338: the compiler may or may not contract it), then a = z * rcp(log2e + log2e * exp2(-z)) (128 wide) or
              z * rcp(1 + exp2(-z log2e)) (stem_generic.hip:25), ONE rounding to bf16 (rows :226, 1x1 :341, generic :195).
  convolution bf16 x bf16 products are exact in fp32; v_mfma_f32_16x16x32_bf16 / 32x32x16_bf16 accumulate them in fp32 in an order this file makes
              irrelevant; the bias is the accumulator's start (rows :284, 1x1 :280) or one addition at the end (generic :294); ONE bf16 store.
  GroupNorm sums of the output  from the fp32 results BEFORE the store: per lane, per wave, per workgroup in fp32 (rows :489-519, 1x1 :416-417 and
              :540-556, generic :296-311 and :43-52, conv0 :119-121 and :222-236), workgroups meet in fp64 atomics.
  first convolution  stem_conv0_kernel<KS> (stem_conv0.hip:160, :207) and stem_conv0_generic_kernel (stem_generic.hip:103) are fp32 chains;
              stem_conv0_split_kernel (stem_conv0.hip:293-304, :326-338) splits image and weights into three bf16 parts each and adds three (default)
              or six (NAF_CONV0_EXACT) part products in fp32, the bias being the accumulator's start (:375-377).  With y == NULL and k = 1
              conv0_moments_kernel (:485-528) adds the image's 9 first and second moments in fp64 and conv0_moment_sums_kernel (:530-557) forms
              sum y = W . S1 + N b and sum y^2 = W^T S2 W + 2 b W . S1 + N b^2 in fp64.

Why the constructions are exact.

  Chosen statistics.  A test passes totals s1 = n m, s2 = n (m^2 + 1 - eps) with eps = double(float32(1e-5)), quantised to 40 significant bits and
              spread over ALL 16 copies in the unequal dyadic shares SHARES / 64 (every partial sum of the copies has at most 46 bits: exact in any
              order).  Then mean == m, var + eps == 1 to 1e-9 and rstd == 1.0f (``gn_vectors32`` restates the statements in fp32; the CPU test checks
              all 16 means at every n).  With gamma and m both 0 or +-powers of two and beta = 0, scale and shift are exact (times fl(log2e): ONE common
              factor), so a pixel holding x = m gives fl(m c) - fl(m c) = 0 in both the fma and the mul+add form, and SiLU(0) = 0 * rcp(2 log2e) = 0.
  Alphabet.   A pixel holding x = m + v gives a = bf16(SiLU(v gamma)) computed with the kernels' fast exp2 / rcp.  z = v gamma is taken only from
              ALPHABET values whose fp64 SiLU lies at least 64 x act_forward(...)["da_"] (tests/stem_backward_reference.py: this project's derived
              fp32 error of the activation, which grows with |m| |gamma|) from a bf16 rounding boundary: the stored bf16 value is then known
              (``allowed_z``).  z = 2 and z = 6 have the smallest margins and are left out; large means leave fewer letters, z = 1 always remains.
  Any order.  A reference value is exact when it survives .float().double(), and exact IN ANY ORDER when abs-sum * 2^(-lsb exponent) < 2^24: all
              partial sums are then multiples of the lsb below 2^24 lsb, i.e. fp32 numbers (``any_order_exact``; the lsb exponents are measured from
              the operands by ``lsb_exponent``, never assumed).
  A binary    x = m + h, h in {0, 1}: a = A1 h with A1 = bf16(SiLU(1)) = 187/256; weights and bias multiples of 1/8: lsb 2^-11, abs-sum < 2^13.
  B low bit   layers: x multiples of 1/4 in [-2, 2), w of 1/8 (lsb 2^-5); conv0: image multiples of 1/8 in [-2, 2), weights of 1/64 (lsb 2^-9):
              image and weights are bf16 numbers, so the middle and low parts of the split are zero.
  C gamma     one hot (pixel, channel) per 3 x 3 neighbourhood (3x3) or per pixel (1x1), gamma_c in {+-0.5, +-1, +-2}: every output is A(z) times
              ONE weight, or A(z) times a sum of two to four mirrored taps at the border: 8 + 13 bits (per-element lsb = lsb(A(z)) 2^-9).
  C beta      gamma = 0: scale = 0, shift = fl(beta log2e) whatever the statistics, a = bf16(SiLU(beta_c)) at every pixel; a one-hot centre tap
              and a power-of-two bias: two terms.
  D census    w = 0, bias_c = g(c) + 1: y is the bias, S1 = (g + 1) n and S2 = (g + 1)^2 n are integers; the fp32 partial sums of a workgroup stay
              below 2^24 (``census_partial_max``), fp64 atomics add integers exactly.
  E split     one hot image pixel per 3 x 3 neighbourhood, none in row / column 1 or H - 2 / W - 2 (a mirrored tap would meet it twice and the sum
              of two 24-bit products is no fp32 number): every output is ONE product.  16 bits x 8 bits = x0 w0 + x1 w0 and 8 x 16 = x0 w0 + x0 w1
              are 24-bit numbers; 16 x 16 (NAF_CONV0_EXACT) is within fp32 roundings of x w, and the inputs are chosen so that no product lies within
              2^-21 relative of a bf16 boundary (eight times the 2^-24 the comparison needs).
  Moments     (k = 1, y == NULL) with the inputs of B every product and sum of the two kernels is a dyadic number of at most 48 bits: the sums
              equal the fp64 sums of the exact outputs EXACTLY (bound 0; ``moments_bits`` counts the bits).

No constant here is measured on the kernels under test.
"""
import functools
import math
import types

import torch
import torch.nn.functional as F

import input_statistics as S
import stem_backward_reference as R
from oracle import naf_oracle as O

F32 = S.F32
GROUPS = 8
SLOTS = 16                                              # NAF_STATS_SLOTS
EPS32 = 1e-5                                            # what the tests pass as eps (a float in the C ABI)
EPS = float(torch.tensor(EPS32, dtype=torch.float32).double())
LOG2E = 1.4426950408889634
A1 = 187.0 / 256.0                                      # bf16(SiLU(1))
MEANS = (0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 8.0, -8.0, 16.0, 0.125, -0.125)
# 0, +-0.25, +-0.5, +-1, +-2, +-4, +-8, 16 are fourteen values; +-0.125 fills 2 images x 8 groups without repeating one
ALPHABET = (1.0, 0.5, -0.5, -1.0, 1.5, -1.5, 3.0, -3.0, 0.25, 0.75, 4.0)
GAMMAS = (1.0, -0.5, 2.0, -1.0, 0.5, -2.0)
SHARES = (1, 7, 2, 6, 3, 5, 4, 4, 5, 3, 6, 2, 7, 1, 4, 4)   # 64ths of a total in the 16 copies
MARGIN_FACTOR = 64.0
DEFAULT_CU = 256                                        # MI355X; the device test passes the device's own count

# shapes (B, H, W) of the device test, per kernel
ROWS_SHAPES = [(1, 2, 2), (1, 5, 20), (1, 7, 48), (1, 22, 48), (2, 9, 33), (2, 64, 64)]
ROWS_KEYS_SHAPES = [(1, 32, 32), (1, 48, 64)]
ROWS_STRIDED_SHAPE = (1, 7, 48)
C1_DENSE_SHAPES = [(1, 4, 8), (1, 8, 20), (2, 16, 32)]
C1_SPARSE_SHAPES = [(1, 5, 9), (2, 9, 33)]
C1_CROP_SHAPE = (1, 8, 20)                              # a crop of a canvas with row stride (W + 3) C
C1_KEYS_SHAPES = [(1, 16, 32), (2, 32, 48)]
GEN_SHAPES = [(1, 2, 2), (2, 9, 33), (1, 10, 18)]
GEN_WIDTHS = [16, 48, 96, 144, 256]
CONV0_SHAPES = [(1, 2, 2), (2, 9, 33), (1, 37, 70)]
CONV0_VEC4_SHAPE = (2, 12, 40)                          # conv0_moments_kernel's four-pixel path: W % 4 == 0, contiguous rows
CONV0_GEN_WIDTHS = [48, 96, 256]
LATTICE_OFFSETS = [(0, 0), (1, 1), (2, 2)]


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def r16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def is_bf16(t):
    return bool((r16(t) == t.double()).all())


def silu64(z):
    z = torch.as_tensor(z, dtype=torch.float64)
    return z * torch.sigmoid(z)


# ---- exactness ------------------------------------------------------------------------------------------------------------------------
def lsb_exponent(t):
    """The exponent e of the lowest set bit over the non-zero elements of t: every element is a multiple of 2^e (0 for an all-zero tensor)."""
    t = t.double().flatten()
    t = t[t != 0]
    if t.numel() == 0:
        return 0
    for k in range(-8, 64):
        s = t * 2.0 ** k
        if bool((s == torch.round(s)).all()):
            return -k
    raise AssertionError("not a dyadic tensor of at most 64 fractional bits")


def lsb_exponent_map(t):
    """Per element: the exponent of its lowest set bit (0 where the element is zero)."""
    m, e = torch.frexp(t.double())
    k = torch.zeros_like(t, dtype=torch.int64)
    frac = m.abs()
    for _ in range(60):
        odd = frac != torch.floor(frac)
        if not bool(odd.any()):
            break
        frac = torch.where(odd, frac * 2.0, frac)
        k = k + odd.long()
    return torch.where(t == 0, torch.zeros_like(k), e.long() - k)


def fp32_exact(t):
    return bool((t.float().double() == t).all())


def any_order_exact(abs_sum, lsb):
    """abs-sum * 2^-lsb < 2^24 at every element (``lsb``: an exponent, or a tensor of exponents): every partial sum, in any order, is a multiple of
    2^lsb below 2^24 * 2^lsb and therefore an fp32 number."""
    scale = torch.exp2(-torch.as_tensor(lsb, dtype=torch.float64))
    return bool((abs_sum.double() * scale < 2.0 ** 24).all())


def bf16_margin(v):
    """Distance of the fp64 values v from the nearest bf16 ROUNDING boundary (a midpoint between neighbouring bf16 numbers); inf at 0."""
    v = torch.as_tensor(v, dtype=torch.float64).abs()
    e = torch.floor(torch.log2(torch.where(v > 0, v, torch.ones_like(v))))
    ulp = torch.exp2(e - 7.0)
    frac = v / ulp - torch.floor(v / ulp)
    return torch.where(v > 0, (frac - 0.5).abs() * ulp, torch.full_like(v, float("inf")))


def da_bound(m, gamma, z):
    """act_forward(...)["da_"] (stem_backward_reference.py:99-112) of a pixel x = m + z / gamma under the chosen statistics (mean m, rstd 1, beta 0)."""
    x = m + z / gamma
    zabs = (abs(x) + abs(m)) * abs(gamma)
    a = float(silu64(z))
    return F32 * (4.4 * zabs + (2.0 * abs(z) + 6.0) * abs(a)) + R.TINY


@functools.lru_cache(maxsize=None)
def allowed_z(m, gamma):
    """The letters of ALPHABET usable at mean m and GroupNorm weight gamma: x = m + z / gamma is a bf16 number and SiLU(z) keeps MARGIN_FACTOR x
    da_ from every bf16 rounding boundary."""
    out = []
    for z in ALPHABET:
        x = torch.tensor(m + z / gamma, dtype=torch.float64)
        if is_bf16(x) and float(bf16_margin(silu64(z))) >= MARGIN_FACTOR * da_bound(m, gamma, z):
            out.append(z)
    return tuple(out)


def act_value(z):
    """A(z) = bf16(SiLU(z)) as fp64."""
    return r16(silu64(z))


# ---- statistics -------------------------------------------------------------------------------------------------------------------------
def quantise40(t):
    m, e = torch.frexp(t.double())
    return torch.ldexp(torch.round(torch.ldexp(m, torch.tensor(40))), e - 40)


def spread_totals(total):
    """[B, 8, 2] totals -> the [16, B, 8, 2] buffer the kernels read: the totals quantised to 40 significant bits, SHARES[i] / 64 of them in copy i.
    Returns (buffer, quantised totals); the copies add up to the quantised totals exactly, front to back and back to front."""
    q = quantise40(total)
    sh = torch.tensor(SHARES, dtype=torch.float64).view(SLOTS, 1, 1, 1) / 64.0
    buf = (q.unsqueeze(0) * sh).contiguous()
    fwd = torch.zeros_like(q)
    bwd = torch.zeros_like(q)
    for i in range(SLOTS):
        fwd = fwd + buf[i]
        bwd = bwd + buf[SLOTS - 1 - i]
    assert bool((fwd == q).all()) and bool((bwd == q).all()), "the 16 copies do not add up exactly"
    return buf, q


def chosen_totals(means, n):
    """means [B, 8] -> totals [B, 8, 2] with s1 = n m, s2 = n (m^2 + 1 - eps)."""
    m = means.double()
    return torch.stack([n * m, n * (m * m + 1.0 - EPS)], dim=-1)


def means_for(B, seed):
    assert B * GROUPS <= len(MEANS)
    p = torch.randperm(len(MEANS), generator=torch.Generator().manual_seed(1000 + seed))
    return torch.tensor(MEANS, dtype=torch.float64)[p][:B * GROUPS].view(B, GROUPS)


def per_channel(v, C):
    """[B, 8] -> [B, 1, 1, C]."""
    return v.repeat_interleave(C // GROUPS, dim=1).view(v.shape[0], 1, 1, C)


def gn_vectors32(stats16, H, W, C, gamma, beta, log2e, eps=EPS32):
    """The kernels' scale / shift statements in fp32 (see the module docstring): returns (scale, shift, rstd) as fp32 [B, C]."""
    acc = torch.zeros_like(stats16[0])
    for sl in range(SLOTS):                                   # naf_gn_sums: copy by copy, fp64
        acc = acc + stats16[sl]
    n = float(H) * float(W) * float(C // GROUPS)
    mean = acc[..., 0] / n
    var = (acc[..., 1] / n - mean * mean).clamp_min(0.0)
    eps64 = float(torch.tensor(eps, dtype=torch.float32).double())
    rstd = (1.0 / torch.sqrt(var + eps64)).float()
    ex = lambda v: v.repeat_interleave(C // GROUPS, dim=1)
    rstd, mean32 = ex(rstd), ex(mean.float())
    gm, bt = gamma.float().view(1, C), beta.float().view(1, C)
    scale = gm * rstd
    shift = bt - mean32 * gm * rstd
    if log2e:
        k = torch.tensor(LOG2E, dtype=torch.float32)
        scale, shift = scale * k, shift * k
    return scale, shift, rstd


def act_emulated(x, scale, shift, log2e, fma=True):
    """bf16(SiLU(z)) as fp32 [B, H, W, C] from the kernels' statements in fp32: z by one fused multiply-add (fma=True: the product is exact in
    fp64, one rounding) or by a rounded product and a rounded sum; the exponential and the reciprocal are torch's fp32 ones (the hardware's
    differ in the last bits, which the alphabet's margin absorbs).  Also returns z."""
    B, C = scale.shape
    sc, sh = scale.view(B, 1, 1, C), shift.view(B, 1, 1, C)
    if fma:
        z = (x.double() * sc.double() + sh.double()).float()
    else:
        z = x.float() * sc + sh
    k = torch.tensor(LOG2E, dtype=torch.float32)
    if log2e:
        a = z * torch.reciprocal(torch.exp2(-z) * k + k)
    else:
        a = z * torch.reciprocal(1.0 + torch.exp2(z * -k))
    return bf16r(a), z


# ---- convolutions -----------------------------------------------------------------------------------------------------------------------
def conv_nhwc64(a, w, bias):
    """fp64 reflect convolution of a [B, H, W, C] with w [oc, ic, k, k] (+ bias) -> [B, H, W, oc]."""
    return S.conv_reflect64(a.permute(0, 3, 1, 2), w, bias).permute(0, 2, 3, 1).contiguous()


def conv_nhwc32(a, w, bias):
    """The same in fp32 (the emulations: where the reference is exact in any order this is the same number)."""
    x = a.float().permute(0, 3, 1, 2)
    pad = w.shape[-1] // 2
    if pad:
        x = F.pad(x, (pad,) * 4, mode="reflect")
    return F.conv2d(x, w.float(), None if bias is None else bias.float()).permute(0, 2, 3, 1).contiguous()


def reflect_index(i, n):
    i = i.abs()
    i = torch.where(i >= n, 2 * n - 2 - i, i)
    return i.clamp(0, n - 1)


def tap_term(a, w, ty, tx, shift=0):
    """One tap's contribution to the reflect convolution, fp64 [B, H, W, oc]; ``shift``: the tap reads the pixel that many columns to the right
    of its own (clamped to the image)."""
    B, H, W, C = a.shape
    r = w.shape[-1] // 2
    ys = reflect_index(torch.arange(H) + ty - r, H)
    xs = reflect_index(torch.arange(W) + tx - r, W)
    if shift:
        xs = (xs + shift).clamp(0, W - 1)
    src = a.double()[:, ys][:, :, xs]
    return torch.einsum("bhwi,oi->bhwo", src, w[:, :, ty, tx].double())


def group_sums(y):
    """fp64 [B, 8, 2] sums and sums of squares of y [B, H, W, C], with the sums of |y| for the bound."""
    t = R.group_totals(y)
    B, C = y.shape[0], y.shape[-1]
    ab = y.double().abs().reshape(B, -1, GROUPS, C // GROUPS).sum((1, 3))
    return t, ab


def sums_bound(sums_ref, sum_abs, n):
    """|S1 - ref| <= n 2^-24 sum |y|, |S2 - ref| <= (n + 1) 2^-24 sum y^2: an n-term fp32 sum in any order (stem_backward_reference.py), the
    squares rounded once more."""
    return torch.stack([n * F32 * sum_abs, (n + 1) * F32 * sums_ref[..., 1]], dim=-1)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def _case(**kw):
    return types.SimpleNamespace(**kw)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


def _finish(c, ref, abs_sum, lsb):
    """Record exactness, the GroupNorm sums of the exact outputs and keep the reference as fp32."""
    c.exact_fp32 = fp32_exact(ref)
    c.any_order = any_order_exact(abs_sum, lsb)
    c.abs_sum_max = float(abs_sum.max())
    c.lsb = lsb if isinstance(lsb, int) else int(lsb.min())
    c.sums_ref, c.sum_abs = group_sums(ref)
    c.n = ref.shape[1] * ref.shape[2] * (ref.shape[3] // GROUPS)
    c.ref = ref.float() if c.exact_fp32 else ref
    return c


def _cached(fn):
    """lru_cache for the small cases; the large shapes (several trips per wave) are rebuilt, not kept."""
    small = functools.lru_cache(maxsize=None)(fn)

    @functools.wraps(fn)
    def wrapper(*args):
        B, H, W = args[0], args[1], args[2]
        return small(*args) if B * H * W <= 20000 else fn(*args)
    return wrapper


def pattern_weight(C, k):
    """The weights of test_plain_impulses_return_every_weight_exactly for any width: a function of (tap, oc, ic) with eight significant bits."""
    oc = torch.arange(C).view(C, 1, 1, 1)
    ic = torch.arange(C).view(1, C, 1, 1)
    tap = torch.arange(k * k).view(1, 1, k, k)
    w = (1.0 + ((oc * 5 + ic * 3 + tap * 7) % 128).double() / 128.0) * torch.exp2(((oc + 2 * ic + tap) % 4 - 2).double())
    w = torch.where((oc + ic + tap) % 2 == 0, w, -w)
    assert is_bf16(w)
    return w


def random_x(B, H, W, C, seed):
    return bf16r(O.hash_normal((B, H, W, C), seed) * 1.5 + 0.3)


def random_affine(C, seed):
    return 1.0 + O.hash_normal((C,), seed, 0.1), O.hash_normal((C,), seed + 1, 0.1)


@_cached
def binary_dense(B, H, W, C, k, seed=0):
    """Construction A."""
    g = _gen(1, B, H, W, C, k, seed)
    means = means_for(B, seed + B + H + W + C + k)
    h = torch.randint(0, 2, (B, H, W, C), generator=g).double()
    x = per_channel(means, C) + h
    w = torch.randint(-8, 8, (C, C, k, k), generator=g).double() / 8.0
    bias = torch.randint(-8, 9, (C,), generator=g).double() / 8.0
    a = A1 * h
    n = H * W * (C // GROUPS)
    stats16, totals = spread_totals(chosen_totals(means, n))
    c = _case(kind="A", B=B, H=H, W=W, C=C, k=k, x=x.float(), x_is_bf16=is_bf16(x), means=means, gamma=torch.ones(C), beta=torch.zeros(C),
              stats16=stats16, totals=totals, w=w.float(), bias=bias.float(), hot=h.bool(), zhot=torch.ones(()), chosen=True)
    ref, ab = conv_nhwc64(a, w, bias), conv_nhwc64(a.abs(), w.abs(), bias.abs())
    return _finish(c, ref, ab, min(lsb_exponent(a) + lsb_exponent(w), lsb_exponent(bias)))


@_cached
def lowbit_dense(B, H, W, C, k, seed=0):
    """Construction B for the PLAIN layers."""
    g = _gen(2, B, H, W, C, k, seed)
    x = torch.randint(-8, 8, (B, H, W, C), generator=g).double() / 4.0
    w = torch.randint(-8, 8, (C, C, k, k), generator=g).double() / 8.0
    bias = torch.randint(-8, 9, (C,), generator=g).double() / 8.0
    c = _case(kind="B", B=B, H=H, W=W, C=C, k=k, x=x.float(), x_is_bf16=is_bf16(x), w=w.float(), bias=bias.float())
    ref, ab = conv_nhwc64(x, w, bias), conv_nhwc64(x.abs(), w.abs(), bias.abs())
    return _finish(c, ref, ab, min(lsb_exponent(x) + lsb_exponent(w), lsb_exponent(bias)))


def gamma_pattern(C):
    c = torch.arange(C)
    return torch.tensor(GAMMAS, dtype=torch.float64)[(3 * (c // 8) + (c % 8) // 4) % 6]


def hot_channel_1x1(B, H, W, C):
    """c(p) of the 1x1 gamma impulses: with p the pixel's index in its image, every (p mod 32, channel) pair occurs once there are C groups."""
    p = torch.arange(H * W).view(1, H, W)
    b = torch.arange(B).view(B, 1, 1)
    return (p // 32 + 5 * (p % 32) + 11 * b) % C


@_cached
def gamma_impulses(B, H, W, C, k, offset=0, seed=0):
    """Construction C, gamma impulses.  The reference is a gather: every output pixel sees at most ONE hot (pixel, channel) -- through one tap, or
    through two to four mirrored taps of the same hot pixel at the border."""
    means = means_for(B, seed + B + H + W + C + k)
    gamma = gamma_pattern(C)
    mc = per_channel(means, C)                                             # [B, 1, 1, C]
    yy, xx = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    bb = torch.arange(B).view(B, 1, 1)
    if k == 3:
        oy, ox = LATTICE_OFFSETS[offset]
        hot_px = ((yy % 3 == oy) & (xx % 3 == ox)).expand(B, H, W)
        hc = ((yy // 3) * (-(-W // 3)) + xx // 3 + 37 * bb + 5 * offset) % C
    else:
        hot_px = torch.ones((B, H, W), dtype=torch.bool)
        hc = hot_channel_1x1(B, H, W, C)
    hc = hc.expand(B, H, W)
    # the letter of every hot pixel: from the letters its (mean, gamma) allows, by the pixel's index
    m_hot = torch.gather(mc.expand(B, H, W, C), 3, hc.unsqueeze(-1)).squeeze(-1)
    g_hot = gamma[hc]
    z_hot = torch.zeros((B, H, W), dtype=torch.float64)
    counter = (yy * W + xx + 3 * bb).expand(B, H, W)
    for m in set(means.flatten().tolist()):
        for gm in GAMMAS:
            sel = hot_px & (m_hot == m) & (g_hot == gm)
            if bool(sel.any()):
                letters = torch.tensor(allowed_z(m, gm), dtype=torch.float64)
                assert letters.numel() > 0, f"no letter of the alphabet is usable at mean {m}, gamma {gm}"
                z_hot[sel] = letters[counter[sel] % letters.numel()]
    v_hot = torch.where(hot_px, z_hot / g_hot, torch.zeros_like(z_hot))
    x = mc.expand(B, H, W, C).clone()
    x.scatter_add_(3, hc.unsqueeze(-1), v_hot.unsqueeze(-1))
    a_hot = torch.where(hot_px, act_value(z_hot), torch.zeros_like(z_hot))   # [B, H, W]: the one non-zero activation of the pixel
    w = pattern_weight(C, k)
    n = H * W * (C // GROUPS)
    stats16, totals = spread_totals(chosen_totals(means, n))
    hot = torch.zeros((B, H, W, C), dtype=torch.bool)
    hot.scatter_(3, hc.unsqueeze(-1), hot_px.unsqueeze(-1))
    c = _case(kind="Cg", B=B, H=H, W=W, C=C, k=k, x=x.float(), x_is_bf16=is_bf16(x), means=means, gamma=gamma.float(), beta=torch.zeros(C),
              stats16=stats16, totals=totals, w=w.float(), bias=torch.zeros(C), hot=hot, zhot=z_hot, hot_px=hot_px, hot_channel=hc, a_hot=a_hot,
              chosen=True)
    ref = torch.zeros((B, H, W, C), dtype=torch.float64)
    ab = torch.zeros((B, H, W, C), dtype=torch.float64)
    lsb_a = torch.zeros((B, H, W), dtype=torch.int64)
    r = k // 2
    for ty in range(k):
        for tx in range(k):
            ys, xs = reflect_index(torch.arange(H) + ty - r, H), reflect_index(torch.arange(W) + tx - r, W)
            src_a = a_hot[:, ys][:, :, xs]
            src_c = hc[:, ys][:, :, xs]
            term = w[:, :, ty, tx].t()[src_c] * src_a.unsqueeze(-1)      # [B, H, W, oc]
            ref += term
            ab += term.abs()
            lsb_a = torch.minimum(lsb_a, lsb_exponent_map(src_a))
    lsb = (lsb_a + lsb_exponent(w)).unsqueeze(-1).expand(B, H, W, C)
    return _finish(c, ref, ab, lsb)


@_cached
def beta_field(B, H, W, C, k, seed=0):
    """Construction C, beta constant field."""
    x = random_x(B, H, W, C, 300 + seed)
    letters = torch.tensor(ALPHABET, dtype=torch.float64)
    beta = letters[(torch.arange(C) * 7 + 3) % len(ALPHABET)]
    perm = (torch.arange(C) * 5 + 3) % C
    assert len(set(perm.tolist())) == C
    w = torch.zeros((C, C, k, k), dtype=torch.float64)
    w[torch.arange(C), perm, k // 2, k // 2] = 1.0
    bias = torch.exp2((torch.arange(C) % 4 - 2).double()) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    stats16, totals = spread_totals(R.group_totals(x))
    a = act_value(beta)                                                     # [C]
    ref = (a[perm] + bias).view(1, 1, 1, C).expand(B, H, W, C).contiguous()
    ab = (a[perm].abs() + bias.abs()).view(1, 1, 1, C).expand(B, H, W, C)
    c = _case(kind="Cb", B=B, H=H, W=W, C=C, k=k, x=x, x_is_bf16=True, gamma=torch.zeros(C), beta=beta.float(), stats16=stats16, totals=totals,
              w=w.float(), bias=bias.float(), perm=perm, chosen=False)
    return _finish(c, ref, ab, min(lsb_exponent(a), lsb_exponent(bias)))


def census_bias(C):
    return (torch.arange(C) // (C // GROUPS) + 1).double()


@_cached
def census(B, H, W, C, k, seed=0):
    """Construction D for a layer."""
    x = random_x(B, H, W, C, 400 + seed)
    gamma, beta = random_affine(C, 410 + seed)
    stats16, totals = spread_totals(R.group_totals(x))
    bias = census_bias(C)
    ref = bias.view(1, 1, 1, C).expand(B, H, W, C).contiguous()
    c = _case(kind="D", B=B, H=H, W=W, C=C, k=k, x=x, x_is_bf16=True, gamma=gamma, beta=beta, stats16=stats16, totals=totals,
              w=torch.zeros((C, C, k, k)), bias=bias.float(), chosen=False)
    return _finish(c, ref, ref.abs(), 0)


def census_sums(B, H, W, C, twice_row=None):
    """[B, 8, 2] of construction D: (g + 1) n and (g + 1)^2 n -- with image row ``twice_row`` counted twice when given (the planted defect)."""
    rows = H + (1 if twice_row is not None else 0)
    n = rows * W * (C // GROUPS)
    g = torch.arange(1, GROUPS + 1, dtype=torch.float64).view(1, GROUPS).expand(B, GROUPS)
    return torch.stack([g * n, g * g * n], dim=-1)


# ---- first convolution ------------------------------------------------------------------------------------------------------------------
@_cached
def conv0_lowbit(B, H, W, C, k, seed=0):
    """Construction B for conv0: image [B, 3, H, W], weight [C, 3, k, k], reference [B, H, W, C]."""
    g = _gen(5, B, H, W, C, k, seed)
    img = torch.randint(-16, 16, (B, 3, H, W), generator=g).double() / 8.0
    w = torch.randint(-64, 64, (C, 3, k, k), generator=g).double() / 64.0
    bias = torch.randint(-8, 9, (C,), generator=g).double() / 8.0
    ref = S.conv_reflect64(img, w, bias).permute(0, 2, 3, 1).contiguous()
    ab = S.conv_reflect64(img.abs(), w.abs(), bias.abs()).permute(0, 2, 3, 1)
    c = _case(kind="B0", B=B, H=H, W=W, C=C, k=k, img=img.float(), w=w.float(), bias=bias.float(), img_is_bf16=is_bf16(img), w_is_bf16=is_bf16(w))
    return _finish(c, ref, ab, min(lsb_exponent(img) + lsb_exponent(w), lsb_exponent(bias)))


@_cached
def conv0_census(B, H, W, C, k, seed=0):
    img = O.hash_normal((B, 3, H, W), 500 + seed)
    bias = census_bias(C)
    ref = bias.view(1, 1, 1, C).expand(B, H, W, C).contiguous()
    c = _case(kind="D0", B=B, H=H, W=W, C=C, k=k, img=img, w=torch.zeros((C, 3, k, k)), bias=bias.float())
    return _finish(c, ref, ref.abs(), 0)


def moments_bits(c):
    """Bits the fp64 sums of conv0_moment_sums_kernel need on the inputs of ``c`` (construction B): magnitude over lsb of its largest term."""
    npx = c.H * c.W
    lsb = 2 * lsb_exponent(c.w) + 2 * lsb_exponent(c.img)          # w_i w_j sum x_i x_j
    mag = npx * (3.0 * float(c.w.abs().max()) * float(c.img.abs().max()) + float(c.bias.abs().max())) ** 2
    return math.ceil(math.log2(mag)) - lsb


def moments_vec4(img):
    """The four-pixel path's condition (stem_conv0.hip:582-583) on a torch image."""
    s = img.stride()
    return s[3] == 1 and img.shape[3] % 4 == 0 and all(v % 4 == 0 for v in s[:3]) and img.data_ptr() % (4 * img.element_size()) == 0


def split3(t):
    """The three bf16 parts of fp32 numbers as the split kernel forms them (stem_conv0.hip:296-299, :330-333), fp64."""
    t = t.float()
    t0 = bf16r(t)
    r1 = t - t0
    t1 = bf16r(r1)
    t2 = bf16r(r1 - t1)
    return t0.double(), t1.double(), t2.double()


SPLIT_TERMS = {3: ((0, 1), (1, 0), (0, 0)), 6: ((0, 2), (1, 1), (0, 1), (2, 0), (1, 0), (0, 0))}   # (image part, weight part), smallest first


def sig_value(j, bits):
    """A number in [1, 2) with exactly ``bits`` significant bits (the last one set), chosen by j."""
    half = 2 ** (bits - 2)
    return 1.0 + (2 * (j % half) + 1) / float(2 ** (bits - 1))


@_cached
def conv0_impulses(B, H, W, xbits, wbits, offset=0):
    """Construction E (k = 3, width 128, bias 0): hot image pixels on the 3-pixel lattice, none in row / column 1 or H - 2 / W - 2, each in one image
    channel; values of ``xbits`` significant bits against weights of ``wbits``.  With 16 x 16 bits the hot values are chosen so that no product
    lies within 2^-21 relative of a bf16 rounding boundary."""
    C = 128
    oy, ox = LATTICE_OFFSETS[offset]
    oc = torch.arange(C).view(C, 1, 1, 1)
    ic = torch.arange(3).view(1, 3, 1, 1)
    tap = torch.arange(9).view(1, 1, 3, 3)
    j = (oc * 5 + ic * 3 + tap * 7)
    if wbits == 8:
        mant = 1.0 + (j % 128).double() / 128.0
    else:
        mant = 1.0 + (2 * ((j * 977 + 131) % 16384) + 1).double() / 32768.0
    w = mant * torch.exp2(((oc + 2 * ic + tap) % 4 - 2).double())
    w = torch.where((oc + ic + tap) % 2 == 0, w, -w)
    img = torch.zeros((B, 3, H, W), dtype=torch.float64)
    count = 0
    for b in range(B):
        for y in range(oy, H, 3):
            if y == 1 or y == H - 2:
                continue
            for x in range(ox, W, 3):
                if x == 1 or x == W - 2:
                    continue
                ch = (y // 3 + x // 3 + b) % 3
                jj = 7 * count + 3 * b + 1
                while True:
                    v = sig_value(jj, xbits) * 2.0 ** ((y + x) % 3 - 1) * (-1.0 if (y + 2 * x) % 2 else 1.0)
                    if not (xbits == 16 and wbits == 16):
                        break
                    prod = v * w[:, ch]                                    # every product this pixel makes
                    if bool((bf16_margin(prod) >= 2.0 ** -21 * prod.abs()).all()):
                        break
                    jj += 1
                img[b, ch, y, x] = v
                count += 1
    ref = S.conv_reflect64(img, w, None).permute(0, 2, 3, 1).contiguous()
    ab = S.conv_reflect64(img.abs(), w.abs(), None).permute(0, 2, 3, 1)
    terms = S.conv_reflect64((img != 0).double(), torch.ones_like(w), None).permute(0, 2, 3, 1)
    c = _case(kind="E", B=B, H=H, W=W, C=C, k=3, img=img.float(), w=w.float(), bias=torch.zeros(C), img_fp32=fp32_exact(img), w_fp32=fp32_exact(w),
              nhot=count, max_terms=int(terms.max()), margin=float((bf16_margin(ref) / ref.abs().clamp_min(1e-300))[ref != 0].min()) if count else float("inf"))
    c.product_fp32 = fp32_exact(ref)
    c.sums_ref, c.sum_abs = group_sums(ref)
    c.n = H * W * (C // GROUPS)
    c.ref = ref                                                             # fp64: a 16 x 16 product has 32 bits
    return c


def conv0_split_emulated(img, w, terms, drop_middle=False):
    """stem_conv0_split_kernel on the host: the part products of SPLIT_TERMS[terms] added smallest first in fp32, one bf16 store (bias 0).
    ``drop_middle``: the planted defect -- the image's middle part is lost."""
    xp, wp = list(split3(img)), list(split3(w))
    if drop_middle:
        xp[1] = torch.zeros_like(xp[1])
    acc = None
    for xi, wi in SPLIT_TERMS[terms]:
        t = S.conv_reflect64(xp[xi], wp[wi], None).permute(0, 2, 3, 1).float()
        acc = t if acc is None else acc + t
    return bf16r(acc)


# ---- the layer on the host, with planted defects ----------------------------------------------------------------------------------------
DEFECTS = ("tap_shift", "clamp_right", "seam_row", "chunk_swap", "means_swap", "gamma_swap", "pipeline_reuse")


def layer_emulated(c, log2e, fma=True, defect=None, seam=None):
    """One GroupNorm -> SiLU -> conv layer in fp32 / bf16 from the case's inputs as the kernels compute it (``log2e``: the 128-wide kernels' form),
    optionally with one planted defect.  Returns the bf16 output as fp32 [B, H, W, C]."""
    B, H, W, C, k = c.B, c.H, c.W, c.C, c.k
    stats16, gamma, w, x = c.stats16, c.gamma, c.w, c.x
    if defect == "means_swap":                                   # groups 2 and 3 of image 0 take each other's statistics
        stats16 = stats16.clone()
        stats16[:, 0, 2], stats16[:, 0, 3] = c.stats16[:, 0, 3], c.stats16[:, 0, 2]
    if defect == "gamma_swap":                                   # two adjacent 8-channel chunks take each other's GroupNorm weights
        gamma = gamma.clone()
        gamma[0:8], gamma[8:16] = c.gamma[8:16], c.gamma[0:8]
    if defect == "chunk_swap":                                   # two 8-channel chunks of one k-step (centre tap) change places
        w = w.clone()
        t = k // 2
        w[:, 0:8, t, t], w[:, 8:16, t, t] = c.w[:, 8:16, t, t], c.w[:, 0:8, t, t]
    if defect == "pipeline_reuse":                               # the third 32-pixel group of a wave reads the first one's pixels
        x = x.clone().view(B, H * W, C)
        x[:, 8 * 32:9 * 32] = x[:, 0:32]
        x = x.view(B, H, W, C)
    scale, shift, _ = gn_vectors32(stats16, H, W, C, gamma, c.beta, log2e)
    a, _ = act_emulated(x, scale, shift, log2e, fma)
    if defect == "clamp_right":                                  # the right border repeats column W - 1 instead of mirroring W - 2
        assert k == 3
        ap = F.pad(a.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect")
        ap[..., W + 1] = ap[..., W]
        y = F.conv2d(ap, w.float(), c.bias.float()).permute(0, 2, 3, 1)
    else:
        y = conv_nhwc32(a, w, c.bias)
    if defect == "tap_shift":                                    # one tap reads the pixel to the right of its own
        ty, tx = (k // 2, 0) if k == 3 else (0, 0)
        y = (y.double() - tap_term(a, w, ty, tx) + tap_term(a, w, ty, tx, shift=1)).float()
    if defect == "seam_row":                                     # the first row of a segment takes its upper halo row from the row itself
        assert k == 3 and seam is not None and 1 <= seam < H
        a2 = a.clone()
        a2[:, seam - 1] = a[:, seam]
        y = y.clone()
        y[:, seam] = conv_nhwc32(a2, w, c.bias)[:, seam]
    return bf16r(y.float())


def plain_emulated(c):
    return bf16r(conv_nhwc32(c.x, c.w, c.bias))


def layer_torch64(c):
    """The real operation in torch fp64 -- conv2d(reflect pad(silu(GroupNorm(x)))) with the activation unrounded -- and the existing single-layer
    bound (input_statistics.layer_reference, bf16_bound(1, .)): (ref, bound, act_forward's dict) as [B, H, W, C].  GroupNorm normalises with the
    totals the case passes to the kernel (stem_backward_reference.act_forward); where those are the tensor's own, ``group_norm_agrees`` ties
    that restatement to F.group_norm."""
    f = R.act_forward(c.x, c.gamma, c.beta, EPS, c.totals)
    ref = conv_nhwc64(f["a"], c.w.double(), c.bias.double())
    ab = conv_nhwc64(f["a"].abs(), c.w.double().abs(), None)
    return ref, S.bf16_bound(1, ab, ref.abs()), f


def group_norm_agrees(c):
    """max |silu(F.group_norm(x)) - act_forward(x, real totals)| in fp64 (a case with real statistics)."""
    f = R.act_forward(c.x, c.gamma, c.beta, EPS, c.totals)
    t = F.silu(F.group_norm(c.x.double().permute(0, 3, 1, 2), GROUPS, c.gamma.double(), c.beta.double(), EPS)).permute(0, 2, 3, 1)
    return float((t - f["a"]).abs().max())


def first_mismatch(got, want, what):
    """None, or the failure message of an exact comparison: first differing (b, y, x, oc) and the count.  ``!=`` so that -0 equals +0 (and a NaN differs)."""
    bad = got != want
    if not bool(bad.any()):
        return None
    i = tuple(int(v) for v in bad.nonzero()[0])
    return (f"{what}: {int(bad.sum())} of {bad.numel()} values differ, first at (b, y, x, oc) = {i}: got {float(got[i])!r}, expected {float(want[i])!r}")


# ---- the launchers' plans, restated -----------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def conv3_plan(B, H, W, keys, cu):
    """naf_stem_conv3_plan and the grid of naf_launch_stem_conv (stem_conv.hip:20-39, :60-62; the XCD remap: stem_rows_kernel.h:114)."""
    tiles_x = _cdiv(W, 32)
    strips = B * tiles_x
    segs = max(1, cu // strips)
    segs = max(1, min(segs, (H + 7) // 8))
    seg_h = _cdiv(_cdiv(H, segs), 4) * 4
    if keys:
        seg_h = min(_cdiv(seg_h, 16) * 16, 128)
    segs_y = _cdiv(H, seg_h)
    grid = strips * segs_y
    return dict(tiles_x=tiles_x, seg_h=seg_h, segs_y=segs_y, grid=grid, xcd_remap=grid % 8 == 0, edge_strip=W % 32 != 0,
                last_rows=H - (segs_y - 1) * seg_h)


def conv1x1_plan(B, H, W, cu, dense_rows=True, keys=False):
    """groups_per_block and the grid of naf_launch_stem_conv1x1 (stem_conv1x1.hip:577-591, :609-611, :644-645): trips = 32-pixel groups (keys: cells)
    every wave of a workgroup walks, as (min, max) over the waves that have work."""
    gpi = _cdiv(H * W, 32)
    slots = cu * 2 * 4
    if keys:
        ncell = (H // 16) * (W // 16)
        per_wave = _cdiv(ncell * B, slots)
        per_block, items = per_wave * 4, ncell
    else:
        per_wave = _cdiv(gpi * B, slots)
        per_block, items = per_wave * 4, gpi
    nbx = max(1, _cdiv(items, per_block))
    trips = []
    for bx in range(nbx):
        end = min(items, (bx + 1) * per_block)
        for wv in range(4):
            g0 = bx * per_block + wv
            if g0 < end:
                trips.append(_cdiv(end - g0, 4))
    return dict(groups=gpi, gpw=per_wave, groups_per_block=per_block, blocks=nbx, dense=dense_rows and (H * W) % 32 == 0,
                partial_last=(H * W) % 32 != 0, trips=(min(trips), max(trips)))


def conv0_plan(k, B, H, W, cu):
    """naf_launch_stem_conv0 (stem_conv0.hip:565-566, :599-604 for the fp32 kernel, :609-613 for the split kernel): segments per wave."""
    gpr = _cdiv(W, 32)
    ng = H * gpr
    if k == 1:
        slots = cu * 2 * 4
        gpw = _cdiv(ng * B, slots)
        nbx = max(1, min(_cdiv(ng, gpw * 4), _cdiv(ng, 4)))
        stride = nbx * 4
        trips = [_cdiv(ng - g0, stride) for g0 in range(min(stride, ng))]
        return dict(kernel="stem_conv0_kernel", ng=ng, gpw=gpw, blocks=nbx, trips=(min(trips), max(trips)))
    slots8 = cu * 12
    gpw8 = _cdiv(ng * B, slots8)
    gpb = gpw8 * 12
    nb8 = max(1, _cdiv(ng, gpb))
    trips = []
    for bx in range(nb8):
        end = min(ng, (bx + 1) * gpb)
        trips += [_cdiv(end - (bx * gpb + wv), 12) for wv in range(12) if bx * gpb + wv < end]
    return dict(kernel="stem_conv0_split_kernel", ng=ng, gpw=gpw8, groups_per_block=gpb, blocks=nb8, trips=(min(trips), max(trips)))


def conv1x1_trips_shape(cu):
    """(1, 256, W*): the smallest W for which every wave of the dense 1x1 kernel walks exactly three groups."""
    for W in range(1, 1 << 16):
        p = conv1x1_plan(1, 256, W, cu)
        if p["gpw"] == 3 and p["trips"] == (3, 3):
            return (1, 256, W)
    raise AssertionError("no width gives three groups per wave")


def conv0_trips_shape(k, cu):
    """(1, H*, 1000): a partial last segment per row and three segments per wave of the conv0 kernel for ksize k (every wave, if some height
    allows it; else at least the longest walk)."""
    fallback = None
    for H in range(2, 1 << 14):
        p = conv0_plan(k, 1, H, 1000, cu)
        if p["gpw"] == 3 and p["trips"] == (3, 3):
            return (1, H, 1000)
        if fallback is None and p["gpw"] == 3 and p["trips"][1] == 3:
            fallback = (1, H, 1000)
        if p["gpw"] > 3 and fallback is not None:
            return fallback
    raise AssertionError("no height gives three segments per wave")


def census_partial_max(kernel, B, H, W, C, cu, k=3):
    """The largest fp32 partial sum of squares a workgroup of ``kernel`` holds in construction D before its fp64 atomics: pixels x channels of a
    group x 64."""
    cpg = C // GROUPS
    if kernel == "rows":
        px = conv3_plan(B, H, W, False, cu)["seg_h"] * 32
    elif kernel == "1x1":
        px = conv1x1_plan(B, H, W, cu)["groups_per_block"] * 32
    elif kernel == "generic":
        px = 8 * 16
    elif kernel == "conv0":
        p = conv0_plan(k, B, H, W, cu)
        px = p["trips"][1] * (4 if k == 1 else 12) * 32
    else:
        raise KeyError(kernel)
    return px * cpg * GROUPS * GROUPS


def generic_seams(H):
    """First rows of the second and later 8-row tiles of stem_convg_kernel."""
    return list(range(8, H, 8))


def rows_seams(B, H, W, cu):
    p = conv3_plan(B, H, W, False, cu)
    return [s * p["seg_h"] for s in range(1, p["segs_y"])]


# ---- the (kernel, construction, shape) pairs of the device test -----------------------------------------------------------------------------
BUILDERS = {"A": binary_dense, "Cb": beta_field, "D": census, "Cg": gamma_impulses, "B": lowbit_dense}


def build_layer(con, shape, C, k, off=0):
    B, H, W = shape
    return gamma_impulses(B, H, W, C, k, off) if con == "Cg" else BUILDERS[con](B, H, W, C, k)


def _layer_cases():
    out = []
    offs = lambda k: range(3) if k == 3 else range(1)
    for s in ROWS_SHAPES:
        out += [("rows", con, s, 128, 3, 0) for con in ("A", "Cb", "D")] + [("rows", "Cg", s, 128, 3, o) for o in range(3)]
    for s in C1_DENSE_SHAPES + C1_SPARSE_SHAPES:
        out += [("1x1", con, s, 128, 1, 0) for con in ("A", "Cg", "Cb", "D")]
    for C in GEN_WIDTHS:
        for k in (1, 3):
            for s in GEN_SHAPES:
                out += [("generic", con, s, C, k, 0) for con in ("A", "Cb", "D")] + [("generic", "Cg", s, C, k, o) for o in offs(k)]
    return out


LAYER_CASES = _layer_cases()                                   # (kernel, construction, (B, H, W), C, k, lattice offset)
KEYS_CASES = [("rows", s, 3) for s in ROWS_KEYS_SHAPES] + [("1x1", s, 1) for s in C1_KEYS_SHAPES]          # construction A, y only
PLAIN_CASES = ([("1x1", s, 128, 1) for s in C1_DENSE_SHAPES + C1_SPARSE_SHAPES] +
               [("generic", s, C, k) for C in GEN_WIDTHS for k in (1, 3) for s in GEN_SHAPES])           # construction B
TRIPS_CONS = ("Cg", "Cb", "D")                                 # at (1, 256, W*): references that need no convolution
CONV0_WIDTHS = [128] + CONV0_GEN_WIDTHS
CONV0_CASES = [(C, k, s) for C in CONV0_WIDTHS for k in (1, 3) for s in CONV0_SHAPES]                    # constructions B and D
E_SHAPES = [(1, 7, 20), (2, 9, 33)]
E_BITS = [(16, 8), (8, 16), (16, 16)]


def case_id(c):
    return "-".join("x".join(str(v) for v in p) if isinstance(p, tuple) else str(p) for p in c)
