"""fp64 restatement of the regression epilogue of the head-summed attention kernel (naf_xna_head_reg_fwd, include/naf_hip.h), from GIVEN
logits: the loss map, its gradient with respect to the logits and the ten error sums of depth evaluation.  Plain helper module (no test
in it), written from the header's definitions with torch's elementwise fp64 arithmetic and nothing of naf_amd.ops, so that the kernel
and the library's torch composition are both held to it.  tests/test_head_regression_cpu.py and tests/test_gpu_head_regression.py use it.

Also here: the inputs of the statistics tests (``stats_target``, ``STATS_CLAMP``) and the condition on them that the tests assert before they
look at a device result (``bracket_widths``)."""
import math

import torch

from oracle import naf_oracle as O

KINDS = ("l1", "mse", "smooth_l1")
NSTAT = 10
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
STATS_CLAMP = (0.5, 2.0)         # with a bias of 1 the head's logits (a sum over heads of unit-variance values) fall below, between and above these


def f32(v):
    """A Python float rounded to float32: what a float field of the C struct holds."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def terms(r, kind, beta):
    """(l(r), l'(r)) elementwise, fp64."""
    if kind == "l1":
        return r.abs(), torch.sign(r)
    if kind == "mse":
        return r * r, 2.0 * r
    assert kind == "smooth_l1"
    a = r.abs()
    small = a < beta
    return torch.where(small, 0.5 * r * r / beta, a - 0.5 * beta), torch.where(small, r / beta, torch.sign(r))


def restate(logits, target, valid, kind, beta=1.0):
    """logits, target [B, N, Ho, Wo], valid [B, Ho, Wo] bool or None -> (loss map [B, Ho, Wo], sum of |terms| per pixel [B, Ho, Wo],
    g [B, Ho, Wo, N]), all fp64; invalid pixels are 0 in all three whatever lies under them."""
    z, t = logits.double(), target.double()
    ok = torch.ones(z.shape[0], *z.shape[2:], dtype=torch.bool, device=z.device) if valid is None else valid.bool()
    r = torch.where(ok.unsqueeze(1), z - t, torch.zeros_like(z))
    l, g = terms(r, kind, float(beta))
    return l.sum(1), l.abs().sum(1), g.permute(0, 2, 3, 1)


def counted(pred, target, valid):
    z, t = pred.double(), target.double()
    c = (t > 0) & torch.isfinite(t) & torch.isfinite(z)
    return c if valid is None else (c & valid.bool())


def error_sums(pred, target, valid, clamp, scale=1.0):
    """pred, target [B, Ho, Wo] -> (sums fp64 [10], sums of |term| fp64 [10], S1 = sum(|ln p| + |ln t|), S2 = sum((|ln p| + |ln t|)^2)).
    ``scale`` multiplies the three thresholds (the tests' brackets)."""
    lo, hi = f32(clamp[0]), f32(clamp[1])
    c = counted(pred, target, valid)
    one = torch.ones_like(pred, dtype=torch.float64)
    p = torch.where(c, pred.double().clamp(lo, hi), one)
    t = torch.where(c, target.double(), one)
    e, lp, lt = p - t, torch.log(p), torch.log(t)
    d = lp - lt
    ratio = torch.maximum(p / t, t / p)
    cf = c.double()
    vals = [cf, e.abs(), e * e, e.abs() / t, e * e / t, d, d * d] + [(ratio < th * scale).double() for th in THRESHOLDS]
    sums = torch.stack([(v * cf).sum() for v in vals])
    mags = torch.stack([(v.abs() * cf).sum() for v in vals])
    S = (lp.abs() + lt.abs()) * cf
    return sums, mags, S.sum(), (S * S).sum()


def bracket_widths(pred, target, valid, clamp):
    """For each threshold: (count at 1.25^k (1 - 2^-20), count at 1.25^k (1 + 2^-20)), and the number of counted pixels."""
    lo = error_sums(pred, target, valid, clamp, 1.0 - 2.0 ** -20)[0]
    hi = error_sums(pred, target, valid, clamp, 1.0 + 2.0 ** -20)[0]
    return [(float(lo[7 + i]), float(hi[7 + i])) for i in range(3)], float(lo[0])


def metrics(sums):
    """The depth figures from the ten sums, in Python floats (nan for n = 0)."""
    n = float(sums[0])
    if n == 0:
        return dict.fromkeys(("mae", "rmse", "abs_rel", "sq_rel", "rmse_log", "silog", "d1", "d2", "d3"), math.nan) | {"n": 0.0}
    s = [float(x) / n for x in sums[1:]]
    return dict(mae=s[0], rmse=math.sqrt(s[1]), abs_rel=s[2], sq_rel=s[3], rmse_log=math.sqrt(s[5]), silog=math.sqrt(max(s[5] - s[4] * s[4], 0.0)),
                d1=s[6], d2=s[7], d3=s[8], n=n)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def dense_target(B, N, Ho, Wo, seed, channels_last=False):
    """A finite fp32 target [B, N, Ho, Wo]; ``channels_last``: the same values as a view of [B, Ho, Wo, N] memory."""
    t = O.hash_normal((B, N, Ho, Wo), seed) * 1.5
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if channels_last else t


def make_valid(B, Ho, Wo, mode, seed=7):
    """Mask modes: "none" (no mask), "tenth" (about a tenth of the pixels invalid, from a hash of the pixel index), "row" (image row 5
    invalid as well), "all" (every pixel invalid)."""
    if mode == "none":
        return None
    idx = torch.arange(B * Ho * Wo, dtype=torch.int64)
    hsh = (idx * 2654435761 + 12345 + seed) & 0xFFFFFFFF
    v = (((hsh >> 3) % 10) != 0).view(B, Ho, Wo)
    if mode == "row":
        v[:, 5] = False
    if mode == "all":
        v[:] = False
    return v


def stats_target(B, Ho, Wo, seed):
    """Depth-like targets [B, 1, Ho, Wo]: exp(0.6 * normal) (positive, around 1) on most pixels; a few that must not be counted -- 0,
    negative, +inf, NaN -- at pixels chosen by a hash of the index (about 1 in 16 in all)."""
    t = torch.exp(0.6 * O.hash_normal((B, 1, Ho, Wo), seed))
    idx = torch.arange(B * Ho * Wo, dtype=torch.int64)
    hsh = ((idx * 2246822519 + 374761393) & 0xFFFFFFFF) >> 5
    flat = t.view(-1)
    flat[(hsh % 64) == 0] = 0.0
    flat[(hsh % 64) == 1] = -1.5
    flat[(hsh % 64) == 2] = math.inf
    flat[(hsh % 64) == 3] = math.nan
    return t
