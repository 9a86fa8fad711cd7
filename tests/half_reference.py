"""float16 features through the attention forward: value families, bound and host emulations (tests/test_half_features_cpu.py without
a device, tests/test_gpu_half_features.py on one).  Plain helper module: no test in it.

The contract (include/naf_hip.h, naf_dtype_supported): float16 values are read as half and never rounded to bf16, P is multiplied by 2^8
and rounded to half, the product runs on the f16 matrix instruction with fp32 accumulation, the accumulator is multiplied by 2^-8 and
stored as half.  Queries, keys and the scores are what they are for every other dtype (input_statistics.py).

The bound, per element, in input_statistics' convention with U16 = 2^-11 (half has 11 significand bits) and SLACK = 1.25:

    half_bound = 1.25 * 2^-11 * (abs_sum + |ref|)  +  k*k * 2^-22 * max|v|  +  2^-14

  term 1  one rounding of every weight P to half (relative 2^-11 each: 2^-11 * sum_j P_j |v_j|) plus the half store of the result;
  term 2  every window weight flushed: 2^8 P below 2^-14 may count as zero whatever the hardware does with subnormal operands, i.e. a
          weight below 2^-22, k*k of them at most, each on a value of at most max|v|;
  term 3  values below 2^-14 (subnormal halves) flushed: the weights sum to 1, so at most 2^-14 -- which also covers a result that is
          itself a subnormal half (spacing 2^-24).
The generic kernel keeps P in fp32: its P term is input_statistics.fp32_score_factor * abs_sum, as forward_bound has it.
"""
import os
import sys

import numpy as np
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402

U16 = 2.0 ** -11       # unit roundoff of float16
PSCALE = 2.0 ** 8      # XnaVal::PSCALE (naf_amd/csrc/naf_common.h)
TINY = 2.0 ** -14      # smallest normal half


def f16r(x):
    return x.to(torch.float16).to(torch.float32)


def make_half_values(shape, family, seed):
    """input_statistics.make_values with ``.half()`` in place of the bf16 rounding: fp16-representable fp32 [B, C, h, w] with 11-bit
    significands.  The largest magnitudes, "big" (3.47 * 2^10 = 3.6e3) and "outlier" (208), are far inside half's 65504."""
    B, C, h, w = shape
    x = O.hash_normal(shape, seed)
    if family == "unit":
        pass
    elif family == "chan_offset":
        x = x + 8.0 * O.hash_normal((1, C, 1, 1), seed + 7001)
    elif family == "outlier":
        x = torch.where(S.outlier_mask(h, w).view(1, 1, h, w), x * 60.0, x)
    elif family == "small":
        x = x * 2.0 ** -10
    elif family == "big":
        x = x * 2.0 ** 10
    elif family == "smooth":
        x = S._smooth(shape, seed)
    else:
        raise ValueError(family)
    assert float(x.abs().max()) < 65504.0
    return f16r(x)


def half_inputs(case, fam):
    """(q, k, v) of a FWD_CASES entry: input_statistics.forward_inputs' queries and keys, half values of the same family and seed."""
    _, _, _, heads, Dq, lr, out_sz, ksz, C, _ = case
    seed = 1000 + 7 * ksz + out_sz[1]
    q, k = S.make_qk((1, heads * Dq, *out_sz), (1, heads * Dq, *lr), fam[1], seed, heads)
    return q, k, make_half_values((1, C, *lr), fam[0], seed + 2)


def half_bound(case, q, k, v, ref, a):
    """The module docstring's bound for a FWD_CASES entry; ``ref``, ``a`` from input_statistics.attention_reference on the half values."""
    _, path, _, heads, _, _, _, ksz, _, _ = case
    kk = ksz * ksz
    p_term = S.fp32_score_factor(q, k, heads, ksz) * a if path == "generic" else S.SLACK * U16 * a
    return p_term + S.SLACK * U16 * ref.abs() + kk * 2.0 ** -22 * float(v.abs().max()) + TINY


def _r_half(x):
    return x.to(torch.float16).to(torch.float64)


def _flush(x):
    """Worst case for an operand of the f16 matrix instruction: everything below the smallest normal half counts as zero."""
    return torch.where(x.abs() < TINY, torch.zeros_like(x), x)


def attention_half_emulated(q, k, v, ksz, heads, route, p_fp32=False, rows_per_chunk=8):
    """The fp64 oracle with the rounding points of one of the two routes a float16 caller can be served by, result rounded to half:
      "native"  P * 2^8 rounded to half, every operand below 2^-14 flushed (P' and the values alike), the sum times 2^-8;
      "bf16"    what the library did before: values through fp32 to bf16, P rounded to bf16, an fp32 map cast to half.
    ``p_fp32``: the generic kernel, whose weights stay fp32 scalars on either route (no rounding of P, nothing to flush)."""
    iy, ix = S._tables(q, k, ksz)
    qh, kh, vh = S._heads(q, heads), S._heads(k, heads), S._heads(v, heads)
    vh = S._r16(vh) if route != "native" else (vh if p_fp32 else _flush(vh))
    scale = qh.shape[-1] ** -0.5
    B, n, Ho, Wo, _ = qh.shape
    out = torch.empty(B, n, Ho, Wo, vh.shape[-1], dtype=torch.float64)
    iyt, ixt = torch.from_numpy(np.ascontiguousarray(iy)), torch.from_numpy(np.ascontiguousarray(ix))
    for r0 in range(0, Ho, rows_per_chunk):
        yy = iyt[r0:r0 + rows_per_chunk]
        kg, vg = S._gather(kh, yy, ixt), S._gather(vh, yy, ixt)
        s = torch.einsum("bnrwd,bnrwkd->bnrwk", qh[:, :, r0:r0 + rows_per_chunk], kg) * scale
        e = torch.exp(s - s.amax(dim=-1, keepdim=True))
        p = e / e.sum(dim=-1, keepdim=True)
        if p_fp32:
            o = torch.einsum("bnrwk,bnrwkd->bnrwd", p, vg)
        elif route == "native":
            o = torch.einsum("bnrwk,bnrwkd->bnrwd", _flush(_r_half(p * PSCALE)), vg) / PSCALE
        else:
            o = torch.einsum("bnrwk,bnrwkd->bnrwd", S._r16(p), vg)
        if route != "native":
            o = o.float().double()          # the fp32 map
        out[:, :, r0:r0 + rows_per_chunk] = o
    return _r_half(out.permute(0, 1, 4, 2, 3).reshape(B, -1, Ho, Wo))


# ---- exact gather (the lane-map check): one-hot attention on integer values ----------------------------------------------------
def gather_inputs(heads, Dq, lr, out_sz, ksz, C):
    """(q, k, v, want) for a forward whose every query attends to exactly one cell of its own window, chosen per query.
    Keys are 16 e_code(cell) with code = (cy % 8) * 8 + cx % 8 -- distinct inside any window up to 7 x 7 -- on the first 64 head dims;
    a query is 16 e_code(target), so with Dq = 64 the matching score is 256 / sqrt(64) = 32 and every other 0: the other weights are
    e^-32 = 1.3e-14, zero as halves even after the 2^8 prescale, and the target's weight rounds to 1.  (Wider heads: 256 / sqrt(Dq), still
    above 18.)  Values are the asymmetric integers (37 cell + 5 channel) mod 2048, exact in half (11 bits), not in bf16 above 256.
    ``want`` [1, C, Ho, Wo]: the value rows of the targets.  All fp32 NCHW; q / k are bf16-exact."""
    assert ksz <= 7 and Dq >= 64
    h, w = lr
    Ho, Wo = out_sz
    iy, ix = O.axis_index_table(Ho, h, ksz), O.axis_index_table(Wo, w, ksz)
    yy, xx = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    ty = iy[yy, (3 * yy + 5 * xx) % ksz]                                    # [Ho, Wo]: a tap of the query's own window, varying per query
    tx = ix[xx, (2 * yy + 3 * xx + 1) % ksz]
    assert int((iy[:, -1] - iy[:, 0]).max()) < 8 and int((ix[:, -1] - ix[:, 0]).max()) < 8      # a window spans < 8 cells: distinct codes
    code = lambda cy, cx: (cy % 8) * 8 + cx % 8
    k = torch.zeros(1, heads, Dq, h, w)
    cyg, cxg = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    k[0, :, torch.from_numpy(code(cyg, cxg)), torch.from_numpy(cyg), torch.from_numpy(cxg)] = 16.0
    q = torch.zeros(1, heads, Dq, Ho, Wo)
    q[0, :, torch.from_numpy(code(ty, tx)), torch.from_numpy(yy + 0 * xx), torch.from_numpy(xx + 0 * yy)] = 16.0
    cell = torch.arange(h * w).view(1, 1, h, w)
    v = ((37 * cell + 5 * torch.arange(C).view(1, C, 1, 1)) % 2048).float()
    want = v[0][:, torch.from_numpy(ty), torch.from_numpy(tx)].unsqueeze(0)
    return q.reshape(1, heads * Dq, Ho, Wo), k.reshape(1, heads * Dq, h, w), v, want
