"""The yardstick of the regression-objective tests (``naf(..., regress=t)``, ``ops.xna_mse_forward``, naf_xna_mse_fwd): the objective of
the reference's training step (train.py:127-132, ``loss = mse(pred.float(), hr_feats.float())``) restated in fp64 on the oracle's
attention, and the bounds the kernel's results are held to.  Three parts.

1. ``reference``: out = the oracle's attention in fp64 (tests/input_statistics.attention_reference), e = out - t,
   loss = sum e^2 / N, dout = (2 / N) e with N = B * C * Ho * Wo.  tests/test_regress_cpu.py holds it against fp64 autograd of F.mse_loss.

2. ``output_bound``: the per-element bound delta on the error of the kernel's IMPLIED output (the fp32 accumulator the target is
   subtracted from).  It is the ``union`` row of the table in tests/test_gpu_input_statistics.py,
       delta = 1.25 * (n * 2^-8 * sum_j P_j |v_j|),   n = 1 (pf = (bf16_t)(s * inv), xna_union_kernel.h),
   WITHOUT a store term: nothing is rounded between the accumulator and the subtraction.

3. The bounds that follow from delta, with no measured constant:
       |dout - ref| <= (2 / N) delta + 2^-8 |ref|                       one bf16 store of (acc - t) * (2 / N)
       |loss - ref| <= (1 / N) sum (2 |e| delta + delta^2) + L * 2^-24 * ref
   (acc = out + d with |d| <= delta gives (e + d)^2 - e^2 = 2 e d + d^2.)  L is the length of the longest chain of fp32 operations
   between an exact square and the stored loss, read from the code: a lane adds, with one fmaf each (xna_union_kernel.h, ``objective``),
   the squares of four channels of every channel tile of every 16-pixel tile its wave owns --
   ceil(ry * (seg / 16) / NW) tiles of dvt / 16 channel tiles (``chain_length``; ry, seg, dvt from naf_xna_union_plan, NW from
   ``union_mse_waves`` = xna_union_mse_waves_rt) -- then six butterfly additions (the wave's sum); the subtraction acc - t rounds once and
   enters the square twice (2); the fp64 sum of the per-wave partials is rounded to fp32 once (1).  The partials are added in fp64.

The exact case (``exact_case``): where every normalised softmax weight is a power of two, the bf16 rounding of P changes nothing (n = 0)
and what is left of delta is the fp32 accumulation, ``output_bound(abs_sum, n=0, fp32_terms=K)`` = K * 2^-24 * abs_sum for a K-slot
window.  It exists for one purpose: a prediction that is rounded to bf16 BEFORE the subtraction (what the composed step does, and what
the fused kernel exists to avoid) errs by at most 2^-9 |out|, and with round-to-nearest the rounding of P by at most 2^-9 abs_sum, so
their sum stays below delta = 1.25 * 2^-8 * abs_sum on EVERY input: the n = 1 bounds cannot see that defect.  The exact case can.

This module is a helper (no tests in it); the cases the GPU tests run are defined here so that the CPU tests can use them too.
"""
import math
import os
import sys

import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402

DQ = 64     # head dim of the table-driven MFMA kernel

# name -> (B, heads, Dv, (h, w), (Ho, Wo), window, target kind, slots per window row (WT), channel chunks: 1 or "many")
#   target kinds: "f32_nchw" plain fp32 NCHW; "bf16_cl" a bf16 ``b (h w) c -> b c h w`` view (channel stride 1: vector loads);
#   "f32_slice" fp32 NCHW channels [8, 8 + C) of a tensor with C + 24 channels (scalar loads, batch stride of the wider tensor);
#   "bf16_cl_slice" channels [4, 4 + C) of a channels-last bf16 tensor with C + 8 channels (8-byte aligned: vector loads)
CASES = {
    "a_train_small": (2, 4, 16, (8, 8), (16, 16), 3, "f32_nchw", 16, 1),          # the training geometry in small; full tiles
    "b_f4_k3": (2, 4, 16, (5, 7), (23, 30), 3, "bf16_cl", 16, 1),                # golden F4's geometry: multiplicities, a 14-pixel partial tile,
    "b_f4_k5": (2, 4, 16, (5, 7), (23, 30), 5, "bf16_cl", 16, 1),                # a partial row block
    "c_ratio1": (1, 2, 32, (20, 20), (20, 20), 5, "f32_nchw", 32, 1),             # ratio 1; WT = 32
    "d_chunks": (1, 1, 512, (4, 4), (8, 8), 3, "bf16_cl", 16, "many"),            # Dv 512 > 256: nchunk >= 2
    "e_k9": (1, 2, 32, (17, 20), (17, 20), 9, "f32_slice", 32, 1),                # WT = 32, window 9: the 8-wave instantiation
    "e_k15": (1, 2, 32, (17, 20), (17, 20), 15, "bf16_cl_slice", 32, 1),          # WT = 32, window 15: the 4-wave instantiation
    "f_k15_w16": (1, 1, 16, (15, 15), (125, 122), 15, "f32_nchw", 16, 1),         # window 15 with WT = 16 (ratio ~8, the smallest NATTEN allows):
                                                                                  # the one instantiation with 8 waves where the plain kernel has 12
}


def union_mse_waves(ks, wt):
    """xna_union_mse_waves_rt (naf_amd/csrc/xna_union_mse_kernel.h)."""
    return (8 if ks >= 15 else 12) if wt == 16 else (4 if ks >= 13 else 8)


def chain_length(ry, seg, dvt, nw):
    """L of the loss bound (module docstring): fmaf chain of a lane + 6 butterfly additions + 2 (acc - t, squared) + 1 (the fp32 store)."""
    return math.ceil(ry * (seg // 16) / nw) * (dvt // 16) * 4 + 6 + 2 + 1


def make_inputs(case, seed=4100):
    """q [B, heads*64, Ho, Wo], k [B, heads*64, h, w], v [B, C, h, w], t [B, C, Ho, Wo]: fp32 tensors holding bf16 values (t: fp32
    values for the fp32 target kinds).  The target is the fp64 prediction plus unit noise times 0.5: errors of the size a training step sees."""
    B, heads, Dv, (h, w), (Ho, Wo), ks, kind = CASES[case][:7]
    C = heads * Dv
    q = S.bf16r(O.hash_normal((B, heads * DQ, Ho, Wo), seed + 1))
    k = S.bf16r(O.hash_normal((B, heads * DQ, h, w), seed + 2))
    v = S.bf16r(O.hash_normal((B, C, h, w), seed + 3))
    out, _ = S.attention_reference(q, k, v, ks, heads)
    t = out.float() + 0.5 * O.hash_normal((B, C, Ho, Wo), seed + 4)
    if kind.startswith("bf16"):
        t = S.bf16r(t)
    return q, k, v, t


def target_view(t, kind, device="cpu"):
    """The target tensor of a case as the kernel gets it: logical [B, C, Ho, Wo] with the strides of ``kind``."""
    B, C, Ho, Wo = t.shape
    if kind == "f32_nchw":
        return t.float().contiguous().to(device)
    if kind == "bf16_cl":
        return t.to(torch.bfloat16).permute(0, 2, 3, 1).reshape(B, Ho * Wo, C).contiguous().to(device).view(B, Ho, Wo, C).permute(0, 3, 1, 2)
    if kind == "f32_slice":
        wide = torch.full((B, C + 24, Ho, Wo), float("nan"), dtype=torch.float32)
        wide[:, 8:8 + C] = t.float()
        return wide.to(device)[:, 8:8 + C]
    if kind == "bf16_cl_slice":
        wide = torch.full((B, Ho, Wo, C + 8), float("nan"), dtype=torch.bfloat16)
        wide[..., 4:4 + C] = t.to(torch.bfloat16).permute(0, 2, 3, 1)
        return wide.to(device)[..., 4:4 + C].permute(0, 3, 1, 2)
    raise ValueError(kind)


def reference(q, k, v, t, ks, heads):
    """fp64: dict(out, abs_sum, e, loss, dout, N) of the objective on the oracle's attention."""
    out, abs_sum = S.attention_reference(q, k, v, ks, heads)
    e = out - t.double()
    N = e.numel()
    return {"out": out, "abs_sum": abs_sum, "e": e, "loss": float((e * e).sum() / N), "dout": e * (2.0 / N), "N": N}


def output_bound(abs_sum, n=1, fp32_terms=0):
    """delta: S.bf16_bound(n, abs_sum) -- the union row, no store term -- plus ``fp32_terms`` * 2^-24 * abs_sum (the exact case only)."""
    return S.bf16_bound(n, abs_sum) + fp32_terms * 2.0 ** -24 * abs_sum


def dout_bound(ref_dout, delta, N):
    return (2.0 / N) * delta + S.U * ref_dout.abs()


def loss_bound(e, delta, N, L, ref_loss):
    return float((2.0 * e.abs() * delta + delta * delta).sum() / N) + L * 2.0 ** -24 * ref_loss


def emulate_kernel(q, k, v, t, ks, heads, *, drop_last_pixel=False, n_without_batch=False, transpose_target=False, round_prediction=False):
    """The kernel's arithmetic on the host: P rounded to bf16 after normalisation, fp32 accumulator, e = acc - t and e * (2 / N) in fp32,
    one bf16 store, squares summed in fp32.  Returns (loss fp32 as float, dout as fp64 [B, C, Ho, Wo]).  The keywords plant one defect each:
    the last pixel of every output row neither stored nor summed (a partial tile masked one lane too early); N = C * Ho * Wo; the
    target read with y and x swapped (square outputs only); the prediction rounded to bf16 before the subtraction."""
    acc = S.attention_emulated(q, k, v, ks, heads, round_p="normalised").float()
    if round_prediction:
        acc = acc.to(torch.bfloat16).float()
    tt = t.float()
    if transpose_target:
        tt = tt.transpose(2, 3)
    e = acc - tt
    N = e.numel() // (e.shape[0] if n_without_batch else 1)
    dout = (e * torch.tensor(2.0 / N, dtype=torch.float32)).to(torch.bfloat16)
    sq = e * e
    if drop_last_pixel:
        dout[..., -1] = 0
        sq = sq[..., :-1]
    loss = (sq.sum(dtype=torch.float32).double() / N).float()
    return float(loss), dout.double()


def exact_case(seed=4200):
    """Ratio 1, window 3, one head: keys that are 64 * ones in the low-res rows y % 3 != 2 of the columns x % 3 == 0 and zero elsewhere,
    queries of ones.  A 3 x 3 window of consecutive rows / columns (NATTEN clamps it at the borders, it never shrinks) holds exactly two
    such keys; their scores exceed the others by 64 * 64 / 8 = 512, so the softmax weights are 1/2, 1/2 and zeros, exactly, in fp32 and
    in bf16.  Values and target as in ``make_inputs``.  -> (q, k, v, t, ks, heads)."""
    B, heads, Dv, n, ks = 1, 1, 16, 12, 3
    q = torch.ones(B, DQ, n, n)
    k = torch.zeros(B, DQ, n, n)
    for y in range(n):
        for x in range(0, n, 3):
            if y % 3 != 2:
                k[:, :, y, x] = 64.0
    v = S.bf16r(O.hash_normal((B, Dv, n, n), seed + 3))
    out, _ = S.attention_reference(q, k, v, ks, heads)
    t = out.float() + 0.5 * O.hash_normal((B, Dv, n, n), seed + 4)
    return q, k, v, t, ks, heads
