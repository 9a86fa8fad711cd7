"""Reference, cases and points of the point-query tests (tests/test_points_cpu.py without a device, tests/test_gpu_points.py on one).
Plain helper module: no test in it.

``point_query`` restates one query pixel of the oracle's attention (O.xna_tables) as a gather in fp64: for a point (b, y, x) the keys and
values of the rows idx_y[y] and the columns idx_x[x] (the oracle's own axis_index_table, duplicates included), per head the scaled
scores, their softmax and the weighted sum of the values -- and ``sum_j P_j |v_j|``, the abs-sum the bounds of tests/input_statistics.py
are stated in.  A point outside [0, B) x [0, Ho) x [0, Wo) gets NaN rows.

The geometries are the smallest at which the index arithmetic can go wrong:
  a  heads 2, Dq 64,  6 x 8  -> 24 x 32, window 5,  C = 48 (Dv = 24: not a multiple of 16)
  b  heads 4, Dq 64,  5 x 7  -> 23 x 30, window 3,  no values (golden F4's non-integer ratio: the tables repeat entries)
  c  heads 1, Dq 96, 16 x 18 -> 16 x 18, window 15, C = 3 (ratio 1; the denoising call's head)
"""
import functools

import numpy as np
import torch

import input_statistics as S
from oracle import naf_oracle as O

CASES = {
    "a": dict(heads=2, Dq=64, lr=(6, 8), out=(24, 32), ksz=5, C=48),
    "b": dict(heads=4, Dq=64, lr=(5, 7), out=(23, 30), ksz=3, C=None),
    "c": dict(heads=1, Dq=96, lr=(16, 18), out=(16, 18), ksz=15, C=3),
}


@functools.lru_cache(maxsize=None)
def inputs(name, B=1, half=False):
    """(q [B, Cq, Ho, Wo], k [B, Cq, h, w], v [B, C, h, w] or None): fp32 holding bf16 (v: half with ``half``) values; the images differ.
    Shared by the tests: never modified."""
    c = CASES[name]
    seed = 4100 + 17 * c["ksz"] + c["out"][1]
    Cq = c["heads"] * c["Dq"]
    q, k = S.make_qk((B, Cq, *c["out"]), (B, Cq, *c["lr"]), "unit", seed, c["heads"])
    v = None
    if c["C"] is not None:
        v = O.hash_normal((B, c["C"], *c["lr"]), seed + 2) + 8.0 * O.hash_normal((1, c["C"], 1, 1), seed + 3)     # per-channel offsets
        v = v.to(torch.float16).float() if half else S.bf16r(v)
    return q, k, v


def make_points(B, Ho, Wo, N):
    """int64 [N, 3] of (b, y, x): the four corners, every border band (rows / columns 1 and 2 from each edge: inside half a window of
    every case), interior pixels; images interleaved from the last to the first (unsorted), duplicates included, cycled to N."""
    yx = [(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1),
          (1, Wo // 2), (2, 1), (Ho - 2, Wo // 3), (Ho - 3, Wo - 2), (Ho // 2, 1), (Ho // 3, 2), (Ho // 2 + 1, Wo - 2), (2, Wo - 3),
          (Ho // 2, Wo // 2), (Ho // 3, Wo // 4), (Ho // 2 - 1, Wo // 2 + 3), (Ho - 5, 5), (Ho // 2, Wo // 2)]
    pts = [((B - 1 - i) % B, y, x) for i, (y, x) in enumerate(yx)]
    if B > 1:
        pts += [(b, y, x) for (y, x) in yx[:6] for b in range(B)]      # the same pixels in every image
    pts = [pts[i % len(pts)] for i in range(N)]
    return torch.tensor(pts, dtype=torch.int64).view(N, 3)


def point_query(q, k, v, points, ksz, heads):
    """fp64 (logits [N, heads, kk], probs [N, heads, kk], out [N, C] or None, abs_sum [N, C] or None, window_y [N, ky], window_x [N, kx])."""
    ky, kx = (ksz, ksz) if isinstance(ksz, int) else ksz
    B, Cq, Ho, Wo = q.shape
    h, w = k.shape[-2:]
    Dq = Cq // heads
    iy = torch.from_numpy(np.ascontiguousarray(O.axis_index_table(Ho, h, ky))).long()
    ix = torch.from_numpy(np.ascontiguousarray(O.axis_index_table(Wo, w, kx))).long()
    N = points.shape[0]
    nan = float("nan")
    logits = torch.full((N, heads, ky * kx), nan, dtype=torch.float64)
    probs = torch.full((N, heads, ky * kx), nan, dtype=torch.float64)
    C = v.shape[1] if v is not None else 0
    out = torch.full((N, C), nan, dtype=torch.float64) if v is not None else None
    abs_sum = torch.full((N, C), nan, dtype=torch.float64) if v is not None else None
    win_y = torch.full((N, ky), -1, dtype=torch.int64)
    win_x = torch.full((N, kx), -1, dtype=torch.int64)
    for n, (b, y, x) in enumerate(points.tolist()):
        if not (0 <= b < B and 0 <= y < Ho and 0 <= x < Wo):
            continue
        ry, rx = iy[y], ix[x]
        win_y[n], win_x[n] = ry, rx
        qv = q[b, :, y, x].double().view(heads, Dq)
        kg = k[b].double().view(heads, Dq, h, w)[:, :, ry][:, :, :, rx].reshape(heads, Dq, ky * kx)
        s = torch.einsum("nd,ndk->nk", qv, kg) * Dq ** -0.5
        p = torch.softmax(s, dim=-1)
        logits[n], probs[n] = s, p
        if v is not None:
            vg = v[b].double().view(heads, C // heads, h, w)[:, :, ry][:, :, :, rx].reshape(heads, C // heads, ky * kx)
            out[n] = torch.einsum("nk,nck->nc", p, vg).reshape(C)
            abs_sum[n] = torch.einsum("nk,nck->nc", p, vg.abs()).reshape(C)
    return logits, probs, out, abs_sum, win_y, win_x
