"""The yardstick of the feature-PCA tests: an fp64 restatement of ``naf_amd.FeaturePCA`` (the fit and the transform the issue of this
feature states, which is the reference's ``pca()`` / ``TorchPCA`` of utils/visualization.py:135-190 on square maps of one size) on the
bf16-rounded inputs, the inputs themselves, and every bound the GPU tests assert.  Every bound is computed from the reference quantities
alone -- nothing here looks at what the kernels return.

Inputs: a planted spectrum, so that the eigengaps are known.  ``x_p = sum_k s_k a_pk u_k + 0.25 noise_p + offset`` with s = (8, 4, 2),
``u_k`` three orthonormal vectors shared by all maps of a case (each with one dominant entry, see ``_orthonormal``), ``a`` and ``noise`` unit normal, ``offset`` one N(0, 1) vector per case;
the values are rounded to bf16.  The covariance has the eigenvalues 64, 16, 4 (+ 1/16) and then 1/16.  All random numbers come from the
project's integer-hash generator (oracle.naf_oracle.hash_normal): bit-identical on every machine.

Bounds (u = 2^-24, the unit roundoff of fp32; L = min(P, 65536), the most fp32 additions between a product and the fp64 sum, as
include/naf_hip.h states):
  moments     |gram[i][j] - ref| <= L u sum_p |x_pi x_pj|,  |sum[i] - ref| <= L u sum_p |x_pi|: the standard bound for L fp32 additions of
              exact products; the fp64 stage contributes nothing at this scale
  covariance  S = (1/M) sum_m gram_m / P_m - mu mu^T, mu = (1/M) sum_m sum_m / P_m.  Elementwise
              |dS| <= B_S = (1/M) sum_m Bg_m / P_m + e |mu|^T + |mu| e^T + e e^T,  e = (1/M) sum_m bs_m / P_m,
              and E = ||B_S||_2 bounds ||dS||_2 (for 0 <= |A| <= B elementwise, ||A||_2 <= ||B||_2)
  basis       Davis-Kahan: sin(theta_r) <= 2 E / gap_r, gap_r the distance of the reference's r-th eigenvalue to its nearest other one
  projection  |raw - ref| <= (C + 4) u (sum_c |x_c V_cr| + |b_r|): C fused multiply-adds, the bias, the fp32 rounding of V and b
  picture     4 Delta / range_ref, Delta = max_p ||x_p - mu||_2 sqrt(2) (2 E / gap_r) + the projection bound

This module is a helper (no tests in it); the cases the GPU tests run are defined here so that the CPU tests can use them too.
"""
import functools
import os

import numpy as np
import torch

from oracle import naf_oracle as O

U32 = 2.0 ** -24
CHAIN = 65536                      # NAF_MOMENTS_CHAIN of include/naf_hip.h
SIN_CAP = 0.06                     # the a-priori bound on sin(theta) every basis / picture case must meet
SCALES = (8.0, 4.0, 2.0)

# name -> list of (C, H, W); the maps of one case share the basis and the offset
PCA_CASES = {
    "32x7x5": [(32, 7, 5)],                     # fewer pixels than one pixel tile
    "96x37x29": [(96, 37, 29)],                 # ragged tails, several slabs with a partial last one
    "384x40x30": [(384, 40, 30)],
    "768x33x20": [(768, 33, 20)],
    "1024x24x24": [(1024, 24, 24)],
    "96x37x29+96x16x16": [(96, 37, 29), (96, 16, 16)],   # two maps of unequal sizes: the 1 / P_m weighting
}
MOMENT_CASES = dict(PCA_CASES)
MOMENT_CASES.update({
    "64x256x256": [(64, 256, 256)],             # P = 65536: the longest chain the planner allows is met, and many slabs
    "4096x9x7": [(4096, 9, 7)],                 # the widest map served: 528 blocks of the upper triangle
    "160x50x41": [(160, 50, 41)],               # a partial last channel block; the GPU test gives it a row stride of C + 8
})
# the a-priori bound grows with the offset (the moments' bound is in sum |x_i x_j|); (1024, 24, 24) comes to 0.0601 with a unit offset and
# gets a smaller one: the cap stays where it is
OFFSET_SCALE = {"1024x24x24": 0.75}
GOLDEN_SHAPES = [(32, 12, 12), (32, 12, 12)]
GOLDEN_SEED = 7100


def bf16r(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


def _orthonormal(C: int, seed: int) -> torch.Tensor:
    """[C, 3] fp64 with orthonormal columns: Gram-Schmidt on three hash-normal vectors, each with one planted entry of half its norm (signs
    +, -, +).  That entry stays the largest by a wide margin (about 0.4 against 3 / sqrt(C)), so the sign convention -- the entry of
    largest magnitude is positive -- is decided far outside the a-priori perturbation bound of every case, and never by a near-tie."""
    g = O.hash_normal((3, C), seed).double()
    for k in range(3):
        g[k, (7 + 13 * k) % C] = (1.0, -1.0, 1.0)[k] * 0.5 * float(g[k].norm())
    cols = []
    for k in range(3):
        v = g[k].clone()
        for q in cols:
            v = v - (v * q).sum() * q
        for q in cols:                              # twice is enough
            v = v - (v * q).sum() * q
        cols.append(v / (v * v).sum().sqrt())
    return torch.stack(cols, dim=1)


def make_maps(shapes, seed: int, offset_scale: float = 1.0):
    """The maps of one case: a list of fp32 [1, C, H, W] tensors whose values are bf16 numbers."""
    C = shapes[0][0]
    U = _orthonormal(C, seed)
    offset = offset_scale * O.hash_normal((C,), seed + 1).double()
    maps = []
    for m, (Cm, H, W) in enumerate(shapes):
        assert Cm == C
        P = H * W
        a = O.hash_normal((P, 3), seed + 10 + m).double() * torch.tensor(SCALES, dtype=torch.float64)
        x = a @ U.t() + 0.25 * O.hash_normal((P, C), seed + 20 + m).double() + offset
        maps.append(bf16r(x.float()).view(H, W, C).permute(2, 0, 1).unsqueeze(0).contiguous())
    return maps


def _seed(name: str) -> int:
    return 7000 + 37 * sorted(MOMENT_CASES).index(name)


@functools.lru_cache(maxsize=None)
def case_maps(name: str):
    return tuple(make_maps(MOMENT_CASES[name], _seed(name), OFFSET_SCALE.get(name, 1.0)))


def rows(map_: torch.Tensor) -> torch.Tensor:
    """[P, C] fp64 of a [1, C, H, W] map."""
    return map_[0].permute(1, 2, 0).reshape(-1, map_.shape[1]).double()


# ---- moments ----------------------------------------------------------------------------------------------------------------------
def moments(map_: torch.Tensor):
    """(gram, sum, gram_bound, sum_bound) in fp64 for one map."""
    X = rows(map_)
    P = X.shape[0]
    L = min(P, CHAIN)
    A = X.abs()
    return X.t() @ X, X.sum(0), L * U32 * (A.t() @ A), L * U32 * A.sum(0)


@functools.lru_cache(maxsize=None)
def case_moments(name: str):
    return tuple(moments(m) for m in case_maps(name))


# ---- fit ---------------------------------------------------------------------------------------------------------------------------
class Fit:
    """mean [C], components [C, n], eigenvalues (all, descending), singular_values [n]; E and sin_bound [n] when bounds were asked for."""


def fix_signs(V: torch.Tensor) -> torch.Tensor:
    idx = V.abs().argmax(dim=0)                     # the first maximum: the lowest index wins ties
    return V * torch.where(V.gather(0, idx.unsqueeze(0)) < 0, -1.0, 1.0).double()


def fit(maps, n: int = 3, with_bounds: bool = True) -> Fit:
    M = len(maps)
    C = maps[0].shape[1]
    G = torch.zeros(C, C, dtype=torch.float64)
    BG = torch.zeros(C, C, dtype=torch.float64)
    mu = torch.zeros(C, dtype=torch.float64)
    e = torch.zeros(C, dtype=torch.float64)
    for m in maps:
        g, s, bg, bs = moments(m)
        P = m.shape[2] * m.shape[3]
        G += g / P
        mu += s / P
        BG += bg / P
        e += bs / P
    G, BG, mu, e = G / M, BG / M, mu / M, e / M
    S = G - torch.outer(mu, mu)
    w, v = torch.linalg.eigh(S)
    f = Fit()
    f.mean = mu
    f.eigenvalues = w.flip(0)
    f.components = fix_signs(v.flip(1)[:, :n].contiguous())
    P0 = maps[0].shape[2] * maps[0].shape[3]
    f.singular_values = (f.eigenvalues[:n].clamp_min(0) * (M * P0)).sqrt()
    if with_bounds:
        BS = BG + torch.outer(e, mu.abs()) + torch.outer(mu.abs(), e) + torch.outer(e, e)
        f.E = float(torch.linalg.matrix_norm(BS, ord=2))
        lam = f.eigenvalues
        gaps = []
        for r in range(n):
            others = torch.cat([lam[:r], lam[r + 1:]])
            gaps.append(float((others - lam[r]).abs().min()))
        f.gaps = gaps
        f.sin_bound = [2.0 * f.E / g for g in gaps]
    return f


@functools.lru_cache(maxsize=None)
def case_fit(name: str) -> Fit:
    return fit(list(case_maps(name)))


# ---- transform ---------------------------------------------------------------------------------------------------------------------
def transform(f: Fit, map_: torch.Tensor) -> torch.Tensor:
    """[1, n, H, W] fp64: (x - mean) . components."""
    _, C, H, W = map_.shape
    y = (rows(map_) - f.mean) @ f.components
    return y.view(H, W, -1).permute(2, 0, 1).unsqueeze(0)


def rgb(raw: torch.Tensor) -> torch.Tensor:
    lo = raw.amin(dim=(2, 3), keepdim=True)
    hi = raw.amax(dim=(2, 3), keepdim=True)
    return (raw - lo) / (hi - lo)


def projection_bound(map_: torch.Tensor, V: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[1, n, H, W] fp64: (C + 4) u (sum_c |x_c V_cr| + |b_r|)."""
    _, C, H, W = map_.shape
    t = rows(map_).abs() @ V.double().abs() + b.double().abs()
    return ((C + 4) * U32 * t).view(H, W, -1).permute(2, 0, 1).unsqueeze(0)


def picture_bound(f: Fit, map_: torch.Tensor) -> torch.Tensor:
    """[n] fp64: 4 Delta_r / range_r."""
    X = rows(map_)
    radius = float((X - f.mean).norm(dim=1).max())
    raw = transform(f, map_)
    pb = projection_bound(map_, f.components, -(f.mean @ f.components)).amax(dim=(0, 2, 3))
    rng = (raw.amax(dim=(0, 2, 3)) - raw.amin(dim=(0, 2, 3)))
    delta = torch.tensor([radius * 2.0 ** 0.5 * s for s in f.sin_bound], dtype=torch.float64) + pb
    return 4.0 * delta / rng


# ---- the golden fixture -----------------------------------------------------------------------------------------------------------------
def golden_maps():
    return make_maps(GOLDEN_SHAPES, GOLDEN_SEED)


def load_golden(golden_dir: str):
    return np.load(os.path.join(golden_dir, "P1_pca.npz"))


def match_up_to_flip(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max over components of min(|got - ref|, |got - (1 - ref)|) maxima: the reference's component signs are arbitrary, and a sign flip
    of a component is y -> 1 - y after the min-max."""
    worst = 0.0
    for r in range(ref.shape[1]):
        a = float((got[:, r].double() - ref[:, r].double()).abs().max())
        b = float((got[:, r].double() - (1.0 - ref[:, r].double())).abs().max())
        worst = max(worst, min(a, b))
    return worst
