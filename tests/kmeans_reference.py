"""fp64 restatement of one k-means (Lloyd) step on the upsampled features and the exact census of its kernel (tests/test_kmeans_cpu.py
without a device, tests/test_gpu_kmeans.py on one).  Plain helper module: no test in it.

    z[b, k, px]   = bias[b, k] + sum_g sum_j P_g[px, j] * PV_g[b, j, k]        label[b, px] = the lowest k with z = max_k z
    A, mass       = mask pooling (tests/mask_pool_reference.py) under the one-hot masks [label == k]
    c_new[b, k]   = sum_j A[b, g(c), k, j] V[b, c, j] / mass[b, k], the old centroid where mass = 0

(pv5, bias) are ``ops.project_kmeans_values``' -- the bf16 operands the kernel reads -- so the logits carry the error model of the head
kernel: ``input_statistics.head_reference64`` / ``head_bound``, one bf16 rounding of the normalised P per weight.  A pixel is DETERMINED
when the oracle's top-2 margin exceeds twice that bound: there the device label must be the oracle's; elsewhere it must be a maximum
up to twice the bound.  A cluster is determined when no undetermined pixel could join or leave it: its new centroid is then mask
pooling's under the same masks and stays within ``mask_pool_reference.pooled_bound`` (n = 1: one-hot operands are exact) over the mass.

Planted inputs: low-res features = centroid[blob] + 0.3 noise + 0.7 (bf16-representable) with blobs on a 3 x 2 partition of the grid,
centroids under test = the planted ones + 0.2 noise, a different set per image.

Census: pv = 0 and a one-hot bias label every pixel k*; with q = 0, A[b, :, k*] / p is the integer census of an all-ones mask.
``census_expectation`` restates it from the cell geometry and can plant the defects the kernel could have: a shifted window, a dropped
clamp, a counted pad pixel, ties to the highest index, the bias row of the wrong image.
"""
import torch

import input_statistics as S
import mask_pool_reference as R
from oracle import naf_oracle as O

DEFECTS = ("shift", "no_clamp", "pad_pixel", "tie_highest", "wrong_bias_row")
# (geometry name of test_gpu_mask_pool.GEOMS, K, logit family): the parity cases; K = 16 leaves clusters empty (six blobs)
PARITY = [("k7", 4, "unit"), ("k7", 16, "unit"), ("k3", 4, "unit"), ("k9", 6, "peaked")]
GEOMS = {"k7": (7, (8, 10), (128, 160)), "k7_patch14": (7, (8, 10), (112, 140)), "k3": (3, (4, 5), (64, 80)), "k9": (9, (10, 12), (160, 192)),
         "k15": (15, (16, 16), (256, 256))}          # test_gpu_mask_pool.GEOMS, restated for the tests without a device (asserted equal on one)


def blob_labels(h, w):
    """[h, w] int64 in 0 .. 5: a 3 x 2 partition of the grid."""
    by = torch.div(torch.arange(h) * 3, h, rounding_mode="floor")
    bx = torch.div(torch.arange(w) * 2, w, rounding_mode="floor")
    return by[:, None] * 2 + bx[None, :]


def planted_inputs(geom, K, fam, seed, B=2, dim=256, heads=4):
    """(q [B, dim, Ho, Wo], k [B, dim, h, w], v [B, dim, h, w], c [B, K, dim], window): bf16-representable q, k, v; fp32 centroids under test."""
    ks, (h, w), (Ho, Wo) = GEOMS[geom]
    q, k = S.make_qk((B, dim, Ho, Wo), (B, dim, h, w), fam, seed, heads)
    planted = O.hash_normal((B, K, dim), seed + 2)
    blob = blob_labels(h, w) % K
    v = planted[:, blob].permute(0, 3, 1, 2) + 0.3 * O.hash_normal((B, dim, h, w), seed + 3) + 0.7
    c = planted + 0.2 * O.hash_normal((B, K, dim), seed + 4)
    return q, k, S.bf16r(v), c, ks


def first_argmax(z, highest=False):
    """The lowest (``highest``: the highest) index among the equal maxima of z along dim 1."""
    K = z.shape[1]
    idx = torch.arange(K).view(1, K, *([1] * (z.dim() - 2))).expand_as(z)
    eq = z == z.amax(dim=1, keepdim=True)
    return torch.where(eq, idx, torch.full_like(idx, -1)).amax(dim=1) if highest else torch.where(eq, idx, torch.full_like(idx, K)).amin(dim=1)


def logits_reference(q, k, pv5, bias, ksz, heads):
    """(z [B, K, Ho, Wo], bound [B, Ho, Wo]) in fp64 on the kernel's operands: pv5 bf16 [B, heads, h, w, Kpad], bias fp32 [B, K]."""
    B, K = bias.shape
    pvn = pv5.float().permute(0, 1, 4, 2, 3).reshape(B, -1, *pv5.shape[2:4])
    zs, bs = [], []
    for b in range(B):
        ref, abs_sum = S.head_reference64(q[b:b + 1], k[b:b + 1], pvn[b:b + 1], ksz, heads, K, bias[b])
        zs.append(ref)
        bs.append(S.head_bound(ref, abs_sum).amax(dim=1))
    return torch.cat(zs), torch.cat(bs)


def determined(z, bound):
    """(det [B, Ho, Wo] bool, share): pixels whose top-2 margin exceeds 2 * bound (K = 1: every pixel)."""
    if z.shape[1] == 1:
        return torch.ones_like(bound, dtype=torch.bool), 1.0
    top = z.topk(2, dim=1).values
    det = (top[:, 0] - top[:, 1]) > 2.0 * bound
    return det, float(det.double().mean())


def lloyd_step_reference(q, k, v, c, ksz, heads):
    """One step in fp64 on the oracle's attention.  dict: z, bound, labels, det, share, A, mass, pooled, pooled_abs, c_new [B, K, C], and
    cluster_det [B, K] bool: no undetermined pixel has cluster k among its candidates (scores within 2 * bound of the best)."""
    from naf_amd import ops
    pv5, bias, _ = ops.project_kmeans_values(c, v, heads)
    z, bound = logits_reference(q, k, pv5, bias, ksz, heads)
    B, K = bias.shape
    labels = first_argmax(z)
    det, share = determined(z, bound)
    onehot = labels[:, None] == torch.arange(K).view(1, K, 1, 1)
    cand = z >= (z.amax(dim=1, keepdim=True) - 2.0 * bound[:, None])
    swing = cand & ~det[:, None]          # the pixels that may join or leave cluster k: undetermined, with k among their candidates
    cluster_det = ~swing.flatten(2).any(dim=2)
    both = R.mask_pool_reference(q, k, torch.cat([onehot, swing], dim=1), ksz, heads, v)          # one pass over the attention for both sets
    r = {n: (t[:, :, :K] if t.dim() == 5 else t[:, :K]) for n, t in both.items()}
    mass = r["mass"]
    c_new = torch.where(mass[..., None] > 0, r["pooled"] / mass.clamp(min=1.0)[..., None], c.double())
    return dict(z=z, bound=bound, labels=labels, det=det, share=share, cluster_det=cluster_det, c_new=c_new, pv5=pv5, bias=bias,
                swing_abs=both["pooled_abs"][:, K:], swing_mass=both["mass"][:, K:], **r)


def centroid_bound(r, hw):
    """(bound [B, K, C], checkable [B, K]) of c_new = S / M.  With n swing pixels (``swing_mass``) of abs-sum sa (``swing_abs``) the device
    sums S_d over its own masks differ from the reference's S by at most sa (the pixels that moved) plus mask pooling's ``pooled_bound``
    (byte masks) on the abs-sum pa + sa, its mass M_d lies in [M - n, M + n], and the fp32 division adds 2^-23:
        |S_d / M_d - S / M| <= |S_d - S| / M_d + |S| n / (M M_d),   M_d >= M - n.
    For a determined cluster (n = 0) this is ``pooled_bound`` over the mass.  Checkable: M > n (the cluster cannot end up empty)."""
    M, n = r["mass"], r["swing_mass"]
    lo = (M - n).clamp(min=1.0)[..., None]
    pa = r["pooled_abs"] + r["swing_abs"]
    b = (R.pooled_bound(pa, hw, False) + r["swing_abs"] + 2.0 * S.F32 * pa) / lo + r["pooled"].abs() * n[..., None] / (M.clamp(min=1.0)[..., None] * lo)
    return b, (M - n) >= 1.0


# ---- Lloyd on the materialised fp64 features: the reference's own sanity ---------------------------------------------------------------
def upsampled_features(q, k, v, ksz, heads):
    return S.attention_reference(q, k, v, ksz, heads)[0]


def lloyd_exact(f, c, iters):
    """Plain Lloyd in fp64 on f [B, C, Ho, Wo]: (centroids, labels, [the objective at every assignment: iters + 1 values])."""
    c = c.double()
    B, K, _ = c.shape
    fp = f.flatten(2)                                            # B C P
    obj = []
    for it in range(iters + 1):
        d = (fp * fp).sum(1)[:, None] - 2.0 * torch.einsum("bkc,bcp->bkp", c, fp) + (c * c).sum(2)[..., None]
        labels = first_argmax(-d)
        obj.append(float(d.gather(1, labels[:, None]).sum()))
        if it < iters:
            onehot = (labels[:, None] == torch.arange(K).view(1, K, 1)).double()
            mass = onehot.sum(2)
            sums = torch.einsum("bkp,bcp->bkc", onehot, fp)
            c = torch.where(mass[..., None] > 0, sums / mass.clamp(min=1.0)[..., None], c)
    return c, labels.view(B, *f.shape[-2:]), obj


# ---- census ------------------------------------------------------------------------------------------------------------------------------
def census_bias(B, K, kstar):
    """fp32 [B, K]: a one-hot at kstar[b] (1.0 there, 0 elsewhere)."""
    bias = torch.zeros(B, K)
    for b in range(B):
        bias[b, kstar[b]] = 1.0
    return bias


def census_expectation(bias, h, w, Ho, Wo, ksz, defect=None):
    """(labels [B] the cluster every pixel of image b takes, counts int64 [B, K, h, w], mass int64 [B, K]) with pv = 0 and q = 0: from the
    bias rows and the cell geometry alone.  ``defect``: one of DEFECTS planted (what a wrong kernel would produce)."""
    B, K = bias.shape
    rows = bias.roll(1, dims=0) if defect == "wrong_bias_row" else bias
    labels = first_argmax(rows.double(), highest=defect == "tie_highest")
    ones = torch.ones(B, 1, Ho, Wo, dtype=torch.bool)
    geo = defect if defect in R.DEFECTS else None
    cnt1 = R.census_counts(ones, h, w, ksz, defect=geo)[:, 0]                      # B h w
    px = Ho * Wo
    if defect == "pad_pixel":
        px += ((-(Wo // w)) % 16) * Ho * w
    counts = torch.zeros(B, K, h, w, dtype=torch.int64)
    mass = torch.zeros(B, K, dtype=torch.int64)
    for b in range(B):
        counts[b, labels[b]] = cnt1[b]
        mass[b, labels[b]] = px
    return labels, counts, mass
