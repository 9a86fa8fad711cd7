"""The yardstick of the cosine-objective tests (``naf(..., head=E, cosine=True, target=t, loss="ce")``, ``ops.xna_cos_objective``,
naf_xna_cos_ce_fwd): an fp64 restatement on top of tests/cosine_reference.py and per-element bounds.  Nothing in the bounds is measured.

1. ``objective``.  With r = cosine_reference.reference(...) (z = r["cos"] = s * c, c the cosines, norms = ||f||) and a target t, per pixel
       lse = logsumexp_n z,  label = argmax_n z,  loss = lse - z[t],  d[n] = softmax(z)[n] - (n == t)
       g'[n] = (s / max(||f||, 1e-12)) * d[n]        the gradient with respect to E^[n] . f (the norm does not depend on E)
       ds    = sum_n d[n] * c[n]                     the pixel's share of dloss / ds
   A pixel is IGNORED when t == ignore_index or t is outside [0, N): loss 0, g' = 0, ds = 0, the label is still defined.  Where ||f|| = 0
   every cosine is 0, the loss of a counted pixel is ln N, and g' = 0: dE^[n] = sum_px g'[px, n] f[px] and f = 0, so the exact gradient row
   is zero (NOT s * 1e12 * d).  ``autograd_reference`` differentiates the definition itself in fp64 (loss summed over the counted pixels)
   and gives dE and ds_total; tests/test_cosine_objective_cpu.py holds the two against each other and against F.cross_entropy.

2. The bounds, from the kernel's rounding points (naf_amd/csrc/xna_cos_kernel.h).  Let b[p, n] = cosine_reference.bound(r) (the bound on
   every scaled cosine) and beta[p] = max_n b[p, n].
   LOSS.  logsumexp is 1-Lipschitz in the max norm and the target logit moves by at most beta:
       |loss~ - loss| <= 2 beta + 1e-5 * (1 + |lse| + |z_t|)          (the last term: fp32 exp / log / sums of the epilogue)
   LABELS.  The kernel's label L satisfies z[L] >= max z - 2 beta, and L = argmax z where the top-2 margin of the reference exceeds 2 beta
   (``decided``); the share of decided pixels is a property of the reference alone.
   G'.  Each z moves by <= beta, so softmax_n changes by a factor in [e^-2beta, e^2beta]: |dp_n| <= p_n (e^2beta - 1) + 16 * 2^-24 p_n (the
   hardware exp2 and reciprocal).  The factor G = s * inv carries rho = fd / (||f|| - fd) relative (fd = feature_delta(r): the norm is
   formed from the implied feature), then one bf16 rounding (2^-9 relative) and a few fp32 roundings (8 * 2^-24):
       |g'~ - g'| <= G * ((1 + rho) * |dp_n| + rho * |d_n|) + (2^-9 + 8 * 2^-24) * (|g'| + that)
   Exactly 0 on ignored pixels, where ||f|| = 0, and in channels >= N.
   DS.  With bc = b / |s| the bound on an unscaled cosine:
       |ds~ - ds| <= sum_n (|dp_n| * (|c_n| + bc_n) + |d_n| * bc_n) + N * 2^-24 * sum_n |d_n c_n|       (0 on ignored pixels)

``emulate_objective`` is the epilogue's arithmetic on the host (fp64 between the rounding points, g' rounded to bf16) on the emulated
cosines of cosine_reference.emulate, with one planted defect per keyword.

This module is a helper (no tests in it)."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_reference as R  # noqa: E402

F32 = R.F32
IGNORE = 255
# the cases the GPU tests run (cosine_reference.CASES): served ones, and the two large windows
GPU_CASES = ("a_c128_k7_n21", "c_dv192_n151", "e_patch14_n21", "f_rows30_n151", "g_k9_n256", "i_k11_n40", "b_whole_grid_n1", "l_two_rounds_n21",
             "j_k13_n21", "k_k15_n40")
# decided-label share of the reference (asserted >= 0.5 from the reference alone; the figures at seed 5100)
SHARE_CASES = ("a_c128_k7_n21", "c_dv192_n151", "e_patch14_n21", "f_rows30_n151", "g_k9_n256", "k_k15_n40")


def gc_of(n):
    npad = (n + 15) // 16 * 16
    return next((c for c in (32, 64, 96, 128, 192, 256) if c >= npad), npad)


def make_target(name, ignore_index=IGNORE, seed=7700):
    """int64 [B, Ho, Wo]: random classes, a block of ``ignore_index`` and a few values outside [0, N)."""
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    Ho, Wo = h * dy, w * dx
    g = torch.Generator().manual_seed(seed + N)
    t = torch.randint(0, N, (B, Ho, Wo), generator=g)
    t[:, Ho // 4: Ho // 4 + max(2, Ho // 8), Wo // 3: Wo // 3 + max(3, Wo // 4)] = ignore_index
    t[:, -1, 0], t[:, -1, 1], t[:, -1, 2], t[:, 0, -1] = N, -3, N + 1000, -1
    return t


def valid_of(target, ignore_index, N):
    return (target != ignore_index) & (target >= 0) & (target < N)


def objective(r, target, ignore_index=IGNORE):
    """fp64 dict on r = cosine_reference.reference(...): z, c [B, Ho, Wo, N]; loss, lse, zt, ds [B, Ho, Wo]; labels; p, d, g [B, Ho, Wo, N];
    valid; G = s / max(||f||, 1e-12), 0 where ||f|| = 0."""
    z = r["cos"].permute(0, 2, 3, 1)
    N = z.shape[-1]
    ls = r["ls"]
    c = z / ls
    valid = valid_of(target, ignore_index, N)
    tc = torch.where(valid, target, torch.zeros_like(target))
    lse = torch.logsumexp(z, dim=3)
    zt = z.gather(3, tc.unsqueeze(3))[..., 0]
    p = torch.exp(z - lse.unsqueeze(3))
    d = (p - F.one_hot(tc, N).double()) * valid.unsqueeze(3)
    G = torch.where(r["norms"] > 0, ls / r["norms"].clamp_min(R.EPS), torch.zeros_like(r["norms"]))
    return {"z": z, "c": c, "valid": valid, "lse": lse, "zt": zt, "loss": torch.where(valid, lse - zt, torch.zeros_like(lse)),
            "labels": z.argmax(dim=3), "p": p, "d": d, "G": G, "g": G.unsqueeze(3) * d, "ds": (d * c).sum(dim=3)}


def autograd_reference(f, E, s, target, ignore_index=IGNORE, normalized=False):
    """fp64 autograd of the definition on the feature map f [B, C, H, W]: (loss summed over the counted pixels, dE [N, C], ds_total).
    ``normalized``: E holds the normalised rows already and the gradient is the one with respect to them."""
    E64 = E.double().clone().requires_grad_(True)
    s64 = torch.tensor(float(s), dtype=torch.float64, requires_grad=True)
    ff = f.double()
    nrm = ff.norm(dim=1, keepdim=True)
    z = s64 * torch.einsum("nc,bchw->bnhw", E64 if normalized else F.normalize(E64, dim=1), ff / nrm.clamp_min(R.EPS))
    N = E.shape[0]
    valid = valid_of(target, ignore_index, N)
    tgt = torch.where(valid, target, torch.full_like(target, -100))
    loss = F.cross_entropy(z, tgt, ignore_index=-100, reduction="sum")
    loss.backward()
    return loss.detach(), E64.grad, s64.grad


def beta_of(r):
    return R.bound(r).amax(dim=1)


def loss_bound(r, o):
    return 2.0 * beta_of(r) + 1e-5 * (1.0 + o["lse"].abs() + o["zt"].abs())


def decided(r, o):
    """[B, Ho, Wo] bool: the reference's top-2 margin exceeds 2 beta (always True for one class)."""
    z = o["z"]
    if z.shape[-1] == 1:
        return torch.ones(z.shape[:-1], dtype=torch.bool)
    top = z.topk(2, dim=3).values
    return (top[..., 0] - top[..., 1]) > 2.0 * beta_of(r)


def check_labels(labels, r, o, what):
    """Every pixel: the label is a maximum of the reference's z up to 2 beta, and the argmax where the margin decides."""
    z, beta = o["z"], beta_of(r)
    lab = labels.long()
    assert bool(((lab >= 0) & (lab < z.shape[-1])).all()), f"{what}: labels outside [0, N)"
    zl = z.gather(3, lab.unsqueeze(3))[..., 0]
    near = zl >= z.amax(dim=3) - 2.0 * beta
    dec = decided(r, o)
    same = lab == o["labels"]
    print(f"{what}: decided share {float(dec.double().mean()):.3f}, equal to the argmax on {float(same.double().mean()):.4f}")
    assert bool(near.all()), f"{what}: {int((~near).sum())} labels are not a maximum up to 2 beta"
    assert bool(same[dec].all()), f"{what}: {int((~same[dec]).sum())} labels differ from a decided argmax"


def _dp(r, o):
    beta = beta_of(r).unsqueeze(3)
    return o["p"] * (torch.expm1(2.0 * beta) + 16.0 * F32)


def g_bound(r, o):
    fd, nrm = R.feature_delta(r), r["norms"]
    rho = torch.where(nrm > fd, fd / (nrm - fd).clamp_min(1e-300), torch.full_like(nrm, float("inf")))
    rho = torch.where(nrm > 0, rho, torch.zeros_like(rho)).unsqueeze(3)
    v = o["valid"].unsqueeze(3).double()
    core = o["G"].unsqueeze(3) * ((1.0 + rho) * _dp(r, o) * v + rho * o["d"].abs())
    core = torch.where(o["G"].unsqueeze(3) > 0, core, torch.zeros_like(core))      # norm 0 (and s = 0): exactly zero
    return core + (2.0 ** -9 + 8.0 * F32) * (o["g"].abs() + core)


def ds_bound(r, o):
    bc = (R.bound(r) / abs(r["ls"])).permute(0, 2, 3, 1)
    v = o["valid"].unsqueeze(3).double()
    N = o["z"].shape[-1]
    return ((_dp(r, o) * (o["c"].abs() + bc) + o["d"].abs() * bc) * v).sum(dim=3) + N * F32 * (o["d"] * o["c"]).abs().sum(dim=3)


def padded(g, gc):
    return F.pad(g, (0, gc - g.shape[-1]))


def emulate_objective(z, nrm, ls, target, ignore_index=IGNORE, gc=None, *, no_inv=False, keep_zero_norm=False, ds_on_scaled=False,
                      onehot_on_ignored=False, pad_value=0.0):
    """The epilogue on emulated scaled cosines z [B, N, Ho, Wo] and norms (cosine_reference.emulate): fp64, g' rounded once to bf16.
    -> (loss, labels, g' [B, Ho, Wo, gc], ds).  One planted defect per keyword: g' not multiplied by 1 / norm; the zero-norm row kept
    (s * 1e12 * d); ds taken on the scaled cosines; the onehot subtracted on an ignored pixel (its row not zeroed); a non-zero pad channel."""
    z = z.permute(0, 2, 3, 1)
    N = z.shape[-1]
    gc = gc_of(N) if gc is None else gc
    c = z / ls
    valid = valid_of(target, ignore_index, N)
    tc = torch.where(valid, target, torch.zeros_like(target))
    lse = torch.logsumexp(z, dim=3)
    loss = torch.where(valid, lse - z.gather(3, tc.unsqueeze(3))[..., 0], torch.zeros_like(lse))
    d = torch.exp(z - lse.unsqueeze(3)) - F.one_hot(tc, N).double()
    if not onehot_on_ignored:
        d = d * valid.unsqueeze(3)
    inv = 1.0 / nrm.clamp_min(R.EPS)
    G = ls * (torch.ones_like(inv) if no_inv else inv)
    if not keep_zero_norm:
        G = torch.where(nrm > 0, G, torch.zeros_like(G))
    g = F.pad(G.unsqueeze(3) * d, (0, gc - N), value=pad_value).to(torch.bfloat16).double()
    ds = (d * (z if ds_on_scaled else c)).sum(dim=3)
    return loss, z.argmax(dim=3), g, ds
