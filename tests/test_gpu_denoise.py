"""GPU tests of the denoising objective (``naf_amd.DenoisingLoss`` / ``denoising_loss`` / ``denoising_metrics``, naf_denoise_objective)
against the fp64 restatement of the reference's ``DenoisingLoss`` and ``MetricsCalculator`` (tests/denoise_reference.py, denoising.py:61-177),
exact checks that need no reference, layouts and dtypes, and the reference's training step.

Every bound is stated against the fp64 form, in units that do not come from the kernel: 2^-24 per fp32 rounding on the few additions the
contract allows, and the deviation of the fp32 torch composition -- what the kernel replaces -- from the fp64 form on the same inputs
(E_map, E_g).  Every test prints the measured value beside its bound (``-s``); profiles/denoise_objective.txt is where they are collected."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_PARAMS = [pytest.param(i, id=R.CASE_IDS[i]) for i in range(len(R.CASES))]
VARIANTS = pytest.mark.parametrize("clamped", [False, True], ids=["unclamped", "clamped"])
U20 = 2.0 ** -20


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _loss(pred, target, w):
    """(dict of the public call, gradient with respect to pred) on device tensors."""
    import naf_amd
    p = pred.detach().requires_grad_(True)
    out = naf_amd.denoising_loss(p, target, *w)
    out["total"].backward()
    return out, p.grad


# ---- A. loss and gradient against the fp64 restatement, every element ----------------------------------------------------------------
@VARIANTS
@pytest.mark.parametrize("ci", CASE_PARAMS)
def test_loss_and_gradient_match_the_fp64_restatement(dev, ci, clamped):
    """L1 and L2 terms: relative error <= 2^-20 -- positive terms, at most 16 fp32 additions on a path (each <= 2^-24), fp64 beyond; exactly
    0 where pred == target everywhere.  SSIM term: |x - ref| <= w3 (2 E_map + 2^-20): a mean is no further off than its worst term, the
    factor 2 covers another summation order and FMA contraction.  Gradient, every element: <= 4 E_g + 2^-20 max|g64|.  total: it is formed
    from the same fp64 sums as the terms and rounded once, so its bound is the sum of the terms' bounds plus 2^-24 |total|."""
    pred, target = R.inputs(ci, clamped)
    pd, td = pred.to(dev), target.to(dev)
    for wi, w in enumerate(R.WEIGHTS):
        ref = R.loss_reference(ci, clamped, wi)
        out, grad = _loss(pd, td, w)
        assert set(out) == set(ref["terms"]), w
        assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in out.values())
        got = {k: float(v) for k, v in out.items()}
        bound_total = 2.0 ** -24 * abs(ref["terms"]["total"])
        for k in ("l1", "l2"):
            if k in got:
                r = ref["terms"][k]
                err = abs(got[k] - r)
                print(f"{R.CASE_IDS[ci]} w={w} {k}: {got[k]:.9g} ref {r:.12g} rel err {err / r if r else 0.0:.3e} (bound {U20:.3e})")
                assert err <= U20 * r
                bound_total += U20 * r
        if "ssim" in got:
            bound = w[2] * (2.0 * ref["E_map"] + U20)
            err = abs(got["ssim"] - ref["terms"]["ssim"])
            print(f"{R.CASE_IDS[ci]} w={w} ssim: {got['ssim']:.9g} ref {ref['terms']['ssim']:.12g} err {err:.3e} (bound {bound:.3e}, E_map {ref['E_map']:.3e})")
            assert err <= bound
            bound_total += bound
        err = abs(got["total"] - ref["terms"]["total"])
        print(f"{R.CASE_IDS[ci]} w={w} total: err {err:.3e} (bound {bound_total:.3e})")
        assert err <= bound_total
        g64 = ref["grad"]
        assert grad.shape == pred.shape and grad.dtype == torch.float32
        gerr = float((grad.double().cpu() - g64).abs().max())
        gmax = float(g64.abs().max())
        gbound = 4.0 * ref["E_g"] + U20 * gmax
        print(f"{R.CASE_IDS[ci]} w={w} grad: max err {gerr:.3e} (bound {gbound:.3e}; E_g {ref['E_g']:.3e}, max|g| {gmax:.3e})")
        assert gerr <= gbound


# ---- B. exact checks ------------------------------------------------------------------------------------------------------------
def test_a_second_call_gives_the_same_bits(dev):
    import naf_amd
    pred, target = (t.to(dev) for t in R.inputs(0, False))
    (a, ga), (b, gb) = _loss(pred, target, (1.0, 5.0, 0.2)), _loss(pred, target, (1.0, 5.0, 0.2))
    assert set(a) == {"l1", "l2", "ssim", "total"}
    assert all(torch.equal(a[k], b[k]) for k in a) and torch.equal(ga, gb)
    ma, mb = naf_amd.denoising_metrics(pred, target, clamp=True), naf_amd.denoising_metrics(pred, target, clamp=True)
    assert all(torch.equal(ma[k], mb[k]) for k in ma)


def test_identical_inputs_have_zero_loss_and_zero_gradient(dev):
    _, target = R.inputs(0, False)
    t = target.to(dev)
    out, grad = _loss(t.clone(), t, (1.0, 1.0, 0.0))
    assert set(out) == {"l1", "l2", "total"}
    assert float(out["l1"]) == 0.0 and float(out["l2"]) == 0.0 and float(out["total"]) == 0.0
    assert torch.equal(grad, torch.zeros_like(grad))


def test_backward_scales_the_gradient_map_exactly(dev):
    import naf_amd
    from naf_amd import ops
    pred, target = (t.to(dev) for t in R.inputs(0, False))
    w = (1.0, 5.0, 0.2)
    out8, gmap = ops.denoise_objective(pred, target, w, grad=True)
    p = pred.clone().requires_grad_(True)
    losses = naf_amd.DenoisingLoss(*w)(p, target)
    assert losses["total"].requires_grad and not (losses["l1"].requires_grad or losses["l2"].requires_grad or losses["ssim"].requires_grad)
    assert torch.equal(losses["total"].detach(), out8[6]) and torch.equal(losses["l2"], out8[4])
    (losses["total"] * 3.0).backward()
    assert torch.equal(p.grad, gmap * 3.0)
    with torch.no_grad():
        assert not naf_amd.DenoisingLoss(*w)(p, target)["total"].requires_grad
    zero = naf_amd.DenoisingLoss(0.0, 0.0, 0.0)(p, target)
    assert set(zero) == {"total"} and float(zero["total"]) == 0.0 and not zero["total"].requires_grad and zero["total"].is_cuda


# ---- C. layouts and dtypes ----------------------------------------------------------------------------------------------------------
def test_every_layout_gives_the_same_bits(dev):
    import naf_amd
    pred, target = (t.to(dev) for t in R.inputs(0, False))
    w = (1.0, 5.0, 0.2)
    base, gbase = _loss(pred, target, w)
    assert gbase.is_contiguous()
    mbase = naf_amd.denoising_metrics(pred, target, clamp=True)
    cl = pred.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                    # the logical-NCHW view of a channels-last buffer
    wide = torch.randn(*pred.shape[:3], 2 * pred.shape[3], device=dev)
    wide[..., ::2] = pred
    twide = torch.randn(*pred.shape[:3], 2 * pred.shape[3], device=dev)
    twide[..., 1::2] = target
    for name, p, t in (("channels-last view", cl, target), ("every other column", wide[..., ::2], target),
                       ("channels-last target", pred, target.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)),
                       ("sliced target", cl, twide[..., 1::2])):
        assert not p.is_contiguous() or not t.is_contiguous()
        out, g = _loss(p, t, w)
        assert all(torch.equal(out[k], base[k]) for k in base), name
        assert torch.equal(g, gbase), name
        m = naf_amd.denoising_metrics(p, t, clamp=True)
        assert all(torch.equal(m[k], mbase[k]) for k in mbase), name
    from naf_amd import ops
    assert ops.denoise_objective(cl, target, w, grad=True)[1].stride() == cl.stride()       # dense: pred's own strides
    assert ops.denoise_objective(wide[..., ::2], target, w, grad=True)[1].is_contiguous()    # not dense: contiguous


def test_bf16_inputs_are_widened_not_rounded_again(dev):
    import naf_amd
    pred, target = (t.to(dev) for t in R.inputs(0, False))
    w = (1.0, 5.0, 0.2)
    pb, tb = pred.bfloat16(), target.bfloat16()
    for p16, t16 in ((pb, target), (pb, tb), (pred, tb)):
        a, ga = _loss(p16, t16, w)
        b, gb = _loss(p16.float(), t16.float(), w)
        assert all(a[k].dtype == torch.float32 and torch.equal(a[k], b[k]) for k in b)
        assert ga.dtype == p16.dtype and torch.equal(ga, gb.to(p16.dtype))             # the fp32 gradient, rounded once
        ma, mb = naf_amd.denoising_metrics(p16, t16, clamp=True), naf_amd.denoising_metrics(p16.float(), t16.float(), clamp=True)
        assert all(torch.equal(ma[k], mb[k]) for k in mb)
    cl16 = pb.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    a, ga = _loss(cl16, target, w)
    b, gb = _loss(pb, target, w)
    assert all(torch.equal(a[k], b[k]) for k in b) and torch.equal(ga, gb) and ga.stride() == cl16.stride()


# ---- D. metrics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [False, True], ids=["as-given", "clamp"])
@pytest.mark.parametrize("ci", CASE_PARAMS)
def test_metrics_match_the_fp64_restatement(dev, ci, clamp):
    """On the unclamped inputs (predictions outside [0, 1]), with and without the folded clamp.  SSIM within 2 E_map + 2^-20 (E_map from
    the fp32 Gaussian composition); PSNR within 4.35 * 2^-20 + |ref| 2^-22 dB: the 2^-20 relative error of the mse through -10 log10
    (10 / ln 10 = 4.35), and the rounding of the result."""
    import naf_amd
    pred, target = R.inputs(ci, False)
    ref = R.metrics_reference(ci, False, clamp)
    m = naf_amd.denoising_metrics(pred.to(dev), target.to(dev), clamp=clamp)
    assert set(m) == {"psnr", "ssim"} and all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in m.values())
    serr, sbound = abs(float(m["ssim"]) - ref["metrics"]["ssim"]), 2.0 * ref["E_map"] + U20
    print(f"{R.CASE_IDS[ci]} clamp={clamp} ssim: {float(m['ssim']):.9g} ref {ref['metrics']['ssim']:.12g} err {serr:.3e} (bound {sbound:.3e}, E_map {ref['E_map']:.3e})")
    assert serr <= sbound
    rp = ref["metrics"]["psnr"]
    if rp == float("inf"):
        assert float(m["psnr"]) == float("inf")
    else:
        perr, pbound = abs(float(m["psnr"]) - rp), 4.35 * U20 + abs(rp) * 2.0 ** -22
        print(f"{R.CASE_IDS[ci]} clamp={clamp} psnr: {float(m['psnr']):.9g} dB ref {rp:.12g} err {perr:.3e} (bound {pbound:.3e})")
        assert perr <= pbound


def test_psnr_of_identical_inputs_is_infinite(dev):
    import naf_amd
    _, target = R.inputs(0, False)
    t = target.to(dev)
    m = naf_amd.denoising_metrics(t.clone(), t)
    assert float(m["psnr"]) == float("inf")
    (m64, map64), (_, map32) = R.metrics(target, target, False, torch.float64), R.metrics(target, target, False, torch.float32)
    assert m64["psnr"] == float("inf")
    assert abs(float(m["ssim"]) - m64["ssim"]) <= 2.0 * float((map32.double() - map64).abs().max()) + U20


# ---- E. the reference's step ----------------------------------------------------------------------------------------------------------
def test_the_reference_training_step(dev):
    """denoising.py:212-225 with criterion = naf_amd.DenoisingLoss(1, 5, 0.2): the gradient that reaches the model's output is the
    standalone call's map bit for bit, and it trains both branches of the encoder."""
    import naf_amd
    from naf_amd import ops
    torch.manual_seed(0)
    model = naf_amd.NAF(dim=96, heads_attn=1, heads_rope=1, kernel_size=15).to(dev).train()
    criterion = naf_amd.DenoisingLoss(1.0, 5.0, 0.2)
    g = torch.Generator().manual_seed(5)
    clean = torch.rand(2, 3, 32, 32, generator=g)
    noisy = (clean + 0.1 * torch.randn(2, 3, 32, 32, generator=g)).to(dev)
    clean = clean.to(dev)
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
    denoised = model((noisy - mean) / std, noisy, (32, 32))
    assert denoised.shape == (2, 3, 32, 32) and denoised.requires_grad
    denoised.retain_grad()
    losses = criterion(denoised, clean)
    losses["total"].backward()
    out8, gmap = ops.denoise_objective(denoised.detach(), clean, (1.0, 5.0, 0.2), grad=True)
    assert torch.equal(losses["total"].detach(), out8[6])
    assert torch.equal(denoised.grad, gmap) and float(gmap.abs().max()) > 0.0
    branches = {"encoder": 0, "sem_encoder": 0}
    for name, prm in model.named_parameters():
        if not prm.requires_grad:
            continue
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
        for b in branches:
            if f".{b}." in f".{name}" and float(prm.grad.abs().max()) > 0.0:
                branches[b] += 1
    print(f"parameters with a non-zero gradient per branch: {branches}")
    assert all(n >= 1 for n in branches.values()), branches
