"""Training through pooled guidance (train.py:126-137: the guidance image is 4x the output): naf_pool_guidance_bwd and
naf_preshrink_image_bwd against the fp64 restatements of tests/guidance_grad_reference.py with per-element bounds counted from the roundings
the kernels make, an exact integer census, bit-reproducibility, the autograd ops, and the training call itself (spies, the profiler's table,
gradients against the fp32 torch-stem arm)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import guidance_grad_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def channels_last(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


def share(err, bound):
    """Largest fraction of its bound any element uses (elements with a zero bound must have a zero error)."""
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max())


# ---- pooling --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_size,out_size,Cc", R.POOL_SHAPES)
def test_pool_adjoint_matches_the_restatement(dev, in_size, out_size, Cc):
    """|dx - ref| <= (2^-8 + (n + 2) * 2^-24) * sum_j |dy_j| / area_j per element: one bf16 rounding, n products, n - 1 additions and the
    rounding of 1 / area, n the pixel's window count; the restatement sees the same bf16 dy.  Two calls are bit-identical."""
    from naf_amd import ops
    g = torch.Generator().manual_seed(in_size[1] * 100 + out_size[0])
    dy = torch.randn(R.POOL_BATCH, Cc, *out_size, generator=g).to(torch.bfloat16)
    ref, n, mag = R.pool_adjoint(dy, in_size)
    d = channels_last(dy, dev)
    got = ops.pool_guidance_bwd(d, in_size)
    assert got.shape == (R.POOL_BATCH, Cc, *in_size) and got.dtype == torch.bfloat16 and got.permute(0, 2, 3, 1).is_contiguous()
    err = (got.double().cpu() - ref).abs()
    bound = (2.0 ** -8 + (n + 2).double() * 2.0 ** -24) * mag
    print(f"pool bwd {in_size} -> {out_size} C={Cc}: max |err| {float(err.max()):.3e}, share of the bound {share(err, bound):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    assert torch.equal(got, ops.pool_guidance_bwd(d, in_size))
    # any incoming gradient is served: fp32, NCHW-contiguous
    assert torch.equal(got, ops.pool_guidance_bwd(dy.float().to(dev).contiguous(), in_size))


@pytest.mark.parametrize("in_size,out_size,Cc", R.POOL_SHAPES[:2])
def test_pool_adjoint_exact_census(dev, in_size, out_size, Cc):
    """Integer dy in [-8, 8] over windows of 4 / 16 pixels: every value is a multiple of 1/16 below 8, exact in bf16 -- so is the result."""
    from naf_amd import ops
    g = torch.Generator().manual_seed(5)
    dy = torch.randint(-8, 9, (R.POOL_BATCH, Cc, *out_size), generator=g).to(torch.bfloat16)
    ref, n, _ = R.pool_adjoint(dy, in_size)
    assert int(n.max()) == 1
    got = ops.pool_guidance_bwd(channels_last(dy, dev), in_size)
    assert torch.equal(got.cpu(), ref.to(torch.bfloat16)) and torch.equal(got.double().cpu(), ref)


# ---- pre-shrink -----------------------------------------------------------------------------------------------------------------
def resize_inputs(case):
    (B, H, W), (Hs, Ws) = R.RESIZE_CASES[case]
    g = torch.Generator().manual_seed(H * 100 + Ws)
    img = torch.randn(B, 3, H, W, generator=g)
    dout = torch.randn(B, 3, Hs, Ws, generator=g)
    return img, dout


def resize_bounds(dout, in_size):
    ref, T, mag, _ = R.resize_adjoint(dout, in_size)
    return ref, (T + 2).double() * 2.0 ** -24 * mag


@pytest.mark.parametrize("case,dtype", [("a", torch.float32), ("a", torch.bfloat16), ("b", torch.float32), ("c", torch.float32)])
def test_preshrink_adjoint_matches_the_restatement(dev, case, dtype):
    """|d - ref| <= (T + 2) * 2^-24 * sum |term| per element for an fp32 image (T terms of two products each, T - 1 additions), plus
    2^-8 * |ref| for a bf16 one; against ATen's fp32 autograd on the device twice the fp32 bound, because both sides round."""
    from naf_amd import ops
    img, dout = resize_inputs(case)
    ref, b32 = resize_bounds(dout, img.shape[-2:])
    like = torch.empty(img.shape, dtype=dtype, device="meta")
    got = ops.preshrink_image_bwd(dout.to(dev), like)
    assert got.shape == img.shape and got.dtype == dtype and got.is_contiguous()
    err = (got.double().cpu() - ref).abs()
    bound = b32 + (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0.0)
    print(f"preshrink bwd {case} {dtype}: max |err| {float(err.max()):.3e}, share of the bound {share(err, bound):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    assert torch.equal(got, ops.preshrink_image_bwd(dout.to(dev), like))
    if dtype == torch.float32:
        x = img.to(dev).requires_grad_(True)
        (aten,) = torch.autograd.grad(F.interpolate(x, size=dout.shape[-2:], mode="bilinear", align_corners=False), x, dout.to(dev))
        e2 = (got.double().cpu() - aten.double().cpu()).abs()
        print(f"preshrink bwd {case} against ATen: max |diff| {float(e2.max()):.3e}, share of twice the bound {share(e2, 2 * b32):.3f}")
        assert bool((e2 <= 2 * b32).all()), float((e2 - 2 * b32).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_preshrink_adjoint_strided_images(dev, dtype):
    """Case a into images that are not NCHW-contiguous: a channels-last one, and a sliced view whose surroundings stay untouched."""
    from naf_amd import ops
    img, dout = resize_inputs("a")
    B, _, H, W = img.shape
    dense = ops.preshrink_image_bwd(dout.to(dev), torch.empty(img.shape, dtype=dtype, device="meta"))
    cl = torch.empty(img.shape, dtype=dtype, device="meta").contiguous(memory_format=torch.channels_last)
    got = ops.preshrink_image_bwd(dout.to(dev), cl)
    assert got.stride() == cl.stride() and torch.equal(got, dense)
    big = torch.full((B, 3, H + 5, W + 7), 77.0, dtype=dtype, device=dev)
    view = big[:, :, 2:2 + H, 3:3 + W]
    assert ops.preshrink_image_bwd(dout.to(dev), view, out=view) is view
    assert torch.equal(view, dense)
    outside = torch.ones_like(big, dtype=torch.bool)
    outside[:, :, 2:2 + H, 3:3 + W] = False
    assert bool((big[outside] == 77.0).all())


# ---- the autograd ops -----------------------------------------------------------------------------------------------------------
def test_pool_guidance_is_differentiable(dev):
    from naf_amd import ops
    (H, W), (Ho, Wo), Cc = R.POOL_SHAPES[2]
    g = torch.Generator().manual_seed(3)
    x = channels_last(torch.randn(2, Cc, H, W, generator=g).to(torch.bfloat16), dev)
    dy = channels_last(torch.randn(2, Cc, Ho, Wo, generator=g).to(torch.bfloat16), dev)
    plain = ops.pool_guidance(x, (Ho, Wo))
    assert plain.grad_fn is None and not plain.requires_grad
    xr = x.clone().requires_grad_(True)
    with torch.no_grad():
        assert ops.pool_guidance(xr, (Ho, Wo)).grad_fn is None
    y = ops.pool_guidance(xr, (Ho, Wo))
    assert y.grad_fn is not None and torch.equal(y.detach(), plain) and y.stride() == plain.stride()
    (dx,) = torch.autograd.grad(y, xr, dy)
    direct = ops.pool_guidance_bwd(dy, (H, W))
    assert torch.equal(dx, direct) and dx.dtype == torch.bfloat16 and dx.stride() == direct.stride()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_preshrink_image_is_differentiable(dev, dtype):
    from naf_amd import ops
    img, dout = resize_inputs("a")
    img, dout = img.to(dev).to(dtype), dout.to(dev)
    size = tuple(dout.shape[-2:])
    plain = ops.preshrink_image(img, size)
    assert plain.grad_fn is None
    xr = img.clone().requires_grad_(True)
    y = ops.preshrink_image(xr, size)
    assert y.grad_fn is not None and torch.equal(y.detach(), plain)
    (dx,) = torch.autograd.grad(y, xr, dout)
    assert dx.dtype == dtype and torch.equal(dx, ops.preshrink_image_bwd(dout, img))
    # a sliced view of a leaf: the gradient reaches the leaf, zero outside the view
    base = torch.zeros(img.shape[0], 3, img.shape[2] + 4, img.shape[3] + 4, dtype=dtype, device=dev).requires_grad_(True)
    (db,) = torch.autograd.grad(ops.preshrink_image(base[:, :, 1:-3, 2:-2], size), base, dout)
    assert torch.equal(db[:, :, 1:-3, 2:-2], dx) and float(db.float().abs().sum()) == float(dx.float().abs().sum())


# ---- the training call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("img_hw,out_hw,lr_hw,shrunk", [((64, 64), (16, 16), (8, 8), False),      # the reference's 4x geometry in miniature
                                                       ((80, 80), (16, 16), (8, 8), True),       # pre-shrunk to 64^2 first
                                                       ((50, 70), (16, 24), (8, 12), False)])    # windows that overlap
def test_training_call_runs_library_kernels_through_the_pooling(dev, monkeypatch, img_hw, out_hw, lr_hw, shrunk):
    """``model(image, feats, size)`` in .train() mode with an image larger than the output: one naf_pool_guidance_bwd (and, past 4x, one
    naf_preshrink_image_bwd) per step, no ATen pooling / bilinear kernel in the step's profile, and output, all 36 parameter gradients and
    the image gradient within the bounds tests/test_gpu_train_stem.py holds this comparison to (2e-2 / 6e-2 relative, against the fp32
    torch-stem arm)."""
    from naf_amd import NAF, ops
    torch.manual_seed(7)
    model = NAF(kernel_size=3).to(dev).train()
    model.image_encoder.rope.rescale_coords = None            # deterministic coordinates: the two arms see the same function
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias") or "norm" in n:
                p.add_(0.2 * torch.randn_like(p))
    calls = {"pool": 0, "shrink": 0}
    real_pool, real_shrink = ops.pool_guidance_bwd, ops.preshrink_image_bwd

    def spy_pool(*a, **k):
        calls["pool"] += 1
        return real_pool(*a, **k)

    def spy_shrink(*a, **k):
        calls["shrink"] += 1
        return real_shrink(*a, **k)

    monkeypatch.setattr(ops, "pool_guidance_bwd", spy_pool)
    monkeypatch.setattr(ops, "preshrink_image_bwd", spy_shrink)
    g = torch.Generator(device="cpu").manual_seed(17)
    image = torch.randn(2, 3, *img_hw, generator=g).to(dev)
    feats = torch.randn(2, 32, *lr_hw, generator=g).to(dev)
    wout = torch.randn(2, 32, *out_hw, generator=g).to(dev)
    res = {}
    for mode in ("call", False):
        model.zero_grad(set_to_none=True)
        im = image.clone().requires_grad_(True)
        if mode == "call":
            acts = [torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]
            with torch.profiler.profile(activities=acts) as prof:
                out = model(im, feats, out_hw)
                (out.float() * wout).sum().backward()
                torch.cuda.synchronize()
            names = {e.key for e in prof.key_averages()}
            assert any("pool_guidance_bwd_kernel" in n for n in names), sorted(names)
            bad = sorted(n for n in names if "adaptive_avg_pool" in n or "upsample_bilinear" in n)
            assert not bad, bad
            assert calls == {"pool": 1, "shrink": int(shrunk)}, calls
        else:
            out = model.forward_train(im, feats, out_hw, amp=False)
            (out.float() * wout).sum().backward()
            assert calls == {"pool": 1, "shrink": int(shrunk)}, calls      # the torch arm stays on ATen
        res[mode] = (out.detach().float(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
                     im.grad.detach().clone())
    out_h, gh, gi_h = res["call"]
    out_r, gr, gi_r = res[False]
    worst = max((rel(gh[n], gr[n]), n) for n in gr)
    print(f"training call {img_hw} -> {out_hw}: out {rel(out_h, out_r):.3e}, worst parameter gradient {worst[0]:.3e} ({worst[1]}), "
          f"image gradient {rel(gi_h, gi_r):.3e}")
    assert out_h.shape == (2, 32, *out_hw)
    assert rel(out_h, out_r) < 2e-2, rel(out_h, out_r)
    assert set(gr) == set(gh) and len(gr) == 36
    assert worst[0] < 6e-2, worst
    assert rel(gi_h, gi_r) < 6e-2, rel(gi_h, gi_r)
