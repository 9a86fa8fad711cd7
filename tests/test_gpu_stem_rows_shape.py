"""The row-streaming 3x3 stem layer on the 16x16x32 bf16 matrix instruction: one layer through its three instantiations
(forward, plain = data gradient, forward with key pooling) at the smallest shapes where the lane mapping can go wrong.

A B fragment is 32 input channels x 16 pixels with the tile's columns standing for permuted pixels and the k-groups for permuted
8-channel chunks (stem_rows_kernel.h), an output row is four 16x16 tiles, and a weight fragment gathers four 256-byte runs of
the packed order.  Shapes: one strip wider than the image (W = 20), a whole strip plus an edge strip (W = 48), fewer rows than a
body and rows % 4 != 0 (H = 5, 7), whole strips with the shortened last body at batch 2 (64 x 64), a height the launcher cuts
into three segments with a masked seam (22), and for the keys one band per segment (32 x 32, 48 x 64) and two (64 x 64 at a batch
that leaves two segments per strip: the only in-loop band boundary below full size).

References and bounds are those of the single-layer checks of test_gpu_parity.py (forward: torch fp32 on the same bf16
activations, |err| <= 2e-2 + 1e-2 |ref|, mean <= 2e-3, sums rtol 2e-3 / atol 0.5 against fp64 sums of the fp32 reference),
test_gpu_train_stem.py (plain: one bf16 rounding of the output + 2e-3) and test_gpu_keys.py (keys: one bf16 rounding of the
oracle's pool(RoPE) of the layer's own bf16 output; the layer's output the bits of the layer without keys).  The impulse test
is exact: every weight reaches the output alone (or in a sum of at most four that fp32 holds exactly), so one wrong
(tap, channel tile, k-step, k-group) gather shows as a wrong bf16 value, which random data would hide under the tolerance."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bf16r(x):
    return x.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _layer(B, H, W):
    """Inputs of one layer and its fp32 reference (computed once per shape, never modified)."""
    x = bf16r(O.hash_normal((B, 128, H, W), 71) * 1.5 + 0.3)
    w = bf16r(O.hash_normal((128, 128, 3, 3), 72, 1.0 / (11.3 * 3)))
    bias = O.hash_normal((128,), 73, 0.1)
    gw, gb = 1.0 + O.hash_normal((128,), 74, 0.1), O.hash_normal((128,), 75, 0.1)
    a = bf16r(F.silu(F.group_norm(x, 8, gw, gb, 1e-5)))          # the kernel feeds the MFMA with bf16 activations
    ref = F.conv2d(F.pad(a, (1,) * 4, mode="reflect"), w, bias)
    g = x.double().view(B, 8, 16, H, W)
    tot = torch.stack([g.sum(dim=(2, 3, 4)), (g * g).sum(dim=(2, 3, 4))], dim=-1)
    return x, w, bias, gw, gb, ref, tot


def _assert_close(got, ref, atol, rtol, what):
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4e}"


FWD_SHAPES = [(1, 5, 20), (1, 7, 48), (2, 64, 64), (1, 22, 48), (2, 9, 33)]


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_layer_and_sums(dev, shape):
    from naf_amd import ops
    B, H, W = shape
    x, w, bias, gw, gb, ref, tot = _layer(B, H, W)
    xd = x.to(dev).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    st_in = ops.stats_from_total(tot.to(dev))
    st_out = ops.new_stats(B, dev)
    y = torch.empty((B, H, W, 128), dtype=torch.bfloat16, device=dev)
    ops.stem_conv(xd, st_in, gw.to(dev), gb.to(dev), 1e-5, ops.pack_conv_weight(w).to(dev), bias.to(dev), y, st_out)
    got = y.float().cpu().permute(0, 3, 1, 2)
    print(f"forward {shape}: max err {float((got - ref).abs().max()):.3e} mean {float((got - ref).abs().mean()):.3e}")
    _assert_close(got, ref, 2e-2, 1e-2, f"stem conv 3x3 {shape}")
    assert float((got - ref).abs().mean()) <= 2e-3
    gr = ref.double().view(B, 8, 16, H, W)
    s = ops.stats_total(st_out).cpu()
    assert torch.allclose(s[..., 0], gr.sum(dim=(2, 3, 4)), rtol=2e-3, atol=0.5)
    assert torch.allclose(s[..., 1], (gr * gr).sum(dim=(2, 3, 4)), rtol=2e-3, atol=0.5)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", [(1, 7, 20), (2, 64, 64), (1, 22, 48)])
def test_plain_layer(dev, shape, with_bias):
    from naf_amd import ops
    B, H, W = shape
    x, w, bias, _, _, _, _ = _layer(B, H, W)
    ref = F.conv2d(F.pad(x, (1,) * 4, mode="reflect"), w, bias if with_bias else None)
    xd = x.to(dev).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    y = torch.empty_like(xd)
    ops.stem_conv_plain(xd, ops.pack_conv_weight(w).to(dev), y, bias=bias.to(dev) if with_bias else None)
    got = y.float().cpu().permute(0, 3, 1, 2)
    err = (got - ref).abs()
    print(f"plain {shape} bias={with_bias}: max err {float(err.max()):.3e}")
    assert float((err - 2 ** -8 * ref.abs()).max()) < 2e-3, float(err.max())     # one bf16 rounding of the output


def test_plain_impulses_return_every_weight_exactly(dev):
    """128 impulses, one per input channel, on a 3-pixel grid of a 24 x 48 image (two strips, three segments): the 3 x 3
    neighbourhood of impulse c holds w[:, c, tap] mirrored, alone in the interior and in exact sums of two to four along the
    reflected border.  The weights are a function of (tap, oc, ic) with eight significant bits."""
    from naf_amd import ops
    H, W = 24, 48
    oc = torch.arange(128).view(128, 1, 1, 1)
    ic = torch.arange(128).view(1, 128, 1, 1)
    tap = torch.arange(9).view(1, 1, 3, 3)
    w = (1.0 + ((oc * 5 + ic * 3 + tap * 7) % 128).float() / 128.0) * torch.exp2(((oc + 2 * ic + tap) % 4 - 2).float())
    w = torch.where((oc + ic + tap) % 2 == 0, w, -w)
    assert torch.equal(bf16r(w), w)
    x = torch.zeros((1, 128, H, W))
    for c in range(128):
        x[0, c, 1 + 3 * (c // 16), 1 + 3 * (c % 16)] = 1.0
    ref = bf16r(F.conv2d(F.pad(x, (1,) * 4, mode="reflect"), w))
    xd = x.to(dev).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    y = torch.empty_like(xd)
    ops.stem_conv_plain(xd, ops.pack_conv_weight(w).to(dev), y)
    got = y.float().cpu().permute(0, 3, 1, 2)
    bad = got != ref
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} values differ, first at {tuple(int(v) for v in bad.nonzero()[0])}"


@pytest.mark.parametrize("shape", [(1, 32, 32), (1, 48, 64), (43, 64, 64)])
def test_keys_layer(dev, shape):
    from naf_amd import ops
    B, H, W = shape
    h, wc = H // 16, W // 16
    x, w, bias, gw, gb, ref, tot = _layer(B, H, W)
    xd = x.to(dev).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    st_in = ops.stats_from_total(tot.to(dev))
    wp = ops.pack_conv_weight(w).to(dev)
    per = O.rope_periods(256, 4, 100.0)
    ty, tx = ops.rope_tables(per.to(dev), H, W)
    y0 = torch.empty((B, H, W, 128), dtype=torch.bfloat16, device=dev)
    ops.stem_conv(xd, st_in, gw.to(dev), gb.to(dev), 1e-5, wp, bias.to(dev), y0, None)
    cat = torch.zeros((B, H, W, 256), dtype=torch.bfloat16, device=dev)
    keys = torch.full((B, h, wc, 256), 7.0, dtype=torch.bfloat16, device=dev)
    ops.stem_conv(xd, st_in, gw.to(dev), gb.to(dev), 1e-5, wp, bias.to(dev), cat[..., 128:], None, keys=(keys[..., 128:], ty, tx))
    torch.cuda.synchronize()
    assert torch.equal(cat[..., 128:], y0), "the layer's output changed"
    assert bool((keys[..., :128] == 7.0).all()) and bool((cat[..., :128] == 0).all()), "wrote outside its slices"
    got = y0.float().cpu().permute(0, 3, 1, 2).contiguous()
    _assert_close(got, ref, 2e-2, 1e-2, f"stem conv 3x3 with keys {shape}")
    kref = O.key_pool(O.rope(got, per, 2), (h, wc))
    kgot = keys[..., 128:].float().cpu().permute(0, 3, 1, 2)
    err = (kgot - kref).abs()
    print(f"keys {shape}: max err {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 2 ** -8 * kref.abs()).all()), f"keys {shape}: max err {float(err.max()):.3e}"
