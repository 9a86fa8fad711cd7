"""GPU tests of the frame preparation (``naf_amd.prepare_views`` / naf_image_prep) against tests/image_prep_reference.py: every result must
be the BITS of ``literal32`` (the semantics of include/naf_hip.h in numpy float32) and within blend + coordinate term of the reference's own
torch calls run on the device.  tests/test_image_prep_cpu.py holds the yardstick against itself on the same cases."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_prep_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _bits(a, b):
    """torch.equal on the stored bits (so that a NaN or a signed zero cannot hide a difference)."""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))


def _check_case(name, got, dev, hflip=False, src=None):
    """Each view: bit-equal to ``literal32``, and within blend + coordinate term (+ the two stores) of the torch composition on the device."""
    src = R.source(name) if src is None else src
    specs = R.specs(name)
    assert len(got) == len(specs)
    for k, (spec, (lit, value, S, coord, wterm), g) in enumerate(zip(specs, R.reference(name, hflip), got)):
        assert g.dtype == spec[-1] and tuple(g.shape) == tuple(lit.shape) and g.is_contiguous()
        differ = int((g.cpu().float() != lit.float()).sum())
        want = R.torch_composition(src, spec, hflip, device=dev)
        bound = R.blend_bound(src.dtype, spec, S, wterm) + coord
        bound = bound + R.store_term(spec[-1], np.abs(value) + bound, sides=2)
        err = np.abs(g.cpu().double().numpy() - want.cpu().double().numpy())
        ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
        print(f"{name}[{k}]{' hflip' if hflip else ''}: {differ} of {lit.numel()} elements differ from literal32; max |kernel - torch| = "
              f"{float(err.max()) / R.U:.1f} x 2^-24, worst err / bound {ratio:.3f}")
        assert _bits(g, lit), f"{name}[{k}]: {differ} elements differ from literal32"
        assert ratio <= 1.0, f"{name}[{k}]"


# ---- A. against the restatements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_bits_of_literal32_and_close_to_torch(dev, name):
    import naf_amd
    got = naf_amd.prepare_views(R.source(name).to(dev), R.views(name))
    _check_case(name, got, dev)


def test_hflip_is_the_call_on_the_flipped_source(dev):
    import naf_amd
    src = R.source("small")
    got = naf_amd.prepare_views(src.to(dev), R.views("small"), hflip=True)
    _check_case("small", got, dev, hflip=True)
    flipped = naf_amd.prepare_views(torch.flip(src, dims=[-2]).to(dev), R.views("small"))           # [1, H, W, 3]: dim -2 is the columns
    plain = naf_amd.prepare_views(src.to(dev), R.views("small"))
    assert _bits(got[0], flipped[0]) and not _bits(got[0], plain[0])
    img = R.source("training").to(dev)
    a = naf_amd.prepare_views(img, R.views("training"), hflip=True)
    b = naf_amd.prepare_views(torch.flip(img, dims=[-1]), R.views("training"))
    assert all(_bits(x, y) for x, y in zip(a, b))


def test_strided_sources(dev):
    """A crop of a larger channels-last fp32 tensor and a crop of a larger uint8 frame are read in place: equal to the call on a dense copy."""
    import naf_amd
    V = naf_amd.PrepView
    views = [V((19, 23), "bilinear", R.BACKBONE_MEAN, R.BACKBONE_STD, then=((8, 31), "bicubic")), V(mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD),
             V((30, 11), "bicubic", dtype=torch.bfloat16)]
    big = R._f32((2, 3, 40, 50), 31).to(dev).contiguous(memory_format=torch.channels_last)
    crop = big[:, :, 5:32, 7:40]
    assert crop.stride() == (6000, 1, 150, 3) and not crop.is_contiguous()
    for x, y in zip(naf_amd.prepare_views(crop, views), naf_amd.prepare_views(crop.contiguous(), views)):
        assert _bits(x, y)
    lit = R.literal32(crop.cpu().contiguous(), R.view_spec(views[0], 27, 33))
    assert _bits(naf_amd.prepare_views(crop, views)[0], lit)
    frame = R._u8((2, 44, 52, 3), 32).to(dev)
    fcrop = frame[:, 3:30, 11:44]
    assert fcrop.stride() == (44 * 52 * 3, 52 * 3, 3, 1) and not fcrop.is_contiguous()
    for x, y in zip(naf_amd.prepare_views(fcrop, views), naf_amd.prepare_views(fcrop.contiguous(), views)):
        assert _bits(x, y)
    assert _bits(naf_amd.prepare_views(fcrop[1], views)[0], R.literal32(fcrop[1].cpu().contiguous(), R.view_spec(views[0], 27, 33)))
    bf = big.to(torch.bfloat16)[:, :, 5:32, 7:40]
    assert _bits(naf_amd.prepare_views(bf, views)[2], R.literal32(bf.cpu().contiguous(), R.view_spec(views[2], 27, 33)))


def test_out_windows_leave_the_sentinel_intact(dev):
    import naf_amd
    V = naf_amd.PrepView
    src = R.source("small").to(dev)
    (want,) = naf_amd.prepare_views(src, R.views("small"))                                           # [1, 3, 5, 14]
    (want16,) = naf_amd.prepare_views(src, [V((6, 5), "bicubic", dtype=torch.bfloat16)])            # [1, 3, 6, 5]
    buf = torch.full((2, 5, 9, 20), -77.0, device=dev)
    buf16 = torch.full((3, 8, 7, 3), -77.0, device=dev, dtype=torch.bfloat16)                        # channels last: [1, 3, 6, 5] inside NHWC
    w32, w16 = buf[1:2, 1:4, 2:7, 3:17], buf16[1:2, 1:7, 1:6, :].permute(0, 3, 1, 2)
    view = R.views("small")[0]
    view.out = w32
    res = naf_amd.prepare_views(src, [view, V((6, 5), "bicubic", dtype=torch.bfloat16, out=w16)])
    assert res[0] is w32 and res[1] is w16
    assert _bits(w32, want) and _bits(w16, want16)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:2, 1:4, 2:7, 3:17] = False
    assert bool((buf[mask] == -77.0).all())
    mask16 = torch.ones_like(buf16, dtype=torch.bool)
    mask16[1:2, 1:7, 1:6, :] = False
    assert bool((buf16[mask16] == -77.0).all())
    for bad in (torch.empty(1, 3, 14, 5, device=dev), torch.empty(1, 3, 5, 14, device=dev, dtype=torch.bfloat16), torch.empty(1, 3, 5, 14),
                torch.empty(3, 5, 14, device=dev), "nothing"):
        view.out = bad
        with pytest.raises(ValueError, match="`out`"):
            naf_amd.prepare_views(src, [view])
    assert bool((buf[mask] == -77.0).all())


def test_identity_views_return_the_source_bits(dev):
    import naf_amd
    V = naf_amd.PrepView
    src = R._f32((2, 3, 9, 13), 21)
    views = [V(), V((9, 13), "bilinear"), V((9, 13), "bicubic"), V((9, 13), "bilinear", then=((9, 13), "bicubic"))]
    for g in naf_amd.prepare_views(src.to(dev), views):
        assert _bits(g, src)
    b16 = src.to(torch.bfloat16)
    for g in naf_amd.prepare_views(b16.to(dev), [V(dtype=torch.bfloat16), V((9, 13), "bicubic", dtype=torch.bfloat16), V()]):
        assert _bits(g, b16 if g.dtype == torch.bfloat16 else b16.float())
    u = torch.arange(256, dtype=torch.uint8).repeat(3).view(3, 16, 16).permute(1, 2, 0).contiguous()
    want = (u.permute(2, 0, 1)[None].double() / 255).float()                                        # exactly u / 255, rounded once
    for g in naf_amd.prepare_views(u.to(dev), [V(), V((16, 16), "bilinear"), V(then=((16, 16), "bicubic"))]):
        assert _bits(g, want)
    probe = naf_amd.prepare_views(src.to(dev), naf_amd.probing_views(R.BACKBONE_MEAN, R.BACKBONE_STD), hflip=True)
    for g, v in zip(probe, naf_amd.probing_views(R.BACKBONE_MEAN, R.BACKBONE_STD)):
        assert _bits(g, R.literal32(src, R.view_spec(v, 9, 13), hflip=True))


def test_the_davis_call_makes_no_host_synchronisation_and_repeats_its_bits(dev):
    import naf_amd
    frame = R.source("davis").to(dev)
    views = R.views("davis")
    first = naf_amd.prepare_views(frame, views)                                                      # warm: allocator, library
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = naf_amd.prepare_views(frame, views)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _check_case("davis", got, dev)
    assert all(_bits(x, y) for x, y in zip(first, got))


def test_the_call_is_capturable(dev):
    """One launch, no workspace, no synchronisation: a captured call replays into the same outputs and follows the source's new content."""
    import naf_amd
    src = R.source("small").to(dev)
    other = torch.flip(R.source("small"), dims=[-2]).to(dev)
    want, want_other = naf_amd.prepare_views(src, R.views("small"))[0], naf_amd.prepare_views(other, R.views("small"))[0]
    static = src.clone()
    out = torch.zeros_like(want)
    view = R.views("small")[0]
    view.out = out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        naf_amd.prepare_views(static, [view])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        naf_amd.prepare_views(static, [view])
    out.zero_()
    graph.replay()
    assert _bits(out, want)
    static.copy_(other)
    graph.replay()
    assert _bits(out, want_other) and not _bits(want, want_other)


# ---- B. what is not served ---------------------------------------------------------------------------------------------------------------
def test_errors(dev):
    import naf_amd
    V = naf_amd.PrepView
    frame = R.source("small").to(dev)
    with pytest.raises(ValueError, match="std != 0"):
        naf_amd.prepare_views(frame, [V(mean=(0.5, 0.5, 0.5), std=(0.2, 0.2, 0.0))])
    with pytest.raises(ValueError, match="1 <= views <= 4"):
        naf_amd.prepare_views(frame, [])
    with pytest.raises(ValueError, match="1 <= views <= 4"):
        naf_amd.prepare_views(frame, [V()] * 5)
    with pytest.raises(ValueError, match="at least 1"):
        naf_amd.prepare_views(frame, [V((4, 0), "bilinear")])
    with pytest.raises(ValueError, match="every size <= 16384"):
        naf_amd.prepare_views(frame, [V((16385, 4), "bilinear")])
    with pytest.raises(ValueError, match="mode none requires equal sizes"):
        naf_amd.prepare_views(frame, [V((4, 4), None)])
    with pytest.raises(ValueError, match="3 channels"):
        naf_amd.prepare_views(torch.zeros(7, 9, 4, dtype=torch.uint8, device=dev), [V()])
    with pytest.raises(ValueError, match="uint8, float32 or bfloat16"):
        naf_amd.prepare_views(torch.zeros(7, 9, 3, dtype=torch.int32, device=dev), [V()])
    with pytest.raises(ValueError, match="`out`"):
        naf_amd.prepare_views(frame, [V(out=torch.empty(1, 3, 9, 7, device=dev))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        naf_amd.prepare_views(frame.cpu(), [V()])
    (ok,) = naf_amd.prepare_views(frame, [V()])                                                      # the device is still usable
    assert tuple(ok.shape) == (1, 3, 7, 9)
