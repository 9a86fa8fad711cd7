"""CPU side of the pooled-guidance training path: the fp64 restatements of tests/guidance_grad_reference.py equal fp64 torch autograd at
every shape the GPU tests use, the closed forms the kernels rely on hold exhaustively, and the two new C entries (naf_pool_guidance_bwd,
naf_preshrink_image_bwd) refuse bad arguments before any device work.  No kernel is launched here."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import guidance_grad_reference as R  # noqa: E402


def test_window_ranges_are_the_membership_test():
    """The closed form [floor(p * out / in), ceil((p + 1) * out / in) - 1] lists exactly the windows that hold p, for all extents below 40;
    when shrinking that is at most two, and exactly one when the output divides the input."""
    for n_in in range(1, 40):
        for n_out in range(1, 40):
            for p in range(n_in):
                member = [i for i in range(n_out) if R.pool_window(i, n_in, n_out)[0] <= p < R.pool_window(i, n_in, n_out)[1]]
                lo, hi = R.pool_windows_of(p, n_in, n_out)
                assert member == list(range(lo, hi + 1)), (n_in, n_out, p)
                if n_in >= n_out:
                    assert len(member) <= 2
                if n_in % n_out == 0:
                    assert len(member) == 1


@pytest.mark.parametrize("in_size,out_size,Cc", R.POOL_SHAPES)
def test_pool_restatement_is_autograd(in_size, out_size, Cc):
    g = torch.Generator().manual_seed(in_size[0] * 100 + out_size[1])
    x = torch.randn(R.POOL_BATCH, Cc, *in_size, dtype=torch.float64, generator=g, requires_grad=True)
    dy = torch.randn(R.POOL_BATCH, Cc, *out_size, dtype=torch.float64, generator=g)
    (ref,) = torch.autograd.grad(F.adaptive_avg_pool2d(x, out_size), x, dy)
    dx, n, mag = R.pool_adjoint(dy, in_size)
    assert float((dx - ref).abs().max()) <= 1e-12
    assert tuple(n.shape) == tuple(in_size) and int(n.min()) >= 1
    assert bool((mag >= dx.abs() - 1e-12).all())
    if in_size[0] >= out_size[0] and in_size[1] >= out_size[1]:
        assert int(n.max()) <= 4


def test_pool_shapes_exercise_the_grid_tail():
    """At least one shape leaves a partial last workgroup of 256 (input pixel, 8-channel chunk) threads."""
    assert any((R.POOL_BATCH * H * W * (Cc // 8)) % 256 for (H, W), _, Cc in R.POOL_SHAPES)


@pytest.mark.parametrize("case", sorted(R.RESIZE_CASES))
def test_resize_restatement_is_autograd(case):
    """fp32 weights against fp64 autograd: the coordinate rounding moves each axis weight by at most about extent * 2^-24 (a product of
    extent-sized numbers rounded to fp32, then a difference of them), the two axes multiply, and a tap that crosses an integer moves to the
    neighbouring pixel with a weight of that size: 4 * max(H, W) * 2^-24 times the |g| of the output pixels within one pixel of the element."""
    (B, H, W), (Hs, Ws) = R.RESIZE_CASES[case]
    g = torch.Generator().manual_seed(H * 100 + Ws)
    img = torch.randn(B, 3, H, W, dtype=torch.float64, generator=g, requires_grad=True)
    dout = torch.randn(B, 3, Hs, Ws, dtype=torch.float64, generator=g)
    (ref,) = torch.autograd.grad(F.interpolate(img, size=(Hs, Ws), mode="bilinear", align_corners=False), img, dout)
    d, T, mag, near = R.resize_adjoint(dout, (H, W))
    tol = 4 * max(H, W) * 2.0 ** -24 * near
    assert bool(((d - ref).abs() <= tol).all()), float(((d - ref).abs() - tol).max())
    assert bool((mag <= near + 1e-12).all())
    # the forward restated from the same taps is the forward
    Mh, Mw = R.bilinear_axis(H, Hs)[0], R.bilinear_axis(W, Ws)[0]
    fwd = torch.einsum("iy,bcyx,jx->bcij", Mh, img.detach(), Mw)
    assert float((fwd - F.interpolate(img.detach(), size=(Hs, Ws), mode="bilinear", align_corners=False)).abs().max()) < 1e-4


def test_resize_scan_covers_every_tap_when_shrinking():
    """naf_preshrink_image_bwd looks for the output rows of input row y among floor(y * Hs / H) - 2 .. + 2 with the forward's own expression as
    the predicate: for every Hs <= H < 200 each tap lies in that range, and a row receives from at most 3 output rows."""
    for n_in in range(1, 200):
        for n_out in range(1, n_in + 1):
            off = R.bilinear_scan_offsets(n_in, n_out)
            assert min(off) >= -2 and max(off) <= 2, (n_in, n_out, sorted(off))
            p0, p1, _, _ = R.bilinear_taps(n_in, n_out)
            rows = {}
            for o in range(n_out):
                rows.setdefault(int(p0[o]), set()).add(o)
                rows.setdefault(int(p1[o]), set()).add(o)
            assert max(len(v) for v in rows.values()) <= 3, (n_in, n_out)


def test_signatures_load(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    for name in ("naf_pool_guidance_bwd", "naf_preshrink_image_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    assert len(_lib.SIGNATURES["naf_pool_guidance_bwd"][1]) == 9 and len(_lib.SIGNATURES["naf_preshrink_image_bwd"][1]) == 10


def test_entries_reject_bad_arguments_without_a_device(built_lib):
    """NAF_ERR_INVALID (1) / NAF_ERR_UNSUPPORTED (2) with a message, before any device work: the pointers are never dereferenced."""
    from naf_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 256)()
    base = C.addressof(buf)
    a16 = (base + 15) // 16 * 16
    st = _lib.I64x4(3 * 8 * 8, 8 * 8, 8, 1)

    def err():
        return _lib.last_error()

    pool = lib.naf_pool_guidance_bwd
    assert pool(None, a16, 1, 8, 8, 4, 4, 16, None) == 1 and "naf_pool_guidance_bwd" in err() and "NULL" in err()
    assert pool(a16, None, 1, 8, 8, 4, 4, 16, None) == 1 and "NULL" in err()
    assert pool(a16, a16 + 64, 1, 8, 8, 4, 4, 12, None) == 1 and "C=12" in err()
    assert pool(a16, a16 + 64, 1, 8, 8, 0, 4, 16, None) == 1 and "non-positive" in err()
    assert pool(a16, a16 + 64, 0, 8, 8, 4, 4, 16, None) == 1 and "non-positive" in err()
    assert pool(a16 + 2, a16 + 64, 1, 8, 8, 4, 4, 16, None) == 1 and "aligned" in err()
    assert pool(a16, a16 + 66, 1, 8, 8, 4, 4, 16, None) == 1 and "aligned" in err()

    rs = lib.naf_preshrink_image_bwd
    assert rs(None, a16, _lib.NAF_F32, 1, 8, 8, 4, 4, C.byref(st), None) == 1 and "naf_preshrink_image_bwd" in err() and "NULL" in err()
    assert rs(a16, None, _lib.NAF_F32, 1, 8, 8, 4, 4, C.byref(st), None) == 1 and "NULL" in err()
    assert rs(a16, a16, _lib.NAF_F32, 1, 8, 8, 4, 4, None, None) == 1 and "NULL" in err()
    assert rs(a16, a16, 7, 1, 8, 8, 4, 4, C.byref(st), None) == 1 and "dtype" in err()
    assert rs(a16, a16, _lib.NAF_F32, 1, 8, 8, 0, 4, C.byref(st), None) == 1 and "non-positive" in err()
    assert rs(a16, a16, _lib.NAF_F32, 1, 8, 8, 9, 4, C.byref(st), None) == 2 and "shrinking" in err()
    assert rs(a16, a16, _lib.NAF_BF16, 1, 8, 8, 4, 9, C.byref(st), None) == 2 and err()


def test_ops_have_no_cpu_fallback(built_lib):
    from naf_amd import ops
    x = torch.zeros(1, 8, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    img = torch.zeros(1, 3, 8, 8)
    for req in (False, True):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.pool_guidance(x.clone().requires_grad_(req), (2, 2))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.preshrink_image(img.clone().requires_grad_(req), (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pool_guidance_bwd(x, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.preshrink_image_bwd(img, torch.zeros(1, 3, 16, 16))
