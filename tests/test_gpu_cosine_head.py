"""GPU tests (-m gpu) of the cosine head: naf_xna_cos_fwd / ``ops.xna_cos_forward`` / ``naf(image, feats, size, head=E, cosine=True)``
against the fp64 restatement of the definition and its derived per-element bounds (tests/cosine_reference.py: nothing measured), the
composition, and the exact properties of the kernel (scale invariance, zero features, rotate-on-load, repeatability, guard bands).

Every fused case first asserts that ``ops.xna_cos_select`` grants the fused kernel, so nothing is silently composed.

Module level: the budget is composed as test_gpu_head.py::test_module_head_matches_oracle_within_the_unfused_error composes its own --
the fused error against the oracle may be at most twice the error of the composition (the plain forward, normalised, times E^) against
the same reference, plus the bf16 rounding of the projected values carried through the division by the smallest norm.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_reference as R  # noqa: E402
import input_statistics as S  # noqa: E402
import layout_contract as L  # noqa: E402
from test_gpu_parity import bf16r, to5  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(name, logit_scale=1.0):
    """Inputs, the fp64 reference and its bounds: computed once per case and shared (never modified)."""
    B, heads, Dv, lr, cell, ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name)
    r = R.reference(q, k, v, E, ks, heads, logit_scale)
    return (q, k, v, E, ks, heads), r, R.bound(r), R.norms_bound(r)


def _operands(q, k, v, heads, dev):
    return to5(q, heads).to(dev), to5(k, heads).to(dev), to5(v, heads).to(dev)


def _granted(q5, v5, N, ks, tabs=None):
    from naf_amd import ops
    assert ops.xna_cos_select(q5, v5.shape[2:4], v5.shape[4], N, ks, rope_tables=tabs) == "fused", "the fused kernel was not granted"


@pytest.mark.parametrize("name", list(R.CASES))
def test_cosine_kernel_matches_the_definition(dev, name):
    """Per element: fused against the fp64 reference within the derived bound (cosines and norms), the composition within its own, fused
    against composed within the sum of the two."""
    from naf_amd import ops
    ls = 1.0 if name[0] in "abcdef" else 14.285714          # a CLIP-style temperature on half of the cases
    (q, k, v, E, ks, heads), r, bnd, nbnd = _case(name, ls)
    B, N = q.shape[0], E.shape[0]
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    Ed = E.to(dev)
    _granted(q5, v5, N, ks)
    cos, nrm = ops.xna_cos_forward(q5, k5, v5, Ed, ks, logit_scale=ls, return_norms=True, path="fused")
    assert cos.shape == (B, N, *q.shape[-2:]) and cos.dtype == torch.float32 and nrm.shape == (B, *q.shape[-2:]) and nrm.dtype == torch.float32
    assert cos.permute(0, 2, 3, 1).is_contiguous() and not cos.requires_grad
    auto = ops.xna_cos_forward(q5, k5, v5, Ed, ks, logit_scale=ls)
    assert torch.equal(auto, cos)                                    # "auto" is the kernel here, and norms are optional
    R.check(cos.cpu(), r["cos"], bnd, f"fused {name}")
    R.check(nrm.cpu(), r["norms"], nbnd, f"fused norms {name}")
    ccos, cnrm = ops.xna_cos_forward(q5, k5, v5, Ed, ks, logit_scale=ls, return_norms=True, path="composed")
    cb, cnb = R.composed_bound(r)
    R.check(ccos.cpu(), r["cos"], cb, f"composed {name}")
    R.check(cnrm.cpu(), r["norms"], cnb, f"composed norms {name}")
    R.check(cos.cpu(), ccos.cpu().double(), bnd + cb, f"fused vs composed {name}")


def test_constant_features_give_the_cosine_of_the_embedding(dev):
    """Every low-res cell holds the same vector v: cos[n, p] = cos(E_n, v) at every pixel, whatever the attention weights; held to the
    reference file's bound, which on this input is the PV rounding (the weights' bf16 sum cancels in the ratio up to the feature term)."""
    from naf_amd import ops
    name = "a_c128_k7_n21"
    B, heads, Dv, lr, cell, ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name, const_v=True)
    r = R.reference(q, k, v, E, ks, heads)
    v0 = v[0, :, 0, 0].double()
    want = (F.normalize(E.float(), dim=1).double() @ v0) / v0.norm()
    assert float((r["cos"] - want.view(1, N, 1, 1)).abs().max()) <= 1e-12
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    _granted(q5, v5, N, ks)
    cos = ops.xna_cos_forward(q5, k5, v5, E.to(dev), ks, path="fused").cpu()
    R.check(cos, r["cos"], R.bound(r), "constant features")


@pytest.mark.parametrize("name", ["a_c128_k7_n21", "c_dv192_n151", "e_patch14_n21"])
def test_power_of_two_scale_changes_no_bit(dev, name):
    """cos(feats) == cos(4 feats) and norms(4 feats) == 4 norms(feats), bit for bit: a power of two changes no mantissa on the path."""
    from naf_amd import ops
    (q, k, v, E, ks, heads), _, _, _ = _case(name, 1.0 if name[0] in "abcdef" else 14.285714)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    _granted(q5, v5, E.shape[0], ks)
    Ed = E.to(dev)
    c1, n1 = ops.xna_cos_forward(q5, k5, v5, Ed, ks, return_norms=True, path="fused")
    c4, n4 = ops.xna_cos_forward(q5, k5, v5 * 4, Ed, ks, return_norms=True, path="fused")
    assert torch.equal(c1, c4)
    assert torch.equal(n4, n1 * 4)
    c8, n8 = ops.xna_cos_forward(q5, k5, v5 * 0.125, Ed, ks, return_norms=True, path="fused")
    assert torch.equal(c1, c8) and torch.equal(n8, n1 * 0.125)


def test_zero_features_give_exact_zeros(dev):
    """A block of zero features wider than the window: cos == 0 exactly and norms == 0 at the pixels that see only zeros, all finite."""
    from naf_amd import ops
    name = "e_patch14_n21"
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    blk = (0, 6, 0, 6)
    q, k, v, E = R.make_inputs(name, zero_block=blk)
    m = R.sees_only(blk, h, w, ks).repeat_interleave(dy, 0).repeat_interleave(dx, 1)
    assert int(m.sum()) >= 2 * dy * dx
    r = R.reference(q, k, v, E, ks, heads, 20.0)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    _granted(q5, v5, N, ks)
    cos, nrm = ops.xna_cos_forward(q5, k5, v5, E.to(dev), ks, logit_scale=20.0, return_norms=True, path="fused")
    cos, nrm = cos.cpu(), nrm.cpu()
    assert bool(torch.isfinite(cos).all()) and bool(torch.isfinite(nrm).all())
    assert float(cos[:, :, m].abs().max()) == 0.0 and float(nrm[:, m].max()) == 0.0
    R.check(cos, r["cos"], R.bound(r), "zero block")
    # all features zero: every pixel is zero
    z, zn = ops.xna_cos_forward(q5, k5, torch.zeros_like(v5), E.to(dev), ks, return_norms=True, path="fused")
    assert float(z.abs().max()) == 0.0 and float(zn.abs().max()) == 0.0


@pytest.mark.parametrize("B,heads,Dv,lr,out_sz,ksz,N", [
    (1, 4, 32, (8, 8), (128, 128), 7, 21),        # d = 16: one row tile per cell row
    (2, 4, 96, (6, 5), (96, 160), 5, 151),        # d = 32: two tiles per cell row; a whole and a half value chunk
    (1, 3, 64, (6, 7), (84, 98), 5, 1),           # patch 14: partial row tiles
])
def test_rotate_on_load_equals_materialised_queries(dev, B, heads, Dv, lr, out_sz, ksz, N):
    """naf_xna_cos_fwd(rope_tab_*) on un-rotated guidance == naf_rope_pool_fwd queries + naf_xna_cos_fwd, bit for bit."""
    from naf_amd import ops
    x = bf16r(O.hash_normal((B, heads * 64, *out_sz), 710))
    v = bf16r(O.hash_normal((B, heads * Dv, *lr), 711))
    E = O.hash_normal((N, heads * Dv), 712).to(dev)
    per = O.rope_periods(heads * 64, heads, 100.0)
    xd = x.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ty, tx = ops.rope_tables(per.to(dev), *out_sz)
    q_mat, k5 = ops.rope_pool(xd, ty, tx, heads, lr)
    q_raw = xd.permute(0, 2, 3, 1).unflatten(3, (heads, 64)).permute(0, 3, 1, 2, 4)
    v5 = to5(v, heads).to(dev)
    _granted(q_raw, v5, N, ksz, (ty, tx))
    a, an = ops.xna_cos_forward(q_mat, k5, v5, E, ksz, return_norms=True, path="fused")
    b, bn = ops.xna_cos_forward(q_raw, k5, v5, E, ksz, return_norms=True, path="fused", rope_tables=(ty, tx))
    assert torch.equal(a, b) and torch.equal(an, bn)
    # and both are the definition on the rotated queries / pooled keys the kernels read
    qr, kr = q_mat.float().cpu().permute(0, 1, 4, 2, 3).reshape(B, heads * 64, *out_sz), k5.float().cpu().permute(0, 1, 4, 2, 3).reshape(B, heads * 64, *lr)
    r = R.reference(qr, kr, v, E.cpu(), ksz, heads)
    R.check(b.cpu(), r["cos"], R.bound(r), "rotate-on-load vs the definition")


def test_two_launches_give_the_same_bits_and_guard_bands_stay(dev):
    """The C entry on caller-owned buffers: `out` as a channel slice of a wider row (x stride N + 5) and `norms`, both inside sentinel
    guard bands.  Nothing but the elements of the two outputs is written; a second launch gives the same bits."""
    from naf_amd import _lib, ops
    name = "e_patch14_n21"          # partial row tiles: the masked lanes must store nothing
    (q, k, v, E, ks, heads), r, bnd, nbnd = _case(name)
    B, N, (Ho, Wo) = q.shape[0], E.shape[0], q.shape[-2:]
    Dv = v.shape[1] // heads
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    _granted(q5, v5, N, ks)
    eh = ops.normalize_embeddings(E.to(dev))
    pv5 = F.pad(torch.einsum("ngd,bghwd->bghwn", eh.reshape(N, heads, Dv), v5.float()), (0, ops.head_npad(N) - N)).to(torch.bfloat16)
    lib = _lib.load()
    results = []
    for _ in range(2):
        wide, arena, inside = L.banded((B, Ho, Wo, N + 5), torch.float32, dev)
        nrm, narena, ninside = L.banded((B, Ho, Wo), torch.float32, dev)
        out = wide[..., 2:2 + N]
        before, nbefore, wbefore = arena.clone(), narena.clone(), wide.clone()
        a = ops._fill_xna_cos(q5, k5, pv5, v5, out, nrm, N, ks, ks, "fused", None, 1.0)
        assert lib.naf_xna_cos_select(C.byref(a)) == _lib.XNA_HEAD_FUSED
        _lib.check(lib.naf_xna_cos_fwd(C.byref(a), ops._stream(q5)), "naf_xna_cos_fwd")
        torch.cuda.synchronize()
        assert L.untouched(arena, before, inside) and L.untouched(narena, nbefore, ninside)
        assert torch.equal(L.bits(wide[..., :2]), L.bits(wbefore[..., :2])) and torch.equal(L.bits(wide[..., 2 + N:]), L.bits(wbefore[..., 2 + N:]))
        assert not bool((L.bits(out) == L.sentinel(torch.float32)).any()) and not bool((L.bits(nrm) == L.sentinel(torch.float32)).any())
        results.append((out.clone(), nrm.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    R.check(results[0][0].permute(0, 3, 1, 2).cpu(), r["cos"], bnd, "strided out")
    # norms = NULL: the same cosines
    out2 = torch.empty((B, Ho, Wo, N), dtype=torch.float32, device=dev)
    a = ops._fill_xna_cos(q5, k5, pv5, v5, out2, None, N, ks, ks, "fused", None, 1.0)
    _lib.check(lib.naf_xna_cos_fwd(C.byref(a), ops._stream(q5)), "naf_xna_cos_fwd")
    assert torch.equal(out2, results[0][0])


def test_ops_routes_and_refusals(dev):
    from naf_amd import ops
    from naf_amd._lib import NafHipError
    (q, k, v, E, ks, heads), r, bnd, _ = _case("a_c128_k7_n21")
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    Eg = E.to(dev).requires_grad_(True)
    # a gradient for the embeddings: "auto" composes (differentiable), "fused" refuses
    c = ops.xna_cos_forward(q5, k5, v5, Eg, ks)
    assert c.requires_grad
    c.square().sum().backward()
    assert Eg.grad is not None and bool(torch.isfinite(Eg.grad).all()) and float(Eg.grad.abs().sum()) > 0
    with pytest.raises(NafHipError, match="inference-only"):
        ops.xna_cos_forward(q5, k5, v5, Eg, ks, path="fused")
    with torch.no_grad():
        assert not ops.xna_cos_forward(q5, k5, v5, Eg, ks, path="fused").requires_grad
    # windows 13 / 15 with more than 64 embeddings, and 257 embeddings: composed under "auto", refused under "fused"
    name = "j_k13_n21"
    (q, k, v, E, ks, heads), _, _, _ = _case(name)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    E151 = O.hash_normal((151, v.shape[1]), 77).to(dev)
    assert ops.xna_cos_select(q5, v5.shape[2:4], v5.shape[4], 151, ks) == "composed"
    with pytest.raises(NafHipError, match="window 13"):
        ops.xna_cos_forward(q5, k5, v5, E151, ks, path="fused")
    r151 = R.reference(q, k, v, E151.cpu(), ks, heads)
    R.check(ops.xna_cos_forward(q5, k5, v5, E151, ks).cpu(), r151["cos"], R.composed_bound(r151)[0], "window 13, N = 151 (composed)")
    with pytest.raises(ValueError, match="do not match"):
        ops.xna_cos_forward(q5, k5, v5, E151[:, :-1], ks)


# ---- module level -----------------------------------------------------------------------------------------------
def _load_model(dev, params, **kw):
    from naf_amd import NAF
    m = NAF(**kw).eval()
    m.load_state_dict(params, strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def module_case(dev):
    """lr 14 x 14 -> 224 x 224, C 384, window 9, N 21, bf16 features: model, inputs, the oracle's forward and the fp64 cosine on it."""
    size, lr, Cc, ksz, N = (224, 224), (14, 14), 384, 9, 21
    p = O.make_params(seed=31)
    m = _load_model(dev, p, kernel_size=ksz)
    img = O.hash_normal((1, 3, *size), 801)
    ft = bf16r(O.hash_normal((1, Cc, *lr), 802))
    E = O.hash_normal((N, Cc), 803)
    up = O.naf_forward(p, img, ft, size, kernel_size=ksz)
    cos, nrm = R.cosine_from_features64(up, E)
    return m, img.to(dev), ft.to(dev).to(torch.bfloat16), E.to(dev), up, cos, nrm, size, N


def test_module_cosine_matches_oracle_within_the_composed_error(dev, module_case):
    from naf_amd import ops
    m, img, ft, E, up, ref, ref_n, size, N = module_case
    heads, Cc, lr = m.upsampler.num_heads, ft.shape[1], ft.shape[-2:]
    with torch.no_grad():
        probe = torch.empty((1, *size, heads, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
        assert ops.xna_cos_select(probe, lr, Cc // heads, N, 9) == "fused"
        fused = m(img, ft, size, head=E, cosine=True)
        assert torch.equal(m(img, ft, size, head=E, cosine=True, cosine_path="fused"), fused)
        comp = m(img, ft, size, head=E, cosine=True, cosine_path="composed")
        plain = m(img, ft, size)
    assert fused.shape == (1, N, *size) and fused.dtype == torch.float32 and not fused.requires_grad
    assert fused.stride() == (size[0] * size[1] * N, 1, size[1] * N, N)
    assert torch.equal(comp, ops.cosine_from_features(plain, ops.normalize_embeddings(E)))      # "composed" IS the definition on the plain forward
    e_f, e_u = (fused.cpu().double() - ref).abs(), (comp.cpu().double() - ref).abs()
    # bf16 rounding of PV: PV_g[n, cell] moves by at most 2^-8 |PV_g[n, cell]|, the attention is a convex combination per head, and the
    # sum is divided by the pixel's norm: at most 2^-8 * sum_g max |PV_g[n]| / min ||f||
    eh = F.normalize(E.float().cpu(), dim=1)
    pvf = torch.einsum("ngd,bgdhw->bgnhw", eh.reshape(N, heads, Cc // heads), ft.float().cpu().reshape(1, heads, Cc // heads, *lr))
    pv_round = 2.0 ** -8 * float(pvf.abs().amax(dim=(0, 3, 4)).sum(0).max()) / float(ref_n.min())
    print(f"module cosine: fused max err {float(e_f.max()):.4e} mean {float(e_f.mean()):.4e}; composed max err {float(e_u.max()):.4e} "
          f"mean {float(e_u.mean()):.4e}; PV rounding bound {pv_round:.4e}")
    assert float(e_f.max()) <= 2.0 * float(e_u.max()) + pv_round
    assert float(e_f.mean()) <= 2.0 * float(e_u.mean()) + pv_round
    # forms of the head, logit_scale, the Guidance call
    with torch.no_grad():
        lin = nn.Linear(Cc, N, bias=False).to(dev)
        lin.weight.copy_(E)
        conv = nn.Conv2d(Cc, N, 1, bias=False).to(dev)
        conv.weight.copy_(E[:, :, None, None])
        assert torch.equal(m(img, ft, size, head=lin, cosine=True), fused) and torch.equal(m(img, ft, size, head=conv, cosine=True), fused)
        assert torch.equal(m(img, ft, size, head=(E.double(), None), cosine=True), fused)
        g = m.guide(img)
        assert torch.equal(m(g, ft, size, head=E, cosine=True), fused)
        s16 = m(img, ft, size, head=E, cosine=True, logit_scale=16.0)
        assert torch.equal(s16, fused * 16.0)               # a power of two: exact
        z = m(img[:0], ft[:0], size, head=E, cosine=True, return_norms=True)
    assert z[0].shape == (0, N, *size) and z[1].shape == (0, *size)


def test_module_norms_labels_and_confusion(dev, module_case):
    from naf_amd import ops
    m, img, ft, E, up, ref, ref_n, size, N = module_case
    with torch.no_grad():
        cos, nrm = m(img, ft, size, head=E, cosine=True, return_norms=True)
        assert torch.equal(cos, m(img, ft, size, head=E, cosine=True))
        plain = m(img, ft, size)
        # sum_j P_j |v_j| from the plain forward on |features| (the weights do not depend on the values), its own bf16 store allowed for
        a_f = m(img, ft.abs(), size).float().cpu().double() * (1.0 + 2.0 ** -7)
    pn = plain.float().norm(dim=1).cpu().double()
    d_fused = S.bf16_bound(1, a_f).pow(2).sum(1).sqrt()                                    # the implied feature: no store term
    d_plain = S.bf16_bound(1, a_f, plain.float().cpu().double().abs()).pow(2).sum(1).sqrt()   # the plain forward: one bf16 store
    Cc = ft.shape[1]
    R.check(nrm.cpu(), pn, d_fused + d_plain + (Cc + 4) * R.F32 * pn, "return_norms vs naf(...).float().norm(dim=1)")
    # labels and confusion: the existing launches on the normalised rows
    eh = F.normalize(E.float(), dim=1)
    tgt = (torch.arange(size[0] * size[1], device=dev).view(1, *size) * 7 % (N + 2)).long()
    tgt[tgt >= N] = 255
    with torch.no_grad():
        lab = m(img, ft, size, head=E, cosine=True, predict=True)
        assert torch.equal(lab, m(img, ft, size, head=(eh, None), predict=True))
        assert torch.equal(lab, m(img, ft, size, head=E, cosine=True, predict=True, logit_scale=50.0))
        cm = m(img, ft, size, head=E, cosine=True, target=tgt, ignore_index=255, confusion=True)
        assert torch.equal(cm, m(img, ft, size, head=(eh, None), target=tgt, ignore_index=255, confusion=True))
        cm2, lab2 = m(img, ft, size, head=E, cosine=True, target=tgt, ignore_index=255, confusion=True, predict=True)
        assert torch.equal(cm2, cm) and torch.equal(lab2, lab)
    # the labels are the argmax of the cosines wherever the top-2 margin exceeds the two rounding paths' bounds: nearly everywhere
    agree = float((cos.argmax(1) == lab).float().mean())
    assert agree >= 0.99, agree


def test_module_auto_composes_what_the_kernel_does_not_serve(dev):
    """A non-integer ratio (28^2 -> 64^2) and fp16 / fp32 features select the composition -- asserted -- and match the reference; "fused"
    raises NafHipError with the reason; a gradient for E takes the composition and reaches E."""
    from naf_amd import ops
    from naf_amd._lib import NafHipError
    p = O.make_params(seed=32)
    m = _load_model(dev, p, kernel_size=7)
    heads = m.upsampler.num_heads
    N, Cc = 21, 128
    E = O.hash_normal((N, Cc), 813)
    img = O.hash_normal((1, 3, 64, 64), 811)
    ft = bf16r(O.hash_normal((1, Cc, 28, 28), 812))
    probe = torch.empty((1, 64, 64, heads, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    assert ops.xna_cos_select(probe, (28, 28), Cc // heads, N, 7) == "composed"
    ref, _ = R.cosine_from_features64(O.naf_forward(p, img, ft, (64, 64), kernel_size=7), E)
    imgd, ftd, Ed = img.to(dev), ft.to(dev).to(torch.bfloat16), E.to(dev)
    with torch.no_grad():
        auto = m(imgd, ftd, (64, 64), head=Ed, cosine=True)
        comp = m(imgd, ftd, (64, 64), head=Ed, cosine=True, cosine_path="composed")
        plain = m(imgd, ftd, (64, 64))
    assert torch.equal(auto, comp) and torch.equal(auto, ops.cosine_from_features(plain, ops.normalize_embeddings(Ed)))
    # the composition's error is the plain forward's (2e-2 + 1e-2 |ref| per feature element) carried through the normalisation:
    # |d cos| <= (|E^| . |d f| + |cos| ||d f||) / ||f|| <= 2 ||d f|| / ||f||
    up = O.naf_forward(p, img, ft, (64, 64), kernel_size=7)
    df = (2e-2 + 1e-2 * up.abs()).norm(dim=1)
    R.check(auto.cpu(), ref, (2.0 * df / up.norm(dim=1)).unsqueeze(1).double().expand_as(ref), "non-integer ratio (composed)")
    with pytest.raises(NafHipError, match="integer ratio"):
        m(imgd, ftd, (64, 64), head=Ed, cosine=True, cosine_path="fused")
    # fp16 / fp32 features on a geometry the kernel serves for bf16
    img2 = O.hash_normal((1, 3, 128, 128), 814).to(dev)
    ft2 = bf16r(O.hash_normal((1, Cc, 8, 8), 815)).to(dev)
    with torch.no_grad():
        b16 = m(img2, ft2.to(torch.bfloat16), (128, 128), head=Ed, cosine=True, cosine_path="fused")
        for dt in (torch.float16, torch.float32):
            a = m(img2, ft2.to(dt), (128, 128), head=Ed, cosine=True)
            assert torch.equal(a, ops.cosine_from_features(m(img2, ft2.to(dt), (128, 128)), ops.normalize_embeddings(Ed)))
            assert float((a - b16).abs().max()) <= 0.05           # the same quantity through another rounding path
            with pytest.raises(NafHipError, match="bfloat16 features"):
                m(img2, ft2.to(dt), (128, 128), head=Ed, cosine=True, cosine_path="fused")
    # a gradient for E: composed and differentiable under "auto", refused under "fused"
    Eg = Ed.clone().requires_grad_(True)
    out = m(img2, ft2.to(torch.bfloat16), (128, 128), head=Eg, cosine=True)
    assert out.requires_grad
    out.square().mean().backward()
    assert Eg.grad is not None and float(Eg.grad.abs().sum()) > 0
    with pytest.raises(NafHipError, match="inference-only"):
        m(img2, ft2.to(torch.bfloat16), (128, 128), head=Eg, cosine=True, cosine_path="fused")


def test_module_refusals_come_before_any_launch(dev, module_case):
    """Every ValueError / NafHipError of the call is raised with no kernel launched: the library's launch timer (which brackets the
    stem, the RoPE pass and the attention) sees nothing until a call that runs."""
    from naf_amd import ops
    from naf_amd._lib import NafHipError
    m, img, ft, E, up, ref, ref_n, size, N = module_case
    tgt = torch.zeros((1, *size), dtype=torch.long, device=dev)
    class Spy:
        def __init__(self):
            self.names = []

        def start(self, name):
            self.names.append(name)

        def stop(self, name):
            pass

    old, spy = ops.KERNEL_TIMER, Spy()
    ops.KERNEL_TIMER = spy
    try:
        for exc, kw in ((ValueError, dict(head=nn.Conv2d(384, N, 1).to(dev))), (ValueError, dict(target=tgt)), (ValueError, dict(regress=up.to(dev))),
                        (ValueError, dict(return_weights=True)), (ValueError, dict(cosine_path="x")), (ValueError, dict(head=E[:, :-1])),
                        (NafHipError, dict(cosine_path="fused", output_size=(100, 100))), (NafHipError, dict(cosine_path="fused", features=ft.float())),
                        (NafHipError, dict(cosine_path="fused", head=E.clone().requires_grad_(True)))):
            kw = dict(kw)
            args = (img, kw.pop("features", ft), kw.pop("output_size", size))
            with pytest.raises(exc):
                m(*args, **{"head": E, "cosine": True, **kw})
        refused = list(spy.names)
        with torch.no_grad():
            m(img, ft, size, head=E, cosine=True)          # the spy does see a call that runs
        ran = list(spy.names)
    finally:
        ops.KERNEL_TIMER = old
    assert refused == [], f"a refused call launched something: {refused}"
    assert "stem" in ran and "xna_cos" in ran, ran
