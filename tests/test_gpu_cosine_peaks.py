"""GPU tests (-m gpu) of the peak search: naf_xna_cos_peaks_fwd / ``ops.xna_cos_peaks``, naf_peaks_topk / ``ops.peaks_topk``, ``naf.locate``
and ``naf.match``.

The arithmetic is the cosine kernel's, so the first yardstick is exact: the definition (tests/cosine_peak_reference.py) applied to what
``ops.xna_cos_forward(path="fused")`` stores for the same inputs, ``torch.equal``.  Against the fp64 reference the maximum is 1-Lipschitz:
the derived per-element bound of tests/cosine_reference.py carries over to the cell maxima, and the reported pixel is optimal within two
bounds (cosine_peak_reference.check_against_fp64).  Nothing is measured.  Every fused case first asserts that the kernel was granted."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_peak_reference as P  # noqa: E402
import cosine_reference as R  # noqa: E402
import layout_contract as L  # noqa: E402
from test_gpu_cosine_head import _case, _load_model, _operands  # noqa: E402  (the shared, cached fp64 references)
from test_gpu_parity import bf16r, to5  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ("a_c128_k7_n21", "b_whole_grid_n1", "c_dv192_n151", "d_dv256_n256", "e_patch14_n21", "f_rows30_n151", "j_k13_n21", "k_k15_n40",
         "l_two_rounds_n21")
SCALES = (14.285714, -3.0)       # a CLIP-style temperature, and a negative scale: the maximum is then the LEAST similar pixel


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _granted(q5, v5, N, ks, tabs=None):
    from naf_amd import ops
    assert ops.xna_cos_peaks_select(q5, v5.shape[2:4], v5.shape[4], N, ks, rope_tables=tabs) == "fused", "the fused kernel was not granted"


def _first_pixels(h, w, dy, dx):
    """[h, w] int32: the flat index of every cell's first pixel."""
    return ((torch.arange(h) * dy).view(h, 1) * (w * dx) + (torch.arange(w) * dx).view(1, w)).to(torch.int32)


# ---- 1. exact against the project's own cosine kernel -------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_peaks_are_the_definition_on_the_cosine_kernels_output(dev, name):
    from naf_amd import ops
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    Ed = E.to(dev)
    _granted(q5, v5, N, ks)
    for ls in SCALES:
        cos = ops.xna_cos_forward(q5, k5, v5, Ed, ks, logit_scale=ls, path="fused")
        want_p, want_w = P.cell_peaks(cos, h, w)
        peak, where, none = ops.xna_cos_peaks(q5, k5, v5, Ed, ks, logit_scale=ls, path="fused")
        assert none is None and peak.shape == where.shape == (B, N, h, w) and peak.dtype == torch.float32 and where.dtype == torch.int32
        assert peak.permute(0, 2, 3, 1).is_contiguous() and where.permute(0, 2, 3, 1).is_contiguous()
        assert torch.equal(peak, want_p), f"{name} scale {ls}: {int((peak != want_p).sum())} peaks differ"
        assert torch.equal(where, want_w), f"{name} scale {ls}: {int((where != want_w).sum())} indices differ"
        p2, w2, c2 = ops.xna_cos_peaks(q5, k5, v5, Ed, ks, logit_scale=ls, want_cos=True, path="fused")
        assert torch.equal(c2, cos) and torch.equal(p2, peak) and torch.equal(w2, where)
        auto = ops.xna_cos_peaks(q5, k5, v5, Ed, ks, logit_scale=ls)
        assert torch.equal(auto[0], peak) and torch.equal(auto[1], where)          # "auto" is the kernel here
        # the composition has its own arithmetic for the cosines, and the same definition on them
        cp, cw, cc = ops.xna_cos_peaks(q5, k5, v5, Ed, ks, logit_scale=ls, want_cos=True, path="composed")
        dp, dw = P.cell_peaks(cc, h, w)
        assert torch.equal(cp, dp) and torch.equal(cw, dw) and cp.permute(0, 2, 3, 1).is_contiguous()


# ---- 2. ties, exactly -----------------------------------------------------------------------------------------------
def test_all_zero_features_tie_to_each_cells_first_pixel(dev):
    from naf_amd import ops
    name = "a_c128_k7_n21"
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    _granted(q5, v5, N, ks)
    peak, where, _ = ops.xna_cos_peaks(q5, k5, torch.zeros_like(v5), E.to(dev), ks, logit_scale=5.0, path="fused")
    first = _first_pixels(h, w, dy, dx).to(dev)
    assert float(peak.abs().max()) == 0.0 and torch.equal(where, first.expand(B, N, h, w))
    vals, idx = ops.peaks_topk(peak, where, h * w)
    assert float(vals.abs().max()) == 0.0
    assert torch.equal(idx, first.reshape(-1).sort().values.expand(B, N, h * w))      # the cells by their first pixels' flat indices


def test_zero_block_ties_on_exactly_the_cells_that_see_only_zeros(dev):
    from naf_amd import ops
    name = "e_patch14_n21"
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    blk = (0, 6, 0, 6)
    q, k, v, E = R.make_inputs(name, zero_block=blk)
    m = R.sees_only(blk, h, w, ks)
    assert int(m.sum()) >= 2 and int((~m).sum()) >= 2
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    _granted(q5, v5, N, ks)
    peak, where, cos = ops.xna_cos_peaks(q5, k5, v5, E.to(dev), ks, logit_scale=20.0, want_cos=True, path="fused")
    peak, where = peak.cpu(), where.cpu()
    first = _first_pixels(h, w, dy, dx)
    assert float(peak[:, :, m].abs().max()) == 0.0 and torch.equal(where[:, :, m], first[m].expand(B, N, -1))
    assert bool((cos.cpu().reshape(B, N, h, dy, w, dx).abs().amax(dim=(3, 5))[:, :, ~m] > 0).all())     # and on no other cell
    want_p, want_w = P.cell_peaks(cos.cpu(), h, w)
    assert torch.equal(peak, want_p) and torch.equal(where, want_w)


def test_identical_embeddings_give_identical_rows(dev):
    from naf_amd import ops
    name = "f_rows30_n151"
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name)
    E = E.clone()
    E[150] = E[3]          # channel 3 (tile 0) and channel 150 (tile 9, the last stored one)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    peak, where, _ = ops.xna_cos_peaks(q5, k5, v5, E.to(dev), ks, logit_scale=-2.0, path="fused")
    assert torch.equal(peak[:, 3], peak[:, 150]) and torch.equal(where[:, 3], where[:, 150])
    assert not torch.equal(peak[:, 3], peak[:, 4])


# ---- 3. against the fp64 definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_peaks_against_the_fp64_reference(dev, name):
    from naf_amd import ops
    ls = 1.0 if name[0] in "abcdef" else 14.285714          # the scales test_gpu_cosine_head.py computed its references for
    (q, k, v, E, ks, heads), r, bnd, _ = _case(name, ls)
    h, w = v.shape[-2:]
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    _granted(q5, v5, E.shape[0], ks)
    peak, where, _ = ops.xna_cos_peaks(q5, k5, v5, E.to(dev), ks, logit_scale=ls, path="fused")
    P.check_against_fp64(peak.cpu(), where.cpu(), r["cos"], bnd, h, w, f"peaks {name}")


def test_peaks_against_the_fp64_reference_negative_scale(dev):
    from naf_amd import ops
    name = "b_whole_grid_n1"
    B, heads, Dv, (h, w), cell, ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name)
    r = R.reference(q, k, v, E, ks, heads, -2.5)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    peak, where, _ = ops.xna_cos_peaks(q5, k5, v5, E.to(dev), ks, logit_scale=-2.5, path="fused")
    P.check_against_fp64(peak.cpu(), where.cpu(), r["cos"], R.bound(r), h, w, "peaks, negative scale")


# ---- 4. the layout contract ---------------------------------------------------------------------------------------------
def _peaks_launch(q, k, pv, v, out, peak, where, N, ks, ls):
    """naf_xna_cos_peaks_fwd on the caller's buffers: ``out`` [B, Ho, Wo, N] or None, ``peak`` / ``where`` [B, h, w, N] by strides {b, cy, cx}."""
    from naf_amd import _lib, ops
    a = _lib.XnaCosPeaksArgs()
    a.cos = ops._fill_xna_cos(q, k, pv, v, out if out is not None else q, None, N, ks, ks, "fused", None, ls)
    if out is None:
        a.cos.out, a.cos.o_stride = None, ops.I64x3(0, 0, 0)
    a.peak, a.where = peak.data_ptr(), where.data_ptr()
    a.peak_stride, a.where_stride = ops._strides3(peak), ops._strides3(where)
    lib = _lib.load()
    assert lib.naf_xna_cos_peaks_select(C.byref(a)) == _lib.XNA_HEAD_FUSED, _lib.last_error()
    with torch.cuda.device(q.device):
        rc = lib.naf_xna_cos_peaks_fwd(C.byref(a), ops._stream(q))
    _lib.check(rc, "naf_xna_cos_peaks_fwd")


@pytest.mark.parametrize("gname", list(L.COS_GEOMS))
def test_strided_operands_and_guard_bands(dev, gname):
    """Inputs in the strides of tests/layout_contract.py's cosine cases, outputs as strided views inside sentinel-filled arenas (a NaN
    pattern for fp32, a marker integer for int32): the result is the dense one, nothing outside the views changes -- the channels past N
    of a padded pixel included, they lie outside the view --, and a second launch gives the same bits."""
    from naf_amd import ops
    B, heads, Dv, (h, w), (dy, dx), ks, N = L.COS_GEOMS[gname]
    ls = L.COS_SCALE[gname]
    q, k, v, E = L.cos_inputs(gname)
    q5, k5, v5 = to5(q, heads).to(dev), to5(k, heads).to(dev), to5(v, heads).to(dev)
    Ed = E.to(dev)
    _granted(q5, v5, N, ks)
    ref_p, ref_w, ref_c = ops.xna_cos_peaks(q5, k5, v5, Ed, ks, logit_scale=ls, want_cos=True, path="fused")
    e_hat = ops.normalize_embeddings(Ed)
    pv = torch.einsum("ngd,bghwd->bghwn", e_hat.reshape(N, heads, Dv), v5.float())
    pv5 = F.pad(pv, (0, ops.head_npad(N) - N)).to(torch.bfloat16)
    Ho, Wo = h * dy, w * dx
    for fam_in, fam_out, with_out in (("crop", "pixel_gap", True), ("pixel_gap", "crop", False), ("head_gap", "row_gap", True)):
        ins = [L.embed(t, fam_in)[0] for t in (q5, k5, pv5, v5)]
        po, pa, pm = L.arena_for((B, 1, h, w, N), torch.float32, fam_out, dev)
        wo_, wa, wm = L.arena_for((B, 1, h, w, N), torch.int32, fam_out, dev)
        oo, oa, om = L.arena_for((B, 1, Ho, Wo, N), torch.float32, fam_out, dev) if with_out else (None, None, None)
        before = [t.clone() for t in (pa, wa)] + ([oa.clone()] if with_out else [])
        _peaks_launch(*ins, L.hw3(oo) if with_out else None, L.hw3(po), L.hw3(wo_), N, ks, ls)
        torch.cuda.synchronize()
        assert L.untouched(pa, before[0], pm) and L.untouched(wa, before[1], wm), f"{gname} {fam_out}: a write outside peak / where"
        assert L.same_bits(L.hw3(po).permute(0, 3, 1, 2), ref_p) and torch.equal(L.hw3(wo_).permute(0, 3, 1, 2), ref_w), f"{gname} {fam_in}/{fam_out}"
        if with_out:
            assert L.untouched(oa, before[2], om) and L.same_bits(L.hw3(oo).permute(0, 3, 1, 2), ref_c)
        first = [pa.clone(), wa.clone()]
        _peaks_launch(*ins, L.hw3(oo) if with_out else None, L.hw3(po), L.hw3(wo_), N, ks, ls)
        torch.cuda.synchronize()
        assert L.unchanged(pa, first[0]) and L.unchanged(wa, first[1]), f"{gname}: two launches differ"


# ---- 5. peaks_topk ----------------------------------------------------------------------------------------------------------
def test_topk_on_the_kernels_outputs(dev):
    from naf_amd import ops
    name = "a_c128_k7_n21"
    B, heads, Dv, (h, w), cell, ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    peak, where, cos = ops.xna_cos_peaks(q5, k5, v5, E.to(dev), ks, want_cos=True, path="fused")
    for kk in (1, 5, h * w):
        vals, idx = ops.peaks_topk(peak, where, kk)
        rv, ri = P.topk_reference(peak.cpu(), where.cpu(), kk)
        assert vals.shape == idx.shape == (B, N, kk) and idx.dtype == torch.int32
        assert torch.equal(vals.cpu(), rv) and torch.equal(idx.cpu(), ri)
    # k = 1: the global maximum of the map, the lowest flat index among ties
    flat = cos.reshape(B, N, -1)
    gmax = flat.amax(dim=2)
    n_px = flat.shape[2]
    gidx = torch.where(flat == gmax[:, :, None], torch.arange(n_px, device=dev), n_px).amin(dim=2)
    v1, i1 = ops.peaks_topk(peak, where, 1)
    assert torch.equal(v1[:, :, 0], gmax) and torch.equal(i1[:, :, 0].long(), gidx)


@pytest.mark.parametrize("h,w,ks_", [(5, 7, (1, 5, 35)), (9, 11, (1, 5, 64))])
def test_topk_on_integer_maps_with_many_ties(dev, h, w, ks_):
    """Integer-valued maps of three levels (a third of the cells tie at each), h * w not a multiple of 64, the flat indices a permutation
    that is not the order of the cells; dense [B, N, h, w] tensors and channels-last views are read alike."""
    from naf_amd import ops
    g = torch.Generator().manual_seed(h * w)
    B, N = 2, 5
    peak = torch.randint(-1, 2, (B, N, h, w), generator=g).float()
    where = torch.stack([torch.randperm(h * w, generator=g) for _ in range(B * N)]).view(B, N, h, w).to(torch.int32) * 7 + 3
    for kk in ks_:
        rv, ri = P.topk_reference(peak, where, kk)
        for form in (lambda t: t.to(dev), lambda t: t.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)):
            vals, idx = ops.peaks_topk(form(peak), form(where), kk)
            assert torch.equal(vals.cpu(), rv) and torch.equal(idx.cpu(), ri), f"k = {kk}"
    with pytest.raises(ValueError, match="k must be"):
        ops.peaks_topk(peak.to(dev), where.to(dev), h * w + 1)
    with pytest.raises(ValueError, match="k must be"):
        ops.peaks_topk(peak.to(dev), where.to(dev), 65)
    with pytest.raises(ValueError, match="k must be"):
        ops.peaks_topk(peak.to(dev), where.to(dev), 0)


# ---- 6. module --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def module_case(dev):
    """lr 14 x 14 -> 224 x 224, C 384, window 9, bf16 features (the geometry of test_gpu_cosine_head.py's module tests)."""
    size, lr, Cc, ksz = (224, 224), (14, 14), 384, 9
    p = O.make_params(seed=31)
    m = _load_model(dev, p, kernel_size=ksz)
    img = O.hash_normal((1, 3, *size), 801).to(dev)
    ft = bf16r(O.hash_normal((1, Cc, *lr), 802)).to(dev).to(torch.bfloat16)
    return m, p, img, ft, size, lr, Cc


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_locate_image_guidance_and_chunks(dev, module_case):
    from naf_amd import Peaks
    m, p, img, ft, size, lr, Cc = module_case
    E = O.hash_normal((300, Cc), 803).to(dev)
    cos = m(img, ft, size, head=E[:21], cosine=True, logit_scale=10.0)
    pk = m.locate(img, ft, size, E[:21], topk=3, logit_scale=10.0)
    assert isinstance(pk, Peaks) and pk.scores.shape == pk.y.shape == pk.x.shape == (1, 21, 3) and pk.y.dtype == pk.x.dtype == torch.int64
    assert pk.cell_scores.shape == pk.cell_index.shape == (1, 21, *lr) and not pk.scores.requires_grad
    want_p, want_w = P.cell_peaks(cos, *lr)
    assert torch.equal(pk.cell_scores, want_p) and torch.equal(pk.cell_index, want_w)
    rv, ri = P.topk_reference(want_p.cpu(), want_w.cpu(), 3)
    assert torch.equal(pk.scores.cpu(), rv) and torch.equal((pk.y * size[1] + pk.x).cpu(), ri.long())
    assert _same(m.locate(m.guide(img), ft, size, E[:21], topk=3, logit_scale=10.0), pk)
    assert _same(m.locate(img, ft, size, E[:21], topk=3, logit_scale=10.0, path="fused"), pk)
    m.train()
    try:
        assert _same(m.locate(img, ft, size, E[:21], topk=3, logit_scale=10.0), pk)      # inference whatever the mode
    finally:
        m.eval()
    # N = 300 runs as 256 + 44
    whole, a, b = m.locate(img, ft, size, E, topk=2), m.locate(img, ft, size, E[:256], topk=2), m.locate(img, ft, size, E[256:], topk=2)
    assert whole.scores.shape == (1, 300, 2) and all(torch.equal(x, torch.cat([y, z], dim=1)) for x, y, z in zip(whole, a, b))
    z = m.locate(img[:0], ft[:0], size, E[:21])
    assert z.scores.shape == (0, 21, 1) and z.cell_index.shape == (0, 21, *lr)


def test_locate_routing(dev, module_case):
    from naf_amd._lib import NafHipError
    m, p, img, ft, size, lr, Cc = module_case
    E = O.hash_normal((151, Cc), 804).to(dev)
    # fp16 features: "auto" composes, "fused" raises
    f16 = ft.to(torch.float16)
    auto = m.locate(img, f16, size, E[:21], topk=2)
    assert _same(auto, m.locate(img, f16, size, E[:21], topk=2, path="composed"))
    want = P.cell_peaks(m(img, f16, size, head=E[:21], cosine=True), *lr)
    assert torch.equal(auto.cell_scores, want[0]) and torch.equal(auto.cell_index, want[1])
    with pytest.raises(NafHipError, match="bfloat16"):
        m.locate(img, f16, size, E[:21], path="fused")
    # window 13 with N = 151: no scratch-free instantiation
    m13 = _load_model(dev, p, kernel_size=13)
    auto = m13.locate(img, ft, size, E)
    assert _same(auto, m13.locate(img, ft, size, E, path="composed"))
    with pytest.raises(NafHipError, match="window 13"):
        m13.locate(img, ft, size, E, path="fused")
    assert _same(m13.locate(img, ft, size, E[:21], path="fused"), m13.locate(img, ft, size, E[:21]))      # N = 21 is served at window 13
    with pytest.raises(ValueError, match="integer ratio"):
        m.locate(img, ft, (220, 224), E[:21])


def test_match_an_image_with_itself(dev, module_case):
    """The vector at a point is the pixel's own feature: its cosine there is 1 up to the kernel's error.  Derived budget b, per point n, with
    E^ the normalised vector, S = sum_g max_cells |E^_g . v_g|, V = || max_cells |v| ||_2 and nmin = the smallest pixel norm of the plain
    forward (less its bf16 store, 2^-8 relative): PV and P are each rounded once to bf16 (2^-9 relative), so the numerator moves by at most
    2^-8 (1 + 2^-10) S; the implied feature by 1.25 * 2^-8 V in norm (cosine_reference.py 2a), once for the kernel's norm and once for the
    queried vector itself; fp32 chains (C / 2 + 6) * 2^-24.  b = ((2^-8 (1 + 2^-10) S + 2.5 * 2^-8 V) / nmin) / (1 - 1.25 * 2^-8 V / nmin) + fp32."""
    from naf_amd import Match
    m, p, img, ft, size, lr, Cc = module_case
    heads = m.upsampler.num_heads
    g = m.guide(img)
    pts = torch.tensor([[5, 7], [100, 37], [223, 0], [111, 222], [64, 64]], device=dev)
    vec = m.query(g, pts, features=ft, output_size=size, weights=None).features
    cos = m(g, ft, size, head=vec, cosine=True)
    at = cos[0, torch.arange(5, device=dev), pts[:, 0], pts[:, 1]]
    res = m.match(g, ft, pts, g, ft, size, topk=2, mutual=True)
    assert isinstance(res, Match) and res.scores.shape == res.y.shape == res.x.shape == (5, 2) and res.distance.shape == (5,)
    eh = F.normalize(vec.float(), dim=1).cpu().double()
    vv = ft.float().cpu().double().reshape(heads, Cc // heads, -1)
    S_ = torch.einsum("ngd,gdc->ngc", eh.reshape(5, heads, Cc // heads), vv).abs().amax(dim=2).sum(dim=1)
    V_ = float(vv.abs().amax(dim=2).reshape(-1).norm())
    nmin = float(m(img, ft, size).float().norm(dim=1).min()) * (1 - 2.0 ** -8)
    rel = 1.25 * 2.0 ** -8 * V_ / nmin
    b = ((2.0 ** -8 * (1 + 2.0 ** -10) * S_ + 2.5 * 2.0 ** -8 * V_) / nmin) / (1 - rel) + (Cc / 2 + 6) * 2.0 ** -24
    print(f"match: cos at the points {at.tolist()}, scores {res.scores[:, 0].tolist()}, budget {b.tolist()}, round trip {res.distance.tolist()}")
    assert bool((res.scores[:, 0] >= at).all())                                  # the found location is at least as good as the point
    assert bool(((at.cpu().double() - 1).abs() <= b).all()) and bool(((res.scores[:, 0].cpu().double() - 1).abs() <= b).all())
    assert bool((res.scores[:, 0] >= res.scores[:, 1]).all())
    pk = m.locate(g, ft, size, vec, topk=2)
    assert torch.equal(res.scores, pk.scores[0]) and torch.equal(res.y, pk.y[0]) and torch.equal(res.x, pk.x[0])
    assert bool(torch.isfinite(res.distance).all()) and bool((res.distance >= 0).all())      # reported, not asserted to be 0: another pixel may tie
    assert m.match(g, ft, pts, g, ft, size).distance is None
