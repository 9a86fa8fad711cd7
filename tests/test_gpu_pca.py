"""GPU tests of feature PCA (``naf_amd.FeaturePCA`` / ``naf_amd.pca`` / ``ops.feature_moments`` / ``ops.pca_project`` / ``ops.pca_minmax``)
against the fp64 restatement in tests/pca_reference.py, which also holds the inputs and every bound: all of them follow from the reference
quantities and the unit roundoff of fp32, none from what the kernels return.  Every test prints the measured value beside its bound (``-s``)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_reference as R  # noqa: E402
from oracle import naf_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

PCA_NAMES = sorted(R.PCA_CASES)
MOMENT_NAMES = sorted(R.MOMENT_CASES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def dev_map(m, dev):
    """The map as ``naf(...)`` returns one: a bf16 channels-last view [1, C, H, W] on the device."""
    return m.to(dev).to(torch.bfloat16).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def strided_map(m, dev, pad=8, fill=float("nan")):
    """The same values at a row stride of C + pad elements, the padding filled with `fill`."""
    _, C, H, W = m.shape
    buf = torch.full((H, W, C + pad), fill, dtype=torch.bfloat16, device=dev)
    buf[..., :C] = m[0].permute(1, 2, 0).to(dev).to(torch.bfloat16)
    return buf[..., :C].permute(2, 0, 1).unsqueeze(0)


# ---- A. moments, every entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MOMENT_NAMES)
def test_moments_match_fp64_within_the_chain_bound(dev, name):
    """|gram - ref| <= L 2^-24 sum_p |x_pi x_pj| and |sum - ref| <= L 2^-24 sum_p |x_pi| for every entry, L = min(P, 65536); gram exactly
    symmetric; a second call gives the same bits."""
    from naf_amd import ops
    for m, (g_ref, s_ref, g_bound, s_bound) in zip(R.case_maps(name), R.case_moments(name)):
        x = strided_map(m, dev) if name == "160x50x41" else dev_map(m, dev)
        if name == "160x50x41":
            assert x.stride(3) == m.shape[1] + 8
        gram, total, P = ops.feature_moments(x)
        assert P == m.shape[2] * m.shape[3] and gram.dtype == total.dtype == torch.float64
        assert tuple(gram.shape) == (m.shape[1], m.shape[1]) and tuple(total.shape) == (m.shape[1],)
        assert torch.equal(gram, gram.t()), "gram is not exactly symmetric"
        gram2, total2, _ = ops.feature_moments(x)
        assert torch.equal(gram, gram2) and torch.equal(total, total2), "a second call gave other bits"
        g, s = gram.cpu(), total.cpu()
        eg, es = (g - g_ref).abs(), (s - s_ref).abs()
        rg, rs = float((eg / g_bound.clamp_min(1e-300)).max()), float((es / s_bound.clamp_min(1e-300)).max())
        print(f"{name} {tuple(m.shape)}: gram max err {float(eg.max()):.3e} = {rg:.3f} of its bound; sum max err {float(es.max()):.3e} = {rs:.3f} of its bound")
        assert bool((eg <= g_bound).all()) and bool((es <= s_bound).all())


def test_moments_never_read_past_the_last_pixel(dev):
    """The tail mask: a map followed by NaN-filled memory gives the bits of the map followed by zeros (P = 1073 ends inside a pixel tile
    and inside the last slab)."""
    from naf_amd import ops
    m = R.case_maps("96x37x29")[0]
    _, C, H, W = m.shape
    out = []
    for fill in (float("nan"), 0.0):
        buf = torch.full(((H * W + 64) * C,), fill, dtype=torch.bfloat16, device=dev)
        buf[:H * W * C] = m[0].permute(1, 2, 0).reshape(-1).to(dev).to(torch.bfloat16)
        x = buf[:H * W * C].view(H, W, C).permute(2, 0, 1).unsqueeze(0)
        assert x.data_ptr() == buf.data_ptr()                                                          # used as it is
        out.append(ops.feature_moments(x))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][0]).all()) and bool(torch.isfinite(out[0][1]).all())


def test_moments_of_fp32_nchw_are_those_of_its_bf16_channels_last_copy(dev):
    from naf_amd import ops
    m = R.case_maps("96x37x29")[0]
    x32 = (m + 1e-3 * O.hash_normal(tuple(m.shape), 7999)).to(dev)                                     # not bf16 numbers
    assert x32.is_contiguous() and not torch.equal(x32, R.bf16r(x32))
    a = ops.feature_moments(x32)
    b = ops.feature_moments(dev_map(x32, dev))
    c = ops.feature_moments(x32[0])                                                                    # [C, H, W]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# ---- B. basis ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(dev):
    """name -> (FeaturePCA fitted on the device, the device maps)."""
    import naf_amd
    cache = {}

    def get(name):
        if name not in cache:
            maps = [dev_map(m, dev) for m in R.case_maps(name)]
            cache[name] = (naf_amd.FeaturePCA().fit(maps if len(maps) > 1 else maps[0]), maps)
        return cache[name]
    return get


@pytest.mark.parametrize("name", PCA_NAMES)
def test_basis_within_davis_kahan(dev, fitted, name):
    """1 - |cos(v_r, ref_r)| <= (2 E / gap_r)^2 / 2 + 2^-40; the sign convention; the attributes."""
    f = R.case_fit(name)
    p, _ = fitted(name)
    C = f.mean.shape[0]
    assert tuple(p.components_.shape) == (C, 3) and tuple(p.mean_.shape) == (C,) and tuple(p.singular_values_.shape) == (3,)
    V = p.components_.double().cpu()
    for r in range(3):
        cos = float((V[:, r] * f.components[:, r]).sum() / V[:, r].norm())
        bound = f.sin_bound[r] ** 2 / 2 + 2.0 ** -40
        print(f"{name} component {r}: 1 - |cos| = {1 - abs(cos):.3e} (bound {bound:.3e}; sin bound {f.sin_bound[r]:.2e}, gap {f.gaps[r]:.3f})")
        assert 1.0 - abs(cos) <= bound
        assert cos > 0, "the sign convention differs from the reference's"
        i = int(V[:, r].abs().argmax())
        assert float(V[i, r]) > 0
    lam = p.explained_variance_.double().cpu()
    assert float((lam - f.eigenvalues[:3]).abs().max()) <= f.E                                         # Weyl
    sv = p.singular_values_.double().cpu()
    assert float(((sv - f.singular_values) / f.singular_values).abs().max()) <= f.E / float(f.eigenvalues[2])
    mean_bound = sum(b[3] / (m.shape[2] * m.shape[3]) for b, m in zip(R.case_moments(name), R.case_maps(name))) / len(R.case_maps(name))
    assert bool(((p.mean_.double().cpu() - f.mean).abs() <= mean_bound + 1e-300).all())


# ---- C. projection, every element ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PCA_NAMES)
def test_projection_matches_fp64_on_the_reference_basis(dev, name):
    """The reference basis is the V given to the kernel, so this does not depend on the fit.
    |raw - ref| <= (C + 4) 2^-24 (sum_c |x_c V_cr| + |b_r|); minmax is raw's minimum and maximum exactly."""
    from naf_amd import ops
    f = R.case_fit(name)
    V32 = f.components.float()
    b32 = (-(f.mean @ f.components)).float()
    for m in R.case_maps(name):
        _, C, H, W = m.shape
        raw, mm = ops.pca_project(dev_map(m, dev), V32.to(dev), b32.to(dev))
        assert tuple(raw.shape) == (1, 3, H, W) and raw.dtype == torch.float32 and raw.stride() == (H * W * 3, 1, W * 3, 3)
        assert torch.equal(mm[0], raw.amin(dim=(0, 2, 3))) and torch.equal(mm[1], raw.amax(dim=(0, 2, 3)))
        ref = (R.rows(m) @ V32.double() + b32.double()).view(H, W, 3).permute(2, 0, 1).unsqueeze(0)
        bound = R.projection_bound(m, V32, b32)
        err = (raw.double().cpu() - ref).abs()
        print(f"{name} {tuple(m.shape)}: max err {float(err.max()):.3e} = {float((err / bound).max()):.3f} of its bound")
        assert bool((err <= bound).all())


@pytest.mark.parametrize("n", [1, 2, 4, 5, 6, 7, 8])
def test_projection_other_component_counts(dev, n):
    """One kernel instantiation per n: the same bound with a random V (n = 3 is the test above)."""
    from naf_amd import ops
    m = R.case_maps("96x37x29")[0]
    _, C, H, W = m.shape
    V32, b32 = O.hash_normal((C, n), 7900 + n) * C ** -0.5, O.hash_normal((n,), 7950 + n)
    raw, mm = ops.pca_project(dev_map(m, dev), V32.to(dev), b32.to(dev))
    assert tuple(raw.shape) == (1, n, H, W)
    assert torch.equal(mm[0], raw.amin(dim=(0, 2, 3))) and torch.equal(mm[1], raw.amax(dim=(0, 2, 3)))
    ref = (R.rows(m) @ V32.double() + b32.double()).view(H, W, n).permute(2, 0, 1).unsqueeze(0)
    bound = R.projection_bound(m, V32, b32)
    err = (raw.double().cpu() - ref).abs()
    print(f"n = {n}: max err {float(err.max()):.3e} = {float((err / bound).max()):.3f} of its bound")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("name", PCA_NAMES)
def test_transform_rgb_is_the_min_max_of_transform(dev, fitted, name):
    """An exact 0 and an exact 1 in every component; the torch formula on raw within 2 fp32 ulps."""
    p, maps = fitted(name)
    for x in maps:
        raw, pic = p.transform(x), p.transform_rgb(x)
        assert pic.shape == raw.shape and pic.dtype == torch.float32
        assert bool((pic.amin(dim=(0, 2, 3)) == 0).all()) and bool((pic.amax(dim=(0, 2, 3)) == 1).all())
        r64 = raw.double()
        lo, hi = r64.amin(dim=(2, 3), keepdim=True), r64.amax(dim=(2, 3), keepdim=True)
        ref = (r64 - lo) / (hi - lo)
        err = float(((pic.double() - ref).abs() / ref.clamp_min(1e-300)).max())
        print(f"{name} {tuple(x.shape)}: max relative error against the formula in fp64 {err / 2.0 ** -23:.3f} ulp")
        assert bool(((pic.double() - ref).abs() <= 2.0 ** -22 * ref).all())
        assert torch.equal(pic, p.normalize(raw))


def test_minmax_of_a_strided_head_logits_view(dev):
    """pca_minmax / normalize on a [B, n, Ho, Wo] view of a [B, Ho, Wo, Npad] buffer (what the head kernel writes) against torch; the
    padding channels hold NaN and are never read.  A layout the kernel does not read in place (NCHW) gives the same numbers."""
    import naf_amd
    from naf_amd import ops
    B, Ho, Wo, npad, n = 2, 37, 29, 16, 3
    buf = torch.full((B, Ho, Wo, npad), float("nan"), dtype=torch.float32, device=dev)
    buf[..., :n] = O.hash_normal((B, Ho, Wo, n), 7800).to(dev)
    view = buf[..., :n].permute(0, 3, 1, 2)
    mm = ops.pca_minmax(view)
    assert tuple(mm.shape) == (B, 2, n)
    assert torch.equal(mm[:, 0], view.amin(dim=(2, 3))) and torch.equal(mm[:, 1], view.amax(dim=(2, 3)))
    pic = naf_amd.FeaturePCA.normalize(view)
    lo, hi = view.amin(dim=(2, 3), keepdim=True), view.amax(dim=(2, 3), keepdim=True)
    assert torch.equal(pic, (view - lo) / (hi - lo))
    assert torch.equal(ops.pca_minmax(view.contiguous()), mm)
    assert torch.equal(ops.pca_minmax(view[0]), mm[0])


# ---- D. the picture, end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PCA_NAMES)
def test_picture_matches_the_fp64_picture(dev, fitted, name):
    """FeaturePCA().fit(maps).transform_rgb(map) against the fp64 picture: <= 4 Delta / range_ref per component,
    Delta = max_p ||x_p - mu|| sqrt(2) (2 E / gap_r) + the projection bound.  No flip: the signs are defined."""
    f = R.case_fit(name)
    p, maps = fitted(name)
    for m, x in zip(R.case_maps(name), maps):
        pic = p.transform_rgb(x).double().cpu()
        ref = R.rgb(R.transform(f, m))
        bound = R.picture_bound(f, m)
        err = (pic - ref).abs().amax(dim=(0, 2, 3))
        print(f"{name} {tuple(m.shape)}: max err per component {[f'{float(e):.3e}' for e in err]} (bounds {[f'{float(b):.3e}' for b in bound]})")
        assert bool((err <= bound).all())


# ---- E. the head route --------------------------------------------------------------------------------------------------------------------
def test_head_route_matches_the_transform_of_the_written_map(dev):
    """pca.head() is a linear head: naf(image, feats, size, head=pca.head()) is pca.transform of a map that is never written.  Both against
    the fp64 projection of the fp32 oracle features: e_f <= max(2 e_u, the bf16 rounding of PV)."""
    import naf_amd
    size, lr, Cc, ksz = (64, 64), (8, 8), 384, 7
    params = O.make_params(seed=31)
    model = naf_amd.NAF(kernel_size=ksz).eval()
    model.load_state_dict(params, strict=True)
    model = model.to(dev)
    heads = model.upsampler.num_heads
    img = O.hash_normal((1, 3, *size), 601)
    ft = R.bf16r(O.hash_normal((1, Cc, *lr), 602))
    with torch.no_grad():
        up = model(img.to(dev), ft.to(dev).to(torch.bfloat16), size)
        pca = naf_amd.FeaturePCA().fit(up)
        weight, bias = pca.head()
        assert tuple(weight.shape) == (3, Cc) and tuple(bias.shape) == (3,) and weight.dtype == bias.dtype == torch.float32
        fused = model(img.to(dev), ft.to(dev).to(torch.bfloat16), size, head=(weight, bias))
        unfused = pca.transform(up)
    assert tuple(fused.shape) == tuple(unfused.shape) == (1, 3, *size)
    up_ref = O.naf_forward(params, img, ft, size, kernel_size=ksz)
    mu, V = pca.mean_.double().cpu(), pca.components_.double().cpu()
    ref = ((R.rows(up_ref) - mu) @ V).view(*size, 3).permute(2, 0, 1).unsqueeze(0)
    e_f = float((fused.double().cpu() - ref).abs().max())
    e_u = float((unfused.double().cpu() - ref).abs().max())
    wt = weight.float().cpu()
    pvf = torch.einsum("ngd,bgdhw->bgnhw", wt.reshape(3, heads, Cc // heads), ft.reshape(1, heads, Cc // heads, *lr))
    pv_round = 2.0 ** -8 * float(pvf.abs().amax(dim=(0, 3, 4)).sum(0).max())
    print(f"head route: fused max err {e_f:.4e}, unfused max err {e_u:.4e}, PV rounding bound {pv_round:.4e}")
    assert e_f <= max(2.0 * e_u, pv_round)
    pic = pca.normalize(fused)
    assert bool((pic.amin(dim=(0, 2, 3)) == 0).all()) and bool((pic.amax(dim=(0, 2, 3)) == 1).all())


# ---- F. the reference's own pca() -----------------------------------------------------------------------------------------------------------
def test_pca_matches_the_reference_on_the_golden_inputs(dev, golden_dir):
    """naf_amd.pca against tests/golden/P1_pca.npz (the reference's pca() on two square maps) up to the flip y -> 1 - y per component (the
    reference's signs are arbitrary), within the reference's spread over its seeds plus the picture bound."""
    import naf_amd
    g = R.load_golden(golden_dir)
    maps = [torch.from_numpy(g["maps"][i:i + 1]) for i in range(2)]
    f = R.fit(maps)
    pics, fit = naf_amd.pca([m.to(dev) for m in maps], dim=3)
    assert isinstance(fit, naf_amd.FeaturePCA) and len(pics) == 2
    for i, (m, pic) in enumerate(zip(maps, pics)):
        assert tuple(pic.shape) == (1, 3, 12, 12) and pic.dtype == torch.float32 and pic.is_cuda
        err = R.match_up_to_flip(pic.cpu(), torch.from_numpy(g["reduced_feats"][i:i + 1]))
        budget = float(g["seed_spread"]) + float(R.picture_bound(f, m).max())
        print(f"golden map {i}: max |rgb - reference| up to the flip {err:.3e} (budget {budget:.3e})")
        assert err <= budget
    again, fit2 = naf_amd.pca([m.to(dev) for m in maps], fit_pca=fit)
    assert fit2 is fit and all(torch.equal(a, b) for a, b in zip(again, pics))
