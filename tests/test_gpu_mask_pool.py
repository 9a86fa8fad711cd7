"""GPU tests (-m gpu) of mask pooling: naf_xna_maskpool_fwd / naf_maskpool_apply, ``ops.xna_mask_pool`` / ``ops.mask_pool_apply`` and
``naf(image, feats, size, masks=M)`` against the exact pixel census and the fp64 restatement with its derived per-element bounds
(tests/mask_pool_reference.py: nothing measured), the adjoint identity with the head kernel, the point kernel, and the composition.

Every fused case first asserts that ``ops.xna_mask_pool_select`` grants the kernel, so nothing is silently composed.  The worst
error / bound ratio of every parity case is appended to profiles/mask_pool.txt when NAF_WRITE_PROFILES=1.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import layout_contract as L  # noqa: E402
import mask_pool_reference as R  # noqa: E402
from test_gpu_parity import bf16r, to5  # noqa: E402

pytestmark = pytest.mark.gpu

B, HEADS, DIM = 2, 4, 256
# name: (window, (h, w), (Ho, Wo))
GEOMS = {
    "k7": (7, (8, 10), (128, 160)),
    "k7_patch14": (7, (8, 10), (112, 140)),        # 14-pixel cells: partial row tiles
    "k3": (3, (4, 5), (64, 80)),
    "k9": (9, (10, 12), (160, 192)),               # 81 slots: a partial key tile
    "k15": (15, (16, 16), (256, 256)),
}
KS_VALUES = (1, 16, 17, 64, 65)                    # 65: chunked (64 + 1)
# (geometry, K, logit family, mask kind)
PARITY = [("k7", 16, "unit", "byte"), ("k7", 17, "peaked", "soft"), ("k7_patch14", 65, "key_offset", "byte"), ("k7_patch14", 1, "unit", "soft"),
          ("k3", 64, "flat", "soft"), ("k9", 17, "peaked", "byte"), ("k15", 16, "unit", "byte"), ("k15", 1, "key_offset", "soft")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _granted(q5, lr, K, ks, tabs=None):
    from naf_amd import ops
    assert ops.xna_mask_pool_select(q5, lr, min(K, ops.MASK_POOL_CHUNK), ks, rope_tables=tabs) == "fused", "the fused kernel was not granted"


def _masks(kind, K, Ho, Wo, seed):
    return R.binary_masks(B, K, Ho, Wo, seed) if kind == "byte" else R.soft_masks(B, K, Ho, Wo, seed)


@functools.lru_cache(maxsize=None)
def _case(geom, K, fam, kind):
    """Inputs and the fp64 restatement: computed once per case and shared (never modified)."""
    ks, lr, out = GEOMS[geom]
    seed = 4100 + 17 * list(GEOMS).index(geom) + K
    q, k = S.make_qk((B, DIM, *out), (B, DIM, *lr), fam, seed, HEADS)
    v = S.make_values((B, DIM, *lr), "chan_offset", seed + 2)
    m = _masks(kind, K, *out, seed + 3)          # the reference is taken on the masks as given: the host's cast to bf16 is part of the bound
    return (q, k, v, m, ks), R.mask_pool_reference(q, k, m, ks, HEADS, v, rows_per_chunk=8)


def _profile(line):
    if os.environ.get("NAF_WRITE_PROFILES") == "1":
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mask_pool.txt")
        with open(path, "a") as f:
            f.write(line + "\n")
    print(line)


# ---- 1. census ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS_VALUES)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_census_counts_every_pixel_once(dev, geom, K):
    """q = 0: A / p is the integer number of masked pixels whose window holds the key, ``torch.equal`` to the count restated from the cell
    geometry; mass is the pixel count.  One wrong gather is a wrong integer at a named (b, head, k, jy, jx)."""
    from naf_amd import ops
    ks, (h, w), (Ho, Wo) = GEOMS[geom]
    assert R.census_is_exact(ks, Ho, Wo)
    m = R.census_masks(B, K, h, w, Ho // h, Wo // w)
    want = R.census_counts(m, h, w, ks)
    q5 = torch.zeros((B, HEADS, Ho, Wo, 64), dtype=torch.bfloat16, device=dev)
    k5 = to5(bf16r(O.hash_normal((B, DIM, h, w), 4001)), HEADS).to(dev)
    _granted(q5, (h, w), K, ks)
    A, mass = ops.xna_mask_pool(q5, k5, m.to(dev), ks)
    assert A.shape == (B, HEADS, K, h, w) and A.dtype == torch.float32 and mass.shape == (B, K)
    got = (A / R.census_p(ks).to(dev)).cpu()
    assert torch.equal(got, got.round())
    got = got.to(torch.int64)
    exp = want[:, None].expand(B, HEADS, K, h, w)
    if not torch.equal(got, exp):
        i = np.unravel_index(int((got != exp).int().flatten().argmax()), tuple(got.shape))
        raise AssertionError(f"{geom} K={K}: {int((got != exp).sum())} wrong counts, first at (b, head, k, jy, jx) = {i}: got {int(got[i])}, want {int(exp[i])}")
    assert torch.equal(mass.cpu(), m.sum(dim=(2, 3)).float())
    # uint8 masks are the same bytes
    A8, mass8 = ops.xna_mask_pool(q5, k5, m.to(dev).to(torch.uint8), ks)
    assert torch.equal(A8, A) and torch.equal(mass8, mass)


# ---- 2. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,K,fam,kind", PARITY)
def test_parity_with_the_fp64_restatement(dev, geom, K, fam, kind):
    """Per element: A within bf16_bound(n, abs_sum) + 2^-22 abs_sum (n = 1 byte masks, 2 soft masks), pooled within the same bound
    propagated through |V| plus h w 2^-24; mass exact for byte masks."""
    from naf_amd import ops
    (q, k, v, m, ks), r = _case(geom, K, fam, kind)
    soft = kind == "soft"
    lr = k.shape[-2:]
    q5, k5 = to5(q, HEADS).to(dev), to5(k, HEADS).to(dev)
    _granted(q5, lr, K, ks)
    A, mass = ops.xna_mask_pool(q5, k5, m.to(dev), ks)
    vd = v.to(dev).to(torch.bfloat16)
    psum = ops.mask_pool_apply(A, vd, mass, "sum")
    pmean = ops.mask_pool_apply(A, vd, mass, "mean")
    ab, pb = R.a_bound(r["abs_sum"], soft), R.pooled_bound(r["pooled_abs"], lr[0] * lr[1], soft)
    eA, eP = (A.cpu().double() - r["A"]).abs(), (psum.cpu().double() - r["pooled"]).abs()
    _profile(f"{geom:<12s} K={K:<3d} {fam:<10s} {kind:<5s} A worst err/bound {S.worst_of_bound(eA, ab):.3f}   pooled worst err/bound {S.worst_of_bound(eP, pb):.3f}")
    S.check(eA, ab, f"A {geom} K={K} {fam} {kind}")
    S.check(eP, pb, f"pooled {geom} K={K} {fam} {kind}")
    if soft:
        # fp32 sum of Ho Wo bf16-rounded masks
        S.check((mass.cpu().double() - r["mass"]).abs(), (S.U + m.shape[2] * m.shape[3] * S.F32) * m.double().abs().sum(dim=(2, 3)), "mass (soft)")
    else:
        assert torch.equal(mass.cpu().double(), r["mass"])
    # the mean is the sum divided by the mass in fp32, exact zeros for the empty mask
    ma = r["mass"]
    S.check((pmean.cpu().double() - R.mean_of(r["pooled"], ma)).abs(),
            R.mean_of(pb + 2.0 * S.F32 * r["pooled_abs"], ma.abs()) + (2.0 * S.U * R.mean_of(r["pooled_abs"], ma.abs()) if soft else 0.0), f"mean {geom}")
    if K > 1:
        assert not bool(A[:, :, K - 1].any()) and not bool(psum[:, K - 1].any()) and not bool(pmean[:, K - 1].any()) and not bool(mass[:, K - 1].any())
        assert bool(torch.isfinite(pmean).all())
    # 6. for every head sum_j A = mass (the weights of a pixel sum to one) within the bound of A on abs-sum = sum |M|
    am = m.double().abs().sum(dim=(2, 3))[:, None].expand(B, HEADS, K)
    S.check((A.cpu().double().sum(dim=(3, 4)) - r["mass"][:, None]).abs(), R.a_bound(am, soft) + lr[0] * lr[1] * S.F32 * am, f"sum_j A = mass {geom}")


# ---- 3. adjoint identity with the head kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,K,fam,kind", [PARITY[0], PARITY[2], PARITY[5]])
def test_adjoint_identity_with_the_head_kernel(dev, geom, K, fam, kind):
    """sum_px M[k, px] head(pv)[px, n] == sum_g sum_j A[g, k, j] pv_g[j, n]: both kernels carry the same bf16 P, so the two sides differ
    by fp32 accumulation alone -- (h w + Ho Wo) 2^-24 of the abs-sum."""
    from naf_amd import ops
    (q, k, v, m, ks), r = _case(geom, K, fam, kind)
    (h, w), (Ho, Wo) = k.shape[-2:], q.shape[-2:]
    N = 16
    q5, k5 = to5(q, HEADS).to(dev), to5(k, HEADS).to(dev)
    pv = bf16r(O.hash_normal((B, HEADS, h, w, N), 4301))
    out = ops.xna_head_forward(q5, k5, pv.to(dev).to(torch.bfloat16), None, ks, n_out=N, out_dtype=torch.float32, path="fused")
    A, _ = ops.xna_mask_pool(q5, k5, m.to(dev), ks)
    lhs = torch.einsum("bkp,bnp->bkn", m.double().reshape(B, K, -1), out.cpu().double().reshape(B, N, -1))
    rhs = torch.einsum("bgkj,bgjn->bkn", A.cpu().double().reshape(B, HEADS, K, -1), pv.double().reshape(B, HEADS, -1, N))
    scale = torch.einsum("bgkj,bgjn->bkn", r["abs_sum"].reshape(B, HEADS, K, -1), pv.double().abs().reshape(B, HEADS, -1, N))
    S.check((lhs - rhs).abs(), (h * w + Ho * Wo) * S.F32 * scale, f"adjoint {geom}")


# ---- 4. single-pixel mask -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["k7", "k7_patch14", "k9"])
def test_single_pixel_masks_are_the_point_kernel(dev, geom):
    """A mask of one pixel: A is that pixel's softmax (``ops.xna_points`` probs, fp32 throughout) scattered to its window, within one bf16
    rounding of P plus the fp32 error of the two softmaxes; pooled is that pixel of the plain forward within its bf16 output rounding."""
    from naf_amd import ops
    (q, k, v, _, ks), _ = _case(*[c for c in PARITY if c[0] == geom][0])          # the parity case's q, k, v
    (h, w), (Ho, Wo) = k.shape[-2:], q.shape[-2:]
    dy, dx = Ho // h, Wo // w
    pts = [(0, 0, 0), (1, Ho - 1, Wo - 1), (0, dy - 1, dx - 1), (1, Ho // 2, dx), (0, 3 * dy + 1, Wo - 1), (1, Ho - 1, 0), (0, Ho // 2 + 1, Wo // 2 - 1)]
    K = len(pts)
    m = torch.zeros(1, K, Ho, Wo, dtype=torch.bool).repeat(B, 1, 1, 1)
    for i, (b, y, x) in enumerate(pts):
        m[b, i, y, x] = True
    q5, k5, v5 = to5(q, HEADS).to(dev), to5(k, HEADS).to(dev), to5(v, HEADS).to(dev)
    A, mass = ops.xna_mask_pool(q5, k5, m.to(dev), ks)
    pooled = ops.mask_pool_apply(A, v.to(dev).to(torch.bfloat16), mass, "mean").cpu().double()
    _, _, probs = ops.xna_points(q5, k5, None, torch.tensor(pts, dtype=torch.int32, device=dev), ks, want_logits=False, want_probs=True)
    probs = probs.cpu().double()
    iy, ix = O.axis_index_table(Ho, h, ks), O.axis_index_table(Wo, w, ks)
    want = torch.zeros(B, HEADS, K, h, w, dtype=torch.float64)
    for i, (b, y, x) in enumerate(pts):
        want[b, :, i][:, torch.from_numpy(iy[y])[:, None], torch.from_numpy(ix[x])[None, :]] = probs[i].view(HEADS, ks, ks)
    # fp32 softmax of a 64-term score, twice (S.fp32_weight_factor with L <= scale * 64 max|q| max|k|)
    ep = S.fp32_weight_factor(64 ** -0.5 * 64 * float(q.abs().max()) * float(k.abs().max()), 64, ks * ks)
    S.check((A.cpu().double() - want).abs(), (S.U + 2.0 * ep) * want, f"single pixel A {geom}")
    plain = ops.xna_forward(q5, k5, v5, ks).permute(0, 1, 4, 2, 3).reshape(B, DIM, Ho, Wo).float().cpu().double()
    absv = torch.einsum("bgkj,bgdj->bkgd", want.reshape(B, HEADS, K, -1), v.double().abs().reshape(B, HEADS, DIM // HEADS, -1)).reshape(B, K, DIM)
    for i, (b, y, x) in enumerate(pts):
        S.check((pooled[b, i] - plain[b, :, y, x]).abs(), S.SLACK * S.U * plain[b, :, y, x].abs() + (ks * ks + h * w + 2.0 * ep / S.F32) * S.F32 * absv[b, i],
                f"single pixel pooled {geom} point {i}")


# ---- 5. columns of one launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["k7_patch14", "k15"])
def test_disjoint_masks_add_up(dev, geom):
    """Masks [M1, M2, M1 | M2] with M1, M2 disjoint: column 3 = column 1 + column 2.  The products with a 0 / 1 mask are exact and a key
    sums at most dy dx pixels in each of at most window^2 cells: two orders of one exact sum, n 2^-24 of it apart (n the number of terms)."""
    from naf_amd import ops
    ks, (h, w), (Ho, Wo) = GEOMS[geom]
    q, k = S.make_qk((B, DIM, Ho, Wo), (B, DIM, h, w), "unit", 4500, HEADS)
    both = R.binary_masks(B, 2, Ho, Wo, 4501, density=0.5)[:, 0]
    side = R.binary_masks(B, 2, Ho, Wo, 4502, density=0.5)[:, 0]
    m = torch.stack([both & side, both & ~side, both], dim=1)
    A, mass = ops.xna_mask_pool(to5(q, HEADS).to(dev), to5(k, HEADS).to(dev), m.to(dev), ks)
    A = A.cpu().double()
    n = (Ho // h) * (Wo // w) * ks * ks
    S.check((A[:, :, 2] - (A[:, :, 0] + A[:, :, 1])).abs(), n * S.F32 * A[:, :, 2], f"columns {geom}")
    assert torch.equal(mass[:, 2], mass[:, 0] + mass[:, 1])


# ---- 7. routing and reuse -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["k7", "k7_patch14"])
def test_rotate_on_load_equals_materialised_queries(dev, geom):
    """naf_xna_maskpool_fwd(rope_tab_*) on un-rotated guidance == naf_rope_pool_fwd queries + naf_xna_maskpool_fwd, bit for bit."""
    from naf_amd import ops
    ks, lr, out = GEOMS[geom]
    x = bf16r(O.hash_normal((B, DIM, *out), 4600))
    per = O.rope_periods(DIM, HEADS, 100.0)
    xd = x.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ty, tx = ops.rope_tables(per.to(dev), *out)
    q_mat, k5 = ops.rope_pool(xd, ty, tx, HEADS, lr)
    q_raw = xd.permute(0, 2, 3, 1).unflatten(3, (HEADS, 64)).permute(0, 3, 1, 2, 4)
    m = R.soft_masks(B, 5, *out, 4601).to(dev)
    _granted(q_raw, lr, 5, ks, (ty, tx))
    a, am = ops.xna_mask_pool(q_mat, k5, m, ks)
    b, bm = ops.xna_mask_pool(q_raw, k5, m, ks, rope_tables=(ty, tx))
    assert torch.equal(a, b) and torch.equal(am, bm)


@pytest.mark.parametrize("geom,dtype", [("k7", torch.bfloat16), ("k7", torch.uint8), ("k7_patch14", torch.bfloat16), ("k7_patch14", torch.uint8)])
def test_strided_masks_guard_bands_and_repeatability(dev, geom, dtype):
    """The C entry on caller-owned buffers: the masks as a channel slice and a crop of a larger canvas whose every other element is NaN
    (255 for bytes), A, mass and the workspace inside sentinel guard bands.  The result equals the dense call's, nothing outside the
    outputs is written, and a second launch gives the same bits."""
    from naf_amd import _lib, ops
    ks, (h, w), (Ho, Wo) = GEOMS[geom]
    K = 17
    q, k = S.make_qk((B, DIM, Ho, Wo), (B, DIM, h, w), "unit", 4700, HEADS)
    q5, k5 = to5(q, HEADS).to(dev), to5(k, HEADS).to(dev)
    dense = (R.binary_masks(B, K, Ho, Wo, 4701) if dtype == torch.uint8 else bf16r(R.soft_masks(B, K, Ho, Wo, 4701))).to(dev).to(dtype)
    canvas = torch.full((B, K + 3, Ho + 5, Wo + 24), 255 if dtype == torch.uint8 else float("nan"), dtype=dtype, device=dev)
    view = canvas[:, 2:2 + K, 3:3 + Ho, 8:8 + Wo]
    view.copy_(dense)
    want_A, want_mass = ops.xna_mask_pool(q5, k5, dense, ks)
    got_A, got_mass = ops.xna_mask_pool(q5, k5, view, ks)          # the operator: a copy only where the vector loads need one
    assert torch.equal(got_A, want_A) and torch.equal(got_mass, want_mass)
    lib = _lib.load()
    results = []
    for _ in range(2):
        A, a_arena, a_in = L.banded((B, HEADS, K, h, w), torch.float32, dev)
        mass, m_arena, m_in = L.banded((B, K), torch.float32, dev)
        a = _lib.XnaMaskPoolArgs()
        a.q, a.k_lr, a.masks, a.A, a.mass = q5.data_ptr(), k5.data_ptr(), view.data_ptr(), A.data_ptr(), mass.data_ptr()
        ops._fill_geometry(a, q5, k5, h, w, ks, ks, None)
        a.K, a.path = K, _lib.XNA_HEAD_FUSED
        a.mask_dtype = _lib.MASK_U8 if dtype == torch.uint8 else _lib.MASK_BF16
        a.m_stride = ops._strides4(view, (0, 1, 2, 3))
        need = int(lib.naf_xna_maskpool_workspace_bytes(C.byref(a)))
        assert need == (B * h * w * HEADS * ks * ks * 32 + B * h * w * 32) * 4
        ws, w_arena, w_in = L.banded((need,), torch.uint8, dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        before = (a_arena.clone(), m_arena.clone(), w_arena.clone(), canvas.clone())
        assert lib.naf_xna_maskpool_select(C.byref(a)) == _lib.XNA_HEAD_FUSED, _lib.last_error()
        _lib.check(lib.naf_xna_maskpool_fwd(C.byref(a), ops._stream(q5)), "naf_xna_maskpool_fwd")
        torch.cuda.synchronize()
        assert L.untouched(a_arena, before[0], a_in) and L.untouched(m_arena, before[1], m_in) and L.untouched(w_arena, before[2], w_in)
        assert L.unchanged(canvas, before[3])
        assert not bool((L.bits(A) == L.sentinel(torch.float32)).any()) and not bool((L.bits(mass) == L.sentinel(torch.float32)).any())
        results.append((A.clone(), mass.clone()))
        a.workspace_bytes = need - 4
        assert lib.naf_xna_maskpool_fwd(C.byref(a), ops._stream(q5)) == 1          # too small a workspace: refused, nothing launched
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert torch.equal(results[0][0], want_A) and torch.equal(results[0][1], want_mass)


def test_ops_refusals(dev):
    from naf_amd import ops
    from naf_amd._lib import NafHipError
    q5 = torch.zeros((1, HEADS, 64, 64, 64), dtype=torch.bfloat16, device=dev)
    k5 = torch.zeros((1, HEADS, 28, 28, 64), dtype=torch.bfloat16, device=dev)
    m = torch.ones((1, 2, 64, 64), dtype=torch.bool, device=dev)
    assert ops.xna_mask_pool_select(q5, (28, 28), 2, 7) == "composed"
    with pytest.raises(NafHipError, match="integer ratio"):
        ops.xna_mask_pool(q5, k5, m, 7)
    with pytest.raises(ValueError, match="masks must be"):
        ops.xna_mask_pool(q5, k5, m[:, :, :-1], 7)
    with pytest.raises(TypeError, match="masks must be"):
        ops.xna_mask_pool(q5, k5, m.long(), 7)
    with pytest.raises(ValueError, match="masks on"):
        ops.xna_mask_pool(q5, k5, m.cpu(), 7)
    with pytest.raises(ValueError, match="reduce"):
        ops.mask_pool_apply(torch.zeros((1, HEADS, 2, 4, 4), device=dev), torch.zeros((1, 64, 4, 4), dtype=torch.bfloat16, device=dev), None, "max")


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------
def _load_model(dev, params, **kw):
    from naf_amd import NAF
    m = NAF(**kw).eval()
    m.load_state_dict(params, strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def module_case(dev):
    """lr 8 x 10 -> 128 x 160, C 256, window 7, bf16 features, K = 17 masks (byte) with an empty one."""
    size, lr, ksz, K = (128, 160), (8, 10), 7, 17
    p = O.make_params(seed=41)
    m = _load_model(dev, p, kernel_size=ksz)
    img = O.hash_normal((B, 3, *size), 4801).to(dev)
    ft = (S.make_values((B, DIM, *lr), "chan_offset", 4802) + S.make_values((B, DIM, *lr), "outlier", 4803)).to(dev).to(torch.bfloat16)
    masks = R.binary_masks(B, K, *size, 4804).to(dev)
    return m, img, ft, masks, size


def test_module_matches_the_composition(dev, module_case):
    """``naf(image, feats, size, masks=M)``: "auto" is the fused route here; it agrees with the composed arm (the definition on the plain
    forward) within the bound of A propagated through |V| plus the plain forward's ``model_bound`` under the mask; followed by
    ``head=pooled, cosine=True`` -- the workflow the feature exists for."""
    from naf_amd import ops
    m, img, ft, masks, size = module_case
    K = masks.shape[1]
    with torch.no_grad():
        probe = torch.empty((B, *size, HEADS, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
        assert ops.xna_mask_pool_select(probe, ft.shape[-2:], K, 7) == "fused"
        pooled, A, mass = m(img, ft, size, masks=masks, return_attention=True)
        assert torch.equal(m(img, ft, size, masks=masks, mask_path="fused"), pooled)
        comp = m(img, ft, size, masks=masks, mask_path="composed")
        plain = m(img, ft, size)
        psum = m(img, ft, size, masks=masks, mask_reduce="sum")
        a_f = m(img, ft.abs(), size).float()           # sum_j P_j |v_j| from the plain forward on |features|
    assert pooled.shape == (B, K, DIM) and pooled.dtype == torch.float32 and not pooled.requires_grad
    assert A.shape == (B, HEADS, K, *ft.shape[-2:]) and mass.shape == (B, K)
    assert torch.equal(comp, ops.mask_pool_from_features(plain, masks))          # "composed" IS the definition on the plain forward
    assert torch.equal(mass.cpu(), masks.sum(dim=(2, 3)).float().cpu())
    assert not bool(pooled[:, K - 1].any()) and not bool(comp[:, K - 1].any()) and bool(torch.isfinite(pooled).all())
    md = masks.double().cpu()
    abs_pool = torch.einsum("bkhw,bchw->bkc", md, a_f.cpu().double() * (1.0 + 2.0 ** -7))          # its own bf16 store allowed for
    ma = md.sum(dim=(2, 3))
    lr = ft.shape[-2:]
    bound_sum = R.pooled_bound(abs_pool, lr[0] * lr[1], False) + torch.einsum("bkhw,bchw->bkc", md, S.model_bound(a_f.cpu().double()))
    S.check((psum.cpu().double() - ops.mask_pool_from_features(plain, masks, "sum").cpu().double()).abs(), bound_sum, "module sum vs composed")
    S.check((pooled.cpu().double() - comp.cpu().double()).abs(), R.mean_of(bound_sum, ma) + 2.0 * S.F32 * R.mean_of(abs_pool, ma), "module mean vs composed")
    with torch.no_grad():
        cos = m(img[:1], ft[:1], size, head=pooled[0, :K - 1], cosine=True)
        assert cos.shape == (1, K - 1, *size) and bool(torch.isfinite(cos).all())
        g = m.guide(img)
        assert torch.equal(m(g, ft, size, masks=masks), pooled)
        assert torch.equal(m(g, ft, size, masks=masks), pooled)          # from the caches
        big = R.binary_masks(B, 65, *size, 4805).to(dev)
        p65 = m(img, ft, size, masks=big)
        assert torch.equal(p65[:, :64], m(img, ft, size, masks=big[:, :64])) and torch.equal(p65[:, 64:], m(img, ft, size, masks=big[:, 64:]))
        for dt in (torch.float16, torch.float32):
            sm = R.soft_masks(B, 3, *size, 4806).to(dev)
            assert torch.equal(m(img, ft, size, masks=sm.to(dt)), m(img, ft, size, masks=sm.to(dt).to(torch.bfloat16)))
        z = m(img[:0], ft[:0], size, masks=masks[:0])
    assert z.shape == (0, K, DIM)


def test_module_auto_composes_what_the_kernel_does_not_serve(dev):
    """A non-integer ratio and fp16 / fp32 features select the composition -- asserted; "fused" raises NafHipError with the reason; a call
    that wants a gradient for the features takes ``forward_train`` and the gradient arrives."""
    from naf_amd import ops
    from naf_amd._lib import NafHipError
    m = _load_model(dev, O.make_params(seed=42), kernel_size=7)
    img = O.hash_normal((1, 3, 64, 64), 4811).to(dev)
    ft = bf16r(O.hash_normal((1, 128, 28, 28), 4812)).to(dev).to(torch.bfloat16)
    masks = R.binary_masks(1, 3, 64, 64, 4813).to(dev)
    probe = torch.empty((1, 64, 64, HEADS, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    assert ops.xna_mask_pool_select(probe, (28, 28), 3, 7) == "composed"
    with torch.no_grad():
        auto = m(img, ft, (64, 64), masks=masks)
        assert torch.equal(auto, m(img, ft, (64, 64), masks=masks, mask_path="composed"))
        assert torch.equal(auto, ops.mask_pool_from_features(m(img, ft, (64, 64)), masks))
        pooled, A, mass = m(img, ft, (64, 64), masks=masks, return_attention=True)
        # with the scores the plain forward runs the kernel that writes them: the definition on THAT forward, one bf16 store away from the other
        assert torch.equal(pooled, ops.mask_pool_from_features(m(img, ft, (64, 64), return_weights=True)[0], masks))
        assert float((pooled - auto).abs().max()) <= 2.0 * S.U * float(m(img, ft.abs(), (64, 64)).float().max())
        assert torch.equal(mass, masks.sum(dim=(2, 3)).float())
        # the composed A: fp32 softmax of the materialised scores summed under the masks; it contracts to the pooled plain forward, whose
        # bf16 P and bf16 store are two roundings of the abs-sum away
        assert A.shape == (1, HEADS, 3, 28, 28) and A.dtype == torch.float32
        S.check((A.sum(dim=(3, 4)) - mass[:, None]).abs().cpu().double(), (1e-5 * mass[:, None].expand(1, HEADS, 3)).cpu().double(), "composed sum_j A = mass")
        v4 = ft.float().reshape(1, HEADS, 32, -1)
        via = torch.einsum("bgkj,bgdj->bkgd", A.reshape(1, HEADS, 3, -1), v4).reshape(1, 3, 128) / mass[..., None]
        scale = torch.einsum("bgkj,bgdj->bkgd", A.reshape(1, HEADS, 3, -1), v4.abs()).reshape(1, 3, 128) / mass[..., None]
        S.check((via - pooled).abs().cpu().double(), (S.SLACK * 2.0 * S.U * scale + 1e-6).cpu().double(), "composed A . V = pooled")
        with pytest.raises(NafHipError, match="integer ratio"):
            m(img, ft, (64, 64), masks=masks, mask_path="fused")
        img2 = O.hash_normal((1, 3, 128, 128), 4814).to(dev)
        ft2 = bf16r(O.hash_normal((1, 128, 8, 8), 4815)).to(dev)
        m2 = R.binary_masks(1, 3, 128, 128, 4816).to(dev)
        b16 = m(img2, ft2.to(torch.bfloat16), (128, 128), masks=m2, mask_path="fused")
        for dt in (torch.float16, torch.float32):
            a = m(img2, ft2.to(dt), (128, 128), masks=m2)
            assert torch.equal(a, ops.mask_pool_from_features(m(img2, ft2.to(dt), (128, 128)), m2))
            assert float((a - b16).abs().max()) <= 0.05          # the same quantity through another rounding path
            with pytest.raises(NafHipError, match="bfloat16 features"):
                m(img2, ft2.to(dt), (128, 128), masks=m2, mask_path="fused")
    fg = ft2.to(torch.bfloat16).clone().requires_grad_(True)
    out = m(img2, fg, (128, 128), masks=m2)
    assert out.requires_grad
    out.square().mean().backward()
    assert fg.grad is not None and float(fg.grad.abs().sum()) > 0
    with pytest.raises(NafHipError, match="inference-only"):
        m(img2, fg, (128, 128), masks=m2, mask_path="fused")


def test_module_refusals_come_before_any_launch(dev, module_case):
    from naf_amd import ops
    m, img, ft, masks, size = module_case

    class Spy:
        def __init__(self):
            self.names = []

        def start(self, name):
            self.names.append(name)

        def stop(self, name):
            pass

    old, spy = ops.KERNEL_TIMER, Spy()
    ops.KERNEL_TIMER = spy
    E = torch.zeros((3, DIM), device=dev)
    try:
        for exc, kw in ((ValueError, dict(head=E)), (ValueError, dict(head=E, cosine=True)), (ValueError, dict(predict=True)),
                        (ValueError, dict(target=torch.zeros((B, *size), dtype=torch.long, device=dev))), (ValueError, dict(confusion=True)),
                        (ValueError, dict(regress=torch.zeros((B, DIM, *size), device=dev))), (ValueError, dict(return_weights=True)),
                        (ValueError, dict(mask_reduce="max")), (ValueError, dict(mask_path="x")), (ValueError, dict(masks=masks[:, :, :-1])),
                        (ValueError, dict(masks=masks.cpu())), (TypeError, dict(masks=masks.long())), (ValueError, dict(masks=masks[0]))):
            with pytest.raises(exc):
                m(img, ft, size, **{"masks": masks, **kw})
        with pytest.raises(ValueError):
            m(img, ft, size, return_attention=True)
        refused = list(spy.names)
        with torch.no_grad():
            m(img, ft, size, masks=masks)
        ran = list(spy.names)
    finally:
        ops.KERNEL_TIMER = old
    assert refused == [], f"a refused call launched something: {refused}"
    assert "stem" in ran and "xna_mask_pool" in ran and "mask_pool_apply" in ran, ran
