"""GPU tests (-m gpu) of k-means on the upsampled features: naf_xna_kmeans_fwd, ``ops.xna_kmeans_step`` and ``naf.kmeans``.

The step is defined by two bit-identities with kernels that have tests of their own -- its labels are the head kernel's
(``ops.xna_head_objective(want_labels=True)`` per image), its A and mass are the pool kernel's for the one-hot masks of those labels
(``ops.xna_mask_pool``) -- and is then checked without either parent: an exact census (pv = 0, a one-hot bias row, q = 0), ties and NaN,
and the fp64 restatement of a Lloyd step with derived bounds (tests/kmeans_reference.py: nothing measured).  Every fused case first
asserts that ``ops.xna_kmeans_select`` grants the kernel, so nothing is silently composed.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import kmeans_reference as KR  # noqa: E402
import layout_contract as L  # noqa: E402
import mask_pool_reference as R  # noqa: E402
from test_gpu_mask_pool import GEOMS  # noqa: E402
from test_gpu_parity import bf16r, to5  # noqa: E402

pytestmark = pytest.mark.gpu

B, HEADS, DIM = 2, 4, 256
K_VALUES = (1, 2, 16, 17, 64)          # 17 crosses a 16-tile, 64 fills the launch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def test_geometries_are_mask_poolings():
    assert KR.GEOMS == GEOMS


def _granted(q5, lr, K, ks, tabs=None):
    from naf_amd import ops
    assert ops.xna_kmeans_select(q5, lr, K, ks, rope_tables=tabs) == "fused", "the fused kernel was not granted"


@functools.lru_cache(maxsize=None)
def _qk(geom):
    ks, lr, out = GEOMS[geom]
    q, k = S.make_qk((B, DIM, *out), (B, DIM, *lr), "unit", 5500 + list(GEOMS).index(geom), HEADS)
    return to5(q, HEADS).cuda(), to5(k, HEADS).cuda()


def _pv_bias(geom, K, seed, dev):
    """Random projected values (pad channels zero) and a DIFFERENT bias row per image."""
    ks, (h, w), _ = GEOMS[geom]
    kpad = (K + 15) // 16 * 16
    pv = torch.zeros(B, HEADS, h, w, kpad)
    pv[..., :K] = bf16r(O.hash_normal((B, HEADS, h, w, K), seed))
    bias = 0.5 * O.hash_normal((B, K), seed + 1)
    return pv.to(dev).to(torch.bfloat16), bias.to(dev)


@functools.lru_cache(maxsize=None)
def _step(geom, K):
    """One launch per (geometry, K), shared by the two identity tests (never modified)."""
    from naf_amd import ops
    ks, lr, _ = GEOMS[geom]
    q5, k5 = _qk(geom)
    pv, bias = _pv_bias(geom, K, 5600 + 31 * list(GEOMS).index(geom) + K, q5.device)
    _granted(q5, lr, K, ks)
    labels, A, mass = ops.xna_kmeans_step(q5, k5, pv, bias, ks, want_labels=True)
    return q5, k5, pv, bias, labels, A, mass


def _onehot(labels, K):
    return labels[:, None] == torch.arange(K, device=labels.device, dtype=labels.dtype)[None, :, None, None]


# ---- 1. labels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", K_VALUES)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_labels_are_the_head_kernels(dev, geom, K):
    """Bit for bit ``ops.xna_head_objective(want_labels=True)`` per image, each image with its own bias row (this proves the bias stride)."""
    from naf_amd import ops
    ks = GEOMS[geom][0]
    q5, k5, pv, bias, labels, A, mass = _step(geom, K)
    assert labels.dtype == torch.uint8 and labels.shape == (B, *GEOMS[geom][2]) and int(labels.max()) < K
    for b in range(B):
        want = ops.xna_head_objective(q5[b:b + 1], k5[b:b + 1], pv[b:b + 1], bias[b], ks, n_out=K, want_labels=True, path="fused")[1]
        assert torch.equal(labels[b:b + 1], want), f"{geom} K={K} image {b}: {int((labels[b:b + 1] != want).sum())} labels differ"
    if K > 1:
        other = ops.xna_head_objective(q5[:1], k5[:1], pv[:1], bias[1], ks, n_out=K, want_labels=True, path="fused")[1]
        assert not torch.equal(other, labels[:1]), "the inputs do not tell the bias rows apart"


# ---- 2. sums ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", K_VALUES)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_sums_are_the_pool_kernels(dev, geom, K):
    """A and mass bit for bit ``ops.xna_mask_pool`` under the bool masks ``labels == k``; mass is the exact pixel count of every label.
    Every instantiation keeps the pool kernel's summation order: the comparison is equality everywhere."""
    from naf_amd import ops
    ks, (h, w), (Ho, Wo) = GEOMS[geom]
    q5, k5, pv, bias, labels, A, mass = _step(geom, K)
    assert A.shape == (B, HEADS, K, h, w) and A.dtype == torch.float32 and mass.shape == (B, K)
    wantA, want_mass = ops.xna_mask_pool(q5, k5, _onehot(labels, K), ks)
    assert torch.equal(mass, want_mass)
    assert torch.equal(A, wantA), f"{geom} K={K}: {int((A != wantA).sum())} elements of A differ"
    counts = torch.stack([torch.bincount(labels[b].flatten().long(), minlength=K) for b in range(B)])
    assert torch.equal(mass, counts.float()) and int(counts.sum()) == B * Ho * Wo
    # labels = NULL: nothing else changes
    _, A2, mass2 = ops.xna_kmeans_step(q5, k5, pv, bias, ks)
    assert torch.equal(A2, A) and torch.equal(mass2, mass)


# ---- 3. census ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (2, 17, 64))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_planted_census_counts_every_pixel_once(dev, geom, K):
    """pv = 0 and a one-hot bias row label every pixel of image b k*(b); with q = 0, A[b, :, k*] / p is the integer census of an all-ones
    mask and every other cluster row is exact zeros.  On the 14-pixel cells a repeated pixel or a dead tile counted is a wrong integer."""
    from naf_amd import ops
    ks, (h, w), (Ho, Wo) = GEOMS[geom]
    assert R.census_is_exact(ks, Ho, Wo)
    kstar = (K - 1, 0)
    bias = KR.census_bias(B, K, kstar)
    lab, cnt, mass_want = KR.census_expectation(bias, h, w, Ho, Wo, ks)
    assert lab.tolist() == list(kstar)
    q5 = torch.zeros((B, HEADS, Ho, Wo, 64), dtype=torch.bfloat16, device=dev)
    k5 = to5(bf16r(O.hash_normal((B, DIM, h, w), 5701)), HEADS).to(dev)
    pv = torch.zeros((B, HEADS, h, w, (K + 15) // 16 * 16), dtype=torch.bfloat16, device=dev)
    _granted(q5, (h, w), K, ks)
    labels, A, mass = ops.xna_kmeans_step(q5, k5, pv, bias.to(dev), ks, want_labels=True)
    for b in range(B):
        assert bool((labels[b] == kstar[b]).all())
    got = (A / R.census_p(ks).to(dev)).cpu()
    assert torch.equal(got, got.round())
    assert torch.equal(got.to(torch.int64), cnt[:, None].expand(B, HEADS, K, h, w)), f"{geom} K={K}: {int((got.to(torch.int64) != cnt[:, None]).sum())} wrong counts"
    assert torch.equal(mass.cpu(), mass_want.float()) and float(mass[0, kstar[0]]) == Ho * Wo


# ---- 4. ties and NaN ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["k7_patch14", "k9"])
def test_ties_and_nan(dev, geom):
    """pv = 0, bias = 0: every pixel takes label 0 (the lowest index among equal maxima).  A NaN in one cell's pv for every cluster: the
    labels of the pixels it reaches are the head kernel's, A and mass the pool kernel's under them; no pixel is counted twice."""
    from naf_amd import ops
    ks, (h, w), (Ho, Wo) = GEOMS[geom]
    K = 17
    q5, k5 = _qk(geom)
    pv = torch.zeros((B, HEADS, h, w, 32), dtype=torch.bfloat16, device=dev)
    zero = torch.zeros((B, K), device=dev)
    labels, A, mass = ops.xna_kmeans_step(q5, k5, pv, zero, ks, want_labels=True)
    assert not bool(labels.any()) and bool((mass[:, 0] == Ho * Wo).all()) and not bool(mass[:, 1:].any()) and not bool(A[:, :, 1:].any())
    pv2, bias = _pv_bias(geom, K, 5801, dev)
    pv2[0, :, h // 2, w // 2, :] = float("nan")
    labels, A, mass = ops.xna_kmeans_step(q5, k5, pv2, bias, ks, want_labels=True)
    for b in range(B):
        want = ops.xna_head_objective(q5[b:b + 1], k5[b:b + 1], pv2[b:b + 1], bias[b], ks, n_out=K, want_labels=True, path="fused")[1]
        assert torch.equal(labels[b:b + 1], want)
    wantA, want_mass = ops.xna_mask_pool(q5, k5, _onehot(labels, K), ks)
    assert torch.equal(A, wantA) and torch.equal(mass, want_mass)
    assert bool(torch.isfinite(A).all()) and float(mass.sum()) <= B * Ho * Wo and bool((mass.sum(1) <= Ho * Wo).all())


# ---- 5. parity with fp64 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_case(geom, K, fam):
    q, k, v, c, ks = KR.planted_inputs(geom, K, fam, 5400 + K)
    return (q, k, v, c, ks), KR.lloyd_step_reference(q, k, v, c, ks, HEADS)


@pytest.mark.parametrize("geom,K,fam", KR.PARITY)
def test_step_matches_the_fp64_lloyd_step(dev, geom, K, fam):
    """The rule of tests/test_gpu_head_objective.py: the chosen label's reference score is within 2 x head_bound of the best; where the
    oracle's top-2 margin exceeds 2 x bound the label is the oracle's; the share of such pixels is asserted from the oracle alone (>= 0.9).
    The new centroids of clusters whose pixels are all determined stay within mask pooling's ``pooled`` bound over the mass."""
    from naf_amd import ops
    (q, k, v, c, ks), r = _parity_case(geom, K, fam)
    print(f"{geom} K={K} {fam}: determined share {r['share']:.3f}, determined clusters {int(r['cluster_det'].sum())} of {r['cluster_det'].numel()}")
    assert r["share"] >= 0.9, f"inputs leave only {r['share']:.3f} of the pixels determined"          # before the device result
    (h, w) = k.shape[-2:]
    q5, k5 = to5(q, HEADS).to(dev), to5(k, HEADS).to(dev)
    pv5, bias = r["pv5"].to(dev), r["bias"].to(dev)
    _granted(q5, (h, w), K, ks)
    labels, A, mass = ops.xna_kmeans_step(q5, k5, pv5, bias, ks, want_labels=True)
    vd = v.to(dev).to(torch.bfloat16)
    sums = ops.mask_pool_apply(A, vd, None, "sum")
    cd = c.to(dev)
    c_new = torch.where(mass[..., None] > 0, sums / mass[..., None], cd).cpu().double()
    lab = labels.long().cpu()
    z, bound = r["z"], r["bound"]
    chosen = z.gather(1, lab[:, None])[:, 0]
    assert bool((chosen >= z.amax(dim=1) - 2.0 * bound).all()), "a label is not a maximum of the oracle's scores up to the score error"
    assert torch.equal(lab[r["det"]], r["labels"][r["det"]])
    cdet = r["cluster_det"]
    assert torch.equal(mass.cpu().double()[cdet], r["mass"][cdet])
    # ... and every cluster that cannot end up empty within that bound widened by the pixels that may join or leave it (KR.centroid_bound)
    (bnd, ok), err = KR.centroid_bound(r, h * w), (c_new - r["c_new"]).abs()
    assert bool(ok[cdet & (r["mass"] > 0)].all()) and bool(ok.any())
    live = cdet & (r["mass"] > 0)
    print(f"    centroids: worst err/bound {S.worst_of_bound(err[ok], bnd[ok]):.3f} over {int(ok.sum())} clusters, "
          f"{S.worst_of_bound(err[live], bnd[live]) if bool(live.any()) else 0.0:.3f} over {int(live.sum())} determined live ones")
    S.check(err[ok], bnd[ok] + 1e-30, f"c_new {geom} K={K}")
    empty = (mass == 0).cpu()
    assert torch.equal(c_new[empty], c.double()[empty])


# ---- 6. rotate-on-load ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["k7", "k7_patch14", "k15"])
def test_rotate_on_load_equals_materialised_queries(dev, geom):
    """naf_xna_kmeans_fwd(rope_tab_*) on un-rotated guidance == naf_rope_pool_fwd queries + naf_xna_kmeans_fwd, bit for bit: both phases
    rotate alike (window 15 fetches the table rows at every rotation, the others once per round)."""
    from naf_amd import ops
    ks, lr, out = GEOMS[geom]
    K = 17
    x = bf16r(O.hash_normal((B, DIM, *out), 5900))
    per = O.rope_periods(DIM, HEADS, 100.0)
    xd = x.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ty, tx = ops.rope_tables(per.to(dev), *out)
    q_mat, k5 = ops.rope_pool(xd, ty, tx, HEADS, lr)
    q_raw = xd.permute(0, 2, 3, 1).unflatten(3, (HEADS, 64)).permute(0, 3, 1, 2, 4)
    pv, bias = _pv_bias(geom, K, 5901, dev)
    _granted(q_raw, lr, K, ks, (ty, tx))
    a = ops.xna_kmeans_step(q_mat, k5, pv, bias, ks, want_labels=True)
    b = ops.xna_kmeans_step(q_raw, k5, pv, bias, ks, want_labels=True, rope_tables=(ty, tx))
    assert all(torch.equal(x_, y_) for x_, y_ in zip(a, b))


# ---- 7. module ----------------------------------------------------------------------------------------------------------------------
def _load_model(dev, params, **kw):
    from naf_amd import NAF
    m = NAF(**kw).eval()
    m.load_state_dict(params, strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def module_case(dev):
    """lr 8 x 10 -> 128 x 160, C 256, window 7, planted bf16 features, K = 16 initial centroids of which the last is far from every pixel."""
    size, K = (128, 160), 16
    m = _load_model(dev, O.make_params(seed=51), kernel_size=7)
    img = O.hash_normal((B, 3, *size), 6001).to(dev)
    _, _, v, c, _ = KR.planted_inputs("k7", K, "unit", 6002)
    c[:, K - 1] = 100.0
    return m, img, v.to(dev).to(torch.bfloat16), c.to(dev), size, K


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_module_fused_equals_composed(dev, module_case):
    """The contract: ``path="fused"`` and ``path="composed"`` return equal labels, centroids, counts and shift over 3 iterations; "auto" is the
    fused route here; an empty cluster keeps its initial centroid bit for bit and has count 0; a ``Guidance`` and an image give equal
    results; ``init="points"`` is reproducible."""
    from naf_amd import KMeans
    m, img, ft, c0, size, K = module_case
    assert m.kmeans_path(ft, size, K) == "fused"
    rf = m.kmeans(img, ft, size, K, iters=3, init=c0, path="fused")
    rc = m.kmeans(img, ft, size, K, iters=3, init=c0, path="composed")
    assert isinstance(rf, KMeans) and _same(rf, rc) and _same(rf, m.kmeans(img, ft, size, K, iters=3, init=c0))
    assert rf.labels.shape == (B, *size) and rf.labels.dtype == torch.int64 and rf.centroids.shape == (B, K, DIM) and rf.centroids.dtype == torch.float32
    assert rf.counts.shape == (B, K) and rf.shift.shape == (3, B) and bool(torch.isfinite(rf.centroids).all()) and bool(torch.isfinite(rf.shift).all())
    assert bool((rf.counts.sum(1) == size[0] * size[1]).all())
    assert torch.equal(rf.counts, torch.stack([torch.bincount(rf.labels[b].flatten(), minlength=K) for b in range(B)]).float())
    assert torch.equal(rf.centroids[:, K - 1], c0[:, K - 1]) and not bool(rf.counts[:, K - 1].any())
    assert bool((rf.counts > 0).sum() >= 2 * B), "the planted blobs should keep several clusters alive"
    g = m.guide(img)
    assert _same(m.kmeans(g, ft, size, K, iters=3, init=c0), rf) and _same(m.kmeans(g, ft, size, K, iters=3, init=c0, path="composed"), rf)
    r0 = m.kmeans(img, ft, size, K, iters=0, init=c0)
    assert torch.equal(r0.centroids, c0) and r0.shift.shape == (0, B)
    p1, p2 = m.kmeans(g, ft, size, 6, iters=2), m.kmeans(g, ft, size, 6, iters=2, path="composed")
    assert _same(p1, p2) and _same(p1, m.kmeans(img, ft, size, 6, iters=2, generator=torch.Generator().manual_seed(0)))


def test_module_shared_centroids_are_the_batch_summed_definition(dev, module_case):
    """``per_image=False``: sums and masses are added over the batch before the division (restated with the ops)."""
    from naf_amd import ops
    m, img, ft, c0, size, K = module_case
    r = m.kmeans(img, ft, size, K, iters=1, init=c0[0], per_image=False)
    assert r.centroids.shape == (K, DIM) and _same(r, m.kmeans(img, ft, size, K, iters=1, init=c0[0], per_image=False, path="composed"))
    with torch.no_grad():
        q5, k5, tabs = m.guidance_qk(img, ft.shape[-2:], size)
        c = c0[0][None].expand(B, K, DIM).contiguous()
        pv5, bias, _ = ops.project_kmeans_values(c, ft, HEADS)
        _, A, mass = ops.xna_kmeans_step(q5, k5, pv5, bias, 7, scale=m.upsampler.scale, rope_tables=tabs)
        sums = ops.mask_pool_apply(A, ft, None, "sum").sum(0)
        ms = mass.sum(0)
        want = torch.where(ms[:, None] > 0, sums / ms[:, None], c0[0])
    assert torch.equal(r.centroids, want)
    assert torch.equal(r.shift[0], (want - c0[0]).norm(dim=1).amax().expand(B))


def test_module_head_labels_other_calls(dev, module_case):
    """``r.head(b)`` fed to ``naf(..., head=..., predict=True)`` on the same images returns ``r.labels[b]`` for image b, bit for bit -- from
    the image and from a ``Guidance``, per image and with shared centroids; and both are nearest-centroid labels of the materialised
    features: maxima of the fp32 scores up to the bf16 roundings of the two routes."""
    m, img, ft, c0, size, K = module_case
    r = m.kmeans(img, ft, size, 6, iters=3)
    g = m.guide(img)
    with torch.no_grad():
        f = m(img, ft, size).float()
        a_f = m(img, ft.abs(), size).float() * (1.0 + 2.0 ** -7)          # sum_j P_j |v_j| from the plain forward on |features|, its bf16 store allowed for
        for b in range(B):
            wgt, bias = r.head(b)
            assert wgt.shape == (6, DIM) and bias.shape == (6,)
            pred = m(img, ft, size, head=(wgt, bias), predict=True)
            assert torch.equal(pred[b], r.labels[b]) and torch.equal(m(g, ft, size, head=r.head(b), predict=True)[b], r.labels[b])
            fb = f[b].flatten(1)                                                    # C P
            score = wgt @ fb + bias[:, None]
            # the route rounds P and the projected values to bf16 (U each of the abs-sum sum_c |w_c| sum_j P_j |v_cj|), the forward rounds its
            # own P and stores f in bf16 (U each): a label scores within SLACK * 4 U of the largest abs-sum of the best fp32 score
            tol = S.SLACK * 4.0 * S.U * (wgt.abs() @ a_f[b].flatten(1)).amax(dim=0)
            got = score.gather(0, r.labels[b].flatten()[None])[0]
            assert bool((got >= score.amax(dim=0) - tol).all()), f"image {b}: a label is not a maximum of the fp32 scores up to the rounding"
        rs = m.kmeans(img, ft, size, 6, iters=2, per_image=False)
        assert torch.equal(m(img, ft, size, head=rs.head(), predict=True), rs.labels)


def test_module_auto_composes_what_the_kernel_does_not_serve(dev, module_case):
    """K = 65 and fp16 features select the composition (asserted) and run; ``"fused"`` raises NafHipError with the reason; so does a
    geometry the head route composes (a non-integer ratio), which materialises the feature map."""
    from naf_amd._lib import NafHipError
    m, img, ft, c0, size, K = module_case
    assert m.kmeans_path(ft, size, 65) == "composed" and m.kmeans_path(ft.half(), size, K) == "composed" and m.kmeans_path(ft, (100, 100), K) == "composed"
    r65 = m.kmeans(img, ft, size, 65, iters=1)
    assert r65.centroids.shape == (B, 65, DIM) and bool((r65.counts.sum(1) == size[0] * size[1]).all()) and int(r65.labels.max()) < 65
    assert _same(r65, m.kmeans(img, ft, size, 65, iters=1, path="composed"))
    r16 = m.kmeans(img, ft.half(), size, K, iters=1, init=c0)
    assert bool((r16.counts.sum(1) == size[0] * size[1]).all()) and bool(torch.isfinite(r16.centroids).all())
    rb = m.kmeans(img, ft, size, K, iters=1, init=c0)
    assert float((r16.labels == rb.labels).float().mean()) >= 0.99          # the same features through another rounding path
    rr = m.kmeans(img, ft, (100, 100), 4, iters=1)
    assert rr.labels.shape == (B, 100, 100) and bool((rr.counts.sum(1) == 100 * 100).all())
    with pytest.raises(NafHipError, match="at most 64"):
        m.kmeans(img, ft, size, 65, path="fused")
    with pytest.raises(NafHipError, match="bfloat16 features"):
        m.kmeans(img, ft.half(), size, K, path="fused")
    with pytest.raises(NafHipError, match="integer ratio"):
        m.kmeans(img, ft, (100, 100), K, path="fused")


def test_module_refusals_come_before_any_launch(dev, module_case):
    from naf_amd import ops
    from naf_amd._lib import NafHipError
    m, img, ft, c0, size, K = module_case

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
        for exc, k, kw in ((ValueError, 0, {}), (ValueError, 257, {}), (ValueError, K, dict(iters=-1)), (ValueError, K, dict(path="x")),
                           (ValueError, K, dict(init="random")), (ValueError, K, dict(init=c0[:, :3])), (ValueError, K, dict(init=c0, per_image=False)),
                           (RuntimeError, K, dict(init=c0.cpu())), (NafHipError, 65, dict(path="fused"))):
            with pytest.raises(exc):
                m.kmeans(img, ft, size, k, **kw)
        with pytest.raises(NafHipError):
            m.kmeans(img, ft.float(), size, K, path="fused")
        refused = list(spy.names)
        m.kmeans(img, ft, size, K, iters=1, init=c0)
        ran = list(spy.names)
    finally:
        ops.KERNEL_TIMER = old
    assert refused == [], f"a refused call launched something: {refused}"
    assert "stem" in ran and "xna_kmeans_step" in ran and "mask_pool_apply" in ran and "xna_head_ce" in ran, ran


# ---- 8. the C entry on caller-owned memory ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["k7", "k7_patch14"])
def test_strided_operands_guard_bands_and_repeatability(dev, geom):
    """pv, labels and bias as strided crops of NaN / 255-filled canvases; A, mass, labels and the workspace inside sentinel guard bands.  The
    result equals the dense call's, nothing outside the outputs is written, a second launch gives the same bits, and labels = NULL
    writes no label and gives the same A."""
    from naf_amd import _lib, ops
    ks, (h, w), (Ho, Wo) = GEOMS[geom]
    K = 17
    q5, k5 = _qk(geom)
    pv, bias = _pv_bias(geom, K, 6101, dev)
    want_labels, want_A, want_mass = ops.xna_kmeans_step(q5, k5, pv, bias, ks, want_labels=True)
    pv_canvas = torch.full((B, HEADS, h + 2, w + 3, 48), float("nan"), dtype=torch.bfloat16, device=dev)
    pv_view = pv_canvas[:, :, 1:1 + h, 2:2 + w, 8:40]
    pv_view.copy_(pv)
    bias_canvas = torch.full((B, 40), float("nan"), dtype=torch.float32, device=dev)
    bias_view = bias_canvas[:, 5:5 + K]
    bias_view.copy_(bias)
    lab_canvas = torch.full((B, Ho + 3, Wo + 9), 255, dtype=torch.uint8, device=dev)
    lab_view = lab_canvas[:, 2:2 + Ho, 5:5 + Wo]
    lab_inside = torch.zeros_like(lab_canvas, dtype=torch.bool)
    lab_inside[:, 2:2 + Ho, 5:5 + Wo] = True
    lib = _lib.load()
    results = []
    for with_labels in (True, True, False):
        lab_canvas.fill_(255)
        A, a_arena, a_in = L.banded((B, HEADS, K, h, w), torch.float32, dev)
        mass, m_arena, m_in = L.banded((B, K), torch.float32, dev)
        a = _lib.XnaKmeansArgs()
        a.q, a.k_lr, a.pv_lr, a.A, a.mass = q5.data_ptr(), k5.data_ptr(), pv_view.data_ptr(), A.data_ptr(), mass.data_ptr()
        a.bias, a.bias_stride_b = bias_view.data_ptr(), bias_view.stride(0)
        if with_labels:
            a.labels, a.labels_stride = lab_view.data_ptr(), ops._strides3(lab_view)
        ops._fill_geometry(a, q5, k5, h, w, ks, ks, None)
        a.K, a.path = K, _lib.XNA_HEAD_FUSED
        a.pv_stride = ops._strides4(pv_view, (0, 1, 2, 3))
        need = int(lib.naf_xna_kmeans_workspace_bytes(C.byref(a)))
        assert need == (B * h * w * HEADS * ks * ks * 32 + B * h * w * 32) * 4
        ws, w_arena, w_in = L.banded((need,), torch.uint8, dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        before = (a_arena.clone(), m_arena.clone(), w_arena.clone(), pv_canvas.clone(), bias_canvas.clone(), lab_canvas.clone())
        assert lib.naf_xna_kmeans_select(C.byref(a)) == _lib.XNA_HEAD_FUSED, _lib.last_error()
        _lib.check(lib.naf_xna_kmeans_fwd(C.byref(a), ops._stream(q5)), "naf_xna_kmeans_fwd")
        torch.cuda.synchronize()
        assert L.untouched(a_arena, before[0], a_in) and L.untouched(m_arena, before[1], m_in) and L.untouched(w_arena, before[2], w_in)
        assert L.unchanged(pv_canvas, before[3]) and L.unchanged(bias_canvas, before[4])
        assert bool((lab_canvas[~lab_inside] == 255).all())
        if with_labels:
            assert torch.equal(lab_view, want_labels)
        else:
            assert L.unchanged(lab_canvas, before[5])
        assert not bool((L.bits(A) == L.sentinel(torch.float32)).any()) and not bool((L.bits(mass) == L.sentinel(torch.float32)).any())
        results.append((A.clone(), mass.clone()))
        a.workspace_bytes = need - 4
        assert lib.naf_xna_kmeans_fwd(C.byref(a), ops._stream(q5)) == 1          # too small a workspace: refused, nothing launched
    for A, mass in results:
        assert torch.equal(A, want_A) and torch.equal(mass, want_mass)
