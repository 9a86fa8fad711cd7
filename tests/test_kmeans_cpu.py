"""Host-side tests of k-means on the upsampled features (no device): the struct layout against the header, ``ops.project_kmeans_values``
against its fp64 definition and the argmax invariance under centring, the fp64 reference's own sanity (the Lloyd objective never rises,
the planted inputs leave >= 0.9 of the pixels determined), the census restatement's sensitivity to planted defects, the refusals of
``naf.kmeans`` before any device work and ``ops.xna_kmeans_select`` on a table of geometries."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import kmeans_reference as KR  # noqa: E402
import mask_pool_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = 4


@pytest.fixture(scope="module")
def lib():
    from naf_amd import _lib
    return _lib.load()


def test_header_declares_and_library_exports_the_entries(lib):
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    raw = C.CDLL(os.path.join(ROOT, "naf_amd", "csrc", "libnaf_hip.so"))
    for sym in ("naf_xna_kmeans_select", "naf_xna_kmeans_workspace_bytes", "naf_xna_kmeans_fwd"):
        assert f"{sym}(const naf_xna_kmeans_args* a" in txt
        assert getattr(raw, sym) is not None
    assert int(__import__("re").search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403      # detected by symbol, not by version


def test_struct_layout_matches_the_header(tmp_path):
    from naf_amd import _lib
    fields = ["q", "k_lr", "pv_lr", "bias", "labels", "A", "mass", "workspace", "workspace_bytes", "rope_tab_y", "rope_tab_x", "B", "heads", "Ho", "Wo",
              "h", "w", "Dq", "K", "ky", "kx", "path", "scale", "bias_stride_b", "q_stride", "k_stride", "pv_stride", "labels_stride", "reserved"]
    assert fields == [f[0] for f in _lib.XnaKmeansArgs._fields_]
    body = 'printf("%zu", sizeof(naf_xna_kmeans_args));' + "".join(f'printf(" %zu", offsetof(naf_xna_kmeans_args, {f}));' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.XnaKmeansArgs)] + [getattr(_lib.XnaKmeansArgs, f).offset for f in fields]


@pytest.mark.parametrize("K,shared", [(1, False), (5, False), (17, True), (64, False)])
def test_project_kmeans_values_is_its_fp64_definition(K, shared):
    """pv5[b, g, y, x, k] = (c_k - mu)[g] . (v - mu)[g], bias = -|c - mu|^2 / 2, mu the per-channel mean of the low-res features: within one
    bf16 rounding of pv (fp32 einsum: Dv 2^-24 of the abs-sum), pad channels exact zeros; and the centred scores differ from
    c . f - |c|^2 / 2 by a term without k, so the argmax over k is that of the squared distance."""
    from naf_amd import ops
    B, Cc, h, w = 2, 64, 5, 6
    v = S.bf16r(S.make_values((B, Cc, h, w), "chan_offset", 5100 + K))
    c = KR.O.hash_normal((K, Cc) if shared else (B, K, Cc), 5200 + K)
    pv5, bias, mean = ops.project_kmeans_values(c, v, HEADS)
    kpad = (K + 15) // 16 * 16
    assert pv5.shape == (B, HEADS, h, w, kpad) and pv5.dtype == torch.bfloat16 and bias.shape == (B, K) and bias.dtype == torch.float32
    assert mean.shape == (B, Cc) and not bool(pv5[..., K:].any())
    cd = (c[None].expand(B, K, Cc) if shared else c).double()
    mu = v.double().mean(dim=(2, 3))
    S.check((mean.double() - mu).abs(), h * w * S.F32 * v.double().abs().mean(dim=(2, 3)) + 1e-30, "mean")
    cc, fc = cd - mu[:, None], v.double() - mu[:, :, None, None]
    Dv = Cc // HEADS
    want = torch.einsum("bkgd,bgdhw->bghwk", cc.view(B, K, HEADS, Dv), fc.view(B, HEADS, Dv, h, w))
    mag = torch.einsum("bkgd,bgdhw->bghwk", cc.abs().view(B, K, HEADS, Dv), fc.abs().view(B, HEADS, Dv, h, w))
    # the operands (c - mu, v - mu) carry the fp32 mean's error and their own fp32 rounding: (h w + 4) 2^-24 of the magnitudes involved
    op_err = (h * w + 4) * S.F32 * torch.einsum("bkgd,bgdhw->bghwk", (cd.abs() + mu.abs()[:, None]).view(B, K, HEADS, Dv),
                                                 (v.double().abs() + mu.abs()[:, :, None, None]).view(B, HEADS, Dv, h, w))
    S.check((pv5[..., :K].double() - want).abs(), S.U * want.abs() + (Dv + 2) * S.F32 * mag + op_err, "pv5")
    wb = -0.5 * (cc * cc).sum(2)
    S.check((bias.double() - wb).abs(), (Cc + 4) * S.F32 * (cc * cc).sum(2) + (h * w + 4) * S.F32 * (cc.abs() * (cd.abs() + mu.abs()[:, None])).sum(2) + 1e-30, "bias")
    # argmax invariance, in fp64 on any vector f = sum_j p_j v_j with sum_j p_j = 1 (here: the features themselves)
    f = v.double().flatten(2)                                                                  # B C P
    centred = torch.einsum("bkc,bcp->bkp", cc, f - mu[..., None]) + wb[..., None]
    plain = torch.einsum("bkc,bcp->bkp", cd, f) - 0.5 * (cd * cd).sum(2)[..., None]
    gap = centred - plain
    assert float((gap - gap[:, :1]).abs().max()) <= 1e-9 * float(plain.abs().max() + 1.0)      # the difference does not depend on k
    dist = ((f[:, None] - cd[..., None]) ** 2).sum(2)
    if K > 1:
        assert torch.equal(KR.first_argmax(centred), KR.first_argmax(-dist)) or \
            float((dist.gather(1, KR.first_argmax(centred)[:, None]) - dist.amin(1, keepdim=True)).abs().max()) <= 1e-9 * float(dist.max())
    with pytest.raises(ValueError, match="centroids must be"):
        ops.project_kmeans_values(c[..., :-1], v, HEADS)
    with pytest.raises(ValueError, match="not divisible"):
        ops.project_kmeans_values(c, v, 3)


def test_lloyd_objective_never_rises_on_the_planted_inputs():
    """The reference's own sanity: plain Lloyd in fp64 on the oracle's upsampled features, 5 iterations from the centroids under test."""
    q, k, v, c, ks = KR.planted_inputs("k3", 4, "unit", 5300)
    f = KR.upsampled_features(q, k, v, ks, HEADS)
    _, labels, obj = KR.lloyd_exact(f, c, 5)
    assert len(obj) == 6 and all(b <= a * (1.0 + 1e-12) for a, b in zip(obj, obj[1:])), obj
    assert obj[-1] < obj[0]
    assert labels.shape == (2, 64, 80) and int(labels.max()) < 4


@pytest.mark.parametrize("geom,K,fam", KR.PARITY)
def test_planted_inputs_leave_the_labels_determined(geom, K, fam):
    """The share of pixels whose label the oracle fixes beyond twice ``head_bound`` is >= 0.9 for every parity case the device test ships
    (0.957 .. 0.987 with centring), and the fp64 step is consistent: masses add up to the pixel count, an empty cluster keeps its centroid."""
    q, k, v, c, ks = KR.planted_inputs(geom, K, fam, 5400 + K)
    r = KR.lloyd_step_reference(q, k, v, c, ks, HEADS)
    print(f"{geom} K={K} {fam}: determined share {r['share']:.3f}, determined clusters {int(r['cluster_det'].sum())} of {r['cluster_det'].numel()}")
    assert r["share"] >= 0.9
    Ho, Wo = q.shape[-2:]
    assert torch.equal(r["mass"].sum(1), torch.full((2,), float(Ho * Wo), dtype=torch.float64))
    empty = r["mass"] == 0
    assert torch.equal(r["c_new"][empty], c.double()[empty])
    bnd, ok = KR.centroid_bound(r, k.shape[-2] * k.shape[-1])
    assert bool(ok[r["mass"] > 0].any()) and bool(torch.isfinite(bnd).all())
    live = ok & (r["mass"] > 0)
    print(f"    centroid bound over the centroids' spread: median {float((bnd[live] / c.double().std()).median()):.3f}, max {float((bnd[live] / c.double().std()).max()):.3f}")
    if K == 16:
        assert bool(empty.any()), "six blobs, sixteen centroids: some cluster must stay empty (the module test needs one)"


@pytest.mark.parametrize("geom", ["k7", "k7_patch14", "k3"])
def test_planted_defects_change_the_census(geom):
    """Every defect the kernel could have changes an integer of the census restatement (or the label), on the geometry where it can show."""
    ks, (h, w), (Ho, Wo) = KR.GEOMS[geom]
    K = 17
    bias = KR.census_bias(2, K, (3, 16))
    lab, cnt, mass = KR.census_expectation(bias, h, w, Ho, Wo, ks)
    assert lab.tolist() == [3, 16] and int(mass[0, 3]) == Ho * Wo and int(mass.sum()) == 2 * Ho * Wo
    assert torch.equal(cnt[0, 3], R.census_counts(torch.ones(1, 1, Ho, Wo, dtype=torch.bool), h, w, ks)[0, 0]) and int(cnt[0, 4].sum()) == 0
    for d in ("shift", "no_clamp", "wrong_bias_row") + (("pad_pixel",) if (Wo // w) % 16 else ()):
        lab2, cnt2, mass2 = KR.census_expectation(bias, h, w, Ho, Wo, ks, defect=d)
        assert not (torch.equal(cnt2, cnt) and torch.equal(mass2, mass) and torch.equal(lab2, lab)), d
    # ties: pv = 0 and bias = 0 label every pixel 0; a kernel that kept the LAST maximum would label them K - 1
    zero = torch.zeros(2, K)
    assert KR.census_expectation(zero, h, w, Ho, Wo, ks)[0].tolist() == [0, 0]
    assert KR.census_expectation(zero, h, w, Ho, Wo, ks, defect="tie_highest")[0].tolist() == [K - 1, K - 1]


SELECT_TABLE = [
    # (Ho, Wo), (h, w), window, K, Dq -> answer, reason
    ((128, 160), (8, 10), 7, 16, 64, "fused", ""), ((112, 140), (8, 10), 7, 1, 64, "fused", ""), ((64, 80), (4, 5), 3, 64, 64, "fused", ""),
    ((160, 192), (10, 12), 9, 17, 64, "fused", ""), ((256, 256), (16, 16), 15, 64, 64, "fused", ""), ((256, 256), (16, 16), 13, 33, 64, "fused", ""),
    ((128, 160), (8, 10), 7, 65, 64, "composed", "at most 64 clusters"), ((64, 64), (28, 28), 7, 4, 64, "composed", "integer ratio"),
    ((96, 96), (12, 12), 7, 4, 64, "composed", "row tiles"), ((128, 128), (8, 8), 7, 4, 32, "composed", "Dq = 64"),
]


@pytest.mark.parametrize("out,lr,ks,K,Dq,want,why", SELECT_TABLE)
def test_select_answers_on_a_table_of_geometries(lib, out, lr, ks, K, Dq, want, why):
    """A host query: meta tensors, nothing launched.  The served geometries are mask pooling's."""
    from naf_amd import _lib, ops
    q = torch.empty((2, *out, 4, Dq), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    assert ops.xna_kmeans_select(q, lr, K, ks) == want
    if why:
        assert why in _lib.last_error(), _lib.last_error()
    if K <= 64:
        assert ops.xna_mask_pool_select(q, lr, K, ks) == want


def test_select_refuses_invalid_arguments(lib):
    from naf_amd import _lib, ops
    q = torch.empty((1, 128, 128, 4, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    with pytest.raises(ValueError, match="odd"):
        ops.xna_kmeans_select(q, (8, 8), 4, 6)
    with pytest.raises(ValueError, match="K must be"):
        ops.xna_kmeans_select(q, (8, 8), 0, 7)
    assert ops.xna_kmeans_select(q.float(), (8, 8), 4, 7) == "composed"

    def args(**kw):
        a = _lib.XnaKmeansArgs()
        a.q = a.k_lr = a.pv_lr = a.A = a.mass = a.workspace = 4096
        a.B, a.heads, a.Ho, a.Wo, a.h, a.w, a.Dq, a.K, a.ky, a.kx = 2, 4, 128, 128, 8, 8, 64, 17, 7, 7
        a.q_stride = _lib.I64x4(128 * 128 * 256, 64, 128 * 256, 256)
        a.k_stride = _lib.I64x4(64 * 256, 64, 8 * 256, 256)
        a.pv_stride = _lib.I64x4(4 * 64 * 32, 64 * 32, 8 * 32, 32)
        for n, v in kw.items():
            setattr(a, n, v)
        return a
    sel = lambda a: lib.naf_xna_kmeans_select(C.byref(a))
    assert sel(args()) == _lib.XNA_HEAD_FUSED
    assert sel(args(bias=4096, bias_stride_b=17)) == _lib.XNA_HEAD_FUSED and sel(args(bias=4096, bias_stride_b=0)) == _lib.XNA_HEAD_FUSED
    assert sel(args(labels=4097, labels_stride=_lib.I64x3(128 * 128, 128, 1))) == _lib.XNA_HEAD_FUSED
    for bad in (dict(pv_lr=None), dict(A=None), dict(mass=None), dict(workspace=None), dict(K=0), dict(path=5), dict(reserved=(C.c_int64 * 2)(0, 1)),
                dict(ky=6, kx=6), dict(rope_tab_y=4096), dict(bias=4096, bias_stride_b=16), dict(bias=4098, bias_stride_b=17),
                dict(pv_stride=_lib.I64x4(4 * 64 * 16, 64 * 16, 8 * 16, 16)), dict(labels=4096)):
        assert sel(args(**bad)) == -1, bad
    for bad, why in ((dict(pv_lr=4104), "16-byte aligned"), (dict(pv_stride=_lib.I64x4(4 * 64 * 36, 64 * 36, 8 * 36, 36)), "multiples of 8"),
                     (dict(K=65, pv_stride=_lib.I64x4(4 * 64 * 80, 64 * 80, 8 * 80, 80)), "at most 64")):
        assert sel(args(**bad)) == -2, bad
        assert why in _lib.last_error()
    assert lib.naf_xna_kmeans_workspace_bytes(C.byref(args())) == (2 * 64 * 4 * 49 * 32 + 2 * 64 * 32) * 4
    assert lib.naf_xna_kmeans_workspace_bytes(C.byref(args())) == lib.naf_xna_maskpool_workspace_bytes(C.byref(_mask_args(_lib)))
    assert lib.naf_xna_kmeans_select(None) == -1 and lib.naf_xna_kmeans_workspace_bytes(None) == 0


def _mask_args(_lib):
    a = _lib.XnaMaskPoolArgs()
    a.B, a.heads, a.h, a.w, a.K, a.ky, a.kx = 2, 4, 8, 8, 17, 7, 7
    return a


def test_kmeans_calls_are_refused_before_any_device_work():
    """Every refusal of ``naf.kmeans`` on CPU tensors: they come before the 'runs only on a ROCm device' error, so nothing was launched."""
    from naf_amd import NAF, KMeans
    m = NAF(kernel_size=7).eval()
    img, ft = torch.zeros(1, 3, 128, 128), torch.zeros(1, 128, 8, 8, dtype=torch.bfloat16)
    call = lambda k=4, **kw: m.kmeans(img, ft, (128, 128), k, **kw)
    for k in (0, -1, 257, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            call(k)
    with pytest.raises(ValueError, match="iters must be"):
        call(iters=-1)
    with pytest.raises(ValueError, match="path must be"):
        call(path="quick")
    with pytest.raises(ValueError, match="init must be"):
        call(init="kmeans++")
    with pytest.raises(ValueError, match="init must be"):
        call(init=torch.zeros(5, 128))
    with pytest.raises(ValueError, match="init must be"):
        call(init=torch.zeros(1, 4, 128), per_image=False)
    with pytest.raises(ValueError, match="distinct pixels"):
        m.kmeans(img, ft, (8, 8), 65)
    with pytest.raises(ValueError, match="expected image"):
        m.kmeans(img, ft[0], (128, 128), 4)
    with pytest.raises(ValueError, match="not divisible"):
        m.kmeans(img, torch.zeros(1, 126, 8, 8), (128, 128), 4)
    with pytest.raises(TypeError, match="features must be"):
        m.kmeans(img, ft.double(), (128, 128), 4)
    for ok in (dict(), dict(k=65), dict(k=256), dict(iters=0), dict(init=torch.zeros(4, 128)), dict(path="composed"), dict(per_image=False)):
        with pytest.raises(RuntimeError, match="ROCm device"):      # a valid call gets as far as the device check, and no further
            call(**ok)
    assert m.kmeans_path(ft, (128, 128), 4) == "fused" and m.kmeans_path(ft, (128, 128), 65) == "composed"
    assert m.kmeans_path(ft.half(), (128, 128), 4) == "composed" and m.kmeans_path(ft, (100, 100), 4) == "composed"
    r = KMeans(torch.zeros(1, 2, 2, dtype=torch.long), torch.tensor([[[3.0, 4.0], [0.0, 1.0]]]), torch.zeros(1, 2), torch.zeros(0, 1))
    wgt, b = r.head()
    assert wgt.shape == (2, 2) and b.tolist() == [-12.5, -0.5]
