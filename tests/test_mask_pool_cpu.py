"""Host-side tests of mask pooling (no device): the fp64 restatement against the dense definition on the oracle's forward, the exactness
of the census inputs and its sensitivity to planted defects, ``naf_xna_maskpool_select`` on a table of geometries, the C entry's argument
checks, the struct layout, and the refusals of ``naf(..., masks=...)`` before any device work."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import mask_pool_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the device test's geometries: (window, (h, w), (Ho, Wo))
GEOMS = {"k7": (7, (8, 10), (128, 160)), "k7_patch14": (7, (8, 10), (112, 140)), "k3": (3, (4, 5), (64, 80)), "k9": (9, (10, 12), (160, 192)),
         "k15": (15, (16, 16), (256, 256))}


@pytest.fixture(scope="module")
def lib():
    from naf_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("ks,lr,out,heads,K,kind", [(3, (4, 5), (16, 20), 2, 5, "soft"), (5, (6, 5), (12, 15), 3, 3, "byte"), (3, (5, 4), (5, 4), 1, 2, "soft")])
def test_restatement_equals_the_dense_definition_on_the_oracle(ks, lr, out, heads, K, kind):
    """pooled = einsum(M, naf(V)) with the oracle's attention, A contracts to it, abs-sums bound it, mass is the mask's sum."""
    B, Dq, Dv = 2, 8, 6
    q, k = S.make_qk((B, heads * Dq, *out), (B, heads * Dq, *lr), "unit", 900, heads)
    v = S.make_values((B, heads * Dv, *lr), "chan_offset", 902)
    m = R.binary_masks(B, K, *out, 903) if kind == "byte" else R.soft_masks(B, K, *out, 903) - 0.05      # soft: some negative weights too
    m[:, K - 1] = 0
    r = R.mask_pool_reference(q, k, m, ks, heads, v, rows_per_chunk=3)
    up, up_abs = S.attention_reference(q, k, v, ks, heads)
    want = torch.einsum("bkhw,bchw->bkc", m.double(), up)
    assert float((r["pooled"] - want).abs().max()) <= 1e-11 * float(want.abs().max())
    assert bool((r["pooled"].abs() <= r["pooled_abs"] * (1 + 1e-12) + 1e-300).all())
    assert float((r["pooled_abs"] - torch.einsum("bkhw,bchw->bkc", m.double().abs(), up_abs)).abs().max()) <= 1e-11 * float(r["pooled_abs"].max())
    assert torch.equal(r["mass"], m.double().sum(dim=(2, 3)))
    # the weights of a pixel sum to one: sum_j A = mass, sum_j abs_sum = sum |M|
    assert float((r["A"].sum(dim=(3, 4)) - r["mass"][:, None]).abs().max()) <= 1e-11 * float(m.double().abs().sum(dim=(2, 3)).max())
    assert float((r["abs_sum"].sum(dim=(3, 4)) - m.double().abs().sum(dim=(2, 3))[:, None]).abs().max()) <= 1e-9
    if K > 1:
        assert not bool(r["A"][:, :, K - 1].any()) and not bool(R.mean_of(r["pooled"], r["mass"])[:, K - 1].any())
    from naf_amd import ops
    assert float((ops.mask_pool_from_features(up, m).double() - R.mean_of(want, r["mass"])).abs().max()) <= 1e-4 * float(want.abs().max())


@pytest.mark.parametrize("ks,lr,out", [(3, (4, 5), (16, 20)), (5, (7, 6), (16, 15)), (3, (5, 4), (5, 4))])
def test_composed_attention_from_scores_is_the_restatement(lib, ks, lr, out):
    """``ops.mask_attention_from_scores`` (the composed arm of ``return_attention``) on the oracle's scores: integer and non-integer ratios
    (repeated keys in a window) and ratio 1; fp32 softmax and sums against fp64."""
    from naf_amd import ops
    from oracle import naf_oracle as O
    B, heads, K = 2, 2, 4
    q, k = S.make_qk((B, heads * 8, *out), (B, heads * 8, *lr), "unit", 910, heads)
    m = R.soft_masks(B, K, *out, 911)
    iy, ix = S._tables(q, k, ks)
    _, scores = O.xna_tables(q.double(), k.double(), k.double(), iy, ix, heads, return_logits=True)
    got = ops.mask_attention_from_scores(scores.float(), m, lr, ks)
    P = torch.softmax(scores, dim=-1)                                    # [B, heads, Ho, Wo, kk] fp64: scattered key by key
    want = torch.zeros(B, heads, K, lr[0] * lr[1], dtype=torch.float64)
    key = torch.from_numpy(iy)[:, None, :, None] * lr[1] + torch.from_numpy(ix)[None, :, None, :]
    for t in range(ks * ks):
        kt = key.reshape(*out, ks * ks)[..., t].reshape(-1)
        want.index_add_(3, kt, torch.einsum("bkp,bgp->bgkp", m.double().reshape(B, K, -1), P[..., t].reshape(B, heads, -1)))
    assert got.shape == (B, heads, K, *lr) and got.dtype == torch.float32
    assert float((got.double().reshape_as(want) - want).abs().max()) <= 1e-5 * float(want.abs().max())
    if out[0] % lr[0] == 0 and out[1] % lr[1] == 0 and out != lr:
        r = R.mask_pool_reference(q, k, m, ks, heads)
        assert float((want.view_as(r["A"]) - r["A"]).abs().max()) <= 1e-11 * float(want.abs().max())


@pytest.mark.parametrize("geom", list(GEOMS))
def test_census_inputs_are_exact_and_defects_change_an_integer(geom):
    """The census is exact in fp32 for every geometry of the device test; with q = 0 the restatement gives NSLOT * A = the count; and every
    planted defect changes at least one count of the census masks (so ``torch.equal`` on the device would see it)."""
    ks, (h, w), (Ho, Wo) = GEOMS[geom]
    dy, dx = Ho // h, Wo // w
    assert R.census_is_exact(ks, Ho, Wo)
    p = float(R.census_p(ks))
    assert abs(p * ks * ks - 1.0) <= 2.0 ** -8
    for K in (1, 17):
        m = R.census_masks(2, K, h, w, dy, dx)
        want = R.census_counts(m, h, w, ks)
        assert int(want.max()) <= Ho * Wo and torch.equal(want.sum(dim=(2, 3)), m.sum(dim=(2, 3)) * ks * ks)
        for d in R.DEFECTS if K == 17 else ():             # the census as a whole sees every defect (one symmetric mask alone need not)
            if d == "pad_pixel" and dx % 16 == 0:
                continue                                   # no partial row tile in this geometry
            assert not torch.equal(R.census_counts(m, h, w, ks, defect=d), want), f"{geom} K={K}: defect {d} changes no count"
    if geom in ("k3", "k7_patch14"):                       # ... and the count IS the restatement at q = 0 (small geometries: host time)
        m = R.census_masks(2, 3, h, w, dy, dx)
        q, k = torch.zeros(2, 16, Ho, Wo), S.make_qk((2, 16, Ho, Wo), (2, 16, h, w), "unit", 905, 2)[1]
        r = R.mask_pool_reference(q, k, m, ks, 2, rows_per_chunk=16)
        assert float((r["A"] * ks * ks - R.census_counts(m, h, w, ks)[:, None].double()).abs().max()) <= 1e-9


def test_a_window_that_is_the_whole_grid_hides_nothing():
    """h = w = window: every cell's clamped window is the grid, and the window defects are invisible there -- which is why no geometry of the
    device test is that small on both axes."""
    for ks, (h, w), _ in GEOMS.values():
        assert h > ks and w > ks
    m =R.census_masks(1, 9, 7, 7, 16, 16)
    assert torch.equal(R.census_counts(m, 7, 7, 7, defect="shift"), R.census_counts(m, 7, 7, 7))


SELECT_TABLE = [
    # (Ho, Wo), (h, w), window, K, Dq -> answer, reason
    ((128, 160), (8, 10), 7, 16, 64, "fused", ""), ((112, 140), (8, 10), 7, 1, 64, "fused", ""), ((64, 80), (4, 5), 3, 64, 64, "fused", ""),
    ((160, 192), (10, 12), 9, 17, 64, "fused", ""), ((256, 256), (16, 16), 15, 64, 64, "fused", ""), ((256, 256), (16, 16), 13, 64, 64, "fused", ""),
    ((256, 256), (16, 16), 11, 33, 64, "fused", ""), ((160, 160), (5, 5), 5, 2, 64, "fused", ""),
    ((128, 160), (8, 10), 7, 65, 64, "composed", "at most 64 masks"), ((64, 64), (28, 28), 7, 4, 64, "composed", "integer ratio"),
    ((64, 64), (64, 64), 7, 4, 64, "composed", "row tiles"), ((96, 96), (12, 12), 7, 4, 64, "composed", "row tiles"),
    ((128, 128), (8, 8), 7, 4, 32, "composed", "Dq = 64"), ((384, 384), (16, 16), 15, 4, 64, "composed", "row tiles"),
    ((480, 480), (16, 16), 15, 4, 64, "fused", ""),
]


@pytest.mark.parametrize("out,lr,ks,K,Dq,want,why", SELECT_TABLE)
def test_select_answers_on_a_table_of_geometries(lib, out, lr, ks, K, Dq, want, why):
    """A host query: meta tensors, nothing launched."""
    from naf_amd import _lib, ops
    q = torch.empty((2, *out, 4, Dq), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    assert ops.xna_mask_pool_select(q, lr, K, ks) == want
    if why:
        assert why in _lib.last_error(), _lib.last_error()


def test_select_refuses_invalid_arguments_and_unaligned_masks(lib):
    from naf_amd import _lib, ops
    q = torch.empty((1, 128, 128, 4, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    with pytest.raises(ValueError, match="odd"):
        ops.xna_mask_pool_select(q, (8, 8), 4, 6)
    with pytest.raises(ValueError, match="exceeds the output extent"):      # window 9 on an 8 x 8 grid: no attention is defined
        ops.xna_mask_pool_select(q, (8, 8), 4, 9)
    with pytest.raises(ValueError, match="K must be"):
        ops.xna_mask_pool_select(q, (8, 8), 0, 7)
    assert ops.xna_mask_pool_select(q.float(), (8, 8), 4, 7) == "composed"

    def args(Wo=128, **kw):
        a = _lib.XnaMaskPoolArgs()
        a.q = a.k_lr = a.masks = a.A = a.mass = a.workspace = 4096
        a.B, a.heads, a.Ho, a.Wo, a.h, a.w, a.Dq, a.K, a.ky, a.kx = 1, 4, 128, Wo, 8, 8, 64, 4, 7, 7
        a.q_stride = _lib.I64x4(128 * Wo * 256, 64, Wo * 256, 256)
        a.k_stride = _lib.I64x4(64 * 256, 64, 8 * 256, 256)
        a.m_stride = _lib.I64x4(4 * 128 * Wo, 128 * Wo, Wo, 1)
        for n, v in kw.items():
            setattr(a, n, v)
        return a
    sel = lambda a: lib.naf_xna_maskpool_select(C.byref(a))
    assert sel(args()) == _lib.XNA_HEAD_FUSED
    assert sel(args(mask_dtype=_lib.MASK_U8)) == _lib.XNA_HEAD_FUSED
    for bad in (dict(masks=None), dict(A=None), dict(mass=None), dict(workspace=None), dict(K=0), dict(mask_dtype=2), dict(path=5), dict(reserved=1),
                dict(ky=6, kx=6), dict(rope_tab_y=4096)):
        assert sel(args(**bad)) == -1, bad
    # 16-pixel cells are read with vector loads: an odd pointer, a row stride that is no multiple of 8 or masks that are not x-contiguous
    for bad, why in ((dict(masks=4098), "16-byte aligned"), (dict(m_stride=_lib.I64x4(4 * 128 * 132, 128 * 132, 132, 1)), "multiples of 8"),
                     (dict(m_stride=_lib.I64x4(4 * 128 * 256, 128 * 256, 256, 2)), "x-contiguous")):
        assert sel(args(**bad)) == -2, bad
        assert why in _lib.last_error()
    # 14-pixel cells are read element by element: any alignment, any row stride
    assert sel(args(Wo=112, masks=4098, m_stride=_lib.I64x4(4 * 128 * 113, 128 * 113, 113, 1))) == _lib.XNA_HEAD_FUSED
    a = args()
    assert lib.naf_xna_maskpool_workspace_bytes(C.byref(a)) == (64 * 4 * 49 * 16 + 64 * 16) * 4
    assert lib.naf_xna_maskpool_workspace_bytes(C.byref(args(K=17))) == (64 * 4 * 49 * 32 + 64 * 32) * 4
    assert lib.naf_maskpool_apply(None, None, None, None, 1, 4, 4, 128, 64, None, 1, None) == 1
    assert lib.naf_maskpool_apply(4096, 4096, 4096, 4096, 1, 3, 4, 128, 64, (C.c_int64 * 2)(8192, 64), 1, None) == 1      # 128 % 3


def test_header_declares_and_library_exports_the_entries(lib):
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    raw = C.CDLL(os.path.join(ROOT, "naf_amd", "csrc", "libnaf_hip.so"))
    for sym in ("naf_xna_maskpool_select", "naf_xna_maskpool_workspace_bytes", "naf_xna_maskpool_fwd"):
        assert f"{sym}(const naf_xna_maskpool_args* a" in txt
        assert getattr(raw, sym) is not None
    assert "int naf_maskpool_apply(" in txt and raw.naf_maskpool_apply is not None
    assert int(__import__("re").search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403      # detected by symbol, not by version


def test_struct_layout_matches_the_header(tmp_path):
    from naf_amd import _lib
    fields = ["q", "masks", "mass", "workspace", "workspace_bytes", "rope_tab_x", "B", "K", "kx", "mask_dtype", "path", "scale", "reserved",
              "q_stride", "k_stride", "m_stride"]
    body = 'printf("%zu", sizeof(naf_xna_maskpool_args));' + "".join(f'printf(" %zu", offsetof(naf_xna_maskpool_args, {f}));' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.XnaMaskPoolArgs)] + [getattr(_lib.XnaMaskPoolArgs, f).offset for f in fields]


def test_mask_calls_are_refused_before_any_device_work():
    """Every refusal of ``naf(..., masks=...)`` on CPU tensors: they come before the 'runs only on a ROCm device' error, so nothing was
    launched.  ``masks`` is a named parameter: it is not swallowed by ``**kwargs``."""
    import inspect
    from naf_amd import NAF
    for name in ("masks", "mask_reduce", "mask_path", "return_attention"):
        assert name in inspect.signature(NAF.forward).parameters
    m = NAF(kernel_size=7).eval()
    img, ft = torch.zeros(1, 3, 128, 128), torch.zeros(1, 128, 8, 8, dtype=torch.bfloat16)
    M = torch.zeros(1, 3, 128, 128, dtype=torch.bool)
    call = lambda **kw: m(img, ft, (128, 128), **{"masks": M, **kw})
    for kw in (dict(head=torch.randn(5, 128)), dict(head=torch.randn(5, 128), cosine=True), dict(target=torch.zeros(1, 128, 128, dtype=torch.long)),
               dict(predict=True), dict(confusion=True), dict(regress=torch.zeros(1, 128, 128, 128)), dict(return_weights=True), dict(cosine=True)):
        with pytest.raises(ValueError, match="does not combine"):
            call(**kw)
    with pytest.raises(ValueError, match="mask_reduce"):
        call(mask_reduce="max")
    with pytest.raises(ValueError, match="mask_path"):
        call(mask_path="quick")
    with pytest.raises(ValueError, match="masks must be"):
        call(masks=M[:, :, :64])
    with pytest.raises(ValueError, match="masks must be"):
        call(masks=M[0])
    with pytest.raises(ValueError, match="masks must be"):
        call(masks=M[:, :0])
    with pytest.raises(ValueError, match="masks must be"):
        call(masks=torch.zeros(2, 3, 128, 128, dtype=torch.bool))
    with pytest.raises(TypeError, match="masks must be"):
        call(masks=M.long())
    with pytest.raises(TypeError, match="must be a tensor"):
        call(masks=[[1]])
    with pytest.raises(ValueError, match="masks on"):
        call(masks=M.to("meta"))
    with pytest.raises(ValueError, match="no gradient"):
        call(masks=M.float().requires_grad_(True))
    with pytest.raises(ValueError, match="goes with masks"):
        m(img, ft, (128, 128), return_attention=True)
    for ok in (M, M.to(torch.uint8), M.to(torch.bfloat16), M.half(), M.float()):
        with pytest.raises(RuntimeError, match="ROCm device"):      # a valid call gets as far as the device check, and no further
            call(masks=ok)
