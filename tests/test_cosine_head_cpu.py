"""CPU tests of the cosine head's yardstick (tests/cosine_reference.py) and of its host-side surface: the fp64 restatement against
F.cosine_similarity on the oracle's attention, argmax invariance, planted defects against the bound, what naf_xna_cos_select grants for
the GPU case list, the exported symbols, the struct layout and the refusals of ``naf(..., cosine=True)`` that need no device."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_reference as R  # noqa: E402
import input_statistics as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = "b_whole_grid_n1", "e_patch14_n21", "f_rows30_n151", "h_three_heads_n1"


@pytest.fixture(scope="module")
def lib():
    from naf_amd import _lib
    return _lib.load()


def _ref(name, **kw):
    B, heads, Dv, lr, cell, ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name, **kw)
    return (q, k, v, E, ks, heads), R.reference(q, k, v, E, ks, heads)


@pytest.mark.parametrize("name", SMALL)
def test_restatement_equals_cosine_similarity_on_the_oracle(name):
    """The cell-wise fp64 restatement == F.cosine_similarity(oracle attention, E) within 1e-6 (fp32 comparison), its feature and abs-sum
    == tests/input_statistics.attention_reference."""
    (q, k, v, E, ks, heads), r = _ref(name)
    out, abs_sum = S.attention_reference(q, k, v, ks, heads)
    assert float((r["f"] - out).abs().max()) <= 1e-12 * max(1.0, float(out.abs().max()))
    assert float((r["a_f"] - abs_sum).abs().max()) <= 1e-12 * max(1.0, float(abs_sum.abs().max()))
    want = F.cosine_similarity(out.float().unsqueeze(1), F.normalize(E.float(), dim=1)[None, :, :, None, None], dim=2, eps=1e-12)
    assert float((r["cos"].float() - want).abs().max()) <= 1e-6
    c2, n2 = R.cosine_from_features64(out, E)
    assert float((c2 - r["cos"]).abs().max()) <= 1e-12 and float((n2 - r["norms"]).abs().max()) <= 1e-12 * float(n2.max())
    assert float(r["cos"].abs().max()) <= 1.0 + 1e-12


def test_labels_do_not_see_the_norm():
    """argmax_n cos == argmax_n E^ . f: the per-pixel positive scale does not move the argmax (predict / confusion run on E^)."""
    (q, k, v, E, ks, heads), r = _ref("e_patch14_n21")
    lin = torch.einsum("nc,bchw->bnhw", r["e_hat"], r["f"])
    assert torch.equal(r["cos"].argmax(1), lin.argmax(1))
    assert torch.equal((7.5 * r["cos"]).argmax(1), lin.argmax(1))


def test_emulated_kernel_is_inside_the_bound():
    for name in SMALL:
        (q, k, v, E, ks, heads), r = _ref(name)
        cos, nrm = R.emulate(q, k, v, E, ks, heads)
        R.check(cos, r["cos"], R.bound(r), f"emulated {name}")
        R.check(nrm, r["norms"], R.norms_bound(r), f"emulated norms {name}")


@pytest.mark.parametrize("defect,kw", [
    ("norm_per_head", dict(norm_per_head=True)),      # input: the unit case, three heads of equal weight -- the per-head norms are ~sqrt(3) smaller
    ("drop_head", dict(drop_head=1)),                 # input: the same -- a third of the squared norm is missing
    ("raw_embeddings", dict(raw_embeddings=True)),    # input: the same -- make_inputs scales E by 3, its rows have norm ~ 3 sqrt(C)
])
def test_planted_defects_leave_the_bound(defect, kw):
    (q, k, v, E, ks, heads), r = _ref("h_three_heads_n1")
    cos, _ = R.emulate(q, k, v, E, ks, heads, **kw)
    n_out = R.outside(cos, r["cos"], R.bound(r))
    assert n_out > 0.5 * cos.numel(), f"{defect}: only {n_out}/{cos.numel()} elements leave the bound"


def test_clamp_on_the_squared_norm_leaves_the_bound():
    """Input: features scaled by 2^-30 (norms ~ 1e-8: above 1e-12, their squares below it).  Right: the cosines of the unscaled input,
    bit for bit in the emulation.  Clamping the squared norm divides by 1e-6 instead."""
    name = "e_patch14_n21"
    B, heads, Dv, lr, cell, ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name)
    vs = v * 2.0 ** -30
    r = R.reference(q, k, vs, E, ks, heads)
    assert 1e-12 < float(r["norms"].min()) and float(r["norms"].max()) < 1e-6
    good, _ = R.emulate(q, k, vs, E, ks, heads)
    R.check(good, r["cos"], R.bound(r), "tiny features")
    assert torch.equal(good, R.emulate(q, k, v, E, ks, heads)[0])
    bad, _ = R.emulate(q, k, vs, E, ks, heads, clamp_squared=True)
    assert R.outside(bad, r["cos"], R.bound(r)) > 0.9 * bad.numel()


def test_zero_feature_pixels_are_zero_and_nan_leaves_the_bound():
    """Input: a block of zero features as wide as the window plus one; the pixels of the cells whose window lies inside it see only zeros."""
    name = "e_patch14_n21"
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    blk = (0, 6, 0, 6)
    q, k, v, E = R.make_inputs(name, zero_block=blk)
    m = R.sees_only(blk, h, w, ks).repeat_interleave(dy, 0).repeat_interleave(dx, 1)
    assert int(m.sum()) >= dy * dx
    r = R.reference(q, k, v, E, ks, heads)
    assert float(r["norms"][:, m].abs().max()) == 0.0 and float(r["cos"][:, :, m].abs().max()) == 0.0
    assert float(R.bound(r)[:, :, m].max()) == 0.0            # exact zero is asked for there
    good, nrm = R.emulate(q, k, v, E, ks, heads)
    assert float(good[:, :, m].abs().max()) == 0.0 and float(nrm[:, m].max()) == 0.0 and bool(torch.isfinite(good).all())
    R.check(good, r["cos"], R.bound(r), "zero block")
    bad, _ = R.emulate(q, k, v, E, ks, heads, zero_nan=True)
    assert bool(torch.isnan(bad[:, :, m]).all())
    assert R.outside(bad, r["cos"], R.bound(r)) == int(m.sum()) * N * B


def test_constant_features_collapse_the_bound_to_the_pv_rounding():
    """Every cell holds the same vector v: cos[n] = cos(E_n, v) at every pixel, the bound is the PV rounding plus fp32 terms."""
    name = "h_three_heads_n1"
    B, heads, Dv, lr, cell, ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name, const_v=True)
    r = R.reference(q, k, v, E, ks, heads)
    v0 = v[0, :, 0, 0].double()
    want = (F.normalize(E.float(), dim=1).double() @ v0) / v0.norm()          # E^ is normalised in fp32 by definition
    assert float((r["cos"] - want.view(1, N, 1, 1)).abs().max()) <= 1e-12
    cos, _ = R.emulate(q, k, v, E, ks, heads)
    R.check(cos, r["cos"], R.bound(r), "constant features")


# ---- the host-side surface --------------------------------------------------------------------------------------
def _select(name_or_geom, N=None, Dv=None):
    from naf_amd import ops
    B, heads, dv, (h, w), (dy, dx), ks, n = R.CASES[name_or_geom] if isinstance(name_or_geom, str) else name_or_geom
    qp = torch.empty((B, h * dy, w * dx, heads, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    return ops.xna_cos_select(qp, (h, w), Dv or dv, N or n, ks)


def test_gpu_case_list_reaches_every_instantiation(lib):
    """naf_xna_cos_select is host-only: every GPU case is granted the fused kernel, and together they reach every window any
    instantiation serves, every channel-tile count, whole and chunked value widths, and partial row tiles."""
    from naf_amd import _lib
    assert all(_select(n) == "fused" for n in R.CASES), [n for n in R.CASES if _select(n) != "fused"]
    served = {(ks, nct) for ks in R.WINDOWS for nct, n in ((2, 21), (4, 40), (10, 151), (16, 256))
              if _select((1, 2, 32, (16, 16), (1, 16), ks, n)) == "fused"}
    assert {ks for ks, _ in served} == {c[5] for c in R.CASES.values()} == set(R.WINDOWS)
    assert {nct for _, nct in served} == {R.NCT_OF(c[6]) for c in R.CASES.values()} == {2, 4, 10, 16}
    # what is refused is refused as "unsupported" with the reason, and it is the wide heads at the two largest windows
    assert {(ks, nct) for ks in R.WINDOWS for nct in (2, 4, 10, 16)} - served == {(13, 10), (13, 16), (15, 10), (15, 16)}
    assert _select((1, 2, 32, (16, 16), (1, 16), 15, 151)) == "composed" and "window 15" in _lib.last_error()
    dvs = {c[2] for c in R.CASES.values()}
    assert any(d <= 64 for d in dvs) and any(d > 64 and d % 64 == 0 for d in dvs) and any(d % 64 for d in dvs)
    assert any(c[4][1] % 16 for c in R.CASES.values()) and any(c[4][0] * ((c[4][1] + 15) // 16) > 16 for c in R.CASES.values())
    widths = [c[6] for c in R.CASES.values()]
    assert all(widths.count(n) >= 2 for n in (1, 21, 151, 256))


def test_select_refuses_what_the_composition_serves(lib):
    from naf_amd import _lib, ops
    g = (1, 4, 32, (8, 8), (16, 16), 7, 21)
    assert _select(g) == "fused"
    assert _select(g, Dv=24) == "composed" and "multiple of 16" in _lib.last_error()
    assert _select((1, 4, 32, (8, 8), (1, 1), 7, 21)) == "composed"                      # ratio 1: no row tiles
    qp = torch.empty((1, 64, 64, 4, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    assert ops.xna_cos_select(qp, (28, 28), 96, 21, 7) == "composed" and "integer ratio" in _lib.last_error()
    assert ops.xna_cos_select(qp, (8, 8), 96, 21, 7, value_dtype=torch.float16) == "composed"
    assert ops.xna_cos_select(qp, (8, 8), 96, 257, 7) == "composed"
    q96 = torch.empty((1, 64, 64, 4, 96), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    assert ops.xna_cos_select(q96, (8, 8), 96, 21, 7) == "composed" and "Dq = 64" in _lib.last_error()
    with pytest.raises(ValueError, match="odd"):
        ops.xna_cos_select(qp, (8, 8), 96, 21, 8)


def test_c_entry_validates_its_arguments(lib):
    """naf_xna_cos_select on hand-filled structs: INVALID (-1) for NULL, a bad N, non-zero reserved, a non-finite logit_scale, a v_lr row
    shorter than Dv; naf_xna_cos_fwd refuses the same before any launch."""
    from naf_amd import _lib

    def args(**kw):
        a = _lib.XnaCosArgs()
        a.q = a.k_lr = a.pv_lr = a.v_lr = a.out = 4096
        a.B, a.heads, a.Ho, a.Wo, a.h, a.w, a.Dq, a.Dv, a.N, a.ky, a.kx = 1, 2, 128, 128, 8, 8, 64, 32, 21, 7, 7
        a.logit_scale = 1.0
        a.q_stride = _lib.I64x4(128 * 128 * 128, 64, 128 * 128, 128)
        a.k_stride = _lib.I64x4(8 * 8 * 128, 64, 8 * 128, 128)
        a.pv_stride = _lib.I64x4(2 * 8 * 8 * 32, 8 * 8 * 32, 8 * 32, 32)
        a.v_stride = _lib.I64x4(8 * 8 * 64, 32, 8 * 64, 64)
        a.o_stride = _lib.I64x3(128 * 128 * 21, 128 * 21, 21)
        for k_, v_ in kw.items():
            setattr(a, k_, v_)
        return a

    assert lib.naf_xna_cos_select(C.byref(args())) == _lib.XNA_HEAD_FUSED
    assert lib.naf_xna_cos_select(C.byref(args(norms=4096, norms_stride=_lib.I64x3(128 * 128, 128, 1)))) == _lib.XNA_HEAD_FUSED
    for bad in (dict(v_lr=None), dict(out=None), dict(N=0), dict(N=257), dict(reserved=(C.c_int32 * 2)(0, 1)), dict(logit_scale=float("inf")),
                dict(logit_scale=float("nan")), dict(ky=8, kx=8), dict(v_stride=_lib.I64x4(8 * 8 * 64, 32, 8 * 64, 16)), dict(path=2),
                dict(o_stride=_lib.I64x3(128 * 128 * 21, 128 * 21, 20))):
        assert lib.naf_xna_cos_select(C.byref(args(**bad))) == -1, bad
        assert lib.naf_xna_cos_fwd(C.byref(args(**bad)), None) == 1, bad
    assert lib.naf_xna_cos_select(C.byref(args(v_lr=4100))) == -2 and "aligned" in _lib.last_error()
    assert lib.naf_xna_cos_select(C.byref(args(v_stride=_lib.I64x4(8 * 8 * 68, 32, 8 * 68, 68)))) == -2
    assert lib.naf_xna_cos_select(C.byref(args(Ho=100))) == -2


def test_header_declares_and_library_exports_the_entries(lib):
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    raw = C.CDLL(os.path.join(ROOT, "naf_amd", "csrc", "libnaf_hip.so"))
    for sym in ("naf_xna_cos_select", "naf_xna_cos_fwd"):
        assert f"int {sym}(const naf_xna_cos_args* a" in txt
        assert getattr(raw, sym) is not None
    assert int(__import__("re").search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403      # detected by symbol, not by version


def test_struct_layout_matches_the_header(tmp_path):
    from naf_amd import _lib
    fields = ["q", "v_lr", "norms", "rope_tab_x", "B", "Dv", "N", "kx", "path", "scale", "logit_scale", "reserved", "q_stride", "v_stride",
              "o_stride", "norms_stride"]
    body = 'printf("%zu", sizeof(naf_xna_cos_args));' + "".join(f'printf(" %zu", offsetof(naf_xna_cos_args, {f}));' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.XnaCosArgs)] + [getattr(_lib.XnaCosArgs, f).offset for f in fields]


def test_cosine_calls_are_refused_before_any_device_work():
    """Every refusal of ``naf(..., cosine=True)`` on CPU tensors: they come before the 'runs only on a ROCm device' error, so nothing
    was launched."""
    from torch import nn
    from naf_amd import NAF
    m = NAF(kernel_size=7).eval()
    img, ft = torch.zeros(1, 3, 128, 128), torch.zeros(1, 128, 8, 8, dtype=torch.bfloat16)
    E = torch.randn(5, 128)
    call = lambda **kw: m(img, ft, (128, 128), **{"head": E, "cosine": True, **kw})
    with pytest.raises(ValueError, match="no bias"):
        call(head=nn.Conv2d(128, 5, 1))
    with pytest.raises(ValueError, match="no bias"):
        call(head=(E, torch.zeros(5)))
    with pytest.raises(ValueError, match="confusion"):
        call(target=torch.zeros(1, 128, 128, dtype=torch.long))
    with pytest.raises(ValueError, match="regress"):
        call(regress=torch.zeros(1, 128, 128, 128))
    with pytest.raises(ValueError, match="return_weights"):
        m(img, ft, (128, 128), True, head=E, cosine=True)
    with pytest.raises(ValueError, match="cosine_path"):
        call(cosine_path="quick")
    with pytest.raises(ValueError, match="needs the embeddings"):
        call(head=None)
    with pytest.raises(ValueError, match="128 channels"):
        call(head=torch.randn(5, 64))
    with pytest.raises(TypeError, match="cosine=True: head must be"):
        call(head="text")
    with pytest.raises(ValueError, match="return_norms"):
        call(predict=True, return_norms=True)
    with pytest.raises(ValueError, match="finite"):
        call(logit_scale=float("nan"))
    with pytest.raises(RuntimeError, match="ROCm device"):      # a valid call gets as far as the device check, and no further
        call()
    for ok in (nn.Conv2d(128, 5, 1, bias=False), nn.Linear(128, 5, bias=False), (E, None), E.half(), E.double()):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call(head=ok)
