"""CPU tests of the point queries and of ``Guidance``'s host side: the fp64 gather restatement (tests/points_reference.py) against the
oracle's dense attention at the same pixels, the argument validation of ``NAF.query`` / ``NAF.guide`` / ``ops.xna_points`` (everything
that is decided before a device is touched), and the C boundary of naf_xna_points.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_reference as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_gather_restatement_matches_the_oracle(name):
    """One pixel of O.xna (dense, fp64) = the gather of that pixel's window: scores, softmax, features, and the windows are the table rows."""
    c = PR.CASES[name]
    B = 2
    q, k, v = PR.inputs(name, B)
    heads, ksz = c["heads"], c["ksz"]
    vv = v if v is not None else torch.zeros(B, heads, *c["lr"])
    ref_out, ref_lg = O.xna(q.double(), k.double(), vv.double(), ksz, heads, return_logits=True)
    pts = PR.make_points(B, *c["out"], 29)
    lg, pr, out, abs_sum, wy, wx = PR.point_query(q, k, v, pts, ksz, heads)
    iy, ix = O.axis_index_table(c["out"][0], c["lr"][0], ksz), O.axis_index_table(c["out"][1], c["lr"][1], ksz)
    assert len({tuple(p) for p in pts.tolist()}) < len(pts) and set(pts[:, 0].tolist()) == {0, 1}        # duplicates, both images
    for n, (b, y, x) in enumerate(pts.tolist()):
        want = ref_lg[b, :, y, x]
        assert float((lg[n] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        assert float((pr[n] - want.softmax(-1)).abs().max()) <= 1e-13
        assert abs(float(pr[n].sum(-1).max()) - 1.0) <= 1e-13
        if v is not None:
            assert float((out[n] - ref_out[b, :, y, x]).abs().max()) <= 1e-12 * max(1.0, float(ref_out[b, :, y, x].abs().max()))
            assert bool((abs_sum[n] >= out[n].abs() - 1e-12).all())
        assert wy[n].tolist() == iy[y].tolist() and wx[n].tolist() == ix[x].tolist()
    if name == "b":
        assert any(len(set(r.tolist())) < ksz for r in iy)          # F4's ratio: a window repeats a low-res row


def test_gather_restatement_marks_points_outside_the_grid():
    q, k, v = PR.inputs("a", 1)
    pts = torch.tensor([[0, 3, 4], [1, 0, 0], [0, -1, 2], [0, 24, 0], [0, 0, 32], [-1, 0, 0]])
    lg, pr, out, abs_sum, wy, wx = PR.point_query(q, k, v, pts, 5, 2)
    assert bool(torch.isfinite(lg[0]).all()) and bool(torch.isfinite(out[0]).all())
    for n in range(1, 6):
        assert bool(torch.isnan(lg[n]).all()) and bool(torch.isnan(pr[n]).all()) and bool(torch.isnan(out[n]).all())
        assert wy[n].tolist() == [-1] * 5 and wx[n].tolist() == [-1] * 5


# ---- argument validation: decided on the host, before any device work ------------------------------------------------------------
def _model():
    from naf_amd import NAF
    return NAF(kernel_size=5).eval()


def test_guide_has_no_cpu_fallback():
    m = _model()
    with pytest.raises(RuntimeError, match="ROCm"):
        m.guide(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="ROCm"):
        m.guide(torch.zeros(1, 3, 16, 16), (16, 16))
    with pytest.raises(ValueError, match="image"):
        m.guide(torch.zeros(3, 16, 16))
    with pytest.raises(ValueError, match="image"):
        m.guide("image.png")


def test_query_validates_its_arguments():
    import naf_amd
    m = _model()
    img, ft = torch.zeros(1, 3, 32, 32), torch.zeros(1, 8, 8, 8)
    pts = torch.tensor([[0, 1, 2]])
    with pytest.raises(ValueError, match="weights"):
        m.query(img, pts, features=ft, output_size=(32, 32), weights="probabilities")
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64), [[0, 1, 2]]):
        with pytest.raises(ValueError, match="points"):
            m.query(img, bad, features=ft, output_size=(32, 32))
    with pytest.raises(TypeError, match="integer"):
        m.query(img, pts.float(), features=ft, output_size=(32, 32))
    with pytest.raises(ValueError, match="output_size"):
        m.query(img, pts, features=ft)
    with pytest.raises(ValueError, match="lr_size"):
        m.query(img, pts, output_size=(32, 32))                                    # neither features nor lr_size
    with pytest.raises(ValueError, match="contradicts"):
        m.query(img, pts, features=ft, output_size=(32, 32), lr_size=(4, 4))
    with pytest.raises(ValueError, match=r"\[B, C, h, w\]"):
        m.query(img, pts, features=ft[0], output_size=(32, 32))
    with pytest.raises(ValueError, match="not divisible"):
        m.query(img, pts, features=torch.zeros(1, 6, 8, 8), output_size=(32, 32))
    with pytest.raises(ValueError, match="nothing asked"):
        m.query(img, pts, output_size=(32, 32), lr_size=(8, 8), weights=None)
    # everything well formed: the device is asked for, and there is none to fall back from
    with pytest.raises(RuntimeError, match="ROCm"):
        m.query(img, pts, features=ft, output_size=(32, 32), weights="both")
    with pytest.raises(RuntimeError, match="ROCm"):
        m.query(img, pts[:, 1:], output_size=(32, 32), lr_size=(8, 8))
    assert naf_amd.Guidance is not None and naf_amd.PointQuery._fields == ("features", "logits", "probs", "window_y", "window_x")


def test_xna_points_validates_its_arguments():
    from naf_amd import ops
    bf = torch.bfloat16
    q, k, v = torch.zeros(1, 2, 8, 8, 64, dtype=bf), torch.zeros(1, 2, 4, 4, 64, dtype=bf), torch.zeros(1, 2, 4, 4, 24, dtype=bf)
    pts = torch.zeros(3, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="5-D"):
        ops.xna_points(q[0], k, v, pts, 3)
    with pytest.raises(ValueError, match="contiguous"):
        ops.xna_points(q, k.transpose(3, 4), v, pts, 3)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.xna_points(q.float(), k, v, pts, 3)
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        ops.xna_points(q, k, v.float(), pts, 3)
    with pytest.raises(ValueError, match="k_lr shape"):
        ops.xna_points(q, k[:, :1], v, pts, 3)
    with pytest.raises(ValueError, match="v_lr shape"):
        ops.xna_points(q, k, v[:, :, :3], pts, 3)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        ops.xna_points(q, k, v, pts[:, :2], 3)
    with pytest.raises(TypeError, match="int32"):
        ops.xna_points(q, k, v, pts.long(), 3)
    with pytest.raises(ValueError, match="nothing to compute"):
        ops.xna_points(q, k, None, pts, 3, want_logits=False)
    with pytest.raises(ValueError, match="needs the values"):
        ops.xna_points(q, k, None, pts, 3, out=torch.zeros(3, 48))
    with pytest.raises(ValueError, match="logits must be"):
        ops.xna_points(q, k, v, pts, 3, logits=torch.zeros(3, 2, 8))
    with pytest.raises(ValueError, match="out must be"):
        ops.xna_points(q, k, v, pts, 3, out=torch.zeros(3, 48, dtype=torch.float64))
    with pytest.raises(ValueError, match="rope_tables"):
        ops.xna_points(q, k, v, pts, 3, rope_tables=(torch.zeros(8, 2, 8), torch.zeros(8, 2, 16)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.xna_points(q, k, v, pts, 3)


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_naf_xna_points(built_lib):
    import subprocess
    import tempfile
    from naf_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "naf_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+naf_xna_points\s*\(\s*const\s+naf_xna_points_args\s*\*\s*a\s*,\s*naf_stream_t\s+stream\s*\)\s*;", txt)
    lib = C.CDLL(built_lib)
    assert hasattr(lib, "naf_xna_points")
    assert "naf_xna_points" in _lib.SIGNATURES
    src = ('#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu\\n", sizeof(naf_xna_points_args), '
           'offsetof(naf_xna_points_args, N), offsetof(naf_xna_points_args, v_stride));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        size, off_n, off_vs = map(int, subprocess.check_output([os.path.join(d, "p")]).split())
    assert size == C.sizeof(_lib.XnaPointsArgs) and off_n == _lib.XnaPointsArgs.N.offset and off_vs == _lib.XnaPointsArgs.v_stride.offset


def test_naf_xna_points_refuses_bad_arguments_without_a_device(built_lib):
    """Invalid arguments come back as a naf_status with naf_last_error set; N = 0 is NAF_OK and launches nothing (no device is touched:
    the pointers below are never dereferenced)."""
    from naf_amd import _lib
    lib = _lib.load()

    def args(**kw):
        a = _lib.XnaPointsArgs()
        a.q = a.k_lr = a.v_lr = a.points = a.idx_y = a.idx_x = a.logits = 0x1000
        a.N, a.B, a.heads, a.Ho, a.Wo, a.h, a.w, a.Dq, a.Dv, a.ky, a.kx = 0, 1, 2, 8, 8, 4, 4, 64, 24, 3, 3
        a.q_stride, a.k_stride, a.v_stride = _lib.I64x4(8192, 64, 1024, 128), _lib.I64x4(2048, 64, 512, 128), _lib.I64x4(768, 24, 192, 48)
        for n, v in kw.items():
            setattr(a, n, v)
        return a

    assert lib.naf_xna_points(C.byref(args()), None) == 0                                   # N = 0
    assert lib.naf_xna_points(None, None) == 1 and "NULL" in _lib.last_error()
    for kw, word in ((dict(N=-1), "N = -1"), (dict(reserved=7), "reserved"), (dict(heads=0), "at least 1"), (dict(ky=0), "at least 1"),
                     (dict(logits=None), "no output"), (dict(out=0x1000, v_lr=None), "v_lr"), (dict(v_dtype=1), "v_dtype"),
                     (dict(rope_tab_y=0x1000), "go together"), (dict(rope_tab_y=0x1000, rope_tab_x=0x1000, Dq=62), "multiple of 4"),
                     (dict(k_stride=_lib.I64x4(2048, -64, 512, 128)), "non-negative")):
        assert lib.naf_xna_points(C.byref(args(**kw)), None) == 1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert lib.naf_xna_points(C.byref(args(ky=63, kx=63, Dq=512)), None) == 2 and "LDS" in _lib.last_error()
