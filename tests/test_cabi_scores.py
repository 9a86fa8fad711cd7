"""C ABI 0.4.3: the attention backward with a gradient of the scores (naf_xna_bwd_scores / naf_xna_bwd_scores_supported).

Host-side checks only (no device call): the entry points are declared, exported and bound, the argument struct matches the header, the
kernel choice for a table of shapes with and without a score gradient, and every validation error.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("naf_xna_bwd_scores", "naf_xna_bwd_scores_supported")


def _xna_bwd_args(h, w, Ho, Wo, Cc, k, heads=4, B=1, Dq=64, path=0):
    from naf_amd._lib import XnaBwdArgs, I64x4
    a = XnaBwdArgs()
    Dv = Cc // heads
    a.q = a.k_lr = a.v_lr = a.dout = a.dq = a.dk_lr = a.dv_lr = 0x1000      # host logic only: never dereferenced
    a.B, a.heads, a.Ho, a.Wo, a.h, a.w, a.Dq, a.Dv, a.ky, a.kx = B, heads, Ho, Wo, h, w, Dq, Dv, k, k
    a.scale, a.path = 0.0, path
    a.q_stride = a.dq_stride = I64x4(Ho * Wo * heads * Dq, Dq, Wo * heads * Dq, heads * Dq)
    a.k_stride = I64x4(h * w * heads * Dq, Dq, w * heads * Dq, heads * Dq)
    a.v_stride = I64x4(h * w * heads * Dv, Dv, w * heads * Dv, heads * Dv)
    a.dout_stride = I64x4(Ho * Wo * heads * Dv, Dv, Wo * heads * Dv, heads * Dv)
    return a


def _scores_args(a, ptr=0x2000):
    """Dense [B, heads, Ho, Wo, ky*kx] score gradient for the shapes of `a`."""
    from naf_amd._lib import XnaBwdScoresArgs, I64x4
    kk = a.ky * a.kx
    s = XnaBwdScoresArgs()
    s.dlogits = ptr
    s.dlogits_stride = I64x4(a.heads * a.Ho * a.Wo * kk, a.Ho * a.Wo * kk, a.Wo * kk, kk)
    return s


def test_scores_entry_points_are_declared_exported_and_bound(built_lib):
    from naf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert name in exported, name
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"#define NAF_HIP_VERSION 403\b", hdr)
    assert _lib.HEADER_VERSION == 403 and lib.naf_version() == 403


def test_scores_struct_layout_matches_header(built_lib):
    from naf_amd import _lib
    src = ('#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu\\n", '
           'sizeof(naf_xna_bwd_scores_args), offsetof(naf_xna_bwd_scores_args, dlogits), '
           'offsetof(naf_xna_bwd_scores_args, dlogits_stride));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        size, off_p, off_s = map(int, subprocess.check_output([os.path.join(d, "p")]).split())
    S = _lib.XnaBwdScoresArgs
    assert size == C.sizeof(S) == 40
    assert off_p == S.dlogits.offset and off_s == S.dlogits_stride.offset


# (h, w, Ho, Wo, C, k, kwargs) -> (kernel without a score gradient, kernel with one)
SHAPES = [
    ((64, 64, 1024, 1024, 768, 7, {}), ("MFMA", "MFMA")),                    # G1: cell kernel
    ((28, 28, 448, 448, 384, 9, {}), ("MFMA", "MFMA")),                      # REF448
    ((32, 32, 512, 512, 1024, 15, {}), ("MFMA", "MFMA")),                    # channel chunks
    ((28, 28, 392, 392, 384, 9, {}), ("MFMA", "MFMA")),                      # partial row tiles (14-pixel cells)
    ((16, 16, 32, 32, 768, 9, {}), ("ROWS", "ROWS")),                        # integer ratio 2 (the reference's training step)
    ((32, 32, 32, 32, 3, 15, {"heads": 1, "Dq": 96}), ("ROWS", "ROWS")),     # ratio 1, one head of Dq 96 (the denoising call)
    ((28, 28, 392, 392, 384, 11, {}), ("ROWS", "ROWS")),                     # patch-14 ratio at 11 x 11
    ((13, 13, 32, 32, 128, 7, {}), ("ROWS", "GENERIC")),                     # non-integer ratio
    ((24, 20, 24, 20, 3, 5, {"heads": 1, "Dq": 80}), ("GENERIC", "GENERIC")),  # Dq != 64 without a matrix-core instantiation
]


@pytest.mark.parametrize("geom,want", SHAPES)
def test_scores_supported_table(built_lib, geom, want):
    from naf_amd import _lib
    lib = _lib.load()
    *g, kw = geom
    a = _xna_bwd_args(*g, **kw)
    code = {"MFMA": _lib.XNA_MFMA, "ROWS": _lib.XNA_ROWS, "GENERIC": _lib.XNA_GENERIC}
    assert lib.naf_xna_bwd_supported(C.byref(a)) == code[want[0]]
    assert lib.naf_xna_bwd_scores_supported(C.byref(a), None) == code[want[0]]          # no score gradient: naf_xna_bwd's choice
    empty = _scores_args(a, ptr=0)
    assert lib.naf_xna_bwd_scores_supported(C.byref(a), C.byref(empty)) == code[want[0]]
    assert lib.naf_xna_bwd_scores_supported(C.byref(a), C.byref(_scores_args(a))) == code[want[1]]


def test_scores_supported_honours_path(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    a = _xna_bwd_args(16, 16, 32, 32, 768, 9, path=_lib.XNA_ROWS)
    assert lib.naf_xna_bwd_scores_supported(C.byref(a), C.byref(_scores_args(a))) == _lib.XNA_ROWS
    a = _xna_bwd_args(13, 13, 32, 32, 128, 7, path=_lib.XNA_ROWS)       # repeated taps: no row-streaming score form
    assert lib.naf_xna_bwd_scores_supported(C.byref(a), C.byref(_scores_args(a))) == -2
    assert "integer ratios" in _lib.last_error()
    a = _xna_bwd_args(64, 64, 1024, 1024, 768, 7, path=_lib.XNA_GENERIC)
    assert lib.naf_xna_bwd_scores_supported(C.byref(a), C.byref(_scores_args(a))) == _lib.XNA_GENERIC
    a = _xna_bwd_args(64, 64, 1024, 1024, 768, 7)
    s = _scores_args(a)
    s.dlogits_stride[3] = 1 << 26                                        # a cell's queries 2^30 elements apart: table-driven kernel
    s.dlogits_stride[2] = 1 << 40
    s.dlogits_stride[1] = s.dlogits_stride[0] = 1 << 50
    assert lib.naf_xna_bwd_scores_supported(C.byref(a), C.byref(s)) == _lib.XNA_GENERIC


def test_scores_validation_without_a_device(built_lib):
    """Every refusal returns a status and names the bad field through naf_last_error; nothing touches a device."""
    from naf_amd import _lib
    lib = _lib.load()
    a = _xna_bwd_args(64, 64, 1024, 1024, 768, 7)

    def refused(s, needle, args=a):
        rc = lib.naf_xna_bwd_scores_supported(C.byref(args) if args is not None else None, C.byref(s) if s is not None else None)
        assert rc == -1, (rc, needle)
        assert needle in _lib.last_error(), (_lib.last_error(), needle)
        rc = lib.naf_xna_bwd_scores(C.byref(args) if args is not None else None, C.byref(s) if s is not None else None, None)
        assert rc == 1, (rc, needle)
        assert needle in _lib.last_error(), (_lib.last_error(), needle)

    refused(_scores_args(a), "args is NULL", args=None)
    bad = _xna_bwd_args(64, 64, 1024, 1024, 768, 7)
    bad.dq = 0
    refused(_scores_args(bad), "NULL tensor pointer", args=bad)
    refused(_scores_args(a, ptr=0x2002), "dlogits must be 4-byte aligned")
    s = _scores_args(a)
    s.dlogits_stride[1] = -49
    refused(s, "dlogits_stride[1] (head) is negative")
    s = _scores_args(a)
    s.dlogits_stride[3] = -1
    refused(s, "dlogits_stride[3] (x) is negative")
    # read only: any non-negative strides serve -- 0 (a gradient expanded over the image, e.g. of a loss on scores.sum(dim=(2, 3))) and rows
    # that overlap
    s = _scores_args(a)
    s.dlogits_stride[2] = s.dlogits_stride[3] = 0
    assert lib.naf_xna_bwd_scores_supported(C.byref(a), C.byref(s)) == _lib.XNA_MFMA
    s.dlogits_stride[2], s.dlogits_stride[3] = 7, 1
    assert lib.naf_xna_bwd_scores_supported(C.byref(a), C.byref(s)) == _lib.XNA_MFMA
    # NULL args with no score gradient: exactly naf_xna_bwd's refusal
    assert lib.naf_xna_bwd_scores(None, None, None) == lib.naf_xna_bwd(None, None) == 1
