"""CPU tests of the fused linear head (``naf(image, feats, size, head=probe)``): the C ABI of the head-summed attention
(header, ctypes mirror, exports, struct layout, host-side select policy), the low-res projection against the oracle identity
    head(naf(V))[n, px] = b[n] + sum_g sum_slot P_g[px, slot] * PV_g[n, cell(slot)],   PV_g = W[:, g*Dv:(g+1)*Dv] @ V_g
and the validation of the ``head`` argument.  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest
import torch
from torch import nn

from oracle import naf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_SYMBOLS = ("naf_xna_head_select", "naf_xna_head_workspace_bytes", "naf_xna_head_fwd")


def _header_text():
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_ctypes_and_exports_agree(built_lib):
    from naf_amd import _lib
    txt = _header_text()
    lib = C.CDLL(built_lib)
    for name in HEAD_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*const naf_xna_head_args\s*\*" % name, txt), f"{name} is not declared in include/naf_hip.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"libnaf_hip.so does not export {name}"
        assert _lib.SIGNATURES[name][1][0] == C.POINTER(_lib.XnaHeadArgs)
    assert _lib.SIGNATURES["naf_xna_head_select"][0] == C.c_int and _lib.SIGNATURES["naf_xna_head_fwd"][0] == C.c_int
    assert _lib.SIGNATURES["naf_xna_head_fwd"][1][1] == C.c_void_p
    assert _lib.SIGNATURES["naf_xna_head_workspace_bytes"][0] == C.c_size_t
    # the entries were added without a version bump (detected by symbol); naf_xna_args keeps its layout
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403 == _lib.HEADER_VERSION
    assert re.search(r"NAF_XNA_HEAD_AUTO\s*=\s*0", txt) and re.search(r"NAF_XNA_HEAD_FUSED\s*=\s*1", txt)
    assert (_lib.XNA_HEAD_AUTO, _lib.XNA_HEAD_FUSED) == (0, 1)


def test_head_struct_layout_matches_header(built_lib):
    """sizeof and the offset of every array / the first scalar of naf_xna_head_args against gcc's view of the header."""
    from naf_amd import _lib
    fields = ("q", "bias", "rope_tab_y", "B", "N", "out_dtype", "scale", "q_stride", "pv_stride", "o_stride")
    body = 'printf("%zu\\n", sizeof(naf_xna_head_args));' + "".join(f'printf("%zu\\n", offsetof(naf_xna_head_args, {f}));' for f in fields)
    body += 'printf("%zu\\n", sizeof(naf_xna_args));'
    src = '#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        vals = list(map(int, subprocess.check_output([os.path.join(d, "p")]).split()))
    assert vals[0] == C.sizeof(_lib.XnaHeadArgs)
    for f, off in zip(fields, vals[1:]):
        assert off == getattr(_lib.XnaHeadArgs, f).offset, f
    assert vals[-1] == C.sizeof(_lib.XnaArgs)


def _head_args(*, B=1, heads=4, lr=(9, 10), ratio=(16, 16), out=None, Dq=64, N=21, ky=7, kx=7, out_dtype=1, path=0):
    from naf_amd import _lib
    h, w = lr
    Ho, Wo = out if out is not None else (h * ratio[0], w * ratio[1])
    npad = (max(N, 1) + 15) // 16 * 16
    a = _lib.XnaHeadArgs()
    a.q = a.k_lr = a.pv_lr = a.out = 4096          # host-only query: pointers are checked, never read
    a.B, a.heads, a.Ho, a.Wo, a.h, a.w, a.Dq, a.N, a.ky, a.kx = B, heads, Ho, Wo, h, w, Dq, N, ky, kx
    a.out_dtype, a.path, a.scale = out_dtype, path, 0.0
    Cq = heads * Dq
    a.q_stride = _lib.I64x4(Ho * Wo * Cq, Dq, Wo * Cq, Cq)
    a.k_stride = _lib.I64x4(h * w * Cq, Dq, w * Cq, Cq)
    a.pv_stride = _lib.I64x4(heads * h * w * npad, h * w * npad, w * npad, npad)
    a.o_stride = _lib.I64x3(Ho * Wo * max(N, 1), Wo * max(N, 1), max(N, 1))
    return a


GRANTED = [dict(ky=k, kx=k, lr=(k + 2, k + 1)) for k in (3, 5, 7, 9, 11, 13, 15)] + [
    dict(N=1), dict(N=19), dict(N=151), dict(N=256), dict(out_dtype=0), dict(heads=1), dict(heads=12), dict(heads=3, B=3),
    dict(ratio=(14, 14)), dict(ratio=(7, 15)), dict(ratio=(3, 30)), dict(ratio=(14, 28)), dict(ratio=(32, 32)), dict(ratio=(1, 16)),
    dict(lr=(7, 7)), dict(path=1),
]


@pytest.mark.parametrize("kw", GRANTED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()).replace(" ", ""))
def test_select_grants_what_the_cell_kernel_serves(built_lib, kw):
    from naf_amd import _lib
    lib = _lib.load()
    a = _head_args(**kw)
    sel = lib.naf_xna_head_select(C.byref(a))
    assert sel == _lib.XNA_HEAD_FUSED, (kw, sel, _lib.last_error())
    assert lib.naf_xna_head_workspace_bytes(C.byref(a)) == 0


REFUSED = [
    ("ratio 2.5", dict(lr=(8, 8), out=(20, 20), ky=3, kx=3), 2),
    ("Dq 96", dict(Dq=96), 2),
    ("N 0", dict(N=0), 1),
    ("N 257", dict(N=257), 1),
    ("rectangular window", dict(ky=7, kx=5), 2),
    ("even window", dict(ky=4, kx=4), 1),
    ("window 17", dict(ky=17, kx=17, lr=(18, 18)), 2),
    ("grid smaller than the window", dict(lr=(5, 9), ky=7, kx=7), 1),
    ("cells of 4 pixels per row", dict(ratio=(4, 4)), 2),
    ("cells of 8 pixels per row", dict(ratio=(8, 8)), 2),
    ("bad path", dict(path=7), 1),
    ("bad dtype", dict(out_dtype=5), 1),
]


@pytest.mark.parametrize("what,kw,status", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_select_refuses_with_a_reason(built_lib, what, kw, status):
    from naf_amd import _lib
    lib = _lib.load()
    lib.naf_xna_head_select(C.byref(_head_args()))          # a granted call in between: the text below is this refusal's
    a = _head_args(**kw)
    sel = lib.naf_xna_head_select(C.byref(a))
    assert sel == -status, (what, sel)
    assert len(_lib.last_error()) > 0 and "naf_xna_head" in _lib.last_error()
    assert lib.naf_xna_head_fwd(C.byref(a), None) == status      # refused before any launch
    assert lib.naf_xna_head_select(None) == -1 and lib.naf_xna_head_fwd(None, None) == 1


def test_select_refuses_misaligned_and_null(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    a = _head_args()
    a.q = 4096 + 8
    assert lib.naf_xna_head_select(C.byref(a)) == -2 and "aligned" in _lib.last_error()
    a = _head_args()
    a.pv_lr = None
    assert lib.naf_xna_head_select(C.byref(a)) == -1 and "NULL" in _lib.last_error()
    a = _head_args()
    a.rope_tab_y = 4096
    assert lib.naf_xna_head_select(C.byref(a)) == -1 and "together" in _lib.last_error()
    a = _head_args(N=21)
    a.pv_stride = _lib.I64x4(4 * 90 * 24, 90 * 24, 10 * 24, 24)       # rows of 24 channels cannot hold Npad = 32
    assert lib.naf_xna_head_select(C.byref(a)) == -1 and "pv_lr" in _lib.last_error()


def _make_head(form, N, Cc, seed):
    w = O.hash_normal((N, Cc), seed) * (Cc ** -0.5)
    b = O.hash_normal((N,), seed + 1)
    if form == "conv":
        m = nn.Conv2d(Cc, N, 1)
        with torch.no_grad():
            m.weight.copy_(w[:, :, None, None])
            m.bias.copy_(b)
        return m, w, b
    if form == "linear":
        m = nn.Linear(Cc, N)
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        return m, w, b
    if form == "tuple4":
        return (w[:, :, None, None].clone(), None), w, None
    return (w.clone(), b.clone()), w, b


@pytest.mark.parametrize("form", ["conv", "linear", "tuple", "tuple4"])
@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("N", [1, 19, 21, 151])
def test_projection_commutes_with_the_attention(form, heads, N):
    """sum_g xna(q, k, PV)[g] + b == conv1x1(xna(q, k, v)) on the CPU oracle in fp32 (before the bf16 cast): the identity the
    fused path rests on.  6x7 cells, ratio 4, window 7, C = 64."""
    from naf_amd import ops
    from naf_amd.model import _linear_head
    B, Cc, h, w, d, ksz = 1, 64, 6, 7, 4, 7
    Cq = heads * 64
    q = O.hash_normal((B, Cq, h * d, w * d), 11)
    k = O.hash_normal((B, Cq, h, w), 12)
    v = O.hash_normal((B, Cc, h, w), 13)
    head, wt, bs = _make_head(form, N, Cc, 20 + N)
    weight, bias = _linear_head(head, Cc)
    with torch.no_grad():
        pv5, b32 = ops.project_head_values(weight, bias, v, heads, dtype=torch.float32)
    npad = (N + 15) // 16 * 16
    assert tuple(pv5.shape) == (B, heads, h, w, npad) and pv5.dtype == torch.float32
    assert float(pv5[..., N:].abs().sum()) == 0.0                       # pad channels are zero
    assert (b32 is None) == (bs is None) and (b32 is None or b32.dtype == torch.float32)
    pvn = pv5.permute(0, 1, 4, 2, 3).reshape(B, heads * npad, h, w)
    with torch.no_grad():
        o = O.xna_lowres(q, k, pvn, ksz, heads).view(B, heads, npad, h * d, w * d).sum(1)[:, :N]
        if b32 is not None:
            o = o + b32.view(1, N, 1, 1)
        ref = torch.nn.functional.conv2d(O.xna_lowres(q, k, v, ksz, heads), wt[:, :, None, None], bs)
    err = float((o - ref).abs().max())
    assert err <= 1e-5, f"identity off by {err:.3e} (ref absmax {float(ref.abs().max()):.3f})"
    # the default product is bf16, one rounding of the fp32 projection
    with torch.no_grad():
        pvb, _ = ops.project_head_values(weight, bias, v, heads)
    assert pvb.dtype == torch.bfloat16 and torch.equal(pvb, pv5.to(torch.bfloat16))


def test_projection_is_differentiable_on_the_cpu():
    from naf_amd import ops
    conv = nn.Conv2d(32, 5, 1)
    v = O.hash_normal((2, 32, 3, 4), 5)
    pv5, b32 = ops.project_head_values(conv.weight, conv.bias, v, 2, dtype=torch.float32)
    (pv5.square().sum() + b32.sum()).backward()
    assert conv.weight.grad is not None and float(conv.weight.grad.abs().sum()) > 0 and torch.equal(conv.bias.grad, torch.ones(5))
    with pytest.raises(ValueError, match="divisible"):
        ops.project_head_values(conv.weight, conv.bias, v, 3)
    with pytest.raises(ValueError, match="channels"):
        ops.project_head_values(conv.weight, conv.bias, v[:, :16], 2)


def test_head_argument_validation_happens_before_any_device_work():
    """Every bad ``head`` raises its TypeError / ValueError on CPU tensors, i.e. before the check that sends CPU tensors away."""
    from naf_amd import NAF
    m = NAF(dim=64, heads_attn=1, heads_rope=1, kernel_size=3).eval()
    img, ft = torch.zeros(1, 3, 32, 32), torch.zeros(1, 48, 4, 4)
    for bad in (nn.ReLU(), "conv", 3, (torch.zeros(5, 48),), nn.Sequential(nn.Conv2d(48, 5, 1)), (torch.zeros(5, 48), "bias")):
        with pytest.raises(TypeError, match="nn.Conv2d with a 1x1 kernel"):
            m(img, ft, (32, 32), head=bad)
    for bad in (nn.Conv2d(48, 5, 3, padding=1), nn.Conv2d(48, 6, 1, groups=2), nn.Conv2d(48, 5, 1, stride=2), nn.Conv2d(48, 5, 1, padding=1),
                nn.Conv2d(32, 5, 1), nn.Linear(32, 5), (torch.zeros(5, 32), None), (torch.zeros(5, 48, 3, 3), None),
                (torch.zeros(5, 48), torch.zeros(4)), (torch.zeros(5, 48, 1), None)):
        with pytest.raises(ValueError, match="head"):
            m(img, ft, (32, 32), head=bad)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        m(img, ft, (32, 32), head=(torch.zeros(5, 48, dtype=torch.float64), None))
    with pytest.raises(ValueError, match="return_weights"):
        m(img, ft, (32, 32), return_weights=True, head=nn.Conv2d(48, 5, 1))
    # a good head on CPU tensors is sent away as every CPU call is
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(img, ft, (32, 32), head=nn.Conv2d(48, 5, 1))
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(img, ft, (32, 32))
