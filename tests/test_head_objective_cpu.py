"""CPU tests of the fused probe objective (``naf(image, feats, size, head=probe, target=t)`` / ``predict=True``): the C ABI of the
classification epilogue (header, ctypes mirror, exports, struct layout, the host-side select policy of naf_xna_head_ce_select), the torch-side
composition the library falls back on against ``F.cross_entropy`` / ``argmax`` in fp64, and the argument validation of the public call.
No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_head_cpu import GRANTED, _head_args, _header_text  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CE_SYMBOLS = ("naf_xna_head_ce_select", "naf_xna_head_ce_fwd")


def test_header_ctypes_and_exports_agree(built_lib):
    from naf_amd import _lib
    txt = _header_text()
    lib = C.CDLL(built_lib)
    for name in CE_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*const naf_xna_head_ce_args\s*\*" % name, txt), f"{name} is not declared in include/naf_hip.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"libnaf_hip.so does not export {name}"
        assert _lib.SIGNATURES[name][0] == C.c_int and _lib.SIGNATURES[name][1][0] == C.POINTER(_lib.XnaHeadCEArgs)
    assert _lib.SIGNATURES["naf_xna_head_ce_fwd"][1][1] == C.c_void_p
    # added the way the head entries were: detected by symbol, no version bump
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403 == _lib.HEADER_VERSION


def test_ce_struct_layout_matches_header(built_lib):
    """sizeof and the offset of every field of naf_xna_head_ce_args against gcc's view of the header; the embedded naf_xna_head_args comes
    first and keeps its size."""
    from naf_amd import _lib
    fields = [f[0] for f in _lib.XnaHeadCEArgs._fields_]
    body = 'printf("%zu\\n", sizeof(naf_xna_head_ce_args));' + "".join(f'printf("%zu\\n", offsetof(naf_xna_head_ce_args, {f}));' for f in fields)
    body += 'printf("%zu\\n", sizeof(naf_xna_head_args));'
    src = '#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        vals = list(map(int, subprocess.check_output([os.path.join(d, "p")]).split()))
    assert vals[0] == C.sizeof(_lib.XnaHeadCEArgs)
    for f, off in zip(fields, vals[1:]):
        assert off == getattr(_lib.XnaHeadCEArgs, f).offset, f
    assert _lib.XnaHeadCEArgs.head.offset == 0 and vals[-1] == C.sizeof(_lib.XnaHeadArgs) == _lib.XnaHeadCEArgs.head.size


def _ce_args(*, outputs=("loss", "labels", "dlogits"), with_target=True, gc=None, logits=False, **kw):
    """naf_xna_head_ce_args around test_head_cpu's naf_xna_head_args; host-only query: pointers are checked, never read."""
    from naf_amd import _lib
    a = _lib.XnaHeadCEArgs()
    a.head = _head_args(**kw)
    if not logits:
        a.head.out = None
    hd = a.head
    Ho, Wo = hd.Ho, hd.Wo
    npad = (max(hd.N, 1) + 15) // 16 * 16
    a.dlogits_channels = gc if gc is not None else next((c for c in (32, 64, 96, 128, 192, 256) if c >= npad), 256)
    a.ignore_index = 255
    if with_target:
        a.target = 8192
    for name in outputs:
        setattr(a, name, 4096)
    a.t_stride = a.loss_stride = a.labels_stride = _lib.I64x3(Ho * Wo, Wo, 1)
    g = a.dlogits_channels
    a.dlogits_stride = _lib.I64x3(Ho * Wo * g, Wo * g, g)
    return a


@pytest.mark.parametrize("kw", GRANTED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()).replace(" ", ""))
def test_ce_select_grants_what_the_head_select_grants(built_lib, kw):
    from naf_amd import _lib
    lib = _lib.load()
    kw = {k: v for k, v in kw.items() if k != "out_dtype"}       # the optional logits of this entry are fp32
    assert lib.naf_xna_head_select(C.byref(_head_args(**kw))) == _lib.XNA_HEAD_FUSED
    for variant in (dict(), dict(outputs=("labels",), with_target=False), dict(outputs=("loss",)), dict(outputs=("dlogits",)),
                    dict(outputs=(), logits=True, with_target=False), dict(logits=True), dict(gc=256)):
        a = _ce_args(**variant, **kw)
        sel = lib.naf_xna_head_ce_select(C.byref(a))
        assert sel == _lib.XNA_HEAD_FUSED, (kw, variant, sel, _lib.last_error())


def test_ce_select_refuses_what_the_head_select_refuses(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    for kw, status in ((dict(lr=(8, 8), out=(20, 20), ky=3, kx=3), 2), (dict(ratio=(8, 8)), 2), (dict(Dq=96), 2), (dict(N=257), 1),
                       (dict(ky=4, kx=4), 1), (dict(path=7), 1)):
        a = _ce_args(**kw)
        assert lib.naf_xna_head_select(C.byref(_head_args(**kw))) == -status
        assert lib.naf_xna_head_ce_select(C.byref(a)) == -status, kw
        assert "naf_xna_head" in _lib.last_error()
        assert lib.naf_xna_head_ce_fwd(C.byref(a), None) == status          # refused before any launch
    assert lib.naf_xna_head_ce_select(None) == -1 and lib.naf_xna_head_ce_fwd(None, None) == 1


CE_REFUSED = [
    ("no output requested", dict(outputs=(), with_target=True), 1, "no output"),
    ("loss without a target", dict(outputs=("loss",), with_target=False), 1, "need a target"),
    ("gradient without a target", dict(outputs=("dlogits",), with_target=False), 1, "need a target"),
    ("dlogits_channels too small", dict(N=21, gc=24), 1, "smaller than N rounded up"),
    ("dlogits_channels below Npad", dict(N=151, gc=152), 1, "smaller than N rounded up"),
    ("dlogits_channels not a multiple of 8", dict(N=21, gc=36), 1, "multiple of 8"),
    ("dlogits_channels above 256", dict(N=21, gc=264), 1, "above 256"),
    ("bf16 logits", dict(logits=True, out_dtype=0), 1, "NAF_F32"),
]


@pytest.mark.parametrize("what,kw,status,text", CE_REFUSED, ids=[r[0].replace(" ", "_") for r in CE_REFUSED])
def test_ce_select_refuses_with_its_own_reason(built_lib, what, kw, status, text):
    from naf_amd import _lib
    lib = _lib.load()
    assert lib.naf_xna_head_ce_select(C.byref(_ce_args())) == _lib.XNA_HEAD_FUSED     # a granted call in between
    a = _ce_args(**kw)
    sel = lib.naf_xna_head_ce_select(C.byref(a))
    assert sel == -status, (what, sel, _lib.last_error())
    assert text in _lib.last_error() and "naf_xna_head_ce" in _lib.last_error(), _lib.last_error()
    assert lib.naf_xna_head_ce_fwd(C.byref(a), None) == status


def test_ce_select_refuses_misaligned_dlogits(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    a = _ce_args()
    a.dlogits = 4096 + 8
    assert lib.naf_xna_head_ce_select(C.byref(a)) == -2 and "aligned dlogits" in _lib.last_error()
    a = _ce_args(outputs=("loss", "labels"))
    a.dlogits_channels = 7                       # no dlogits requested: its width is not looked at
    assert lib.naf_xna_head_ce_select(C.byref(a)) == _lib.XNA_HEAD_FUSED
    a = _ce_args()
    g = a.dlogits_channels
    a.dlogits_stride = _lib.I64x3(a.head.Ho * a.head.Wo * g + 4, a.head.Wo * g, g)
    assert lib.naf_xna_head_ce_select(C.byref(a)) == -2 and "dlogits strides" in _lib.last_error()
    a = _ce_args()
    a.dlogits_stride = _lib.I64x3(a.head.Ho * a.head.Wo * 16, a.head.Wo * 16, 16)       # rows of 16 cannot hold 32 channels
    assert lib.naf_xna_head_ce_select(C.byref(a)) == -1 and "x stride" in _lib.last_error()


# ---- the torch-side composition ----------------------------------------------------------------------------------
def _targets(B, Ho, Wo, N, ignore_index, seed, oob_row=None):
    t = (O.hash_normal((B, Ho, Wo), seed).mul(1000.0).abs().long() % N)
    ign = O.hash_normal((B, Ho, Wo), seed + 1) > 1.28             # about a tenth of a normal sample
    t[ign] = ignore_index
    if oob_row is not None:
        t[:, oob_row] = N + 3
    return t


@pytest.mark.parametrize("N,ignore_index", [(1, -100), (2, 255), (21, 255), (151, -100), (256, 255), (300, 255)])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_composition_equals_torch_cross_entropy_and_argmax(N, ignore_index, reduction):
    """head_objective_from_logits + reduce_head_loss on fp64 logits == F.cross_entropy / argmax for all three reductions with ignored pixels
    (N = 256 with ignore_index = 255 ignores that class, as torch does); softmax - onehot == the autograd gradient of the summed loss."""
    from naf_amd import ops
    B, Ho, Wo = 2, 9, 11
    z = O.hash_normal((B, N, Ho, Wo), 70 + N).double() * 3.0
    t = _targets(B, Ho, Wo, N, ignore_index, 80 + N)
    assert bool((t == ignore_index).any()) and bool((t != ignore_index).any())
    loss_map, labels, g = ops.head_objective_from_logits(z, t, ignore_index, want_loss=True, want_labels=True, want_dlogits=True)
    got = ops.reduce_head_loss(loss_map, t, ignore_index, N, reduction)
    ref = F.cross_entropy(z, t, ignore_index=ignore_index, reduction=reduction)
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * (1.0 + float(ref.abs().max()))
    assert torch.equal(labels.long(), z.argmax(1)) and labels.dtype == (torch.uint8 if N <= 256 else torch.int64)
    assert bool((loss_map[t == ignore_index] == 0).all())
    zz = z.clone().requires_grad_(True)
    F.cross_entropy(zz, t, ignore_index=ignore_index, reduction="sum").backward()
    gc = ops.head_dlogits_channels(N)
    assert g.dtype == torch.bfloat16 and tuple(g.shape) == (B, Ho, Wo, gc) and gc >= N
    ref_g = zz.grad.permute(0, 2, 3, 1)
    assert float((g[..., :N].double() - ref_g).abs().max()) <= 2.0 ** -8            # one rounding to bf16 of values in [-1, 1]
    assert float(g[..., N:].abs().sum()) == 0.0 and float(g[t == ignore_index].abs().sum()) == 0.0


def test_composition_ignores_out_of_range_targets_and_empty_sets():
    from naf_amd import ops
    B, N, Ho, Wo = 1, 21, 6, 7
    z = O.hash_normal((B, N, Ho, Wo), 91).double()
    t = _targets(B, Ho, Wo, N, 255, 92, oob_row=2)
    t[0, 3, 0] = -7
    clean = t.clone()
    clean[(t < 0) | ((t >= N) & (t != 255))] = 255
    for red in ("mean", "sum", "none"):
        lm, _, g = ops.head_objective_from_logits(z, t, 255, want_loss=True, want_dlogits=True)
        got = ops.reduce_head_loss(lm, t, 255, N, red)
        ref = F.cross_entropy(z, clean, ignore_index=255, reduction=red)
        assert float((got - ref).abs().max()) <= 1e-12
        assert float(lm[0, 2].abs().sum()) == 0.0 and float(g[0, 2].abs().sum()) == 0.0 and float(lm[0, 3, 0]) == 0.0
    assert int(ops.head_valid_pixels(t, 255, N).sum()) == int((clean != 255).sum())
    # no valid pixel: nan / 0 / zeros, as torch
    allign = torch.full((B, Ho, Wo), 255)
    lm, lab, _ = ops.head_objective_from_logits(z.float(), allign, 255, want_loss=True, want_labels=True)
    assert torch.isnan(ops.reduce_head_loss(lm, allign, 255, N, "mean")) and torch.isnan(F.cross_entropy(z, allign, ignore_index=255))
    assert float(ops.reduce_head_loss(lm, allign, 255, N, "sum")) == 0.0 and float(lm.abs().sum()) == 0.0 and lm.dtype == torch.float32
    assert torch.equal(lab.long(), z.argmax(1))
    # labels alone need no target; loss / gradient do
    assert ops.head_objective_from_logits(z, want_labels=True)[1] is not None
    with pytest.raises(ValueError, match="need a target"):
        ops.head_objective_from_logits(z, want_loss=True)


def test_first_maximum_wins():
    from naf_amd import ops
    z = torch.zeros(1, 5, 2, 2)
    z[0, 3, 0, 0] = z[0, 1, 0, 0] = 2.0
    z[0, 4, 1, 1] = z[0, 2, 1, 1] = 1.0
    lab = ops.head_objective_from_logits(z, want_labels=True)[1]
    assert lab.tolist() == [[[1, 0], [0, 2]]]


# ---- the public call ---------------------------------------------------------------------------------------------
def test_objective_argument_validation_happens_before_any_device_work():
    """Every bad objective argument raises on CPU tensors, i.e. before the check that sends CPU tensors away."""
    from naf_amd import NAF
    m = NAF(dim=64, heads_attn=1, heads_rope=1, kernel_size=3).eval()
    img, ft = torch.zeros(2, 3, 32, 32), torch.zeros(2, 48, 4, 4)
    conv = nn.Conv2d(48, 5, 1)
    t = torch.zeros(2, 32, 32, dtype=torch.long)
    with pytest.raises(ValueError, match="head=probe"):
        m(img, ft, (32, 32), target=t)
    with pytest.raises(ValueError, match="head=probe"):
        m(img, ft, (32, 32), predict=True)
    for bad in (t.float(), t.double(), t.to(torch.bfloat16), t.bool(), [[0]]):
        with pytest.raises(TypeError, match="integer tensor"):
            m(img, ft, (32, 32), head=conv, target=bad)
    for bad in (t[:1], t[:, :31], t[:, :, :16], t[0], t[..., None]):
        with pytest.raises(ValueError, match=r"\[B, Ho, Wo\]"):
            m(img, ft, (32, 32), head=conv, target=bad)
    for bad in ("avg", "batchmean", None, 1):
        with pytest.raises(ValueError, match="reduction"):
            m(img, ft, (32, 32), head=conv, target=t, reduction=bad)
    with pytest.raises(ValueError, match="return_weights"):
        m(img, ft, (32, 32), return_weights=True, head=conv, target=t)
    with pytest.raises(ValueError, match="return_weights"):
        m(img, ft, (32, 32), return_weights=True, head=conv, predict=True)
    with pytest.raises(TypeError, match="nn.Conv2d with a 1x1 kernel"):
        m(img, ft, (32, 32), head=nn.ReLU(), target=t)
    with pytest.raises(ValueError, match="head"):
        m(img, ft, (32, 32), head=nn.Conv2d(32, 5, 1), predict=True)
    # good arguments on CPU tensors are sent away as every CPU call is; int32 / uint8 targets are accepted
    for kw in (dict(target=t), dict(target=t.int(), ignore_index=255), dict(target=t.to(torch.uint8), reduction="none"), dict(predict=True),
               dict(target=t, predict=True, reduction="sum")):
        with pytest.raises(RuntimeError, match="ROCm device"):
            m(img, ft, (32, 32), head=conv, **kw)
    # the logits call is untouched by the new keywords' defaults
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(img, ft, (32, 32), head=conv)
