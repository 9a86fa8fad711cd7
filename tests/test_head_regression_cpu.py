"""CPU tests of the fused dense regression probe (``naf(image, feats, size, head=probe, dense_target=t)``): the C ABI of the regression
epilogue (header, ctypes mirror, exports, struct layout, the host-side policy of naf_xna_head_reg_select), the torch-side composition
the library falls back on against ``F.l1_loss`` / ``F.mse_loss`` / ``F.smooth_l1_loss``, the error sums against a Python double loop,
``depth_metrics``, ``dist.reduce_errors`` and the argument validation of the public call.  No kernel is launched here."""
import ctypes as C
import math
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
import head_regression_reference as R  # noqa: E402
from test_head_cpu import _head_args, _header_text  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG_SYMBOLS = ("naf_xna_head_reg_select", "naf_xna_head_reg_workspace_bytes", "naf_xna_head_reg_fwd")
WINDOWS = (3, 5, 7, 9, 11, 13, 15)


def test_header_ctypes_and_exports_agree(built_lib):
    from naf_amd import _lib
    txt = _header_text()
    lib = C.CDLL(built_lib)
    for name in REG_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*const naf_xna_head_reg_args\s*\*" % name, txt), f"{name} is not declared in include/naf_hip.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"libnaf_hip.so does not export {name}"
        assert _lib.SIGNATURES[name][1][0] == C.POINTER(_lib.XnaHeadRegArgs)
    assert _lib.SIGNATURES["naf_xna_head_reg_select"][0] == C.c_int and _lib.SIGNATURES["naf_xna_head_reg_fwd"][0] == C.c_int
    assert _lib.SIGNATURES["naf_xna_head_reg_workspace_bytes"][0] == C.c_size_t
    assert _lib.SIGNATURES["naf_xna_head_reg_fwd"][1][1] == C.c_void_p
    # added the way the _ce / _cm entries were: detected by symbol, no version bump
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403 == _lib.HEADER_VERSION
    assert int(re.search(r"#define\s+NAF_HEAD_REG_STATS\s+(\d+)", txt).group(1)) == _lib.HEAD_REG_STATS == R.NSTAT
    kinds = re.search(r"enum naf_head_reg_kind \{([^}]*)\}", txt).group(1)
    for name, val in _lib.HEAD_REG_KINDS.items():
        assert re.search(r"NAF_HEAD_REG_%s\s*=\s*%d\b" % (name.upper(), val), kinds), name
    raw = open(os.path.join(ROOT, "include", "naf_hip.h")).read()          # with the comments: the documented contract
    assert "must be zero-initialised" in raw and "LONGEST FP32 ADDITION CHAIN" in raw


def test_reg_struct_layout_matches_header(built_lib):
    """sizeof and the offset of every field of naf_xna_head_reg_args against gcc's view of the header; the embedded naf_xna_head_args comes
    first and keeps its size."""
    from naf_amd import _lib
    fields = [f[0] for f in _lib.XnaHeadRegArgs._fields_]
    body = 'printf("%zu\\n", sizeof(naf_xna_head_reg_args));' + "".join(f'printf("%zu\\n", offsetof(naf_xna_head_reg_args, {f}));' for f in fields)
    body += 'printf("%zu\\n", sizeof(naf_xna_head_args));'
    src = '#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        vals = list(map(int, subprocess.check_output([os.path.join(d, "p")]).split()))
    assert vals[0] == C.sizeof(_lib.XnaHeadRegArgs)
    for f, off in zip(fields, vals[1:]):
        assert off == getattr(_lib.XnaHeadRegArgs, f).offset, f
    assert _lib.XnaHeadRegArgs.head.offset == 0 and vals[-1] == C.sizeof(_lib.XnaHeadArgs) == _lib.XnaHeadRegArgs.head.size


def _reg_args(*, outputs=("loss", "dlogits"), with_target=True, with_valid=True, errors=False, gc=None, logits=False, kind=0, beta=1.0,
              clamp=(1e-3, math.inf), **kw):
    """naf_xna_head_reg_args around test_head_cpu's naf_xna_head_args; host-only query: pointers are checked, never read."""
    from naf_amd import _lib
    a = _lib.XnaHeadRegArgs()
    a.head = _head_args(**kw)
    if not logits:
        a.head.out = None
    hd = a.head
    Ho, Wo, N = hd.Ho, hd.Wo, max(hd.N, 1)
    npad = (N + 15) // 16 * 16
    a.dlogits_channels = gc if gc is not None else next((c for c in (32, 64, 96, 128, 192, 256) if c >= npad), 256)
    a.kind, a.beta, a.clamp_lo, a.clamp_hi = kind, beta, clamp[0], clamp[1]
    if with_target:
        a.target = 8192
    if with_valid:
        a.valid = 12288
    if errors:
        a.errors = 16384
    for name in outputs:
        setattr(a, name, 4096)
    a.t_stride = _lib.I64x4(N * Ho * Wo, Ho * Wo, Wo, 1)
    a.valid_stride = a.loss_stride = _lib.I64x3(Ho * Wo, Wo, 1)
    g = a.dlogits_channels
    a.dlogits_stride = _lib.I64x3(Ho * Wo * g, Wo * g, g)
    return a


@pytest.mark.parametrize("N", [1, 3, 32])
@pytest.mark.parametrize("k", WINDOWS)
def test_reg_select_grants_every_window(built_lib, k, N):
    from naf_amd import _lib
    lib = _lib.load()
    kw = dict(ky=k, kx=k, lr=(k + 2, k + 1), N=N)
    assert lib.naf_xna_head_select(C.byref(_head_args(**kw))) == _lib.XNA_HEAD_FUSED
    variants = [dict(), dict(outputs=("loss",)), dict(outputs=("dlogits",), with_valid=False), dict(outputs=(), logits=True, with_target=False),
                dict(logits=True, kind=1), dict(kind=2, beta=0.25), dict(gc=64)]
    if N == 1:
        variants += [dict(outputs=(), errors=True), dict(errors=True, logits=True), dict(outputs=(), errors=True, clamp=(0.5, 0.5))]
    for variant in variants:
        a = _reg_args(**variant, **kw)
        sel = lib.naf_xna_head_reg_select(C.byref(a))
        assert sel == _lib.XNA_HEAD_FUSED, (kw, variant, sel, _lib.last_error())
        want = a.head.B * a.head.h * a.head.w * R.NSTAT * 8 if variant.get("errors") else 0
        assert lib.naf_xna_head_reg_workspace_bytes(C.byref(a)) == want


def test_reg_select_refuses_more_than_32_outputs(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    for k in WINDOWS:
        a = _reg_args(ky=k, kx=k, lr=(k + 2, k + 1), N=33)
        assert lib.naf_xna_head_reg_select(C.byref(a)) == -2, _lib.last_error()
        assert "N <= 32" in _lib.last_error() and "naf_xna_head_reg" in _lib.last_error()
        assert lib.naf_xna_head_reg_fwd(C.byref(a), None) == 2          # refused before any launch


def test_reg_select_refuses_what_the_head_select_refuses(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    for kw, status in ((dict(lr=(8, 8), out=(20, 20), ky=3, kx=3), 2), (dict(ratio=(8, 8)), 2), (dict(Dq=96), 2), (dict(N=257), 1),
                       (dict(ky=4, kx=4), 1), (dict(path=7), 1)):
        a = _reg_args(**{"N": 3, **kw})
        assert lib.naf_xna_head_select(C.byref(_head_args(**{"N": 3, **kw}))) == -status
        assert lib.naf_xna_head_reg_select(C.byref(a)) == -status, kw
        assert "naf_xna_head" in _lib.last_error()
        assert lib.naf_xna_head_reg_fwd(C.byref(a), None) == status
    assert lib.naf_xna_head_reg_select(None) == -1 and lib.naf_xna_head_reg_fwd(None, None) == 1
    assert lib.naf_xna_head_reg_workspace_bytes(None) == 0


REG_REFUSED = [
    ("loss without a target", dict(N=3, outputs=("loss",), with_target=False), 1, "need a target"),
    ("gradient without a target", dict(N=3, outputs=("dlogits",), with_target=False), 1, "need a target"),
    ("errors without a target", dict(N=1, outputs=(), errors=True, with_target=False), 1, "need a target"),
    ("errors with three outputs", dict(N=3, errors=True), 1, "N = 1"),
    ("smooth l1 with beta zero", dict(N=3, kind=2, beta=0.0), 1, "beta > 0"),
    ("smooth l1 with a negative beta", dict(N=3, kind=2, beta=-1.0), 1, "beta > 0"),
    ("smooth l1 with a nan beta", dict(N=3, kind=2, beta=math.nan), 1, "beta > 0"),
    ("clamp_lo zero", dict(N=1, errors=True, clamp=(0.0, 1.0)), 1, "clamp_lo"),
    ("clamp_lo negative", dict(N=1, errors=True, clamp=(-1.0, 1.0)), 1, "clamp_lo"),
    ("clamp_hi below clamp_lo", dict(N=1, errors=True, clamp=(2.0, 1.0)), 1, "clamp_lo"),
    ("unknown kind", dict(N=3, kind=3), 1, "unknown kind"),
    ("negative kind", dict(N=3, kind=-1), 1, "unknown kind"),
    ("nothing asked for", dict(N=3, outputs=()), 1, "nothing asked"),
    ("bf16 logits", dict(N=3, logits=True, out_dtype=0), 1, "NAF_F32"),
    ("dlogits_channels too small", dict(N=17, gc=24), 1, "smaller than N rounded up"),
    ("dlogits_channels not a multiple of 8", dict(N=3, gc=36), 1, "multiple of 8"),
    ("dlogits_channels above 256", dict(N=3, gc=264), 1, "above 256"),
    ("a channel count the backward does not serve", dict(N=3, gc=40), 2, "attention backward serves"),
]


@pytest.mark.parametrize("what,kw,status,text", REG_REFUSED, ids=[r[0].replace(" ", "_") for r in REG_REFUSED])
def test_reg_select_refuses_with_its_own_reason(built_lib, what, kw, status, text):
    from naf_amd import _lib
    lib = _lib.load()
    assert lib.naf_xna_head_reg_select(C.byref(_reg_args(N=kw["N"]))) == _lib.XNA_HEAD_FUSED     # a granted call in between
    a = _reg_args(**kw)
    sel = lib.naf_xna_head_reg_select(C.byref(a))
    assert sel == -status, (what, sel, _lib.last_error())
    assert text in _lib.last_error() and "naf_xna_head_reg" in _lib.last_error(), _lib.last_error()
    assert lib.naf_xna_head_reg_fwd(C.byref(a), None) == status
    assert lib.naf_xna_head_reg_workspace_bytes(C.byref(a)) == 0 or status == 2


def test_reg_select_refuses_misaligned_pointers_and_reserved_fields(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    a = _reg_args(N=1, errors=True)
    a.errors = 16384 + 4
    assert lib.naf_xna_head_reg_select(C.byref(a)) == -1 and "8-byte aligned" in _lib.last_error()
    a = _reg_args(N=3)
    a.dlogits = 4096 + 8
    assert lib.naf_xna_head_reg_select(C.byref(a)) == -2 and "aligned dlogits" in _lib.last_error()
    a = _reg_args(N=3)
    g = a.dlogits_channels
    a.dlogits_stride = _lib.I64x3(a.head.Ho * a.head.Wo * g + 4, a.head.Wo * g, g)
    assert lib.naf_xna_head_reg_select(C.byref(a)) == -2 and "dlogits strides" in _lib.last_error()
    a = _reg_args(N=3)
    a.dlogits_stride = _lib.I64x3(a.head.Ho * a.head.Wo * 16, a.head.Wo * 16, 16)       # rows of 16 cannot hold 32 channels
    assert lib.naf_xna_head_reg_select(C.byref(a)) == -1 and "x stride" in _lib.last_error()
    a = _reg_args(N=3, outputs=("loss",))
    a.dlogits_channels = 7                       # no dlogits requested: its width is not looked at
    assert lib.naf_xna_head_reg_select(C.byref(a)) == _lib.XNA_HEAD_FUSED
    for i in range(3):
        a = _reg_args(N=3)
        a.reserved[i] = 1
        assert lib.naf_xna_head_reg_select(C.byref(a)) == -1 and "reserved" in _lib.last_error()
        assert lib.naf_xna_head_reg_fwd(C.byref(a), None) == 1
    # the statistics need their workspace at launch time: refused before any launch, the select (which has no workspace to look at) grants
    a = _reg_args(N=1, errors=True)
    assert lib.naf_xna_head_reg_select(C.byref(a)) == _lib.XNA_HEAD_FUSED
    assert lib.naf_xna_head_reg_fwd(C.byref(a), None) == 1 and "workspace" in _lib.last_error()
    a.workspace, a.workspace_bytes = 32768, 8
    assert lib.naf_xna_head_reg_fwd(C.byref(a), None) == 1 and "workspace" in _lib.last_error()


# ---- the torch-side composition ----------------------------------------------------------------------------------
def _torch_loss(kind, beta):
    return {"l1": F.l1_loss, "mse": F.mse_loss, "smooth_l1": lambda a, b, reduction: F.smooth_l1_loss(a, b, reduction=reduction, beta=beta)}[kind]


@pytest.mark.parametrize("N", [1, 3, 17])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("mode", ["none", "tenth", "all"])
def test_composition_equals_the_torch_losses(N, kind, mode):
    """head_regression_from_logits + reduce_regression_loss on fp64 logits == F.l1_loss / F.mse_loss / F.smooth_l1_loss on the selected
    elements for all three reductions ("none": the channel sums of the elementwise loss, 0 where invalid); the gradient == autograd's of
    the summed loss; both equal to the restatement of tests/head_regression_reference.py."""
    from naf_amd import ops
    B, Ho, Wo, beta = 2, 9, 11, 0.4
    z = O.hash_normal((B, N, Ho, Wo), 70 + N).double() * 1.5
    t = O.hash_normal((B, N, Ho, Wo), 80 + N).double()
    valid = R.make_valid(B, Ho, Wo, mode)
    if valid is not None:
        t[(~valid).unsqueeze(1).expand_as(t)] = math.nan               # what lies under an invalid pixel reaches nothing
    sel = torch.ones_like(z, dtype=torch.bool) if valid is None else valid.unsqueeze(1).expand_as(z)
    fn = _torch_loss(kind, beta)
    loss_map, g = ops.head_regression_from_logits(z, t, valid, kind, beta, want_loss=True, want_dlogits=True)
    assert loss_map.dtype == torch.float64 and tuple(loss_map.shape) == (B, Ho, Wo)
    for red in ("mean", "sum"):
        got, ref = ops.reduce_regression_loss(loss_map, valid, N, red), fn(z[sel], t[sel], reduction=red)
        if mode == "all" and red == "mean":
            assert torch.isnan(got) and torch.isnan(ref)
        else:
            assert abs(float(got) - float(ref)) <= 1e-12 * (1.0 + abs(float(ref))), (red, float(got), float(ref))
    elem = torch.zeros_like(z)
    elem[sel] = fn(z[sel], t[sel], reduction="none")
    assert ops.reduce_regression_loss(loss_map, valid, N, "none") is loss_map
    assert float((loss_map - elem.sum(1)).abs().max()) <= 1e-12
    if valid is not None:
        assert float(loss_map[~valid].abs().sum()) == 0.0
    ref_l, _, ref_g = R.restate(z, t, valid, kind, beta)
    assert float((loss_map - ref_l).abs().max()) <= 1e-12
    zz = z.clone().requires_grad_(True)
    if bool(sel.any()):
        fn(zz[sel], t[sel], reduction="sum").backward()
        auto = zz.grad.permute(0, 2, 3, 1)
    else:
        auto = torch.zeros(B, Ho, Wo, N, dtype=torch.float64)
    assert float((ref_g - auto).abs().max()) <= 1e-12
    gc = ops.head_dlogits_channels(N)
    assert g.dtype == torch.bfloat16 and tuple(g.shape) == (B, Ho, Wo, gc) and gc == 32
    assert bool(((g[..., :N].double() - auto).abs() <= 2.0 ** -8 * auto.abs()).all())          # one rounding to bf16
    assert float(g[..., N:].abs().sum()) == 0.0
    if valid is not None:
        assert float(g[~valid].float().abs().sum()) == 0.0
    # fp32 logits give an fp32 map; a uint8 mask is a bool mask
    l32, _ = ops.head_regression_from_logits(z.float(), t.float(), None if valid is None else valid.to(torch.uint8), kind, beta, want_loss=True)
    assert l32.dtype == torch.float32 and float((l32.double() - loss_map).abs().max()) <= 1e-4
    # the loss is differentiable with respect to the logits (the unfused route of the public call), NaN under the mask or not
    zz = z.clone().requires_grad_(True)
    ops.head_regression_from_logits(zz, t, valid, kind, beta, want_loss=True)[0].sum().backward()
    assert float((zz.grad.permute(0, 2, 3, 1) - auto).abs().max()) <= 1e-12


def test_composition_argument_checks():
    from naf_amd import ops
    z, t = torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3, 3)
    with pytest.raises(ValueError, match="one of"):
        ops.head_regression_from_logits(z, t, None, "huber", want_loss=True)
    with pytest.raises(ValueError, match="beta"):
        ops.head_regression_from_logits(z, t, None, "smooth_l1", 0.0, want_loss=True)
    assert ops.head_regression_from_logits(z, t, None, "l1") == (None, None)
    assert ops.head_regression_from_logits(torch.zeros(1, 33, 2, 2), torch.zeros(1, 33, 2, 2), want_dlogits=True)[1].shape[-1] == 64


def test_error_sums_equal_a_python_double_loop():
    from naf_amd import ops
    B, Ho, Wo = 2, 6, 7
    pred = O.hash_normal((B, 1, Ho, Wo), 11) * 1.5 + 1.0
    t = R.stats_target(B, Ho, Wo, 12)
    t[0, 0, 0, :4] = torch.tensor([0.0, -2.0, math.inf, math.nan])
    pred[1, 0, 0, 0], pred[1, 0, 0, 1] = math.nan, math.inf
    valid = R.make_valid(B, Ho, Wo, "tenth")
    clamp = (0.3, 2.5)
    lo, hi = R.f32(clamp[0]), R.f32(clamp[1])
    want = [0.0] * 10
    for b in range(B):
        for y in range(Ho):
            for x in range(Wo):
                z, tt = float(pred[b, 0, y, x]), float(t[b, 0, y, x])
                if not bool(valid[b, y, x]) or not tt > 0 or not math.isfinite(tt) or not math.isfinite(z):
                    continue
                p = min(max(z, lo), hi)
                d = math.log(p) - math.log(tt)
                r = max(p / tt, tt / p)
                for i, v in enumerate((1.0, abs(p - tt), (p - tt) ** 2, abs(p - tt) / tt, (p - tt) ** 2 / tt, d, d * d,
                                       float(r < 1.25), float(r < 1.25 ** 2), float(r < 1.25 ** 3))):
                    want[i] += v
    got = ops.head_errors_from_prediction(pred, t, valid, clamp)
    assert got.dtype == torch.float64 and tuple(got.shape) == (10,)
    assert 0 < want[0] < B * Ho * Wo and want[7] < want[8] < want[9]
    for i in range(10):
        assert abs(float(got[i]) - want[i]) <= 1e-12 * (1.0 + abs(want[i])), (i, float(got[i]), want[i])
    ref = R.error_sums(pred[:, 0], t[:, 0], valid, clamp)[0]
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert torch.equal(ops.head_errors_from_prediction(pred[:, 0], t[:, 0], valid.to(torch.uint8), clamp), got)       # [B, Ho, Wo] forms, uint8 mask
    none = ops.head_errors_from_prediction(pred, t, torch.zeros_like(valid), clamp)
    assert float(none.abs().sum()) == 0.0
    assert float(ops.head_errors_from_prediction(pred, t)[0]) > want[0]           # no mask, default clamp
    for bad in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0)):
        with pytest.raises(ValueError, match="clamp"):
            ops.head_errors_from_prediction(pred, t, valid, bad)


def test_stats_inputs_leave_narrow_threshold_brackets():
    """The condition the GPU statistics test puts on its inputs, checked here on a stand-in prediction of the same spread: fewer than 1 % of
    the counted pixels lie within 2^-20 (relative) of a threshold, and the uncounted targets are there."""
    B, Ho, Wo = 1, 128, 128
    t = R.stats_target(B, Ho, Wo, 903)[:, 0]
    pred = O.hash_normal((B, Ho, Wo), 904) * 1.2 + 1.0
    assert bool((t == 0).any()) and bool((t < 0).any()) and bool(torch.isinf(t).any()) and bool(torch.isnan(t).any())
    assert bool((pred < R.STATS_CLAMP[0]).any()) and bool((pred > R.STATS_CLAMP[1]).any())
    widths, n = R.bracket_widths(pred, t, R.make_valid(B, Ho, Wo, "tenth"), R.STATS_CLAMP)
    assert 0.7 * B * Ho * Wo < n < 0.9 * B * Ho * Wo
    for lo, hi in widths:
        assert 0 <= hi - lo < 0.01 * n and lo > 0.05 * n


def test_depth_metrics_on_hand_written_sums():
    import naf_amd
    from naf_amd import ops
    assert naf_amd.depth_metrics is ops.depth_metrics and "depth_metrics" in naf_amd.__all__
    acc = torch.tensor([4.0, 2.0, 16.0, 1.0, 8.0, -2.0, 5.0, 1.0, 2.0, 3.0], dtype=torch.float64)
    m = naf_amd.depth_metrics(acc)
    assert m._fields == ("mae", "rmse", "abs_rel", "sq_rel", "rmse_log", "silog", "d1", "d2", "d3", "n")
    assert all(v.dtype == torch.float64 for v in m)
    want = dict(mae=0.5, rmse=2.0, abs_rel=0.25, sq_rel=2.0, rmse_log=math.sqrt(1.25), silog=1.0, d1=0.25, d2=0.5, d3=0.75, n=4.0)
    for k, v in want.items():
        assert abs(float(getattr(m, k)) - v) <= 1e-15, k
    ref = R.metrics(acc)
    assert all(abs(float(getattr(m, k)) - ref[k]) <= 1e-15 for k in want)
    # a constant ratio: the variance is 0 up to rounding, never the root of a negative number
    c = torch.tensor([3.0, 0, 0, 0, 0, 3 * 0.1, 3 * 0.1 * 0.1, 0, 0, 0], dtype=torch.float64)
    assert float(naf_amd.depth_metrics(c).silog) < 1e-7
    empty = naf_amd.depth_metrics(torch.zeros(10, dtype=torch.float64))
    assert all(math.isnan(float(v)) for v in empty[:9]) and float(empty.n) == 0.0
    assert math.isnan(float(torch.zeros(0).mean()))                    # "as an empty mean does in torch"
    assert float(naf_amd.depth_metrics(acc.float()).rmse) == 2.0       # other float dtypes are widened
    for bad in (torch.zeros(9), torch.zeros(2, 10), [0.0] * 10):
        with pytest.raises(ValueError, match="error sums"):
            naf_amd.depth_metrics(bad)


def test_reduce_errors_without_a_process_group_is_the_identity():
    from naf_amd import dist as ndist
    acc = torch.arange(10, dtype=torch.float64)
    out = ndist.reduce_errors(acc)
    assert out is acc and torch.equal(acc, torch.arange(10, dtype=torch.float64))


# ---- the public call ---------------------------------------------------------------------------------------------
def test_regression_argument_validation_happens_before_any_device_work():
    """Every bad regression argument raises on CPU tensors, i.e. before the check that sends CPU tensors away."""
    from naf_amd import NAF
    m = NAF(dim=64, heads_attn=1, heads_rope=1, kernel_size=3).eval()
    img, ft = torch.zeros(2, 3, 32, 32), torch.zeros(2, 48, 4, 4)
    conv, conv1 = nn.Conv2d(48, 3, 1), nn.Conv2d(48, 1, 1)
    t, t1 = torch.zeros(2, 3, 32, 32), torch.zeros(2, 1, 32, 32)
    v = torch.ones(2, 32, 32, dtype=torch.bool)
    acc = torch.zeros(10, dtype=torch.float64)
    size = (32, 32)
    with pytest.raises(ValueError, match="head=probe"):
        m(img, ft, size, dense_target=t)
    for kw in (dict(target=torch.zeros(2, 32, 32, dtype=torch.long)), dict(confusion=True), dict(regress=torch.zeros(2, 48, 32, 32)), dict(cosine=True),
               dict(masks=torch.ones(2, 1, 32, 32)), dict(return_weights=True)):
        with pytest.raises(ValueError, match="does not combine"):
            m(img, ft, size, head=conv, dense_target=t, **kw)
    for kw in (dict(valid=v), dict(errors=True), dict(errors=acc), dict(clamp=(0.1, 10.0))):
        with pytest.raises(ValueError, match="dense_target"):
            m(img, ft, size, head=conv1, **kw)
        with pytest.raises(ValueError, match="dense_target"):
            m(img, ft, size, **kw)
    # shapes, dtypes and devices
    for bad in (t[:1], t[:, :2], t[:, :, :31], t[..., :16], t[0], t1):
        with pytest.raises(ValueError, match=r"\[B, N, Ho, Wo\]"):
            m(img, ft, size, head=conv, dense_target=bad)
    for bad in (t.long(), t.bool(), [[0.0]]):
        with pytest.raises(TypeError, match="floating-point"):
            m(img, ft, size, head=conv, dense_target=bad)
    with pytest.raises(ValueError, match="is on"):
        m(img, ft, size, head=conv, dense_target=t.to("meta"))
    for bad in (v[:1], v[:, :31], v[..., :16], v[:, None]):
        with pytest.raises(ValueError, match=r"\[B, Ho, Wo\]"):
            m(img, ft, size, head=conv, dense_target=t, valid=bad)
    for bad in (v.float(), v.long()):
        with pytest.raises(TypeError, match="bool or uint8"):
            m(img, ft, size, head=conv, dense_target=t, valid=bad)
    with pytest.raises(ValueError, match="is on"):
        m(img, ft, size, head=conv, dense_target=t, valid=v.to("meta"))
    for bad in ("huber", "L1", None, 1):
        with pytest.raises(ValueError, match="one of"):
            m(img, ft, size, head=conv, dense_target=t, dense_loss=bad)
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="beta"):
            m(img, ft, size, head=conv, dense_target=t, dense_loss="smooth_l1", beta=bad)
    for bad in ("avg", None):
        with pytest.raises(ValueError, match="reduction"):
            m(img, ft, size, head=conv, dense_target=t, reduction=bad)
    # the error statistics: one output only, a float64 [10] accumulator, a clamp with 0 < lo <= hi
    for e in (True, acc):
        with pytest.raises(ValueError, match="one output"):
            m(img, ft, size, head=conv, dense_target=t, errors=e)
    for bad in (acc.float(), torch.zeros(10, dtype=torch.int64), 1.0):
        with pytest.raises(TypeError, match="float64"):
            m(img, ft, size, head=conv1, dense_target=t1, errors=bad)
    for bad in (torch.zeros(9, dtype=torch.float64), torch.zeros(2, 10, dtype=torch.float64), torch.zeros(20, dtype=torch.float64)[::2]):
        with pytest.raises(ValueError, match="contiguous"):
            m(img, ft, size, head=conv1, dense_target=t1, errors=bad)
    with pytest.raises(ValueError, match="is on"):
        m(img, ft, size, head=conv1, dense_target=t1, errors=acc.to("meta"))
    for bad in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0)):
        with pytest.raises(ValueError, match="clamp"):
            m(img, ft, size, head=conv1, dense_target=t1, errors=True, clamp=bad)
    with pytest.raises(TypeError, match="nn.Conv2d with a 1x1 kernel"):
        m(img, ft, size, head=nn.ReLU(), dense_target=t)
    # good arguments on CPU tensors are sent away as every CPU call is
    for kw in (dict(dense_target=t), dict(dense_target=t.double(), valid=v, dense_loss="mse", reduction="none"),
               dict(dense_target=t.to(torch.bfloat16), valid=v.to(torch.uint8), dense_loss="smooth_l1", beta=0.5, predict=True, reduction="sum")):
        with pytest.raises(RuntimeError, match="ROCm device"):
            m(img, ft, size, head=conv, **kw)
    for kw in (dict(errors=True), dict(errors=acc, valid=v, clamp=(0.5, 80.0), predict=True)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            m(img, ft, size, head=conv1, dense_target=t1, **kw)
    # the existing calls are untouched by the new keywords' defaults
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(img, ft, size, head=conv)
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(img, ft, size, head=conv, target=torch.zeros(2, 32, 32, dtype=torch.long))
