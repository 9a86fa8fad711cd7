"""CPU tests of the fused probe evaluation (``naf(image, feats, size, head=probe, target=t, confusion=...)``): the C ABI of the confusion
matrix entry (header, ctypes mirror, exports, struct layout, the host-side policy of naf_xna_head_cm_select), the torch-side definition
``head_confusion_from_labels`` against a plain double loop, ``confusion_metrics`` on hand-written matrices, the argument validation of the
public call and ``dist.reduce_confusion`` under gloo.  No kernel is launched here."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch import nn

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_head_cpu import _head_args, _header_text  # noqa: E402
from test_head_objective_cpu import _ce_args, _targets  # noqa: E402
from test_dist import _free_port  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CM_SYMBOLS = ("naf_xna_head_cm_select", "naf_xna_head_cm_fwd")


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def test_header_ctypes_and_exports_agree(built_lib):
    from naf_amd import _lib
    txt = _header_text()
    lib = C.CDLL(built_lib)
    for name in CM_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*const naf_xna_head_cm_args\s*\*" % name, txt), f"{name} is not declared in include/naf_hip.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"libnaf_hip.so does not export {name}"
        assert _lib.SIGNATURES[name][0] == C.c_int and _lib.SIGNATURES[name][1][0] == C.POINTER(_lib.XnaHeadCMArgs)
    assert _lib.SIGNATURES["naf_xna_head_cm_fwd"][1][1] == C.c_void_p
    # added the way the head and classification entries were: detected by symbol, no version bump
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403 == _lib.HEADER_VERSION
    assert lib.naf_version() == 403


def test_cm_struct_layout_matches_header(built_lib):
    """sizeof and the offset of every field of naf_xna_head_cm_args against gcc's view of the header; the embedded naf_xna_head_ce_args
    comes first and keeps the size it has in the ctypes mirror that the classification entries use."""
    from naf_amd import _lib
    fields = [f[0] for f in _lib.XnaHeadCMArgs._fields_]
    assert fields[:3] == ["ce", "confusion", "cm_stride"]
    body = 'printf("%zu\\n", sizeof(naf_xna_head_cm_args));' + "".join(f'printf("%zu\\n", offsetof(naf_xna_head_cm_args, {f}));' for f in fields)
    body += 'printf("%zu\\n", sizeof(naf_xna_head_ce_args));printf("%zu\\n", sizeof(naf_xna_head_args));'
    src = '#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        vals = list(map(int, subprocess.check_output([os.path.join(d, "p")]).split()))
    assert vals[0] == C.sizeof(_lib.XnaHeadCMArgs)
    for f, off in zip(fields, vals[1:]):
        assert off == getattr(_lib.XnaHeadCMArgs, f).offset, f
    assert _lib.XnaHeadCMArgs.ce.offset == 0 and vals[-2] == C.sizeof(_lib.XnaHeadCEArgs) == _lib.XnaHeadCMArgs.ce.size
    assert vals[-1] == C.sizeof(_lib.XnaHeadArgs)
    # the structs of the earlier entries are what they were at 403 (nothing was placed in their padding or reserved fields)
    assert (C.sizeof(_lib.XnaHeadArgs), C.sizeof(_lib.XnaHeadCEArgs)) == (232, 376)


def _cm_args(*, matrix=1 << 20, cm_stride=None, **kw):
    """naf_xna_head_cm_args around test_head_objective_cpu's naf_xna_head_ce_args; host-only query: pointers are checked, never read."""
    from naf_amd import _lib
    m = _lib.XnaHeadCMArgs()
    m.ce = _ce_args(**kw)
    m.confusion = matrix
    m.cm_stride = m.ce.head.N if cm_stride is None else cm_stride
    return m


@pytest.mark.parametrize("ks", [3, 5, 7, 9, 11, 13, 15])
def test_cm_select_grants_every_window(built_lib, ks):
    from naf_amd import _lib
    lib = _lib.load()
    kw = dict(ky=ks, kx=ks, lr=(ks + 2, ks + 1))
    for variant in (dict(outputs=()), dict(outputs=("labels",)), dict(), dict(outputs=(), logits=True), dict(outputs=(), N=151), dict(outputs=(), N=256),
                    dict(outputs=(), N=1), dict(outputs=(), cm_stride=40), dict(outputs=(), ratio=(14, 14)), dict(outputs=(), ratio=(32, 32))):
        a = _cm_args(**variant, **kw)
        sel = lib.naf_xna_head_cm_select(C.byref(a))
        assert sel == _lib.XNA_HEAD_FUSED, (ks, variant, sel, _lib.last_error())


def test_cm_select_refuses_what_the_ce_select_refuses(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    for kw, status in ((dict(lr=(8, 8), out=(20, 20), ky=3, kx=3), 2), (dict(ratio=(8, 8)), 2), (dict(Dq=96), 2), (dict(N=257), 1),
                       (dict(ky=4, kx=4), 1), (dict(path=7), 1), (dict(outputs=("loss", "dlogits"), N=21, gc=24), 1)):
        assert lib.naf_xna_head_ce_select(C.byref(_ce_args(**kw))) == -status
        a = _cm_args(**kw)
        assert lib.naf_xna_head_cm_select(C.byref(a)) == -status, kw
        assert "naf_xna_head" in _lib.last_error()
        assert lib.naf_xna_head_cm_fwd(C.byref(a), None) == status          # refused before any launch
    assert lib.naf_xna_head_cm_select(None) == -1 and lib.naf_xna_head_cm_fwd(None, None) == 1


CM_REFUSED = [
    ("no target", dict(outputs=(), with_target=False), "needs a target"),
    ("labels but no target", dict(outputs=("labels",), with_target=False), "needs a target"),
    ("NULL matrix", dict(outputs=("labels",), matrix=None), "confusion is NULL"),
    ("matrix not 8-byte aligned", dict(outputs=(), matrix=(1 << 20) + 4), "8-byte aligned"),
    ("odd matrix address", dict(outputs=(), matrix=(1 << 20) + 1), "8-byte aligned"),
    ("row stride below N", dict(outputs=(), N=21, cm_stride=20), "cm_stride 20 smaller than N 21"),
    ("zero row stride", dict(outputs=(), N=2, cm_stride=0), "smaller than N"),
    ("negative row stride", dict(outputs=(), cm_stride=-21), "smaller than N"),
]


@pytest.mark.parametrize("what,kw,text", CM_REFUSED, ids=[r[0].replace(" ", "_") for r in CM_REFUSED])
def test_cm_select_refuses_with_its_own_reason(built_lib, what, kw, text):
    from naf_amd import _lib
    lib = _lib.load()
    assert lib.naf_xna_head_cm_select(C.byref(_cm_args(outputs=()))) == _lib.XNA_HEAD_FUSED     # a granted call in between
    a = _cm_args(**kw)
    sel = lib.naf_xna_head_cm_select(C.byref(a))
    assert sel == -1, (what, sel, _lib.last_error())
    assert text in _lib.last_error() and "naf_xna_head_cm" in _lib.last_error(), _lib.last_error()
    assert lib.naf_xna_head_cm_fwd(C.byref(a), None) == 1


def test_cm_select_reserved_fields_and_the_matrix_as_only_output(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    a = _cm_args(outputs=())
    a.reserved[1] = 1
    assert lib.naf_xna_head_cm_select(C.byref(a)) == -1 and "reserved" in _lib.last_error()
    # the same request without a matrix is "no output requested" for the classification entry
    assert lib.naf_xna_head_ce_select(C.byref(_ce_args(outputs=()))) == -1 and "no output" in _lib.last_error()


# ---- the definition: head_confusion_from_labels ---------------------------------------------------------------------
def _double_loop(labels, target, ignore_index, N):
    cm = [[0] * N for _ in range(N)]
    for p, t in zip(labels.reshape(-1).tolist(), target.reshape(-1).tolist()):
        if t != ignore_index and 0 <= t < N:
            cm[t][p] += 1
    return torch.tensor(cm, dtype=torch.int64).reshape(N, N)


@pytest.mark.parametrize("N,ignore_index", [(1, 255), (2, 255), (21, 255), (21, 7), (256, 255), (256, -100), (2, 0)])
def test_confusion_from_labels_equals_a_double_loop(N, ignore_index):
    """Hashed labels and targets with ignored pixels, targets outside the classes (a row of N + 3, one negative), ignore_index inside
    [0, N) (that class is then never counted), and an ``out=`` that already holds counts."""
    from naf_amd import ops
    B, Ho, Wo = 2, 13, 17
    labels = (O.hash_normal((B, Ho, Wo), 300 + N).mul(997.0).abs().long() % N).to(torch.uint8 if N <= 256 else torch.int64)
    t = _targets(B, Ho, Wo, N, ignore_index, 310 + N, oob_row=4)
    t[1, 5, 3] = -7
    ref = _double_loop(labels, t, ignore_index, N)
    got = ops.head_confusion_from_labels(labels, t, ignore_index, N)
    assert got.dtype == torch.int64 and tuple(got.shape) == (N, N) and torch.equal(got, ref)
    assert int(got.sum()) == int(ops.head_valid_pixels(t, ignore_index, N).sum())
    if 0 <= ignore_index < N:
        assert int(got[ignore_index].sum()) == 0
    # accumulation: dense, and with a row stride that leaves a gap untouched
    pre = (O.hash_normal((N, N), 320 + N).mul(50.0).abs().long())
    out = pre.clone()
    assert ops.head_confusion_from_labels(labels, t, ignore_index, N, out=out) is out and torch.equal(out, pre + ref)
    ops.head_confusion_from_labels(labels, t.int(), ignore_index, N, out=out)           # other integer targets are accepted
    assert torch.equal(out, pre + 2 * ref)
    wide = torch.full((N, N + 5), -3, dtype=torch.int64)
    view = wide[:, :N]
    view.copy_(pre)
    ops.head_confusion_from_labels(labels.long(), t, ignore_index, N, out=view)
    assert torch.equal(wide[:, :N], pre + ref) and bool((wide[:, N:] == -3).all())


def test_confusion_from_labels_edge_cases():
    from naf_amd import ops
    N = 5
    t = torch.full((1, 4, 4), 255)
    lab = torch.zeros(1, 4, 4, dtype=torch.uint8)
    assert int(ops.head_confusion_from_labels(lab, t, 255, N).abs().sum()) == 0          # every pixel ignored
    assert tuple(ops.head_confusion_from_labels(lab[:0], t[:0], 255, N).shape) == (N, N)  # empty batch
    t = torch.tensor([[[0, 1, 2, 3]]])
    lab = torch.tensor([[[0, 9, -1, 3]]])                                                # labels outside the classes count nothing
    assert ops.head_confusion_from_labels(lab, t, 255, N).nonzero().tolist() == [[0, 0], [3, 3]]
    with pytest.raises(ValueError, match="shape"):
        ops.head_confusion_from_labels(lab, t[:, :, :3], 255, N)
    for bad in (torch.zeros(N, N), torch.zeros(N, N, dtype=torch.int32)):
        with pytest.raises(TypeError, match="int64"):
            ops.head_confusion_from_labels(lab, t, 255, N, out=bad)
    for bad in (torch.zeros(N, N + 1, dtype=torch.int64), torch.zeros(N * N, dtype=torch.int64), torch.zeros(N, N, dtype=torch.int64).t()[:, :],
                torch.zeros(N, 2 * N, dtype=torch.int64)[:, ::2]):
        with pytest.raises(ValueError, match=r"\[N, N\]"):
            ops.head_confusion_from_labels(lab, t, 255, N, out=bad)


# ---- confusion_metrics ---------------------------------------------------------------------------------------------
def test_confusion_metrics_on_hand_written_matrices():
    import naf_amd
    from naf_amd import ops
    assert naf_amd.confusion_metrics is ops.confusion_metrics and "confusion_metrics" in naf_amd.__all__
    # class 2 is absent from targets and predictions; class 3 is predicted (twice) but never a target
    cm = torch.tensor([[5, 1, 0, 2],
                       [2, 6, 0, 0],
                       [0, 0, 0, 0],
                       [0, 0, 0, 0]])
    r = naf_amd.confusion_metrics(cm)
    assert r.accuracy.dtype == r.iou.dtype == r.miou.dtype == torch.float64 and r.present.dtype == torch.bool
    assert float(r.accuracy) == 11.0 / 16.0
    assert r.present.tolist() == [True, True, False, True]
    iou = [5.0 / (8 + 7 - 5), 6.0 / (8 + 7 - 6), 0.0, 0.0]
    assert r.iou.tolist() == iou
    assert float(r.miou) == pytest.approx((iou[0] + iou[1] + 0.0) / 3.0, rel=0, abs=1e-15)
    assert r._fields == ("accuracy", "iou", "miou", "present")
    # a perfect prediction; counts beyond 2^31
    big = torch.diag(torch.tensor([3_000_000_000, 7, 0]))
    r = naf_amd.confusion_metrics(big)
    assert float(r.accuracy) == 1.0 and r.iou.tolist() == [1.0, 1.0, 0.0] and float(r.miou) == 1.0 and r.present.tolist() == [True, True, False]
    # no counted pixel: 0 / 0
    r = naf_amd.confusion_metrics(torch.zeros(4, 4, dtype=torch.int64))
    assert math.isnan(float(r.accuracy)) and math.isnan(float(r.miou)) and r.iou.tolist() == [0.0] * 4 and not bool(r.present.any())
    for bad in (torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 3), [[1]]):
        with pytest.raises(ValueError, match="integer"):
            naf_amd.confusion_metrics(bad)


def test_confusion_metrics_of_counted_labels_equal_the_pixel_definitions():
    """accuracy == mean(pred == target) over the valid pixels, iou[c] == |pred = c and target = c| / |pred = c or target = c| over them."""
    from naf_amd import ops
    N = 6
    lab = O.hash_normal((2, 19, 23), 401).mul(997.0).abs().long() % N
    t = _targets(2, 19, 23, N, 255, 402, oob_row=3)
    t[t == 4] = 255                                       # class 4 never a target
    lab[lab == 5] = 0
    t[t == 5] = 255                                       # class 5 absent from both
    r = ops.confusion_metrics(ops.head_confusion_from_labels(lab, t, 255, N))
    v = ops.head_valid_pixels(t, 255, N)
    p, q = lab[v], t[v]
    assert float(r.accuracy) == pytest.approx(float((p == q).double().mean()), abs=1e-15)
    for c in range(N):
        union = int(((p == c) | (q == c)).sum())
        assert bool(r.present[c]) == (union != 0)
        assert float(r.iou[c]) == pytest.approx(int(((p == c) & (q == c)).sum()) / union if union else 0.0, abs=1e-15)
    assert r.present.tolist() == [True, True, True, True, True, False] and float(r.iou[4]) == 0.0


# ---- the public call ---------------------------------------------------------------------------------------------
def test_confusion_argument_validation_happens_before_any_device_work():
    """Every bad evaluation argument raises on CPU tensors, i.e. before the check that sends CPU tensors away."""
    from naf_amd import NAF
    m = NAF(dim=64, heads_attn=1, heads_rope=1, kernel_size=3).eval()
    img, ft = torch.zeros(2, 3, 32, 32), torch.zeros(2, 48, 4, 4)
    conv = nn.Conv2d(48, 5, 1)
    t = torch.zeros(2, 32, 32, dtype=torch.long)
    cm = torch.zeros(5, 5, dtype=torch.int64)
    for kw in (dict(confusion=True), dict(confusion=cm), dict(confusion=True, predict=True)):
        with pytest.raises(ValueError, match="target="):
            m(img, ft, (32, 32), head=conv, **kw)
    with pytest.raises(ValueError, match="head=probe"):
        m(img, ft, (32, 32), target=t, confusion=True)
    for bad in (1, "yes", [[0]], cm.tolist()):
        with pytest.raises(TypeError, match="True or an int64"):
            m(img, ft, (32, 32), head=conv, target=t, confusion=bad)
    for bad in (cm.float(), cm.int(), cm.bool()):
        with pytest.raises(TypeError, match="int64"):
            m(img, ft, (32, 32), head=conv, target=t, confusion=bad)
    for bad in (torch.zeros(5, 6, dtype=torch.int64), torch.zeros(4, 4, dtype=torch.int64), torch.zeros(25, dtype=torch.int64),
                torch.zeros(5, 10, dtype=torch.int64)[:, ::2], torch.zeros(1, 5, 5, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[N, N\]"):
            m(img, ft, (32, 32), head=conv, target=t, confusion=bad)
    with pytest.raises(TypeError, match="integer tensor"):
        m(img, ft, (32, 32), head=conv, target=t.float(), confusion=True)
    with pytest.raises(ValueError, match=r"\[B, Ho, Wo\]"):
        m(img, ft, (32, 32), head=conv, target=t[:1], confusion=cm)
    with pytest.raises(ValueError, match="reduction"):
        m(img, ft, (32, 32), head=conv, target=t, confusion=True, reduction="avg")
    with pytest.raises(ValueError, match="return_weights"):
        m(img, ft, (32, 32), return_weights=True, head=conv, target=t, confusion=True)
    with pytest.raises(TypeError, match="nn.Conv2d with a 1x1 kernel"):
        m(img, ft, (32, 32), head=nn.ReLU(), target=t, confusion=True)
    # good arguments on CPU tensors are sent away as every CPU call is; a row-strided matrix is accepted
    for kw in (dict(confusion=True), dict(confusion=cm), dict(confusion=torch.zeros(5, 8, dtype=torch.int64)[:, :5], predict=True),
               dict(confusion=True, ignore_index=255, predict=True)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            m(img, ft, (32, 32), head=conv, target=t, **kw)
    assert int(cm.abs().sum()) == 0
    # confusion=None / False: the objective call, untouched
    for kw in (dict(), dict(confusion=None), dict(confusion=False)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            m(img, ft, (32, 32), head=conv, target=t, **kw)


def test_docstrings_no_longer_list_the_confusion_matrix_as_not_offered():
    from naf_amd import NAF
    doc = NAF.forward.__doc__
    not_offered = doc[doc.rindex("Not offered"):]
    assert "confusion" not in not_offered and "confusion=True" in doc


# ---- several ranks -------------------------------------------------------------------------------------------------
def test_reduce_confusion_is_the_identity_without_a_process_group():
    from naf_amd import dist as nd
    cm = torch.arange(9, dtype=torch.int64).view(3, 3)
    keep = cm.clone()
    assert not dist.is_initialized()
    assert nd.reduce_confusion(cm) is cm and torch.equal(cm, keep)


def _cm_of_rank(rank, N):
    return (O.hash_normal((N, N), 500 + rank).mul(1000.0).abs().long()) + (3_000_000_000 if rank == 0 else 0)


def _reduce_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from naf_amd import dist as nd
        N = 7
        total = sum(_cm_of_rank(r, N) for r in range(world))
        cm = _cm_of_rank(rank, N)
        assert nd.reduce_confusion(cm) is cm and cm.dtype == torch.int64 and torch.equal(cm, total)
        wide = torch.full((N, N + 3), -1, dtype=torch.int64)          # a matrix with a row stride
        view = wide[:, :N]
        view.copy_(_cm_of_rank(rank, N))
        assert nd.reduce_confusion(view) is view and torch.equal(wide[:, :N], total) and bool((wide[:, N:] == -1).all())
        ret[rank] = True
    finally:
        dist.destroy_process_group()


def test_reduce_confusion_sums_over_two_gloo_ranks():
    world, port = 2, _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_reduce_worker, args=(world, port, ret), nprocs=world, join=True)
    assert dict(ret) == {0: True, 1: True}
