"""GPU tests (-m gpu) of the fused probe evaluation: the confusion matrix counted in the classification epilogue of the head-summed
attention kernel (naf_xna_head_cm_fwd) and ``naf(image, feats, size, head=probe, target=t, confusion=...)`` end to end.

The matrix is made of integers, so every assertion but one is exact:
  A. One launch against itself: the launch also stores its labels, so matrix == head_confusion_from_labels(those labels, target) exactly,
     its sum is the number of valid pixels, and every other output is bit-equal to naf_xna_head_ce_fwd's for the same arguments.
  B. Accumulation, row strides, reproducibility, all pixels on one counter: exact.
  C. Against the oracle (test_gpu_head.head_reference, inputs and per-pixel ``bound`` of test_gpu_head_objective.test_objective_matches_oracle):
     a valid pixel whose top-2 margin in the oracle's logits exceeds 2 * bound has the oracle's label; one of the others (the set U) moves
     at most one count from one column to another, so sum |cm - cm_oracle| <= 2 |U|, and every row sum (the histogram of the targets) is
     exactly the oracle's.  That the bound is not empty is asserted from the oracle alone: at least 0.75 of the pixels are determined.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_head import _load_model, _probe, head_reference  # noqa: E402
from test_gpu_head_objective import LABEL_GEOM, SELF_CASES, make_inputs, make_target, valid_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def prefill(N, seed, dev, stride=None):
    """An int64 [N, N] matrix of hashed counts (some beyond 2^32); with ``stride`` a view of a wider buffer whose gap holds -7."""
    pre = O.hash_normal((N, N), seed).mul(1000.0).abs().long()
    pre[0, 0] += 5_000_000_000
    if stride is None:
        return pre.to(dev)
    wide = torch.full((N, stride), -7, dtype=torch.int64)
    wide[:, :N] = pre
    return wide.to(dev)[:, :N]


# ... and the two-round geometry (32 x 16 cells) with pixels that count: SELF_CASES has it with every pixel ignored
CM_CASES = SELF_CASES + [((1, 7, 8, 32, 16, 7, 0, 6), 21, 255, "oob")]


@pytest.mark.parametrize("geom,N,ign,mode", CM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_one_launch_against_itself(dev, geom, N, ign, mode):
    """A of the module docstring, on the geometries of test_gpu_head_objective.SELF_CASES: every window 3 .. 15, every channel-tile count,
    14-, 15- and 30-pixel cell rows, 32 x 16 cells, two images, twelve heads, targets outside the classes, ignore_index inside them, every
    pixel ignored."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, _, heads = geom
    Ho, Wo = h * dy, w * dx
    s = sum(geom) + N
    _, (q5, k5, pv5, bd) = make_inputs(geom, N, (s + 1, s + 2, s + 3, s + 4), dev)
    t = make_target(B, Ho, Wo, N, ign, mode).to(dev)
    kw = dict(n_out=N, ignore_index=ign, path="fused", target=t)
    pre = prefill(N, s + 5, dev)
    cm = pre.clone()
    loss, labels, g, L = ops.xna_head_objective(q5, k5, pv5, bd, ksz, want_loss=True, want_labels=True, want_dlogits=True, return_logits=True,
                                                confusion=cm, **kw)
    counts = cm - pre
    valid = valid_of(t, ign, N)
    nvalid = int(valid.sum())
    print(f"cm self {geom} N={N} {mode}: {nvalid} valid pixels of {B * Ho * Wo}, {int((counts != 0).sum())} non-zero entries")
    assert (nvalid == 0) == (mode == "all")
    assert bool((counts >= 0).all()) and int(counts.sum()) == nvalid, f"matrix sums to {int(counts.sum())}, {nvalid} valid pixels"
    ref = ops.head_confusion_from_labels(labels, t, ign, N)
    assert torch.equal(counts, ref), f"matrix differs from the launch's own labels on {int((counts != ref).sum())} entries"
    assert torch.equal(counts.sum(dim=1), torch.bincount(t[valid], minlength=N)), "row sums are not the targets' histogram"
    if mode == "all":
        assert torch.equal(cm, pre)
    if 0 <= ign < N:
        assert int(counts[ign].sum()) == 0
    # every other output is what naf_xna_head_ce_fwd stores for the same arguments
    ce = ops.xna_head_objective(q5, k5, pv5, bd, ksz, want_loss=True, want_labels=True, want_dlogits=True, return_logits=True, **kw)
    for name, a, b in zip(("loss", "labels", "dlogits", "logits"), (loss, labels, g, L), ce):
        assert a.dtype == b.dtype and torch.equal(a, b), f"{name} differs from naf_xna_head_ce_fwd's"
    # the matrix alone (no label map written), and beside the labels only: the NULL branches change nothing
    alone = torch.zeros(N, N, dtype=torch.int64, device=dev)
    assert ops.xna_head_objective(q5, k5, pv5, bd, ksz, confusion=alone, **kw) == (None, None, None, None)
    assert torch.equal(alone, ref)
    beside = torch.zeros(N, N, dtype=torch.int64, device=dev)
    lab2 = ops.xna_head_objective(q5, k5, pv5, bd, ksz, want_labels=True, confusion=beside, **kw)[1]
    assert torch.equal(beside, ref) and torch.equal(lab2, labels)
    # the composition has the same contract
    comp = torch.zeros(N, N, dtype=torch.int64, device=dev)
    lc = ops.xna_head_objective(q5, k5, pv5, bd, ksz, n_out=N, ignore_index=ign, target=t, want_labels=True, confusion=comp, path="composed")[1]
    assert torch.equal(comp, ops.head_confusion_from_labels(lc, t, ign, N)) and int(comp.sum()) == nvalid


def test_accumulation_and_row_stride(dev):
    """B: pre-fill + counts after one launch, pre-fill + 2 x counts after a second identical one; a row stride larger than N leaves the gap
    untouched; a strided int32 target counts the same."""
    from naf_amd import ops
    geom, N = (1, 6, 7, 14, 14, 5, 192, 4), 21            # 14 x 14 cells: partial row tiles
    B, h, w, dy, dx, ksz, _, heads = geom
    _, (q5, k5, pv5, bd) = make_inputs(geom, N, (11, 12, 13, 14), dev)
    t = make_target(B, h * dy, w * dx, N, 255, "oob").to(dev)
    kw = dict(n_out=N, ignore_index=255, path="fused", target=t)
    counts = torch.zeros(N, N, dtype=torch.int64, device=dev)
    labels = ops.xna_head_objective(q5, k5, pv5, bd, ksz, want_labels=True, confusion=counts, **kw)[1]
    assert torch.equal(counts, ops.head_confusion_from_labels(labels, t, 255, N)) and int(counts.sum()) == int(valid_of(t, 255, N).sum()) > 0
    pre = prefill(N, 15, dev)
    cm = pre.clone()
    ops.xna_head_objective(q5, k5, pv5, bd, ksz, confusion=cm, **kw)
    assert torch.equal(cm, pre + counts)
    ops.xna_head_objective(q5, k5, pv5, bd, ksz, confusion=cm, **kw)
    assert torch.equal(cm, pre + 2 * counts)
    view = prefill(N, 15, dev, stride=N + 11)
    wide = view._base
    assert view.stride(0) == N + 11 and torch.equal(view, pre)
    ops.xna_head_objective(q5, k5, pv5, bd, ksz, confusion=view, **kw)
    assert torch.equal(wide[:, :N], pre + counts) and bool((wide[:, N:] == -7).all()), "the gap of a row-strided matrix was written"
    t2 = torch.zeros(B, h * dy, 2 * w * dx, dtype=torch.int32, device=dev)
    t2[:, :, ::2] = t
    other = torch.zeros(N, N, dtype=torch.int64, device=dev)
    ops.xna_head_objective(q5, k5, pv5, bd, ksz, n_out=N, ignore_index=255, path="fused", target=t2[:, :, ::2], confusion=other)
    assert torch.equal(other, counts)
    with pytest.raises(ValueError, match="needs a target"):
        ops.xna_head_objective(q5, k5, pv5, bd, ksz, n_out=N, confusion=other)
    with pytest.raises(TypeError, match="int64"):
        ops.xna_head_objective(q5, k5, pv5, bd, ksz, confusion=other.int(), **kw)
    with pytest.raises(ValueError, match=r"\[N, N\]"):
        ops.xna_head_objective(q5, k5, pv5, bd, ksz, confusion=torch.zeros(N, N + 1, dtype=torch.int64, device=dev), **kw)


def test_two_launches_are_bit_equal(dev):
    from naf_amd import ops
    geom, N = (2, 9, 9, 14, 14, 9, 0, 12), 151
    B, h, w, dy, dx, ksz, _, heads = geom
    _, (q5, k5, pv5, bd) = make_inputs(geom, N, (21, 22, 23, 24), dev)
    t = make_target(B, h * dy, w * dx, N, 255).to(dev)
    a, b = (torch.zeros(N, N, dtype=torch.int64, device=dev) for _ in range(2))
    for cm in (a, b):
        ops.xna_head_objective(q5, k5, pv5, bd, ksz, n_out=N, ignore_index=255, path="fused", target=t, confusion=cm)
    assert torch.equal(a, b) and int(a.sum()) == int(valid_of(t, 255, N).sum())


def test_all_pixels_on_one_counter(dev):
    """The contended path, once, at 1024 x 1024 from 64 x 64 (window 7, four heads, N = 21): a constant target and a bias that makes one class
    win everywhere put every pixel on one entry."""
    from naf_amd import ops
    N, H, h, heads, ksz = 21, 1024, 64, 4, 7
    gen = torch.Generator(device=dev).manual_seed(7)
    q5 = torch.randn((1, H, H, heads, 64), device=dev, generator=gen).to(torch.bfloat16).permute(0, 3, 1, 2, 4)
    k5 = torch.randn((1, h, h, heads, 64), device=dev, generator=gen).to(torch.bfloat16).permute(0, 3, 1, 2, 4)
    pv5 = torch.randn((1, heads, h, h, 32), device=dev, generator=gen).to(torch.bfloat16)
    pv5[..., N:] = 0
    bias = torch.zeros(N, device=dev)
    bias[13] = 1.0e4
    t = torch.full((1, H, H), 4, dtype=torch.int64, device=dev)
    cm = torch.zeros(N, N, dtype=torch.int64, device=dev)
    ops.xna_head_objective(q5, k5, pv5, bias, ksz, n_out=N, ignore_index=255, path="fused", target=t, confusion=cm)
    assert int(cm[4, 13]) == H * H, f"{int(cm[4, 13])} of {H * H} pixels counted"
    cm[4, 13] = 0
    assert int(cm.abs().sum()) == 0


@pytest.mark.parametrize("N,mode", [(21, "oob"), (151, "ignore")])
def test_confusion_matches_oracle(dev, N, mode):
    """C of the module docstring.  Inputs: seeds 901 / 902 / 903 / 904 of hash_normal for q / k / PV / bias on LABEL_GEOM."""
    from naf_amd import ops
    geom = LABEL_GEOM
    B, h, w, dy, dx, ksz, _, heads = geom
    Ho, Wo = h * dy, w * dx
    (q, k, pvn, bias), (q5, k5, pv5, bd) = make_inputs(geom, N, (901, 902, 903, 904), dev)
    ref, abs_sum = head_reference(q, k, pvn, ksz, heads, N, bias)
    bound = (heads * 6e-3 + 6e-3 * abs_sum).amax(dim=1).double()              # [B, Ho, Wo]
    ref64 = ref.double()
    top = ref64.topk(2, dim=1).values
    det = (top[:, 0] - top[:, 1]) > 2.0 * bound
    share = float(det.double().mean())
    print(f"cm oracle {geom} N={N}: determined share {share:.3f}")
    assert share >= 0.75, f"inputs leave only {share:.3f} of the pixels determined"      # a condition on the inputs, before the device result
    ign = 255
    t = make_target(B, Ho, Wo, N, ign, mode)
    valid = valid_of(t, ign, N)
    n_u = int((valid & ~det).sum())
    cm_ref = ops.head_confusion_from_labels(ref64.argmax(1), t, ign, N)
    cm = torch.zeros(N, N, dtype=torch.int64, device=dev)
    ops.xna_head_objective(q5, k5, pv5, bd, ksz, n_out=N, target=t.to(dev), ignore_index=ign, path="fused", confusion=cm)
    cm = cm.cpu()
    diff = int((cm - cm_ref).abs().sum())
    print(f"    sum |cm - cm_oracle| = {diff}, 2 |U| = {2 * n_u} ({int(valid.sum())} valid pixels)")
    assert torch.equal(cm.sum(dim=1), cm_ref.sum(dim=1)), "row sums (the targets' histogram) differ from the oracle's"
    assert diff <= 2 * n_u


def _np_metrics(labels, t, ignore_index, N):
    p, q = labels.cpu().numpy().reshape(-1), t.cpu().numpy().reshape(-1)
    v = (q != ignore_index) & (q >= 0) & (q < N)
    p, q = p[v], q[v]
    acc = np.float64((p == q).sum()) / np.float64(v.sum())
    inter = np.array([((p == c) & (q == c)).sum() for c in range(N)], dtype=np.float64)
    union = np.array([((p == c) | (q == c)).sum() for c in range(N)], dtype=np.float64)
    present = union != 0
    iou = np.where(present, inter / np.where(present, union, 1.0), 0.0)
    return acc, iou, iou[present].mean(), present


def test_module_confusion(dev):
    """Module level: confusion=True equals the matrix of predict=True's labels on a served geometry and on one the kernel does not serve
    (non-integer ratio: the composition); three batches into one tensor; predict=True beside it; no graph under enable_grad with a probe
    that requires grad; confusion_metrics against numpy float64; all ignored; an empty batch; more than 256 classes."""
    import naf_amd
    from naf_amd import ops
    p = O.make_params(seed=32)
    m = _load_model(dev, p, kernel_size=7)
    N = 19
    img, ft = O.hash_normal((2, 3, 96, 128), 611).to(dev), O.hash_normal((2, 128, 8, 8), 612).to(dev)
    conv = _probe(128, N, 613, dev)
    for size, mode in (((96, 128), "ignore"), ((50, 70), "oob")):
        t = make_target(2, *size, N, 255, mode).to(dev)
        with torch.no_grad():
            pred = m(img, ft, size, head=conv, predict=True)
            cm = m(img, ft, size, head=conv, target=t, ignore_index=255, confusion=True)
            cm2, lab = m(img, ft, size, head=conv, target=t, ignore_index=255, confusion=True, predict=True)
        ref = ops.head_confusion_from_labels(pred, t, 255, N)
        assert cm.dtype == torch.int64 and tuple(cm.shape) == (N, N) and cm.device == t.device
        assert torch.equal(cm, ref) and int(cm.sum()) == int(valid_of(t, 255, N).sum()) > 0, size
        assert torch.equal(cm2, ref) and lab.dtype == torch.int64 and torch.equal(lab, pred)
        # under enable_grad with a probe that requires grad: an evaluation, no graph
        assert conv.weight.requires_grad
        with torch.enable_grad():
            cg, lg = m(img, ft, size, head=conv, target=t, ignore_index=255, confusion=True, predict=True)
        assert torch.equal(cg, ref) and cg.grad_fn is None and not cg.requires_grad and lg.grad_fn is None and conv.weight.grad is None
        r = naf_amd.confusion_metrics(cm)
        acc, iou, miou, present = _np_metrics(pred, t, 255, N)
        assert r.accuracy.device == cm.device and r.iou.dtype == torch.float64
        assert abs(float(r.accuracy) - acc) <= 1e-15 and abs(float(r.miou) - miou) <= 1e-15
        assert np.abs(r.iou.cpu().numpy() - iou).max() <= 1e-15 and r.present.cpu().numpy().tolist() == present.tolist()
    # an evaluation loop: three batches into one tensor == the sum of three fresh matrices
    size = (96, 128)
    total = torch.zeros(N, N, dtype=torch.int64, device=dev)
    fresh = []
    with torch.no_grad():
        for i in range(3):
            im, f = O.hash_normal((2, 3, 96, 128), 620 + i).to(dev), O.hash_normal((2, 128, 8, 8), 630 + i).to(dev)
            ti = make_target(2, *size, N, 255).roll(17 * i, dims=2).to(dev)
            assert m(im, f, size, head=conv, target=ti, ignore_index=255, confusion=total) is total
            fresh.append(m(im, f, size, head=conv, target=ti, ignore_index=255, confusion=True))
        assert torch.equal(total, fresh[0] + fresh[1] + fresh[2])
        # every pixel ignored, an empty batch: the matrix stays what it was (zeros for True)
        t = make_target(2, *size, N, 255).to(dev)
        keep = total.clone()
        m(img, ft, size, head=conv, target=torch.full_like(t, 255), ignore_index=255, confusion=total)
        assert torch.equal(total, keep)
        z, zl = m(img[:0], ft[:0], size, head=conv, target=t[:0], confusion=total, predict=True)
        assert z is total and torch.equal(total, keep) and zl.shape == (0, *size) and zl.dtype == torch.int64
        z = m(img[:0], ft[:0], size, head=conv, target=t[:0], confusion=True)
        assert tuple(z.shape) == (N, N) and int(z.abs().sum()) == 0
        # more than 256 classes: the composition counts its labels
        big = _probe(128, 300, 614, dev)
        tb = make_target(2, *size, 300, 255).to(dev)
        cb = m(img, ft, size, head=big, target=tb, ignore_index=255, confusion=True)
        assert tuple(cb.shape) == (300, 300)
        assert torch.equal(cb, ops.head_confusion_from_labels(m(img, ft, size, head=big, predict=True), tb, 255, 300))
    with pytest.raises(ValueError, match=r"\[N, N\]"):
        m(img, ft, size, head=conv, target=t, confusion=torch.zeros(N + 1, N + 1, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="confusion is on"):
        m(img, ft, size, head=conv, target=t, confusion=torch.zeros(N, N, dtype=torch.int64))
