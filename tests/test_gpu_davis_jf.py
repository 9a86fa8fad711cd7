"""GPU tests of the DAVIS J and F measures (``naf_amd.davis_jf``, naf_davis_jf): against the disk form of the restatement of the reference
(tests/davis_reference.py, evaluation/eval_video_seg.py:145-248), exact checks that need no reference, and the forms the public call
accepts its label maps in."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import davis_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _t(x, dev):
    return torch.tensor(np.asarray(x)).to(dev)             # a copy: the shared reference arrays are read-only


def _check(res, counts, what):
    """counts equal, J and F within 1e-15 of the fp64 restatement: at most six correctly rounded fp64 operations on values <= 1 lie between the
    integer counts and J or F (2^-53 each)."""
    J, F = R.jf_from_counts(counts)
    got = res.counts.cpu()
    assert res.counts.dtype == torch.int64 and res.J.dtype == res.F.dtype == torch.float64 and not res.J.requires_grad
    assert tuple(got.shape) == counts.shape and tuple(res.J.shape) == tuple(res.F.shape) == counts.shape[:2]
    bad = (got != torch.tensor(counts)).nonzero()
    eJ, eF = float((res.J.cpu() - torch.tensor(J)).abs().max()), float((res.F.cpu() - torch.tensor(F)).abs().max())
    print(f"{what}: {bad.shape[0]} of {counts.size} counters differ; max |J - ref| = {eJ:.3e}, max |F - ref| = {eF:.3e}")
    assert bad.shape[0] == 0, [(tuple(i.tolist()), int(got[tuple(i)]), int(counts[tuple(i.tolist())])) for i in bad[:8]]
    assert eJ <= 1e-15 and eF <= 1e-15


# ---- A. against the disk-form restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [pytest.param(i, id=R.CASE_IDS[i]) for i in range(len(R.CASES))])
def test_matches_the_disk_form(dev, ci):
    import naf_amd
    N, bound_th = R.CASES[ci][3], R.CASES[ci][4]
    (ann, seg), counts, J, F = R.reference(ci)
    res = naf_amd.davis_jf(_t(ann, dev), _t(seg, dev), num_objects=N, bound_th=bound_th)
    _check(res, counts, R.CASE_IDS[ci])
    if ci == 3:                                   # the object absent from both maps: J = 1, F = 0
        assert bool((res.J[4] == 1).all()) and bool((res.F[4] == 0).all()) and bool((res.F[2:4] == 0).all())
    if ci == 5:
        assert R.bound_pix(bound_th, 480, 854) == 8.0


# ---- B. exact checks that need no reference ---------------------------------------------------------------------------------------------
def test_identical_maps(dev):
    import naf_amd
    (ann, _), _, _, _ = R.reference(3)
    a = _t(ann, dev)
    c = naf_amd.davis_jf(a, a.clone(), num_objects=5, bound_th=8).counts
    assert torch.equal(c[..., 0], c[..., 1]) and torch.equal(c[..., 4], c[..., 2]) and torch.equal(c[..., 5], c[..., 3])
    assert torch.equal(c[..., 2], c[..., 3]) and int(c[:3, :, 2].min()) > 0


def _rectangles():
    ann = np.zeros((1, 40, 48), dtype=np.uint8)
    seg = np.zeros_like(ann)
    ann[0, 10:22, 14:32] = 1
    seg[0, 13:25, 18:36] = 1                      # shifted by (3, 4): every boundary pixel's nearest partner is exactly 5 away
    return ann, seg


def test_the_disks_exact_rim(dev):
    import naf_amd
    ann, seg = _rectangles()
    a, s = _t(ann, dev), _t(seg, dev)
    c = naf_amd.davis_jf(a, s, num_objects=1, bound_th=5).counts.cpu()
    assert c[0, 0, 2:].tolist() == [120, 120, 120, 120]
    c = naf_amd.davis_jf(a, s, num_objects=1, bound_th=4.9).counts.cpu()
    ref = R.counts_disk(ann, seg, 1, 4.9)
    assert ref[0, 0, 4] < 120 and ref[0, 0, 5] < 120
    assert c.numpy().tolist() == ref.tolist()


def test_a_mask_edge_on_the_tile_borders(dev):
    import naf_amd
    from naf_amd import _lib
    TW, TH = _lib.DAVIS_TILE_W, _lib.DAVIS_TILE_H
    H, W = 2 * TH + 9, 2 * TW + 7
    ann = np.zeros((2, H, W), dtype=np.uint8)
    seg = np.zeros_like(ann)
    ann[0, :TH, :TW] = 1                           # the mask ends on the last row / column of a tile ...
    ann[0, TH:2 * TH, TW:2 * TW] = 2               # ... and begins on the first ones of the next
    seg[0, :TH + 1, :TW - 1] = 1
    seg[0, TH - 1:2 * TH, TW + 1:2 * TW] = 2
    ann[1, TH:, :] = 1                             # a straight edge on a tile's row border, and one on its column border
    seg[1, :, TW:] = 1
    for bound_th in (1, 3):
        res = naf_amd.davis_jf(_t(ann, dev), _t(seg, dev), num_objects=2, bound_th=bound_th)
        _check(res, R.counts_disk(ann, seg, 2, bound_th), f"tile borders, bound_th {bound_th}")


def test_labels_above_n_are_ignored_and_missing_objects_are_empty(dev):
    import naf_amd
    (ann, seg), _, _, _ = R.reference(1)           # three objects
    a, s = _t(ann, dev), _t(seg, dev)
    two = naf_amd.davis_jf(a, s, num_objects=2, bound_th=3).counts
    za, zs = a.clone(), s.clone()
    za[za > 2] = 0
    zs[zs > 2] = 0
    assert torch.equal(two, naf_amd.davis_jf(za, zs, num_objects=2, bound_th=3).counts)
    assert torch.equal(two, naf_amd.davis_jf(a, s, num_objects=3, bound_th=3).counts[:2])
    s200 = s.clone()
    s200[s == 3] = 200                             # a label far above N
    res = naf_amd.davis_jf(a, s200, num_objects=3, bound_th=3)
    assert torch.equal(res.counts[:2], two)
    c3 = res.counts[2]                             # the reference's zero padding: an empty segmentation mask for object 3
    assert bool((c3[:, 0] == 0).all()) and bool((c3[:, 2] == 0).all()) and bool((c3[:, 4:] == 0).all()) and bool((c3[:, 1] > 0).all())
    assert bool((res.J[2] == 0).all()) and bool((res.F[2] == 0).all())
    five = naf_amd.davis_jf(a, s, num_objects=5, bound_th=3)
    assert bool((five.counts[3:] == 0).all()) and bool((five.J[3:] == 1).all()) and bool((five.F[3:] == 0).all())


def test_input_forms(dev):
    import naf_amd
    (ann, seg), counts, _, _ = R.reference(1)
    a, s = _t(ann, dev), _t(seg, dev)
    base = naf_amd.davis_jf(a, s, num_objects=3, bound_th=3).counts
    assert torch.equal(base.cpu(), torch.tensor(counts))
    assert torch.equal(base, naf_amd.davis_jf(a.long(), s.long(), num_objects=3, bound_th=3).counts)
    assert torch.equal(base, naf_amd.davis_jf(a.long(), s, num_objects=3, bound_th=3).counts)
    wide = torch.zeros(2, 37, 2 * 53 + 1, dtype=torch.uint8, device=dev)
    wide[:, :, 1::2] = a
    view = wide[:, :, 1::2]
    assert not view.is_contiguous()
    assert torch.equal(base, naf_amd.davis_jf(view, s, num_objects=3, bound_th=3).counts)
    tview = a.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not tview.is_contiguous()
    assert torch.equal(base, naf_amd.davis_jf(tview, s, num_objects=3, bound_th=3).counts)
    one = naf_amd.davis_jf(a[1], s[1], num_objects=3, bound_th=3)
    assert tuple(one.counts.shape) == (3, 1, 6) and torch.equal(one.counts[:, 0], base[:, 1])
    neg = a.long()
    neg[neg == 0] = -7                             # an int64 map may hold anything: below 1 is background
    assert torch.equal(base, naf_amd.davis_jf(neg, s, num_objects=3, bound_th=3).counts)


def test_two_calls_give_the_same_bits(dev):
    import naf_amd
    (ann, seg), _, _, _ = R.reference(3)
    a, s = _t(ann, dev), _t(seg, dev)
    r1, r2 = naf_amd.davis_jf(a, s, num_objects=5, bound_th=8), naf_amd.davis_jf(a, s, num_objects=5, bound_th=8)
    assert torch.equal(r1.counts, r2.counts) and torch.equal(r1.J, r2.J) and torch.equal(r1.F, r2.F)


def test_num_objects_none_derives_n_and_refuses_higher_labels(dev):
    import naf_amd
    (ann, seg), counts, _, _ = R.reference(1)
    a, s = _t(ann, dev), _t(seg, dev)
    res = naf_amd.davis_jf(a, s, bound_th=3)
    assert tuple(res.counts.shape) == (3, 2, 6) and torch.equal(res.counts.cpu(), torch.tensor(counts))
    s4 = s.clone()
    s4[0, 5, 5] = 4
    with pytest.raises(ValueError, match="index higher than the number of objects"):
        naf_amd.davis_jf(a, s4, bound_th=3)
    with pytest.raises(ValueError, match="no object"):
        naf_amd.davis_jf(torch.zeros_like(a), s, bound_th=3)
    with pytest.raises(ValueError, match="1 <= N <= 32"):
        naf_amd.davis_jf(a + 40, s, bound_th=3)
