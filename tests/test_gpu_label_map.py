"""GPU tests of the label-map path (``naf_amd.masks_to_labels`` / naf_mask_labels, ``labels_to_masks``, ``VideoTracker``) against the
restatement of the reference (tests/label_map_reference.py, evaluation/eval_video_seg.py:389-457, :611-643).  tests/test_label_map_cpu.py
asserts, from the reference alone, the condition each case rests on (the undecided share, and that the two forms of the restatement
agree)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_map_reference as R  # noqa: E402
import propagate_reference as P  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pil_nearest_tables.npz"))


def _check(got, ci):
    """Equal to ``exact`` on every decided pixel; the undecided share is capped (asserted again: it is a condition of the comparison)."""
    _, lab, margin, tau = R.reference(ci)
    und = R.undecided(margin, tau)
    got = got.cpu()
    assert got.dtype == torch.uint8 and got.shape == lab.shape
    bad = (got != lab) & ~und
    print(f"{R.CASE_IDS[ci]}: {int(bad.sum())} of {int((~und).sum())} decided pixels differ; {int(und.sum())} undecided, "
          f"{int(((got != lab) & und).sum())} of them differ")
    assert float(und.double().mean()) <= R.MAX_UNDECIDED_SHARE
    assert not bool(bad.any()), [(tuple(i.tolist()), int(got[tuple(i)]), int(lab[tuple(i)])) for i in bad.nonzero()[:8]]


# ---- A. against the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [pytest.param(i, id=R.CASE_IDS[i]) for i in range(len(R.CASES))])
def test_matches_the_restatement_on_decided_pixels(dev, ci):
    import naf_amd
    K, _, mid, out, kind = R.CASES[ci]
    seg = R.reference(ci)[0].to(dev)
    got = naf_amd.masks_to_labels(seg, mid, out)
    assert tuple(got.shape) == tuple(out) and got.device == seg.device
    _check(got, ci)
    # exact ties, a channel without a positive value and the NaN rule are decided: stated here as well, without the restatement
    if kind in ("constant", "identical") or K == 1:
        assert not bool(got.any())
    if kind == "one-constant":
        assert bool((got == 2).all())
    if kind == "two-constant":
        assert bool((got == 1).all())
    if kind == "zero-among-disjoint":
        assert set(got.unique().tolist()) == {0, 2}
    assert torch.equal(got, naf_amd.masks_to_labels(seg[None], mid, out))          # [1, K, h, w], as propagate_labels returns it


def test_table_on_the_device_equals_the_fixture(dev, golden):
    from naf_amd import ops
    for n_in, n_out in R.FIXTURE_PAIRS:
        t = ops.device_nearest_table(n_in, n_out, dev)
        assert t.dtype == torch.int32 and t.device.type == "cuda"
        assert np.array_equal(t.cpu().numpy(), golden[f"t_{n_in}_{n_out}"]), (n_in, n_out)
        assert ops.device_nearest_table(n_in, n_out, dev) is t                     # cached per (n_in, n_out, device)


# ---- B. the forms the call accepts -----------------------------------------------------------------------------------------------------------
def test_a_seg_that_is_not_contiguous(dev):
    import naf_amd
    ci = 1
    K, (h, w), mid, out, _ = R.CASES[ci]
    seg = R.reference(ci)[0].to(dev)
    base = naf_amd.masks_to_labels(seg, mid, out)
    wide = torch.full((K, h + 3, 2 * w + 5), float("nan"), device=dev)             # every other column of a window of a larger buffer
    view = wide[:, 2:2 + h, 3:3 + 2 * w:2]
    view.copy_(seg)
    assert not view.is_contiguous()
    assert torch.equal(naf_amd.masks_to_labels(view, mid, out), base)
    hwk = seg.permute(1, 2, 0).contiguous().permute(2, 0, 1)                       # channels last
    assert not hwk.is_contiguous()
    assert torch.equal(naf_amd.masks_to_labels(hwk, mid, out), base)
    _check(base, ci)


def test_out_is_written_in_place_and_nothing_else(dev):
    import naf_amd
    ci = 1
    _, _, mid, (oh, ow), _ = R.CASES[ci]
    seg = R.reference(ci)[0].to(dev)
    base = naf_amd.masks_to_labels(seg, mid, (oh, ow))
    big = torch.full((3, oh + 4, ow + 9), 201, dtype=torch.uint8, device=dev)      # a sequence buffer with margins, filled with a sentinel
    view = big[1, 2:2 + oh, 4:4 + ow]
    res = naf_amd.masks_to_labels(seg, mid, (oh, ow), out=view)
    assert res.data_ptr() == view.data_ptr() and torch.equal(view, base)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[1, 2:2 + oh, 4:4 + ow] = False
    assert bool((big[mask] == 201).all())
    seq = torch.full((3, oh, ow), 201, dtype=torch.uint8, device=dev)              # row t of a dense [T, H, W] buffer, as davis_jf reads it
    naf_amd.masks_to_labels(seg, mid, (oh, ow), out=seq[1])
    assert torch.equal(seq[1], base) and bool((seq[0] == 201).all()) and bool((seq[2] == 201).all())
    with pytest.raises(ValueError, match="torch.uint8 tensor of shape"):
        naf_amd.masks_to_labels(seg, mid, (oh, ow), out=seq)
    with pytest.raises(ValueError, match="adjacent columns"):
        naf_amd.masks_to_labels(seg, mid, (oh, ow), out=torch.zeros(ow, oh, dtype=torch.uint8, device=dev).t())


def test_two_runs_give_the_same_bits(dev):
    import naf_amd
    for ci in (2, 4):
        _, _, mid, out, _ = R.CASES[ci]
        seg = R.reference(ci)[0].to(dev)
        assert torch.equal(naf_amd.masks_to_labels(seg, mid, out), naf_amd.masks_to_labels(seg, mid, out))


# ---- C. the first frame and the tracker ----------------------------------------------------------------------------------------------------
def test_labels_to_masks_is_the_fixtures_gather_and_one_hot(dev, golden):
    import naf_amd
    _, labels = R.tracker_inputs()
    ty, tx = torch.tensor(golden["t_13_9"]).long(), torch.tensor(golden["t_23_13"]).long()
    want = F.one_hot(labels[ty][:, tx].long(), 3).permute(2, 0, 1)[None].float()
    got = naf_amd.labels_to_masks(labels.to(dev), (9, 13))
    assert got.device.type == "cuda" and got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    assert torch.equal(naf_amd.labels_to_masks(labels.long().to(dev), (9, 13), num_classes=3).cpu(), want)


def test_video_tracker_steps(dev):
    """T = 5 frames through a queue of 2, so the queue fills and pops.  Every step is recomputed from the tracker's OWN context, captured
    before the step: the soft masks it pushed against ``propagate_reference.windowed`` on that context (that module's bound, its ambiguous
    pixels excluded under its cap), and the label map it returned against the label yardstick on the masks it pushed -- the very input
    ``masks_to_labels`` received, so an ambiguous propagated pixel does not enter the label comparison a second time."""
    import naf_amd
    t = R.TRACKER
    frames, labels = R.tracker_inputs()
    (h, w), K, C_ = t["grid"], t["K"], t["C"]
    trk = naf_amd.VideoTracker(frames[0].to(dev), labels.to(dev), ps=t["ps"], ups_factor=t["ups_factor"], n_last_frames=t["n_last_frames"],
                               radius=t["radius"], topk=t["topk"], temperature=t["temperature"], num_classes=K)
    assert trk.mid_size == (15, 22) and trk.out_size == t["out"]
    assert len(trk.context_feats) == len(trk.context_segs) == 1
    assert torch.equal(trk.context_segs[0].cpu(), R.one_hot_first_frame(labels, (h, w), K))
    pred = torch.full((t["T"], *t["out"]), 201, dtype=torch.uint8, device=dev)
    delta_s = (C_ + 8) * 2.0 ** -24
    for i, f in enumerate(frames[1:], start=1):
        ctx_f, ctx_s = trk.context_feats, trk.context_segs
        assert len(ctx_f) == len(ctx_s) == 1 + min(i - 1, t["n_last_frames"])
        f_dev = f.to(dev)
        torch.cuda.set_sync_debug_mode("error")                                     # a step makes no host synchronisation: torch raises on one
        try:
            if i % 2:
                lab = trk.step(f_dev)
                pred[i] = lab
            else:
                lab = trk.step(naf_amd.pack_frame(f_dev), out=pred[i])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        if i % 2 == 0:
            assert lab.data_ptr() == pred[i].data_ptr()
        assert lab.dtype == torch.uint8 and tuple(lab.shape) == t["out"]
        assert trk.context_feats[0] is ctx_f[0] and trk.context_segs[0] is ctx_s[0]
        pushed = trk.context_segs[-1]
        assert tuple(pushed.shape) == (1, K, h, w) and torch.equal(trk.context_feats[-1].data.cpu(), f.permute(1, 2, 0))
        if i > 1:
            assert trk.context_segs[-2] is ctx_s[-1]                                # the order of the queue
        segs = torch.cat([s.cpu() for s in ctx_s])
        ref, ambiguous, _ = P.windowed(f, [c.data.cpu().permute(2, 0, 1) for c in ctx_f], segs, t["radius"], t["topk"], t["temperature"])
        assert float(ambiguous.double().mean()) <= P.MAX_AMBIGUOUS_SHARE
        err = (pushed.double().cpu() - ref).abs().amax(1)[0]
        bound = 2.0 * (delta_s / t["temperature"] + 2.0 ** -20) * float(segs.abs().max())
        want, margin, tau = R.exact(pushed[0].cpu(), trk.mid_size, trk.out_size)
        und = R.undecided(margin, tau)
        bad = (lab.cpu() != want) & ~und
        print(f"frame {i}: context {len(ctx_f)}, propagation max err {float(err[~ambiguous].max()):.3e} (bound {bound:.3e}), "
              f"{int(ambiguous.sum())} ambiguous; labels: {int(bad.sum())} of {int((~und).sum())} decided pixels differ, {int(und.sum())} undecided")
        assert float(err[~ambiguous].max()) <= bound
        assert float(und.double().mean()) <= R.MAX_UNDECIDED_SHARE
        assert not bool(bad.any())
    assert bool((pred[0] == 201).all()) and int(pred[1:].max()) <= K - 1
    with pytest.raises(ValueError, match="first frame"):
        trk.step(torch.zeros(C_, h, w + 1, dtype=torch.bfloat16, device=dev))
    assert len(trk.context_feats) == 1 + t["n_last_frames"]                        # a refused step leaves the queue as it was
