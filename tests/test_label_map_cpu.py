"""CPU tests of the label-map path (``naf_amd.nearest_index_table``, ``masks_to_labels``, ``labels_to_masks``, ``VideoTracker``): Pillow's
nearest resize as index tables, the limits the library names, and the yardstick of the GPU tests (tests/label_map_reference.py) held
against itself -- the condition every GPU case rests on is asserted here from the reference alone."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_map_reference as R  # noqa: E402
import propagate_reference as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(built_lib):
    from naf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pil_nearest_tables.npz"))


# ---- A. Pillow's nearest resize -------------------------------------------------------------------------------------------------------------
def test_table_replay_equals_the_golden_fixture(lib, golden):
    import naf_amd
    pairs = [tuple(int(v) for v in p) for p in golden["pairs"]]
    assert set(R.FIXTURE_PAIRS) <= set(pairs) and set(R.DAVIS_PAIRS) <= set(pairs)
    for n_in, n_out in pairs:
        want = golden[f"t_{n_in}_{n_out}"]
        got = naf_amd.nearest_index_table(n_in, n_out)
        assert got.dtype == torch.int32 and got.shape == (n_out,)
        assert np.array_equal(got.numpy(), want), (n_in, n_out)
        assert R.pil_table(n_in, n_out) == want.tolist(), (n_in, n_out)


def test_table_replay_equals_pillow(lib):
    Image = pytest.importorskip("PIL.Image")
    import naf_amd

    def pillow(n_in, n_out, axis):
        idx = np.arange(n_in, dtype=np.int32)
        if axis == 1:
            return np.array(Image.fromarray(np.repeat(idx[None], 2, 0)).resize((n_out, 2), 0))[0]
        return np.array(Image.fromarray(np.repeat(idx[:, None], 2, 1)).resize((2, n_out), 0))[:, 0]

    pairs = R.FIXTURE_PAIRS + [(a, b) for a in range(1, 64, 3) for b in range(1, 64, 5)] + [(255, 257), (257, 255), (259, 1), (1, 259)]
    for n_in, n_out in pairs:
        got = naf_amd.nearest_index_table(n_in, n_out).numpy()
        for axis in (0, 1):
            assert np.array_equal(got, pillow(n_in, n_out, axis)), (n_in, n_out, axis)


def test_the_closed_form_is_not_the_replay(lib):
    """floor((2x + 1) n_in / (2 n_out)) is NOT what Pillow reads: the double accumulation drifts below an integer the exact quotient reaches.
    Nobody simplifies the replay into it."""
    import naf_amd
    got = naf_amd.nearest_index_table(976, 854).tolist()
    closed = R.closed_form_table(976, 854)
    assert sum(int(a != b) for a, b in zip(got, closed)) == 64
    floor_form = [min(int(x * (976 / 854)), 975) for x in range(854)]           # F.interpolate(mode="nearest")
    assert floor_form != got


def test_table_arguments(lib):
    import naf_amd
    assert naf_amd.nearest_index_table(5, 1).tolist() == [2] and naf_amd.nearest_index_table(1, 4).tolist() == [0, 0, 0, 0]
    assert naf_amd.nearest_index_table(7, 7).tolist() == list(range(7))
    for bad in ((0, 4), (4, 0), (-1, 4), (4.0, 4), (True, 4)):
        with pytest.raises(ValueError):
            naf_amd.nearest_index_table(*bad)
    assert lib.naf_nearest_resize_table(None, 4, 4) == 1


# ---- B. the C ABI's limits ---------------------------------------------------------------------------------------------------------------
def _args(K=4, h=30, w=53, mid=(60, 106), out=(67, 119)):
    from naf_amd import _lib
    a = _lib.MaskLabelsArgs()
    a.K, a.h, a.w, a.mid_h, a.mid_w, a.out_h, a.out_w = K, h, w, *mid, *out
    return a


def test_select_accepts_and_refuses_at_each_limit(lib):
    from naf_amd import _lib
    sel = lambda a: (lib.naf_mask_labels_select(C.byref(a)), _lib.last_error())   # noqa: E731
    assert lib.naf_mask_labels_select(None) == 1
    assert sel(_args())[0] == 0
    assert sel(_args(K=1, h=1, w=1, mid=(1, 1), out=(1, 1)))[0] == 0
    assert sel(_args(K=64, h=16384, w=16384, mid=(16384, 16384), out=(16384, 16384)))[0] == 0
    rc, msg = sel(_args(K=65))
    assert rc == 2 and "1 <= K <= 64" in msg
    for kw, named in ((dict(h=16385), "h, w <= 16384"), (dict(w=16385), "h, w <= 16384"), (dict(mid=(16385, 4)), "mid_h, mid_w <= 16384"),
                      (dict(mid=(4, 16385)), "mid_h, mid_w <= 16384"), (dict(out=(16385, 4)), "out_h, out_w <= 16384"),
                      (dict(out=(4, 16385)), "out_h, out_w <= 16384")):
        rc, msg = sel(_args(**kw))
        assert rc == 2 and named in msg, (kw, msg)
    for kw in (dict(K=0), dict(h=0), dict(w=-3), dict(mid=(0, 4)), dict(mid=(4, 0)), dict(out=(0, 4)), dict(out=(4, 0))):
        rc, msg = sel(_args(**kw))
        assert rc == 1 and "at least 1" in msg, (kw, msg)
    a = _args()
    a.reserved = 1
    rc, msg = sel(a)
    assert rc == 1 and "reserved" in msg


def test_the_call_refuses_bad_pointers_before_any_device_work(lib):
    from naf_amd import _lib
    a = _args()
    assert lib.naf_mask_labels(C.byref(a), None) == 1 and "NULL" in _lib.last_error()
    a.seg, a.tab_y, a.tab_x, a.out, a.workspace = 4096, 4096, 4096, 4096, 4096
    a.workspace_bytes, a.out_stride = _lib.MASK_LABELS_WORKSPACE_BYTES - 1, 119
    assert lib.naf_mask_labels(C.byref(a), None) == 1 and "workspace" in _lib.last_error()
    a.workspace_bytes, a.out_stride = _lib.MASK_LABELS_WORKSPACE_BYTES, 118
    assert lib.naf_mask_labels(C.byref(a), None) == 1 and "out_stride" in _lib.last_error()
    a.out_stride, a.seg = 119, 4098
    assert lib.naf_mask_labels(C.byref(a), None) == 1 and "aligned" in _lib.last_error()


def test_header_and_mirror_agree(lib):
    from naf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403 == _lib.HEADER_VERSION        # detected by symbol
    for name, value in (("MAX_CHANNELS", _lib.MASK_LABELS_MAX_CHANNELS), ("MAX_SIZE", _lib.MASK_LABELS_MAX_SIZE),
                        ("WORKSPACE_BYTES", _lib.MASK_LABELS_WORKSPACE_BYTES)):
        assert int(re.search(rf"#define\s+NAF_MASK_LABELS_{name}\s+(\d+)", txt).group(1)) == value
    body = re.search(r"typedef struct naf_mask_labels_args \{(.*?)\} naf_mask_labels_args;", txt, re.S).group(1)
    names = [n.split("[")[0] for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in
             re.sub(r"^\s*(const\s+)?\w+\s*\**", "", decl.strip()).replace(" ", "").split(",") if n]
    assert names == [f[0] for f in _lib.MaskLabelsArgs._fields_]
    assert C.sizeof(_lib.MaskLabelsArgs) == 5 * 8 + 8 + 3 * 8 + 8 + 8 * 4


def test_public_names_and_host_checks(lib):
    import naf_amd
    assert {"nearest_index_table", "masks_to_labels", "labels_to_masks", "VideoTracker"} <= set(naf_amd.__all__)
    seg = torch.rand(4, 6, 7)
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        naf_amd.masks_to_labels(torch.rand(65, 3, 3), (6, 6), (5, 5))
    with pytest.raises(ValueError, match="mid_h, mid_w <= 16384"):
        naf_amd.masks_to_labels(seg, (16385, 6), (5, 5))
    with pytest.raises(ValueError, match="at least 1"):
        naf_amd.masks_to_labels(seg, (6, 6), (0, 5))
    with pytest.raises(ValueError, match="float32"):
        naf_amd.masks_to_labels(seg.double(), (6, 6), (5, 5))
    with pytest.raises(ValueError, match=r"\[1, K, h, w\]"):
        naf_amd.masks_to_labels(torch.rand(2, 4, 6, 7), (6, 6), (5, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # a served request on the CPU: no torch fallback
        naf_amd.masks_to_labels(seg, (12, 14), (5, 5))
    with pytest.raises(ValueError, match="label map"):
        naf_amd.labels_to_masks(torch.zeros(4, 4), (2, 2))


def test_labels_to_masks_is_read_seg_and_to_one_hot(lib):
    """Plain torch indexing, so it runs on the CPU as well: equal to the restatement of read_seg + to_one_hot."""
    import naf_amd
    _, labels = R.tracker_inputs()
    got = naf_amd.labels_to_masks(labels, (9, 13))
    want = R.one_hot_first_frame(labels, (9, 13))
    assert got.dtype == torch.float32 and got.shape == (1, 3, 9, 13) and torch.equal(got, want)
    assert torch.equal(naf_amd.labels_to_masks(labels.long(), (9, 13), num_classes=3), want)
    five = naf_amd.labels_to_masks(labels, (9, 13), num_classes=5)
    assert five.shape == (1, 5, 9, 13) and torch.equal(five[:, :3], want) and not bool(five[:, 3:].any())
    two = naf_amd.labels_to_masks(labels, (9, 13), num_classes=2)                  # label 2 belongs to no channel
    assert torch.equal(two, want[:, :2])


# ---- C. the yardstick against itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [pytest.param(i, id=R.CASE_IDS[i]) for i in range(len(R.CASES))])
def test_cases_meet_the_cap_and_the_two_forms_agree(ci):
    """The undecided share of every GPU case is at most 0.5 % (a condition on the inputs), ``literal`` (ATen's own fp32 interpolation)
    equals ``exact`` on every decided pixel, and so does the host emulation of the library's two passes."""
    K, _, mid, out, kind = R.CASES[ci]
    seg, lab, margin, tau = R.reference(ci)
    und = R.undecided(margin, tau)
    share = float(und.double().mean())
    lit, emu = R.literal(seg, mid, out), R.emulate(seg, mid, out)
    ok = ~und
    print(f"{R.CASE_IDS[ci]}: tau {tau:.3e}, undecided {100 * share:.3f} %; literal differs on {int((lit != lab)[ok].sum())} decided pixels "
          f"({int((lit != lab).sum())} in all), the emulation on {int((emu != lab)[ok].sum())} ({int((emu != lab).sum())} in all)")
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == tuple(out)
    assert share <= R.MAX_UNDECIDED_SHARE
    assert torch.equal(lit[ok], lab[ok])
    assert torch.equal(emu[ok], lab[ok])
    if kind in ("constant", "identical"):
        assert not bool(lab.any()) and not bool(und.any())
    if kind == "one-constant":
        assert bool((lab == 2).all()) and not bool(und.any())
    if kind == "two-constant":
        assert bool((lab == 1).all()) and not bool(und.any())
    if kind == "zero-among-disjoint":
        assert set(lab.unique().tolist()) == {0, 2} and not bool(und.any())       # the all-zero channel 1 never wins: 0 ties with it first
    if kind == "blurred":
        assert len(lab.unique()) == 64
    if K == 1:
        assert not bool(lab.any())


def test_the_smooth_construction_fails_the_cap_at_64_channels():
    """Why the K = 64 case is a blurred one-hot map: the softmax construction leaves ranges near 0.001 there, and the rule excludes too much."""
    seg = R._smooth(64, 12, 20, 0)
    _, margin, tau = R.exact(seg, (21, 35), (40, 33))
    assert float(R.undecided(margin, tau).double().mean()) > R.MAX_UNDECIDED_SHARE


def test_the_tracker_case_meets_the_propagation_cap():
    """The tracker's GPU test recomputes every step with propagate_reference.windowed and excludes the pixels it marks ambiguous under that
    module's cap; here the same loop runs on the host with ``windowed`` as the propagation, and every step meets the cap -- and the label
    rule's -- from the references alone."""
    t = R.TRACKER
    frames, labels = R.tracker_inputs()
    (h, w), mid = t["grid"], tuple(v * t["ps"] // t["ups_factor"] for v in t["grid"])
    assert mid == (15, 22)
    first_seg = R.one_hot_first_frame(labels, (h, w), t["K"])
    assert first_seg.shape == (1, t["K"], h, w) and bool(first_seg.sum((0, 2, 3)).gt(0).all())
    queue = []
    for f in frames[1:]:
        ctx = [frames[0]] + [q[0] for q in queue]
        segs = torch.cat([first_seg] + [q[1] for q in queue])
        out, ambiguous, _ = P.windowed(f, ctx, segs, t["radius"], t["topk"], t["temperature"])
        assert float(ambiguous.double().mean()) <= P.MAX_AMBIGUOUS_SHARE
        seg = out.float()
        if len(queue) == t["n_last_frames"]:
            queue.pop(0)
        queue.append((f, seg))
        lab, margin, tau = R.exact(seg[0], mid, t["out"])
        und = R.undecided(margin, tau)
        assert float(und.double().mean()) <= R.MAX_UNDECIDED_SHARE
        assert torch.equal(R.literal(seg[0], mid, t["out"])[~und], lab[~und])
        assert len(lab.unique()) >= 2                                              # the objects are still there
    assert len(queue) == t["n_last_frames"]
