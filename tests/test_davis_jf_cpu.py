"""CPU tests of the DAVIS J and F measures (``naf_amd.davis_jf`` / ``davis_statistics``): the restatement of the reference
(tests/davis_reference.py, citing evaluation/eval_video_seg.py:145-269) equals the reference's own results in tests/golden/davis_jf.npz; its
disk form and its distance-transform form agree; the boundary facts of the specification hold exactly; ``davis_statistics`` equals the
restatement; the argument validation of the public call and the C ABI without a device.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import davis_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("naf_davis_jf_select", "naf_davis_jf")
SMALL_CASES = [pytest.param(i, id=R.CASE_IDS[i]) for i in range(5)]          # the 480 x 854 frame is left to the GPU test


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [pytest.param(i, id=R.CASE_IDS[i]) for i in R.GOLDEN_CASES])
def test_restatement_equals_the_references_own_results(ci, golden_dir):
    """J, F and the statistics of the restatement (disk form) against what the reference's functions returned for the same label maps,
    within 1e-15 absolute; the fixture's maps are the seeded case's."""
    z = np.load(os.path.join(golden_dir, "davis_jf.npz"))
    ann, seg = z[f"ann_{ci}"], z[f"seg_{ci}"]
    (a0, s0), _, _, _ = R.reference(ci)
    assert ann.dtype == np.uint8 and np.array_equal(ann, a0) and np.array_equal(seg, s0)
    N, bound_th = R.CASES[ci][3], float(z[f"bound_th_{ci}"])
    assert bound_th == R.CASES[ci][4]
    J, F = R.jf_from_counts(R.counts_disk(ann, seg, N, bound_th))
    eJ, eF = float(np.abs(J - z[f"J_{ci}"]).max()), float(np.abs(F - z[f"F_{ci}"]).max())
    sJ = np.array([R.statistics(J[o]) for o in range(N)])
    sF = np.array([R.statistics(F[o]) for o in range(N)])
    eS = max(float(np.abs(sJ - z[f"stats_J_{ci}"]).max()), float(np.abs(sF - z[f"stats_F_{ci}"]).max()))
    print(f"{R.CASE_IDS[ci]}: max |J - golden| = {eJ:.3e}, |F - golden| = {eF:.3e}, statistics {eS:.3e}")
    assert eJ <= 1e-15 and eF <= 1e-15 and eS <= 1e-15
    assert "BORDER_REFLECT_101" in str(z["report"])


@pytest.mark.parametrize("ci", SMALL_CASES)
def test_disk_form_equals_distance_transform_form(ci):
    """F is equal in every case, empty boundaries included; the counts are equal wherever both boundaries are non-empty."""
    pytest.importorskip("scipy.ndimage", reason="the distance-transform form needs scipy.ndimage.distance_transform_edt")
    (ann, seg), counts, J, F = R.reference(ci)
    edt = R.counts_edt(ann, seg, R.CASES[ci][3], R.CASES[ci][4])
    J2, F2 = R.jf_from_counts(edt)
    assert np.array_equal(F, F2) and np.array_equal(J, J2)
    both = (counts[..., 2] > 0) & (counts[..., 3] > 0)
    assert both.any()
    assert np.array_equal(counts[both], edt[both])
    assert np.array_equal(counts[..., :4], edt[..., :4])
    if ci == 3:                                              # objects 3, 4, 5: absent from one map or from both
        assert not both[2].any() and not both[3].any() and not both[4].any()
        assert (J[4] == 1).all() and (F[2:] == 0).all() and (counts[2:, :, 4:] == 0).all()


def test_empty_boundary_all_forms_give_f_zero():
    """A full-frame mask has no boundary: the distance transform of it is arbitrary (spurious hits), the disk form counts 0, F is 0 in both."""
    pytest.importorskip("scipy.ndimage", reason="the distance-transform form needs scipy.ndimage.distance_transform_edt")
    ann = np.ones((1, 5, 7), dtype=np.uint8)
    seg = np.zeros((1, 5, 7), dtype=np.uint8)
    seg[0, 1:4, 2:5] = 1
    d, e = R.counts_disk(ann, seg, 1, 8), R.counts_edt(ann, seg, 1, 8)
    assert d[0, 0].tolist() == [9, 35, int(R.boundary(seg[0] == 1).sum()), 0, 0, 0]
    assert np.array_equal(d[..., :4], e[..., :4])
    assert R.jf_from_counts(d)[1][0, 0] == 0.0 == R.jf_from_counts(e)[1][0, 0]


def test_boundary_facts():
    m = np.zeros((9, 11), dtype=bool)
    m[0, 0] = True
    b = R.boundary(m)
    assert b.sum() == 3 and b[0, 1] and b[1, 0] and b[1, 1] and not b[0, 0]                 # a corner pixel
    m = np.zeros((9, 11), dtype=bool)
    m[4, 5] = True
    b = R.boundary(m)
    assert b.sum() == 8 and not b[4, 5] and b[3:6, 4:7].sum() == 8                           # an isolated pixel: a ring, not itself
    assert R.boundary(np.ones((9, 11), dtype=bool)).sum() == 0                               # a full frame
    m = np.zeros((40, 48), dtype=bool)
    m[10:22, 14:32] = True
    assert R.boundary(m).sum() == 120                                                        # a 12 x 18 rectangle: two pixels thick
    m = np.zeros((9, 11), dtype=bool)
    m[:, :5] = True
    b = R.boundary(m)
    assert b[:, 4:6].all() and b.sum() == 18                                                 # a straight edge is two pixels thick
    m = np.zeros((9, 11), dtype=bool)
    m[:4, :] = True                                                                           # ex is 0 everywhere; at the side columns by reflection
    b = R.boundary(m)
    assert b[3:5, :].all() and b.sum() == 22
    assert R.bound_pix(0.008, 480, 854) == 8.0 and R.bound_pix(0.008, 20, 24) == 1.0 and R.bound_pix(2.5, 37, 53) == 2.5


def test_disk_rim_of_the_shifted_rectangle():
    ann = np.zeros((1, 40, 48), dtype=np.uint8)
    seg = np.zeros_like(ann)
    ann[0, 10:22, 14:32] = 1
    seg[0, 13:25, 18:36] = 1                                  # shifted by (3, 4): distance 5
    assert R.counts_disk(ann, seg, 1, 5)[0, 0, 2:].tolist() == [120, 120, 120, 120]
    c = R.counts_disk(ann, seg, 1, 4.9)[0, 0]
    assert c[2] == c[3] == 120 and c[4] < 120 and c[5] < 120


# ---- davis_statistics -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 68])
def test_statistics_against_the_restatement(T):
    """Both sides add at most T fp64 terms <= 1 per mean, in different orders: each mean is within (T - 1) 2^-53 of exact, so two means
    differ by at most 2 (T - 1) 2^-53 and the decay, a difference of two means, by twice that (+ 2^-53 for T = 1)."""
    import naf_amd
    rng = np.random.default_rng(T)
    v = rng.random((3, T))
    if T >= 5:
        v[1, 2] = np.nan                                      # nanmean skips it, `v > 0.5` counts it as False
    mean, recall, decay = naf_amd.davis_statistics(torch.from_numpy(v))
    assert mean.dtype == recall.dtype == decay.dtype == torch.float64 and mean.shape == (3,)
    tol = 2 * (T - 1) * 2.0 ** -53 + 2.0 ** -53
    for o in range(3):
        M, O, D = R.statistics(v[o])
        assert abs(float(mean[o]) - M) <= tol and abs(float(recall[o]) - O) <= tol and abs(float(decay[o]) - D) <= 2 * tol, (o, T)
    m1, r1, d1 = naf_amd.davis_statistics(torch.from_numpy(v[0]))
    assert m1.dim() == 0 and abs(float(m1) - float(mean[0])) <= tol and abs(float(d1) - float(decay[0])) <= 2 * tol and float(r1) == float(recall[0])
    if T == 68:
        assert R.bin_edges(68) == [0, 17, 34, 50, 67]
        x = torch.arange(68, dtype=torch.float64)
        _, _, d = naf_amd.davis_statistics(x)
        assert float(d) == float(x[0:18].mean() - x[50:68].mean())


def test_statistics_refuses_what_the_reference_gets_wrong():
    import naf_amd
    with pytest.raises(ValueError, match="256"):
        naf_amd.davis_statistics(torch.zeros(2, 257, dtype=torch.float64))
    naf_amd.davis_statistics(torch.zeros(2, 256, dtype=torch.float64))
    with pytest.raises(ValueError, match="T = 0"):
        naf_amd.davis_statistics(torch.zeros(2, 0, dtype=torch.float64))
    with pytest.raises(ValueError, match="floating"):
        naf_amd.davis_statistics(torch.zeros(2, 5, dtype=torch.int64))


# ---- validation -------------------------------------------------------------------------------------------------------------------------
def test_public_names():
    import naf_amd
    from naf_amd import ops
    assert {"davis_jf", "davis_statistics", "DavisJF"} <= set(naf_amd.__all__)
    assert naf_amd.davis_jf is ops.davis_jf and naf_amd.davis_statistics is ops.davis_statistics and naf_amd.DavisJF is ops.DavisJF
    assert naf_amd.DavisJF._fields == ("J", "F", "counts")


def test_validation_raises_value_error_before_any_device(built_lib):
    """Every ValueError that does not depend on the maps' contents is raised on CPU tensors, i.e. before the ROCm check and any device work."""
    import naf_amd
    a = torch.zeros(2, 20, 24, dtype=torch.uint8)
    bad = [
        (dict(annotation=a[0, 0]), r"\[T, H, W\] or \[H, W\]"),
        (dict(annotation=a[None]), r"\[T, H, W\] or \[H, W\]"),
        (dict(annotation=a.float()), "uint8 or torch.int64"),
        (dict(segmentation=a.to(torch.int32)), "uint8 or torch.int64"),
        (dict(segmentation=a[:, :, :23]), "one shape"),
        (dict(segmentation=a[0]), "one shape"),
        (dict(annotation=a.numpy()), "must be a tensor"),
        (dict(num_objects=0), "N"),
        (dict(num_objects=33), "1 <= N <= 32"),
        (dict(num_objects=1 << 40), "1 <= N <= 32"),
        (dict(num_objects=2.0), "int or None"),
        (dict(num_objects=True), "int or None"),
        (dict(bound_th=0.0), r"1 <= floor\(bound_pix\) <= 32"),
        (dict(bound_th=-1.0), "negative"),
        (dict(bound_th=33), r"1 <= floor\(bound_pix\) <= 32"),
        (dict(bound_th=1e30), r"1 <= floor\(bound_pix\) <= 32"),
        (dict(bound_th=float("nan")), "finite"),
        (dict(bound_th="x"), "number"),
        (dict(annotation=a[:, :1], segmentation=a[:, :1]), "H, W >= 2"),
        (dict(annotation=a[:, :, :1], segmentation=a[:, :, :1]), "H, W >= 2"),
        (dict(annotation=a[:0], segmentation=a[:0]), "T"),
        (dict(annotation=torch.zeros(1, 2, 16385, dtype=torch.uint8), segmentation=torch.zeros(1, 2, 16385, dtype=torch.uint8), bound_th=2),
         "H, W <= 16384"),
    ]
    for kw, pat in bad:
        args = dict(annotation=a, segmentation=a, num_objects=2)
        args.update(kw)
        with pytest.raises(ValueError, match=pat):
            naf_amd.davis_jf(**args)
    with pytest.raises(ValueError, match=r"1 <= floor\(bound_pix\) <= 32"):      # the other limits are checked before N is derived
        naf_amd.davis_jf(a, a, bound_th=40)


def test_well_formed_cpu_call_raises_the_rocm_error(built_lib):
    import naf_amd
    a = torch.ones(2, 20, 24, dtype=torch.uint8)
    for kw in (dict(num_objects=2), dict(), dict(num_objects=1, bound_th=2.5)):
        with pytest.raises(RuntimeError, match="ROCm"):
            naf_amd.davis_jf(a, a, **kw)
    with pytest.raises(RuntimeError, match="ROCm"):
        naf_amd.davis_jf(a[0].long(), a[0].long(), num_objects=3)


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------------
def _header_text():
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_ctypes_and_exports_agree(built_lib):
    from naf_amd import _lib
    txt = _header_text()
    lib = C.CDLL(built_lib)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/naf_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert name not in _lib.EXPORTED_AS
    assert _lib.SIGNATURES["naf_davis_jf"][1] == [C.POINTER(_lib.DavisJFArgs), C.c_void_p]
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == _lib.HEADER_VERSION            # detected by symbol: no bump
    for macro, value in (("NAF_DAVIS_TILE_W", _lib.DAVIS_TILE_W), ("NAF_DAVIS_TILE_H", _lib.DAVIS_TILE_H),
                         ("NAF_DAVIS_MAX_OBJECTS", _lib.DAVIS_MAX_OBJECTS), ("NAF_DAVIS_MAX_HALF_WIDTH", _lib.DAVIS_MAX_HALF_WIDTH)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, txt).group(1)) == value


def test_struct_layout_matches_header(built_lib, tmp_path):
    import subprocess
    from naf_amd import _lib
    fields = [f[0] for f in _lib.DavisJFArgs._fields_]
    body = 'printf("%zu\\n", sizeof(naf_davis_jf_args));' + "".join(f'printf("%zu\\n", offsetof(naf_davis_jf_args, {f}));' for f in fields)
    src = '#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n'
    (tmp_path / "p.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "p")]).split()))
    assert vals[0] == C.sizeof(_lib.DavisJFArgs)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_lib.DavisJFArgs, f).offset == off, f


def _args(**kw):
    from naf_amd import _lib
    a = _lib.DavisJFArgs()
    a.T, a.H, a.W, a.N, a.r2, a.half_width = 70, 480, 854, 3, 64, 8
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_select_is_a_host_only_policy(built_lib):
    """naf_davis_jf_select reads the scalar fields only (every pointer here is NULL): 0 served, 2 (NAF_ERR_UNSUPPORTED) outside the served
    range with the limit in naf_last_error, 1 (NAF_ERR_INVALID) for arguments that are not well formed."""
    from naf_amd import _lib
    lib = _lib.load()
    assert lib.naf_davis_jf_select(None) == 1 and lib.naf_davis_jf(None, None) == 1 and "NULL" in _lib.last_error()
    assert lib.naf_davis_jf_select(C.byref(_args())) == 0
    for kw in (dict(N=1), dict(N=32), dict(H=2, W=2), dict(H=16384, W=16384, T=1), dict(T=1), dict(r2=1, half_width=1), dict(r2=3, half_width=1),
               dict(r2=6, half_width=2), dict(r2=80, half_width=8), dict(r2=1024, half_width=32), dict(r2=1088, half_width=32)):
        assert lib.naf_davis_jf_select(C.byref(_args(**kw))) == 0, kw
    for kw, text in ((dict(N=33), "1 <= N <= 32"), (dict(H=1), "H, W >= 2"), (dict(W=1), "H, W >= 2"), (dict(W=16385), "H, W <= 16384"),
                     (dict(r2=0, half_width=0), "1 <= floor(bound_pix) <= 32"), (dict(r2=1089, half_width=33), "1 <= floor(bound_pix) <= 32"),
                     (dict(H=16384, W=16384, T=1 << 15), "2^31")):
        assert lib.naf_davis_jf_select(C.byref(_args(**kw))) == 2, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    for kw, text in ((dict(N=0), "N"), (dict(T=0), "T"), (dict(H=0), "H"), (dict(half_width=-1), "negative"), (dict(r2=-1), "negative"),
                     (dict(r2=63, half_width=8), "belong together"), (dict(r2=81, half_width=8), "belong together")):
        assert lib.naf_davis_jf_select(C.byref(_args(**kw))) == 1, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    a = _args()
    a.reserved[0] = 1
    assert lib.naf_davis_jf_select(C.byref(a)) == 1 and "reserved" in _lib.last_error()
    # a served geometry with NULL pointers: refused by the launch entry before anything touches a device
    assert lib.naf_davis_jf(C.byref(_args()), None) == 1 and "NULL" in _lib.last_error()
