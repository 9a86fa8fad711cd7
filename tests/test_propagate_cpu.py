"""CPU tests of label propagation (``naf_amd.propagate_labels`` / ``pack_frame``): the two forms of the fp64 restatement of the reference
(tests/propagate_reference.py, citing evaluation/eval_video_seg.py:499-561) agree; the condition under which the GPU test may exclude
pixels holds for every GPU case, from the reference alone; the argument validation of the public call; the C ABI without a device.
No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import propagate_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("naf_propagate_select", "naf_propagate_fwd", "naf_propagate_plan", "naf_feature_inv_norm")
CASE_PARAMS = [pytest.param(i, id=R.CASE_IDS[i]) for i in range(len(R.CASES))]
LIMIT_PARAMS = [pytest.param(i, id=R.LIMIT_IDS[i]) for i in range(len(R.LIMIT_CASES))]


# ---- the yardstick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", CASE_PARAMS)
def test_dense_form_equals_windowed_form(ci):
    """The reference as it is written (dense matmul, mask, topk, threshold, normalise, matmul) and the per-pixel windowed form are the same
    function, to 1e-12 in fp64 -- including the duplicate-frame case (exact ties, all kept) and the case whose corner pixels have fewer
    candidates than topk (all kept)."""
    case = R.CASES[ci]
    (target, context, segs), (out, _, kept) = R.reference(ci)
    ref = R.dense(target, context, segs, radius=case[4], topk=case[5])
    assert out.shape == ref.shape == (1, case[6], case[2], case[3])
    err = float((out - ref).abs().max())
    print(f"{R.CASE_IDS[ci]}: max |dense - windowed| = {err:.3e}; kept set sizes {int(kept.min())} .. {int(kept.max())}")
    assert err <= 1e-12
    n, r, topk = case[0], case[4], case[5]
    if n * (r + 1) ** 2 < topk:
        assert int(kept[0, 0]) == n * (r + 1) ** 2 < topk          # a corner: fewer candidates than topk, every one of them kept
    if case[7]:
        assert int(kept.min()) > topk                              # a duplicated frame ties every score: "all ties" keeps more than k


@pytest.mark.parametrize("ci", CASE_PARAMS)
def test_ambiguous_share_of_every_gpu_case_is_within_the_cap(ci):
    """The GPU test skips AMBIGUOUS pixels (a candidate within 0 < |s - threshold| < 4 * C * 2^-24 of the threshold: a kernel whose scores
    carry the contract's error may keep a different set there).  That exclusion is capped at 3 % of a case's pixels, and the cap is a
    property of the inputs: it is asserted here from the fp64 reference alone, on the bf16 features the kernel receives (raw bf16 values,
    normalised in fp64 -- the form the kernel's contract specifies)."""
    _, (_, ambiguous, _) = R.reference(ci)
    share = float(ambiguous.double().mean())
    print(f"{R.CASE_IDS[ci]}: ambiguous share {100 * share:.2f} % ({int(ambiguous.sum())} of {ambiguous.numel()} pixels)")
    assert share <= R.MAX_AMBIGUOUS_SHARE


# ---- the limits of the served range -------------------------------------------------------------------------------------
@pytest.mark.parametrize("li", LIMIT_PARAMS)
def test_limit_case_forms_agree_and_ambiguous_share_is_within_the_cap(li):
    """Every LIMIT_CASES entry: the dense form equals the windowed form to 1e-12, and the ambiguous share is within the same 3 % cap --
    exactly 0 on the lattice cases, whose scores are multiples of 1 / m >= 1 / 1024 (propagate_reference.lattice_features)."""
    case = R.LIMIT_CASES[li]
    n, C_, h, w, r, topk, K, features = case
    (target, context, segs), (out, ambiguous, kept) = R.limit_reference(li)
    ref = R.dense(target, context, segs, radius=r, topk=topk)
    assert out.shape == ref.shape == (1, K, h, w)
    err = float((out - ref).abs().max())
    share = float(ambiguous.double().mean())
    print(f"{R.LIMIT_IDS[li]}: max |dense - windowed| = {err:.3e}; kept set sizes {int(kept.min())} .. {int(kept.max())}; "
          f"ambiguous share {100 * share:.2f} %")
    assert err <= 1e-12
    assert share <= R.MAX_AMBIGUOUS_SHARE
    if n * min(h, r + 1) * min(w, r + 1) < topk:
        assert int(kept[0, 0]) == n * min(h, r + 1) * min(w, r + 1)      # a corner: fewer candidates than topk, every one of them kept
    if features == "lattice":
        assert int(ambiguous.sum()) == 0
        m = R.lattice_m(C_)
        for x in [target, *context]:
            assert x.dtype == torch.bfloat16 and set(x.float().unique().tolist()) <= {-1.0, 0.0, 1.0}
            assert bool((x.float().abs().sum(0) == m).all())                                    # exactly m live channels per pixel
            assert bool((x.float().abs().reshape(C_ // 32, 32, h, w).sum(1) > 0).all())         # every 32-channel chunk of every pixel is live
        s = torch.einsum("chw,nchw->nhw", target.double(), torch.stack(context).double())       # same-position scores times m: integers
        assert bool((s == s.round()).all()) and float(s.abs().max()) <= m <= 1024
    if K == 1:
        assert float(segs.max() - segs.min()) > 0.5                      # not the constant 1 a normalisation over K = 1 would give


def test_lattice_m_is_the_largest_power_of_four():
    assert [R.lattice_m(c) for c in (32, 63, 64, 160, 255, 256, 416, 512, 768, 800, 1023, 1024)] == [16, 16, 64, 64, 64, 256, 256, 256, 256, 256, 256, 1024]
    assert {R.lattice_m(c[1]) for c in R.LIMIT_CASES if c[7] == "lattice"} == {16, 64, 256, 1024}


def _case_args(case):
    from naf_amd import _lib
    a = _lib.PropagateArgs()
    a.n, a.C, a.h, a.w, a.radius, a.topk, a.K = case[:7]
    a.temperature = R.TEMPERATURE
    return a


def test_the_cases_reach_every_kernel_instance_and_both_key_streams(built_lib):
    """Coverage read from the library (naf_propagate_plan, which the launch takes its choices from), not from a copied formula: CASES and
    LIMIT_CASES together launch every propagate_kernel<KSMAX>, the single-buffered key stream at KSMAX 24 and 32 with 2 and with 3 key
    blocks, and the double-buffered one at KSMAX 32.  A change of the LDS budget or of the dispatch that moves a case fails here."""
    from naf_amd import _lib, ops
    lib = _lib.load()
    plans = []
    for case in list(R.CASES) + list(R.LIMIT_CASES):
        out = (C.c_int32 * 4)()
        assert lib.naf_propagate_plan(C.byref(_case_args(case)), out) == 0, (case, _lib.last_error())
        ksmax, nkb, nbuf, lds = (int(v) for v in out)
        n, C_, h, w, r, topk, K = case[:7]
        assert ops.propagate_plan(n, C_, h, w, K, radius=r, topk=topk) == dict(ksmax=ksmax, nkb=nkb, nbuf=nbuf, lds=lds)
        assert C_ // 32 <= ksmax and nkb * 16 >= 16 + 2 * r > (nkb - 1) * 16 and nbuf in (1, 2) and 0 < lds <= 160 * 1024
        print(f"{case}: KSMAX {ksmax}, nkb {nkb}, nbuf {nbuf}, LDS {lds}")
        plans.append((ksmax, nkb, nbuf))
    assert {p[0] for p in plans} == {4, 8, 12, 16, 24, 32}
    assert (24, 3, 1) in plans                                            # single buffer at KSMAX 24
    assert {(32, 2, 1), (32, 3, 1)} <= set(plans)                         # single buffer at KSMAX 32, with 2 and with 3 key blocks
    assert any(p[0] == 32 and p[2] == 2 for p in plans)                   # double buffer at KSMAX 32
    assert {p[1] for p in plans if p[2] == 1} >= {2, 3}


GPU_BOUND_DEFECTS = ("exactly_topk", "drop_last_chunk", "stale_row0")
WIDE_LATTICE = [i for i, c in enumerate(R.LIMIT_CASES) if c[7] == "lattice" and c[1] >= 416]


def _defect_error(li, defect):
    case = R.LIMIT_CASES[li]
    (target, context, segs), (ref, ambiguous, kept) = R.limit_reference(li)
    bad = R.windowed_with_defect(defect, target, context, segs, radius=case[4], topk=case[5])
    err = float((bad - ref).abs().amax(1)[0][~ambiguous].max())
    bound = R.gpu_bound(case[1], int(kept.max()), float(segs.abs().max()))
    print(f"{R.LIMIT_IDS[li]}: {defect} moves the output by {err:.3e}; GPU bound {bound:.3e}; largest kept set {int(kept.max())}")
    return err, bound


@pytest.mark.parametrize("defect", GPU_BOUND_DEFECTS)
@pytest.mark.parametrize("li", [pytest.param(i, id=R.LIMIT_IDS[i]) for i in WIDE_LATTICE])
def test_wide_lattice_cases_tell_a_planted_defect_from_the_reference(li, defect):
    """Sensitivity of the yardstick: a kernel that kept exactly topk instead of all ties, lost the target's last 32-channel fragment, or
    multiplied image row 0 of a frame against the previous frame's keys would miss the GPU test's bound on EVERY lattice case with
    C >= 416 (the instantiations and the single-buffered stream no other case launches)."""
    assert len(WIDE_LATTICE) == 7
    err, bound = _defect_error(li, defect)
    assert err > bound


def test_cases_with_large_kept_sets_tell_a_kept_set_cut_at_the_list_size():
    """Pass 2 keeps every tie, however many: on each limit case whose largest kept set exceeds the 16 list slots, cutting the kept set at
    16 misses the GPU bound.  There are at least three such cases (n = 16, topk = 16 at C = 512, and the all-limits case)."""
    large = [i for i in range(len(R.LIMIT_CASES)) if int(R.limit_reference(i)[1][2].max()) > 16]
    assert {R.LIMIT_CASES[i][:2] for i in large} >= {(16, 32), (2, 512), (3, 1024)}
    for li in large:
        err, bound = _defect_error(li, "cut_at_16")
        assert err > bound


# ---- validation -----------------------------------------------------------------------------------------------------
def _inputs(n=2, C_=64, h=6, w=7, K=3, dtype=torch.bfloat16):
    return torch.randn(C_, h, w).to(dtype), [torch.randn(C_, h, w).to(dtype) for _ in range(n)], torch.rand(n, K, h, w)


def test_public_names():
    import naf_amd
    from naf_amd import ops
    assert {"propagate_labels", "pack_frame", "FrameFeatures"} <= set(naf_amd.__all__)
    assert naf_amd.propagate_labels is ops.propagate_labels and naf_amd.pack_frame is ops.pack_frame and naf_amd.FrameFeatures is ops.FrameFeatures


def test_validation_raises_value_error_before_any_device(built_lib):
    import naf_amd
    t, ctx, sg = _inputs()
    bad = [
        (dict(target=t[0]), r"\[C, h, w\]"),                                           # wrong rank
        (dict(target=t[None, None]), r"\[C, h, w\]"),
        (dict(context=torch.stack(ctx)[0]), r"\[n, C, h, w\]"),                        # a stacked context must be 4-D
        (dict(segs=sg[0]), r"\[n, K, h, w\]"),
        (dict(segs=[sg[0], sg[1][0]]), r"\[K, h, w\]"),
        (dict(target=torch.randn(32, 6, 7).bfloat16()), "context"),                     # mismatched C
        (dict(context=[ctx[0], torch.randn(64, 7, 7).bfloat16()]), "context"),          # mismatched h
        (dict(context=[ctx[0], torch.randn(64, 6, 8).bfloat16()]), "context"),          # mismatched w
        (dict(segs=torch.rand(2, 3, 6, 8)), "label map"),
        (dict(segs=torch.rand(3, 3, 6, 7)), "n = 2"),                                   # mismatched n
        (dict(segs=[sg[0]]), "n = 2"),
        (dict(radius=0), "dense"),
        (dict(radius=16), "radius <= 15"),
        (dict(radius=-1), "radius"),
        (dict(topk=0), "topk"),
        (dict(topk=17), "topk <= 16"),
        (dict(temperature=0.0), "temperature"),
        (dict(target=torch.randn(40, 6, 7).bfloat16(), context=[torch.randn(40, 6, 7).bfloat16()] * 2), "C % 32 == 0"),
        (dict(target=torch.randn(1056, 2, 2).bfloat16(), context=[torch.randn(1056, 2, 2).bfloat16()] * 2, segs=torch.rand(2, 3, 2, 2)), "C <= 1024"),
        (dict(segs=torch.rand(2, 65, 6, 7)), "K <= 64"),
        (dict(context=[ctx[0]] * 17, segs=torch.rand(17, 3, 6, 7)), "n <= 16"),
        (dict(context=[], segs=[]), "n <= 16"),
        (dict(segs=torch.randint(0, 2, (2, 3, 6, 7))), "floating"),
        (dict(target=t.to(torch.float16)), "bfloat16 or float32"),
    ]
    for kw, pat in bad:
        args = dict(target=t, context=ctx, segs=sg)
        args.update(kw)
        with pytest.raises(ValueError, match=pat):
            naf_amd.propagate_labels(**args)
    with pytest.raises(ValueError, match="C % 32 == 0"):
        naf_amd.pack_frame(torch.randn(40, 6, 7))
    with pytest.raises(ValueError, match=r"\[C, h, w\]"):
        naf_amd.pack_frame(torch.randn(2, 64, 6, 7))


def test_well_formed_cpu_call_raises_the_rocm_error(built_lib):
    import naf_amd
    t, ctx, sg = _inputs()
    with pytest.raises(RuntimeError, match="ROCm"):
        naf_amd.propagate_labels(t, ctx, sg, radius=2)
    with pytest.raises(RuntimeError, match="ROCm"):
        naf_amd.propagate_labels(t.float(), torch.stack(ctx).float(), list(sg.unbind(0)))
    with pytest.raises(RuntimeError, match="ROCm"):
        naf_amd.pack_frame(t[None])


# ---- the C ABI without a device ---------------------------------------------------------------------------------------
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
        assert not re.search(r"#define\s+%s\s+NAF_ABI_PASTE" % name, txt)          # these entries read no GroupNorm buffers
        assert name not in _lib.EXPORTED_AS
    assert _lib.SIGNATURES["naf_propagate_fwd"][1] == [C.POINTER(_lib.PropagateArgs), C.c_void_p]
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403 == _lib.HEADER_VERSION     # detected by symbol


def test_struct_layout_matches_header(built_lib, tmp_path):
    import subprocess
    from naf_amd import _lib
    fields = [f[0] for f in _lib.PropagateArgs._fields_]
    body = 'printf("%zu\\n", sizeof(naf_propagate_args));' + "".join(f'printf("%zu\\n", offsetof(naf_propagate_args, {f}));' for f in fields)
    src = '#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n'
    (tmp_path / "p.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "p")]).split()))
    assert vals[0] == C.sizeof(_lib.PropagateArgs)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_lib.PropagateArgs, f).offset == off, f


def _args(**kw):
    from naf_amd import _lib
    a = _lib.PropagateArgs()
    a.n, a.C, a.h, a.w, a.K, a.radius, a.topk, a.temperature = 8, 384, 34, 61, 8, 12, 5, 0.1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_select_is_a_host_only_policy(built_lib):
    """naf_propagate_select reads the scalar fields only (every pointer here is NULL): 0 served, 2 (NAF_ERR_UNSUPPORTED) outside the served
    range with the limit in naf_last_error, 1 (NAF_ERR_INVALID) for arguments that are not well formed."""
    from naf_amd import _lib
    lib = _lib.load()
    assert lib.naf_propagate_fwd(None, None) == 1 and "NULL" in _lib.last_error()
    assert lib.naf_propagate_select(None) == 1
    assert lib.naf_feature_inv_norm(None, None, 4, 4, 64, None) == 1 and "NULL" in _lib.last_error()
    assert lib.naf_propagate_select(C.byref(_args())) == 0
    for kw in (dict(C=32), dict(C=1024), dict(K=1), dict(K=64), dict(topk=1), dict(topk=16), dict(radius=1), dict(radius=15), dict(n=1),
               dict(n=16), dict(h=1, w=1), dict(h=272, w=488)):
        assert lib.naf_propagate_select(C.byref(_args(**kw))) == 0, kw
    for kw, text in ((dict(C=40), "C % 32 == 0"), (dict(C=1056), "C <= 1024"), (dict(C=16), "32 <= C"), (dict(K=65), "K <= 64"),
                     (dict(topk=17), "topk <= 16"), (dict(radius=16), "radius <= 15"), (dict(radius=0), "dense"), (dict(n=17), "n <= 16"),
                     (dict(h=1 << 15, w=1 << 15), "2^31")):
        assert lib.naf_propagate_select(C.byref(_args(**kw))) == 2, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    for kw, text in ((dict(n=0), "n"), (dict(h=0), "h"), (dict(K=0), "K"), (dict(topk=0), "topk"), (dict(radius=-1), "radius"),
                     (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature")):
        assert lib.naf_propagate_select(C.byref(_args(**kw))) == 1, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    a = _args()
    a.reserved[1] = 1
    assert lib.naf_propagate_select(C.byref(a)) == 1 and "reserved" in _lib.last_error()
    # a served geometry with NULL pointers: refused by the launch entry before anything touches a device
    assert lib.naf_propagate_fwd(C.byref(_args()), None) == 1 and "NULL" in _lib.last_error()


def test_plan_is_a_host_only_query_with_selects_status(built_lib):
    """naf_propagate_plan reads the scalar fields only (every pointer here is NULL) and returns what naf_propagate_select returns; on NAF_OK
    it fills {KSMAX, nkb, nbuf, LDS bytes}, otherwise it leaves `out` alone."""
    from naf_amd import _lib, ops
    lib = _lib.load()
    untouched = (C.c_int32 * 4)(-7, -7, -7, -7)
    assert lib.naf_propagate_plan(None, None) == 1 and "NULL" in _lib.last_error()
    assert lib.naf_propagate_plan(None, untouched) == 1 and "NULL" in _lib.last_error()
    assert lib.naf_propagate_plan(C.byref(_args()), None) == 1 and "out is NULL" in _lib.last_error()
    for kw, rc, text in ((dict(C=40), 2, "C % 32 == 0"), (dict(C=1056), 2, "C <= 1024"), (dict(K=65), 2, "K <= 64"), (dict(topk=17), 2, "topk <= 16"),
                         (dict(radius=16), 2, "radius <= 15"), (dict(radius=0), 2, "dense"), (dict(n=17), 2, "n <= 16"),
                         (dict(h=1 << 15, w=1 << 15), 2, "2^31"), (dict(n=0), 1, "n"), (dict(K=0), 1, "K"), (dict(radius=-1), 1, "radius"),
                         (dict(temperature=0.0), 1, "temperature")):
        a = _args(**kw)
        assert lib.naf_propagate_plan(C.byref(a), untouched) == rc == lib.naf_propagate_select(C.byref(a)), kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    a = _args()
    a.reserved[0] = 1
    assert lib.naf_propagate_plan(C.byref(a), untouched) == 1 and "reserved" in _lib.last_error()
    assert list(untouched) == [-7, -7, -7, -7]
    # the benchmarked setting, worked out by hand: 384 / 32 = 12 fragments; 16 + 24 = 40 keys -> 3 blocks; sums 128 * (8 + 1) * 4 = 4608 bytes,
    # per buffer 48 inverse norms (192 bytes) and 48 keys of 2 * 384 + 16 = 784 bytes (37632): two buffers fit, 4608 + 2 * 37824 = 80256
    out = (C.c_int32 * 4)()
    assert lib.naf_propagate_plan(C.byref(_args()), out) == 0 and list(out) == [12, 3, 2, 80256]
    # the largest request of the served range, single-buffered: 128 * 65 * 4 + 192 + 48 * 2064
    assert lib.naf_propagate_plan(C.byref(_args(C=1024, K=64, radius=15, topk=16, n=16)), out) == 0 and list(out) == [32, 3, 1, 132544]
    # every corner of the served range launches (the plan never exceeds the 160 KiB it sizes the buffers for)
    for C_ in (32, 1024):
        for K in (1, 64):
            for r in (1, 15):
                assert lib.naf_propagate_plan(C.byref(_args(C=C_, K=K, radius=r)), out) == 0 and 0 < out[3] <= 160 * 1024
    assert ops.propagate_plan(8, 384, 34, 61, 8, radius=12, topk=5) == dict(ksmax=12, nkb=3, nbuf=2, lds=80256)
    with pytest.raises(ValueError, match="radius <= 15"):
        ops.propagate_plan(8, 384, 34, 61, 8, radius=16)
