"""CPU tests of feature PCA (``naf_amd.FeaturePCA`` / ``naf_amd.pca``, naf_feature_moments / naf_pca_project / naf_pca_minmax): the fp64
restatement (tests/pca_reference.py) against the results of the reference's own ``pca()`` (tests/golden/P1_pca.npz, written by
tools/make_pca_golden.py); the a-priori cap on the cases the GPU tests run; the C ABI without a device (argument checks, the slab plan, the
workspace cap); the Python API's error paths.  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("naf_feature_moments", "naf_feature_moments_workspace_bytes", "naf_feature_moments_plan", "naf_pca_project",
           "naf_pca_project_workspace_bytes", "naf_pca_minmax")


# ---- 1. the restatement against the reference's own pca() ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return R.load_golden(golden_dir)


def test_golden_fixture_is_small_square_and_made_by_the_input_maker(golden):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "P1_pca.npz")) < 100 * 1024
    maps = golden["maps"]
    assert maps.shape == (2, 32, 12, 12) and maps.dtype == np.float32
    assert np.array_equal(maps, torch.from_numpy(maps).to(torch.bfloat16).float().numpy())           # bf16 numbers
    assert len(golden["seeds"]) == 5 and 0.0 <= float(golden["seed_spread"]) < 1e-5
    made = torch.cat(R.golden_maps(), dim=0).numpy()
    assert float(np.abs(made - maps).max()) <= 2.0 ** -7 * float(np.abs(maps).max())                 # the same construction (at most a bf16 ulp apart)


def test_restatement_matches_the_reference_pca(golden):
    """Components up to sign; the min-max normalised pictures up to the flip y -> 1 - y, within the reference's own spread over its seeds
    plus 1e-6 (the reference computes in fp32)."""
    maps = [torch.from_numpy(golden["maps"][i:i + 1]) for i in range(2)]
    f = R.fit(maps, with_bounds=False)
    V = torch.from_numpy(golden["components"]).double()
    cos = (V * f.components).sum(0) / V.norm(dim=0)
    print(f"|cos| of the three components: {[f'{abs(float(c)):.9f}' for c in cos]}")
    assert all(1.0 - abs(float(c)) <= 1e-6 for c in cos)
    sv = torch.from_numpy(golden["singular_values"]).double()
    assert float(((f.singular_values - sv) / sv).abs().max()) <= 1e-5
    assert float((f.mean - torch.from_numpy(golden["mean"]).double()).abs().max()) <= 1e-5
    budget = float(golden["seed_spread"]) + 1e-6
    for i, m in enumerate(maps):
        got = R.rgb(R.transform(f, m))
        err = R.match_up_to_flip(got, torch.from_numpy(golden["reduced_feats"][i:i + 1]))
        print(f"map {i}: max |rgb - reference| up to the flip {err:.3e} (budget {budget:.3e})")
        assert err <= budget
    idx = f.components.abs().argmax(dim=0)
    assert bool((f.components.gather(0, idx.unsqueeze(0)) > 0).all())                               # the defined signs


# ---- 2. the cap on the cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.PCA_CASES))
def test_a_priori_bound_of_every_case_is_under_the_cap(name):
    f = R.case_fit(name)
    print(f"{name}: E = {f.E:.3e}, gaps {[f'{g:.3f}' for g in f.gaps]}, sin(theta) bounds {[f'{s:.2e}' for s in f.sin_bound]} (cap {R.SIN_CAP})")
    assert all(s <= R.SIN_CAP for s in f.sin_bound)
    assert all(g > 3.0 for g in f.gaps)                                                             # the planted spectrum: 64, 16, 4 over 1/16
    for m in R.case_maps(name):
        assert torch.equal(m, R.bf16r(m))


# ---- 3. the C ABI without a device ------------------------------------------------------------------------------------------------------
def _header_text():
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_ctypes_and_exports_agree(built_lib):
    """Fails on the parent commit: the symbols do not exist there."""
    from naf_amd import _lib
    txt = _header_text()
    lib = C.CDLL(built_lib)
    bound = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/naf_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name) and hasattr(bound, name)
        assert name not in _lib.EXPORTED_AS
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403 == _lib.HEADER_VERSION        # detected by symbol
    full = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert int(re.search(r"#define\s+NAF_MOMENTS_CHAIN\s+(\d+)", full).group(1)) == _lib.MOMENTS_CHAIN == R.CHAIN
    assert int(re.search(r"#define\s+NAF_PCA_MAX_C\s+(\d+)", full).group(1)) == _lib.PCA_MAX_C
    assert int(re.search(r"#define\s+NAF_PCA_MAX_COMPONENTS\s+(\d+)", full).group(1)) == _lib.PCA_MAX_COMPONENTS
    assert re.search(r"#define\s+NAF_MOMENTS_WORKSPACE_CAP\s+\(\(size_t\)256 << 20\)", full) and _lib.MOMENTS_WORKSPACE_CAP == 256 << 20


def test_struct_layouts_match_header(built_lib, tmp_path):
    from naf_amd import _lib
    structs = (("naf_feature_moments_args", _lib.FeatureMomentsArgs), ("naf_pca_project_args", _lib.PcaProjectArgs),
               ("naf_pca_minmax_args", _lib.PcaMinmaxArgs))
    body = ""
    for cname, ct in structs:
        body += f'printf("%zu\\n", sizeof({cname}));' + "".join(f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in ct._fields_)
    src = '#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n'
    (tmp_path / "p.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")])
    vals = iter(map(int, subprocess.check_output([str(tmp_path / "p")]).split()))
    for cname, ct in structs:
        assert next(vals) == C.sizeof(ct), cname
        for f in ct._fields_:
            assert getattr(ct, f[0]).offset == next(vals), (cname, f[0])


def _moments_args(**kw):
    """Well-formed arguments whose pointers are made-up, non-NULL addresses: validation must refuse before anything dereferences them."""
    from naf_amd import _lib
    a = _lib.FeatureMomentsArgs()
    a.x, a.gram, a.sum, a.workspace = 0x1000, 0x2000, 0x3000, 0x4000
    a.P, a.ld, a.C = 1073, 96, 96
    a.workspace_bytes = 1 << 30
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _project_args(**kw):
    from naf_amd import _lib
    a = _lib.PcaProjectArgs()
    a.x, a.V, a.b, a.y, a.minmax, a.workspace = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    a.P, a.ld, a.C, a.n = 1073, 96, 96, 3
    a.workspace_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _minmax_args(**kw):
    from naf_amd import _lib
    a = _lib.PcaMinmaxArgs()
    a.y, a.minmax, a.workspace = 0x1000, 0x2000, 0x3000
    a.P, a.ld, a.n = 1073, 32, 3
    a.workspace_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entries_validate_before_any_device_call(built_lib):
    """NAF_ERR_INVALID (1) / NAF_ERR_UNSUPPORTED (2) with the field or the limit named, on a machine that has no device to call."""
    from naf_amd import _lib
    lib = _lib.load()
    I2 = C.c_int32 * 2
    for fn in (lib.naf_feature_moments, lib.naf_pca_project, lib.naf_pca_minmax):
        assert fn(None, None) == 1 and "NULL" in _lib.last_error()
    bad = [
        (dict(x=None), 1, "x"), (dict(gram=None), 1, "gram"), (dict(sum=None), 1, "sum"), (dict(workspace=None), 1, "workspace"),
        (dict(x=0x1008), 1, "aligned"), (dict(gram=0x2004), 1, "aligned"), (dict(workspace=0x4008), 1, "aligned"),
        (dict(P=0), 1, "P"), (dict(C=0), 1, "C"), (dict(ld=95), 1, "ld"), (dict(ld=100), 1, "ld"), (dict(reserved=1), 1, "reserved"),
        (dict(workspace_bytes=1024), 1, "workspace_bytes"),
        (dict(C=48, ld=48), 2, "C = 48"), (dict(C=4128, ld=4128), 2, "4096"), (dict(C=16, ld=16), 2, "C = 16"), (dict(P=1 << 31), 2, "2^31"),
    ]
    for kw, code, text in bad:
        assert lib.naf_feature_moments(C.byref(_moments_args(**kw)), None) == code, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    bad = [
        (dict(x=None), 1, "x"), (dict(V=None), 1, "V"), (dict(b=None), 1, "b"), (dict(y=None), 1, "y"), (dict(minmax=None), 1, "minmax"),
        (dict(workspace=None), 1, "workspace"), (dict(x=0x1002), 1, "aligned"), (dict(y=0x4002), 1, "aligned"), (dict(workspace=0x6004), 1, "aligned"),
        (dict(P=-3), 1, "P"), (dict(n=0), 1, "n"), (dict(C=-32), 1, "C"), (dict(ld=88), 1, "ld"), (dict(reserved=I2(0, 1)), 1, "reserved"),
        (dict(workspace_bytes=64), 1, "workspace_bytes"),
        (dict(n=9), 2, "n = 9"), (dict(C=48, ld=48), 2, "C = 48"),
    ]
    for kw, code, text in bad:
        assert lib.naf_pca_project(C.byref(_project_args(**kw)), None) == code, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    bad = [
        (dict(y=None), 1, "y"), (dict(minmax=None), 1, "minmax"), (dict(workspace=None), 1, "workspace"), (dict(y=0x1001), 1, "aligned"),
        (dict(workspace=0x3008), 1, "aligned"), (dict(P=0), 1, "P"), (dict(n=0), 1, "n"), (dict(ld=2), 1, "ld"), (dict(reserved=7), 1, "reserved"),
        (dict(workspace_bytes=64), 1, "workspace_bytes"), (dict(n=9), 2, "n = 9"),
    ]
    for kw, code, text in bad:
        assert lib.naf_pca_minmax(C.byref(_minmax_args(**kw)), None) == code, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    # one 64-byte line per workgroup of 16 pixels, at most 1024 workgroups
    assert lib.naf_pca_project_workspace_bytes(C.byref(_project_args())) == -(-1073 // 16) * 64
    assert lib.naf_pca_project_workspace_bytes(C.byref(_project_args(P=1 << 20))) == 1024 * 64
    assert lib.naf_pca_project_workspace_bytes(C.byref(_project_args(P=0))) == 0 and lib.naf_pca_project_workspace_bytes(None) == 0
    assert lib.naf_feature_moments_workspace_bytes(C.byref(_moments_args(C=48))) == 0 and lib.naf_feature_moments_workspace_bytes(None) == 0


def _plan(P, Cc):
    from naf_amd import _lib
    ns, slab = C.c_int32(-1), C.c_int32(-1)
    assert _lib.load().naf_feature_moments_plan(C.byref(_moments_args(P=P, C=Cc, ld=Cc)), C.byref(ns), C.byref(slab)) == 0
    return ns.value, slab.value


def test_moments_plan_and_workspace_cap(built_lib):
    """The decomposition the launch would use, from P and C alone: whole 32-pixel tiles per slab, every pixel covered once, no slab longer
    than the chain the header states; the cases of the GPU tests include several slabs with a partial last one, and fewer pixels than a
    slab; the workspace stays under the stated cap at the sizes of the notebook's largest call."""
    from naf_amd import _lib, ops
    lib = _lib.load()
    partial_last, short = [], []
    for name, shapes in sorted(R.MOMENT_CASES.items()):
        for Cc, H, W in shapes:
            P = H * W
            ns, slab = _plan(P, Cc)
            assert (ns, slab) == ops.feature_moments_plan(P, Cc)
            assert ns >= 1 and slab % 32 == 0 and 32 <= slab <= _lib.MOMENTS_CHAIN
            assert (ns - 1) * slab < P <= ns * slab
            nb = -(-Cc // 128)
            need = ns * (nb * (nb + 1) // 2 * 128 * 128 + nb * 128) * 4
            assert lib.naf_feature_moments_workspace_bytes(C.byref(_moments_args(P=P, C=Cc, ld=Cc))) == need
            if ns >= 2 and P % slab:
                partial_last.append((Cc, H, W))
            if P < slab:
                short.append((Cc, H, W))
            print(f"({Cc}, {H}, {W}): {ns} slabs of {slab} pixels, workspace {need / 2 ** 20:.2f} MiB")
    assert partial_last and short, (partial_last, short)
    assert _plan(65536, 64)[0] >= 2                                                                   # many slabs at the long-chain case
    for Cc, H, W in ((768, 1024, 1024), (4096, 512, 512)):
        ns, slab = _plan(H * W, Cc)
        nbytes = lib.naf_feature_moments_workspace_bytes(C.byref(_moments_args(P=H * W, C=Cc, ld=Cc)))
        print(f"({Cc}, {H}, {W}): {ns} slabs of {slab} pixels, workspace {nbytes / 2 ** 20:.1f} MiB (cap {_lib.MOMENTS_WORKSPACE_CAP >> 20} MiB)")
        assert 0 < nbytes <= _lib.MOMENTS_WORKSPACE_CAP and slab <= _lib.MOMENTS_CHAIN and ns * slab >= H * W
    assert lib.naf_feature_moments_plan(C.byref(_moments_args(C=48, ld=48)), C.byref(C.c_int32()), C.byref(C.c_int32())) == 2
    assert lib.naf_feature_moments_plan(C.byref(_moments_args()), None, None) == 1
    assert lib.naf_feature_moments_plan(None, None, None) == 1


# ---- 4. the Python API's error paths ------------------------------------------------------------------------------------------------------
def test_public_surface_and_error_paths(built_lib):
    """Fails on the parent commit: the names do not exist there."""
    import naf_amd
    from naf_amd import ops
    assert {"FeaturePCA", "pca"} <= set(naf_amd.__all__)
    x = torch.randn(1, 64, 6, 5)
    with pytest.raises(ValueError, match="n_components"):
        naf_amd.FeaturePCA(n_components=0)
    with pytest.raises(ValueError, match="n_components"):
        naf_amd.FeaturePCA(n_components=9)
    with pytest.raises(TypeError, match="int"):
        naf_amd.FeaturePCA(n_components=3.0)
    p = naf_amd.FeaturePCA()
    assert p.n_components == 3 and p.components_ is None
    for call in (lambda t: p.fit(t), lambda t: p.fit([t, t]), lambda t: naf_amd.pca([t]), lambda t: ops.feature_moments(t),
                 lambda t: ops.pca_project(t, torch.zeros(64, 3), torch.zeros(3)), lambda t: ops.pca_minmax(t[:, :3])):
        with pytest.raises(RuntimeError, match="ROCm"):                                               # well formed, but on the CPU: no fallback
            call(x)
    with pytest.raises(RuntimeError, match="ROCm"):
        p.fit(x.bfloat16()[0])
    with pytest.raises(ValueError, match="B = 2"):
        p.fit(torch.randn(2, 64, 6, 5))
    with pytest.raises(ValueError, match="B = 2"):
        naf_amd.pca([torch.randn(2, 64, 6, 5)])
    with pytest.raises(ValueError, match="channels"):
        p.fit([x, torch.randn(1, 96, 6, 5)])                                                          # mismatching C
    with pytest.raises(ValueError, match="C = 48"):
        p.fit(torch.randn(1, 48, 6, 5))
    with pytest.raises(ValueError, match="no maps"):
        p.fit([])
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        p.fit(x.double())
    with pytest.raises(TypeError, match="tensor"):
        p.fit([x.numpy()])
    with pytest.raises(ValueError, match=r"\[C, H, W\]"):
        p.fit(torch.randn(64, 5))
    for call in (p.transform, p.transform_rgb):
        with pytest.raises(RuntimeError, match="fit"):
            call(x)
    with pytest.raises(RuntimeError, match="fit"):
        p.head()
    with pytest.raises(TypeError, match="FeaturePCA"):
        naf_amd.pca([x], fit_pca=object())
    with pytest.raises(TypeError, match="list"):
        naf_amd.pca(x)
    with pytest.raises(ValueError, match="V"):
        ops.pca_project(x, torch.zeros(32, 3), torch.zeros(3))
    with pytest.raises(ValueError, match="V"):
        ops.pca_project(x, torch.zeros(64, 9), torch.zeros(9))
    with pytest.raises(ValueError, match="`b`"):
        ops.pca_project(x, torch.zeros(64, 3), torch.zeros(4))
    with pytest.raises(TypeError, match="float32"):
        ops.pca_project(x, torch.zeros(64, 3, dtype=torch.float64), torch.zeros(3))
    with pytest.raises(TypeError, match="float32"):
        ops.pca_minmax(x.bfloat16())
    with pytest.raises(ValueError, match="n = 64"):
        ops.pca_minmax(x)
    with pytest.raises(ValueError, match=r"\[B, n, H, W\]"):
        naf_amd.FeaturePCA.normalize(torch.zeros(3, 4, 5))
