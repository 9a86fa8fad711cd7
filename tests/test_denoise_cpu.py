"""CPU tests of the denoising objective (``naf_amd.DenoisingLoss`` / ``denoising_loss`` / ``denoising_metrics``, naf_denoise_objective): the
fp64 restatement (tests/denoise_reference.py) against the results of the reference's own classes (tests/golden/denoise_objective.npz,
written by tools/make_denoise_golden.py); the closed-form gradient the kernel evaluates against fp64 autograd; the public surface and its
argument validation; the C ABI without a device.  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("naf_denoise_objective", "naf_denoise_workspace_bytes")


# ---- 1. the restatement against the reference's own classes ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "denoise_objective.npz"))


def test_golden_inputs_are_the_input_makers(golden):
    pred, target = R.make_inputs(R.GOLDEN_SHAPE, clamped=False)
    assert np.array_equal(golden["pred"], pred.numpy()) and np.array_equal(golden["target"], target.numpy())
    assert float(pred.min()) < 0.0 and float(pred.max()) > 1.0                      # the unclamped variant leaves [0, 1]
    assert bool((target == 0).any()) and bool((target == 1).any()) and bool((pred == target).any())


def test_loss_restatement_matches_the_reference_classes(golden):
    """DenoisingLoss(1, 5, 0.2) of the reference in fp64 with total.backward(): terms and total to 1e-12 relative, gradient to 1e-12 max|g|."""
    pred, target = torch.from_numpy(golden["pred"]), torch.from_numpy(golden["target"])
    terms, _, grad = R.loss_and_grad(pred, target, R.GOLDEN_WEIGHTS, torch.float64)
    for k in ("l1", "l2", "ssim", "total"):
        ref = float(golden[k])
        rel = abs(float(terms[k]) - ref) / abs(ref)
        print(f"{k}: {float(terms[k]):.15g} (reference {ref:.15g}, relative error {rel:.2e})")
        assert rel <= 1e-12
    g = torch.from_numpy(golden["grad"])
    err = float((grad - g).abs().max())
    print(f"gradient: max error {err:.2e}, max|g| {float(g.abs().max()):.3e}")
    assert g.dtype == torch.float64 and err <= 1e-12 * float(g.abs().max())


def test_metrics_restatement_matches_the_reference_classes(golden):
    """MetricsCalculator.calculate_batch_metrics of the reference in fp32 on the clamped prediction, against the fp64 restatement."""
    pred, target = torch.from_numpy(golden["pred"]), torch.from_numpy(golden["target"])
    m, _ = R.metrics(pred, target, clamp=True, dtype=torch.float64)
    print(f"psnr {m['psnr']:.8f} dB (reference {float(golden['psnr']):.8f}); ssim {m['ssim']:.10f} (reference {float(golden['ssim_metric']):.10f})")
    assert abs(m["ssim"] - float(golden["ssim_metric"])) <= 2e-6
    assert abs(m["psnr"] - float(golden["psnr"])) <= 1e-4
    same, _ = R.metrics(pred.clamp(0, 1), target, clamp=False)
    assert same == m                                                                  # clamp=True IS torch.clamp(pred, 0, 1)


# ---- 2. the closed-form gradient ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamped", [False, True], ids=["unclamped", "clamped"])
@pytest.mark.parametrize("ci", [pytest.param(i, id=R.CASE_IDS[i]) for i in range(len(R.CASES))])
def test_analytic_gradient_equals_autograd(ci, clamped):
    pred, target = R.inputs(ci, clamped)
    for wi, w in enumerate(R.WEIGHTS):
        g64 = R.loss_reference(ci, clamped, wi)["grad"]
        err = float((R.analytic_grad(pred, target, w) - g64).abs().max())
        gmax = float(g64.abs().max())
        print(f"{R.CASE_IDS[ci]} weights {w}: max error {err:.2e}, max|g| {gmax:.3e}")
        assert err <= 1e-12 * gmax


def test_case_inputs_have_the_properties_the_gpu_tests_rely_on():
    for ci, shape in enumerate(R.CASES):
        for clamped in (False, True):
            pred, target = R.inputs(ci, clamped)
            assert tuple(pred.shape) == tuple(target.shape) == shape and pred.dtype == target.dtype == torch.float32
            assert bool((pred == target).any())
            assert float(target.min()) >= 0.0 and float(target.max()) <= 1.0
            if clamped:
                assert float(pred.min()) >= 0.0 and float(pred.max()) <= 1.0
        if shape[2] * shape[3] >= 64:
            pred, target = R.inputs(ci, False)
            assert bool((target == 0).any()) and bool((target == 1).any()) and float(pred.min()) < 0.0 and float(pred.max()) > 1.0


# ---- 3. the public surface ------------------------------------------------------------------------------------------------------
def test_public_surface_and_validation(built_lib):
    """Fails on the parent commit: the three names do not exist there."""
    import naf_amd
    from naf_amd import ops
    assert {"DenoisingLoss", "denoising_loss", "denoising_metrics"} <= set(naf_amd.__all__)
    assert naf_amd.DenoisingLoss is ops.DenoisingLoss and naf_amd.denoising_loss is ops.denoising_loss
    assert naf_amd.denoising_metrics is ops.denoising_metrics
    crit = naf_amd.DenoisingLoss()
    assert isinstance(crit, torch.nn.Module) and (crit.l1_weight, crit.l2_weight, crit.ssim_weight) == (1.0, 1.0, 0.1)
    crit = naf_amd.DenoisingLoss(l1_weight=1.0, l2_weight=5.0, ssim_weight=0.2)
    assert (crit.l1_weight, crit.l2_weight, crit.ssim_weight) == (1.0, 5.0, 0.2) and not list(crit.parameters())

    p, t = torch.rand(2, 3, 8, 9), torch.rand(2, 3, 8, 9)
    calls = (lambda a, b: crit(a, b), lambda a, b: naf_amd.denoising_loss(a, b, 1.0, 1.0, 0.1), lambda a, b: naf_amd.denoising_metrics(a, b),
             lambda a, b: naf_amd.denoising_metrics(a, b, clamp=True))
    for call in calls:
        with pytest.raises(RuntimeError, match="ROCm"):                               # well formed, but on the CPU: no fallback
            call(p, t)
        with pytest.raises(RuntimeError, match="ROCm"):
            call(p.bfloat16(), t)
        with pytest.raises(ValueError, match="one shape"):
            call(p, t[:, :, :, :8])
        with pytest.raises(ValueError, match="one shape"):
            call(p[0], t[0])
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            call(p, (t * 255).to(torch.uint8))
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            call(p.long(), t)
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            call(p.double(), t.double())
        with pytest.raises(TypeError, match="tensor"):
            call(p, t.numpy())
        with pytest.raises(ValueError, match="requires grad"):
            call(p, t.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="negative"):
        naf_amd.denoising_loss(p, t, 1.0, -1.0, 0.1)
    with pytest.raises(ValueError, match="negative"):
        naf_amd.DenoisingLoss(ssim_weight=float("nan"))(p, t)
    with pytest.raises(RuntimeError, match="ROCm"):                                   # all weights 0 is still a device call's contract
        naf_amd.denoising_loss(p, t, 0.0, 0.0, 0.0)


def test_key_presence_follows_the_weights(monkeypatch):
    """The dict's keys, what carries a gradient, and backward's scaling -- with the launch replaced by a stand-in that fills the entry's
    result vector and gradient map, so that this runs without a device (the launch itself is the GPU tests')."""
    import naf_amd
    from naf_amd import ops
    monkeypatch.setattr(ops, "_gpu", lambda t, name: None)
    seen = []

    def fake(pred, target, weights=(1.0, 1.0, 0.1), *, grad=False, metrics=False, clamp=False):
        seen.append((tuple(weights), grad, metrics, clamp))
        out = torch.arange(8, dtype=torch.float32) + 1.0
        return out, (torch.full_like(pred, 0.5) if grad else None)

    monkeypatch.setattr(ops, "denoise_objective", fake)
    p, t = torch.rand(1, 3, 4, 5), torch.rand(1, 3, 4, 5)
    for w, keys in (((1.0, 1.0, 0.1), {"l1", "l2", "ssim", "total"}), ((1.0, 5.0, 0.0), {"l1", "l2", "total"}),
                    ((0.0, 0.0, 1.0), {"ssim", "total"}), ((1.0, 0.0, 0.0), {"l1", "total"}), ((0.0, 0.0, 0.0), {"total"})):
        out = naf_amd.DenoisingLoss(*w)(p, t)
        assert set(out) == keys, w
        assert all(v.dim() == 0 and v.dtype == torch.float32 and not v.requires_grad for v in out.values())
    assert float(out["total"]) == 0.0 and len(seen) == 4                              # all weights 0: a zero tensor, nothing launched
    assert not any(s[1] for s in seen)                                                # pred does not require grad: no gradient map asked for
    out = naf_amd.DenoisingLoss(1.0, 5.0, 0.2)(p, t)
    assert (float(out["l1"]), float(out["l2"]), float(out["ssim"]), float(out["total"])) == (4.0, 5.0, 6.0, 7.0)

    q = p.clone().requires_grad_(True)
    out = naf_amd.DenoisingLoss(1.0, 5.0, 0.2)(q, t)
    assert seen[-1] == ((1.0, 5.0, 0.2), True, False, False)
    assert out["total"].requires_grad and not (out["l1"].requires_grad or out["l2"].requires_grad or out["ssim"].requires_grad)
    (out["total"] * 3.0).backward()
    assert torch.equal(q.grad, torch.full_like(p, 1.5))
    with torch.no_grad():
        assert not naf_amd.DenoisingLoss()(q, t)["total"].requires_grad and seen[-1][1] is False
    m = naf_amd.denoising_metrics(p, t, clamp=True)
    assert set(m) == {"psnr", "ssim"} and seen[-1][2:] == (True, True) and (float(m["psnr"]), float(m["ssim"])) == (1.0, 2.0)


# ---- 4. the C ABI without a device ------------------------------------------------------------------------------------------------
def _header_text():
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_ctypes_and_exports_agree(built_lib):
    from naf_amd import _lib
    txt = _header_text()
    lib = C.CDLL(built_lib)
    bound = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/naf_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name) and hasattr(bound, name)
        assert name not in _lib.EXPORTED_AS
    assert _lib.SIGNATURES["naf_denoise_objective"] == (C.c_int, [C.POINTER(_lib.DenoiseArgs), C.c_void_p])
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403 == _lib.HEADER_VERSION     # detected by symbol


def test_struct_layout_matches_header(built_lib, tmp_path):
    from naf_amd import _lib
    fields = [f[0] for f in _lib.DenoiseArgs._fields_]
    body = 'printf("%zu\\n", sizeof(naf_denoise_args));' + "".join(f'printf("%zu\\n", offsetof(naf_denoise_args, {f}));' for f in fields)
    src = '#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n'
    (tmp_path / "d.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "d.c"), "-o", str(tmp_path / "d")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "d")]).split()))
    assert vals[0] == C.sizeof(_lib.DenoiseArgs)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_lib.DenoiseArgs, f).offset == off, f


def _args(**kw):
    """Well-formed arguments whose pointers are made-up, non-NULL addresses: validation must refuse before anything dereferences them."""
    from naf_amd import _lib
    a = _lib.DenoiseArgs()
    a.pred, a.target, a.out, a.workspace = 0x1000, 0x2000, 0x3000, 0x4000
    a.B, a.C, a.H, a.W = 2, 3, 37, 45
    a.pred_dtype, a.target_dtype, a.grad_dtype, a.mode = _lib.NAF_F32, _lib.NAF_BF16, _lib.NAF_F32, _lib.DENOISE_LOSS
    a.l1_weight, a.l2_weight, a.ssim_weight = 1.0, 5.0, 0.2
    a.workspace_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entry_validates_before_any_device_call(built_lib):
    """NAF_ERR_INVALID (1) with the field named, on a machine that has no device to call."""
    from naf_amd import _lib
    lib = _lib.load()
    assert lib.naf_denoise_objective(None, None) == 1 and "NULL" in _lib.last_error()
    bad = [
        (dict(pred=None), "pred"), (dict(target=None), "target"), (dict(out=None), "out"), (dict(workspace=None), "workspace"),
        (dict(C=0), "C"), (dict(B=0), "B"), (dict(H=-1), "H"), (dict(W=0), "W"),
        (dict(pred_dtype=7), "pred_dtype"), (dict(target_dtype=-1), "target_dtype"), (dict(grad=0x5000, grad_dtype=2), "grad_dtype"),
        (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
        (dict(l1_weight=-1.0), "l1_weight"), (dict(ssim_weight=-0.5), "ssim_weight"), (dict(l2_weight=float("nan")), "l2_weight"),
        (dict(workspace_bytes=16), "workspace_bytes"), (dict(workspace=0x4004), "aligned"), (dict(reserved=1), "reserved"),
        (dict(mode=1, grad=0x5000), "grad"),
    ]
    for kw, text in bad:
        assert lib.naf_denoise_objective(C.byref(_args(**kw)), None) == 1, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    assert lib.naf_denoise_objective(C.byref(_args(B=1 << 15, C=1 << 15)), None) == 2 and "2^24" in _lib.last_error()
    # one 16-byte line per 32 x 32 tile of every plane
    assert lib.naf_denoise_workspace_bytes(C.byref(_args())) == 2 * 3 * 2 * 2 * 16
    assert lib.naf_denoise_workspace_bytes(C.byref(_args(H=64, W=64))) == 2 * 3 * 2 * 2 * 16
    assert lib.naf_denoise_workspace_bytes(C.byref(_args(H=65, W=1))) == 2 * 3 * 3 * 16
    assert lib.naf_denoise_workspace_bytes(C.byref(_args(C=0))) == 0 and lib.naf_denoise_workspace_bytes(None) == 0
