"""Every window instance of the attention kernels once (-m gpu), at the smallest shape that selects it.

The windowed kernels are compiled one object per (family, window[, value type]) from naf_amd/build.py's INSTANCES table and the
dispatchers pick one with a switch built from the same window list.  A missing or mis-wired instance shows here: each case asserts through
the library's own ``*_select`` / ``*_supported`` entry that the intended family serves it, runs it and holds the result to the reference
and tolerance the family's existing tests use.  No new tolerance:

  cell / sliding / table-driven, bf16 values:  the library's scalar table-driven kernel (path="generic", fp32 throughout), under the fuzz
      tests' bound of tests/test_gpu_parity.py (test_xna_mfma_fuzz_geometries / test_xna_union_fuzz_geometries):
      |a - b|max <= tol (1 + |b|max), tol 6e-3 for fp32 output, 1.2e-2 for bf16 output.
  float16 values:  the fp64 oracle and tests/half_reference.py's per-element half_bound (tests/test_gpu_half_features.py).
  xna_mse_forward:  tests/regress_reference.py's per-element bounds (tests/test_gpu_regress.py).
  head:  the head sum of the generic kernel's fp32 attention on the projected values, under tests/test_gpu_head.py's assert_head_close (its
      "fused vs composed" check); the classification epilogue and the confusion matrix against the launch's own logits and labels, as
      tests/test_gpu_head_objective.py (A) and tests/test_gpu_head_confusion.py (A) hold them.
  cell backward, plain and with a score gradient:  the generic backward under test_xna_backward_fuzz_geometries' bound (tests/test_gpu_parity.py):
      |a - b|max <= 2.5e-2 |b|max + 1e-3.

Shapes: B = 1, two heads, Dq = 64, Dv = 32 per head, a 15 x 15 grid (the smallest every window 3 .. 15 accepts); ratio 2 for the cell kernel,
ratio 16 for the sliding kernel, the head and the backward; 16 x 16 -> 40 x 40 (ratio 2.5) for the table-driven kernel and its objective.

Half windows no common shape reaches: the sliding kernel at 7 x 7 and 9 x 9.  With 16-bit output and a Dv tile of 32 the cell plan stages its
stores there (xna_mfma_plan), so those calls run the cell kernel; a 48-channel head reaches them (tests/test_gpu_half_features.py, "sliding").
test_forward_instances_run_the_kernel_they_name reads which kernel ran from the profiler instead of guessing.
"""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_reference as H  # noqa: E402
import input_statistics as S  # noqa: E402
import regress_reference as R  # noqa: E402
from test_gpu_half_features import kernels_run, v5_half  # noqa: E402
from test_gpu_head import assert_head_close, make_pv  # noqa: E402
from test_gpu_head_objective import make_target, valid_of  # noqa: E402
from test_gpu_parity import bf16r, to5  # noqa: E402

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
WINDOWS = (3, 5, 7, 9, 11, 13, 15)
SLIDE_WINDOWS = (7, 9, 11, 13, 15)
SLIDE_HALF_WINDOWS = (11, 13, 15)           # 7, 9: staged cell plan at Dv = 32 (module docstring)
HEADS, DQ, DV = 2, 64, 32
C = HEADS * DV
GRID, CELL_OUT, SLIDE_OUT = (15, 15), (30, 30), (240, 240)
UNION_GRID, UNION_OUT = (16, 16), (40, 40)
N_CLASSES = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_DATA = {}


def operands(dev, lr, out_sz, half=False):
    """(q5, k5, v5) on the device plus their fp32 NCHW forms (q, k, v): seeded, computed once per geometry, never modified."""
    key = (lr, out_sz, half)
    if key not in _DATA:
        seed = 7000 + out_sz[1]
        q, k = S.make_qk((1, HEADS * DQ, *out_sz), (1, HEADS * DQ, *lr), "unit", seed, HEADS)
        v = H.make_half_values((1, C, *lr), "unit", seed + 2) if half else S.make_values((1, C, *lr), "unit", seed + 2)
        v5 = v5_half(v, HEADS, dev) if half else to5(v, HEADS).to(dev)
        _DATA[key] = (to5(q, HEADS).to(dev), to5(k, HEADS).to(dev), v5, q, k, v)
    return _DATA[key]


_GENERIC = {}


def generic_forward(dev, lr, out_sz, ksz):
    """The scalar table-driven kernel's fp32 output for the bf16 operands of a geometry: the reference of the bf16 cases."""
    from naf_amd import ops
    key = (lr, out_sz, ksz)
    if key not in _GENERIC:
        q5, k5, v5 = operands(dev, lr, out_sz)[:3]
        assert ops.xna_select(q5, k5, v5, ksz, out_dtype=F32, path="generic") == "generic"
        _GENERIC[key] = ops.xna_forward(q5, k5, v5, ksz, out_dtype=F32, path="generic")
    return _GENERIC[key]


def check_against_generic(dev, lr, out_sz, ksz, path, out_dtype):
    from naf_amd import ops
    q5, k5, v5 = operands(dev, lr, out_sz)[:3]
    assert ops.xna_select(q5, k5, v5, ksz, out_dtype=out_dtype, path=path) == path
    a = ops.xna_forward(q5, k5, v5, ksz, out_dtype=out_dtype, path=path)
    b = generic_forward(dev, lr, out_sz, ksz)
    assert a.dtype == out_dtype and bool(torch.isfinite(a).all())
    tol = 6e-3 if out_dtype == F32 else 1.2e-2
    err = float((a.float() - b).abs().max())
    print(f"{path} k={ksz} {out_dtype}: max err {err:.3e}, bound {tol + tol * float(b.abs().max()):.3e}")
    assert err <= tol + tol * float(b.abs().max()), (path, ksz, out_dtype, err)


_HALF_REF = {}


def check_half(dev, lr, out_sz, ksz, path):
    """float16 values: every element inside half_reference.half_bound of the fp64 oracle (evaluated on the device: same oracle code)."""
    from naf_amd import ops
    q5, k5, v5, q, k, v = operands(dev, lr, out_sz, half=True)
    case = (f"{path}-k{ksz}", path, None, HEADS, DQ, lr, out_sz, ksz, C, None)
    key = (lr, out_sz, ksz)
    if key not in _HALF_REF:
        qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
        ref, a = S.attention_reference(qd, kd, vd, ksz, HEADS)
        _HALF_REF[key] = (ref, H.half_bound(case, qd, kd, vd, ref, a))
    ref, bound = _HALF_REF[key]
    assert ops.xna_select(q5, k5, v5, ksz, out_dtype=F16, path=path) == path
    out = ops.xna_forward(q5, k5, v5, ksz, out_dtype=F16, path=path)
    assert out.dtype == F16 and bool(torch.isfinite(out).all())
    B, n, Ho, Wo, D = out.shape
    err = (out.permute(0, 1, 4, 2, 3).reshape(B, n * D, Ho, Wo).double() - ref).abs()
    print(f"{path} k={ksz} float16: worst err / bound {S.worst_of_bound(err, bound):.3f}")
    S.check(err, bound, f"half {path} k={ksz}")


# ---- forward: cell, sliding, table-driven ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksz", WINDOWS)
def test_cell_kernel_bf16(dev, ksz):
    check_against_generic(dev, GRID, CELL_OUT, ksz, "mfma", BF16)


@pytest.mark.parametrize("ksz", WINDOWS)
def test_cell_kernel_half(dev, ksz):
    check_half(dev, GRID, CELL_OUT, ksz, "mfma")


@pytest.mark.parametrize("ksz", SLIDE_WINDOWS)
def test_sliding_kernel_fp32(dev, ksz):
    assert S.sliding_runs(ksz, GRID, SLIDE_OUT, F32) is True
    check_against_generic(dev, GRID, SLIDE_OUT, ksz, "mfma", F32)


@pytest.mark.parametrize("ksz", SLIDE_HALF_WINDOWS)
def test_sliding_kernel_half(dev, ksz):
    assert S.sliding_runs(ksz, GRID, SLIDE_OUT, F16) is True
    check_half(dev, GRID, SLIDE_OUT, ksz, "mfma")


def test_forward_instances_run_the_kernel_they_name(dev):
    """path="mfma" covers the cell and the sliding kernel: which one ran, at which window and value type, is read from the kernel names of one
    profiled pass over the cases above (xna_*_kernel<KS, DVT, OutT, ...>: mangled "ILi7ELi32EDF16_", demangled "<7, 32, _Float16,").  The half
    calls at 7 x 7 and 9 x 9 on the sliding geometry are in the pass too: they must run the cell kernel (the staged plan), which is why no
    sliding case holds them."""
    from naf_amd import ops
    runs = [("xna_mfma_kernel", k, CELL_OUT, od) for od in (BF16, F16) for k in WINDOWS]
    runs += [("xna_slide_kernel", k, SLIDE_OUT, F32) for k in SLIDE_WINDOWS] + [("xna_slide_kernel", k, SLIDE_OUT, F16) for k in SLIDE_HALF_WINDOWS]
    runs += [("xna_mfma_kernel", k, SLIDE_OUT, F16) for k in (7, 9)]

    def launch_all():
        for _, ksz, out_sz, od in runs:
            q5, k5, v5 = operands(dev, GRID, out_sz, od == F16)[:3]
            ops.xna_forward(q5, k5, v5, ksz, out_dtype=od, path="mfma")

    _, names = kernels_run(launch_all)
    attn = sorted(n for n in names if re.search(r"xna_[a-z]+_kernel", n))

    def ran(kernel, ksz, od):
        # OutT: mangled DF16b / DF16_ / f; the tracer's demangler prints float and _Float16 and garbles __bf16 ("bool _Accum")
        for n in attn:
            m_ = re.search(rf"{kernel}(?:ILi{ksz}ELi\d+E(DF16b|DF16_|f)|<{ksz}, \d+, ([^,]+),)", n)
            if m_ is not None:
                t_ = m_.group(1) or m_.group(2)
                if od == (F16 if t_ in ("DF16_", "_Float16") else F32 if t_ in ("f", "float") else BF16):
                    return True
        return False

    for kernel, ksz, out_sz, od in runs:
        assert ran(kernel, ksz, od), (kernel, ksz, out_sz, od, attn)
    assert not ran("xna_slide_kernel", 7, F16) and not ran("xna_slide_kernel", 9, F16), attn


@pytest.mark.parametrize("ksz", WINDOWS)
def test_table_driven_kernel_bf16(dev, ksz):
    from naf_amd import ops
    assert ops.xna_union_plan(*operands(dev, UNION_GRID, UNION_OUT)[:3], ksz) is not None
    check_against_generic(dev, UNION_GRID, UNION_OUT, ksz, "union", BF16)


@pytest.mark.parametrize("ksz", WINDOWS)
def test_table_driven_kernel_half(dev, ksz):
    check_half(dev, UNION_GRID, UNION_OUT, ksz, "union")


# ---- the regression objective in the table-driven kernel's epilogue ----------------------------------------------------------------
@pytest.mark.parametrize("ksz", WINDOWS)
def test_mse_objective(dev, ksz):
    """Loss and gradient as tests/test_gpu_regress.py::test_loss_and_gradient_within_the_derived_bounds holds them."""
    from naf_amd import ops
    q5, k5, v5, q, k, v = operands(dev, UNION_GRID, UNION_OUT)
    t = bf16r(O.hash_normal((1, C, *UNION_OUT), 7300 + ksz))
    td = t.to(dev)
    plan = ops.xna_union_plan(q5, k5, v5, ksz)
    assert plan is not None and ops.xna_select(q5, k5, v5, ksz) == "union" and ops.xna_mse_supported(q5, k5, v5, td, ksz)
    ref = R.reference(q, k, v, t, ksz, HEADS)
    loss, dout5 = ops.xna_mse_forward(q5, k5, v5, td, ksz)
    torch.cuda.synchronize()
    assert loss.shape == () and dout5.dtype == BF16 and tuple(dout5.shape) == (1, HEADS, *UNION_OUT, DV)
    got = dout5.permute(0, 1, 4, 2, 3).reshape(1, C, *UNION_OUT).double().cpu()
    delta = R.output_bound(ref["abs_sum"])
    err = (got - ref["dout"]).abs()
    bound = R.dout_bound(ref["dout"], delta, ref["N"])
    L = R.chain_length(plan["ry"], plan["seg"], plan["dvt"], R.union_mse_waves(ksz, plan["wt"]))
    lb = R.loss_bound(ref["e"], delta, ref["N"], L, ref["loss"])
    print(f"mse k={ksz}: plan {plan}; dout worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}; "
          f"loss |diff| / bound {abs(float(loss) - ref['loss']) / lb:.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert abs(float(loss) - ref["loss"]) <= lb


# ---- the head kernel: logits, classification objective, confusion matrix --------------------------------------------------------------
@pytest.mark.parametrize("ksz", WINDOWS)
def test_head_kernel(dev, ksz):
    from naf_amd import ops
    q5, k5 = operands(dev, GRID, SLIDE_OUT)[:2]
    pv, _ = make_pv(1, HEADS, *GRID, N_CLASSES, 7400 + ksz)
    pv5 = pv.to(dev).to(BF16)
    bias = O.hash_normal((N_CLASSES,), 7500 + ksz).to(dev)
    assert ops.xna_head_select(q5, GRID, N_CLASSES, ksz, out_dtype=F32) == "fused"
    L = ops.xna_head_forward(q5, k5, pv5, bias, ksz, n_out=N_CLASSES, out_dtype=F32, path="fused")
    assert L.dtype == F32 and tuple(L.shape) == (1, N_CLASSES, *SLIDE_OUT) and bool(torch.isfinite(L).all())
    # reference: the generic kernel's attention on the projected values (and on their magnitudes), summed over the heads
    assert ops.xna_select(q5, k5, pv5, ksz, out_dtype=F32, path="generic") == "generic"
    per_head = ops.xna_forward(q5, k5, pv5, ksz, out_dtype=F32, path="generic")
    abs_head = ops.xna_forward(q5, k5, pv5.abs(), ksz, out_dtype=F32, path="generic")
    ref = per_head.sum(1)[..., :N_CLASSES].permute(0, 3, 1, 2) + bias.view(1, -1, 1, 1)
    abs_sum = abs_head.sum(1)[..., :N_CLASSES].permute(0, 3, 1, 2)
    assert_head_close(L, ref, abs_sum, HEADS, F32, f"head k={ksz} vs generic")
    # classification epilogue and confusion matrix: against the launch's own logits and labels
    t = make_target(1, *SLIDE_OUT, N_CLASSES, 255).to(dev)
    cm = torch.zeros(N_CLASSES, N_CLASSES, dtype=torch.int64, device=dev)
    kw = dict(n_out=N_CLASSES, ignore_index=255, path="fused", target=t, want_loss=True, want_labels=True, want_dlogits=True, return_logits=True)
    ce = ops.xna_head_objective(q5, k5, pv5, bias, ksz, **kw)
    loss, labels, g, L2 = ops.xna_head_objective(q5, k5, pv5, bias, ksz, confusion=cm, **kw)
    for name, a, b in zip(("loss", "labels", "dlogits", "logits"), (loss, labels, g, L2), ce):
        assert torch.equal(a, b), f"{name}: the confusion-matrix launch differs from the classification launch"
    assert torch.equal(L2, L) and torch.equal(labels.long(), L.argmax(1))
    valid = valid_of(t, 255, N_CLASSES)
    L64 = L.double()
    lse = torch.logsumexp(L64, dim=1)
    tc = torch.where(valid, t, torch.zeros_like(t))
    Lt = L64.gather(1, tc.unsqueeze(1))[:, 0]
    assert not bool(((loss.double() - (lse - Lt)).abs() > 1e-5 * (1.0 + lse.abs() + Lt.abs()))[valid].any())
    assert float(loss[~valid].abs().sum()) == 0.0
    ref_g = ((torch.softmax(L64, dim=1) - F.one_hot(tc, N_CLASSES).permute(0, 3, 1, 2).double()) * valid.unsqueeze(1)).permute(0, 2, 3, 1)
    assert not bool(((g[..., :N_CLASSES].double() - ref_g).abs() > 2.0 ** -8 * ref_g.abs() + 1e-5).any())
    assert torch.equal(cm, ops.head_confusion_from_labels(labels, t, 255, N_CLASSES)) and int(cm.sum()) == int(valid.sum())


# ---- the cell backward, plain and with a gradient of the scores --------------------------------------------------------------------
_BWD_REF = {}


@pytest.mark.parametrize("scores", [False, True], ids=["plain", "scores"])
@pytest.mark.parametrize("ksz", WINDOWS)
def test_cell_backward(dev, ksz, scores):
    from naf_amd import ops
    q5, k5, v5 = operands(dev, GRID, SLIDE_OUT)[:3]
    g5 = to5(S.make_values((1, C, *SLIDE_OUT), "unit", 7600), HEADS).to(dev)
    G = (O.hash_normal((1, HEADS, *SLIDE_OUT, ksz * ksz), 7700 + ksz) * 0.1).to(dev) if scores else None
    assert ops.xna_backward_select(q5, k5, v5, ksz, dlogits=G) == "mfma"
    a = ops.xna_backward(q5, k5, v5, g5, ksz, dlogits=G)
    if (ksz, scores) not in _BWD_REF:
        _BWD_REF[(ksz, scores)] = ops.xna_backward(q5, k5, v5, g5, ksz, path="generic", dlogits=G)
    for x, y, name in zip(a, _BWD_REF[(ksz, scores)], ("dq", "dk", "dv")):
        scale = float(y.float().abs().max())
        err = float((x.float() - y.float()).abs().max())
        print(f"bwd k={ksz} scores={scores} {name}: max err {err:.3e}, bound {2.5e-2 * scale + 1e-3:.3e}")
        assert bool(torch.isfinite(x.float()).all()) and err <= 2.5e-2 * scale + 1e-3, (name, ksz, scores, err, scale)
