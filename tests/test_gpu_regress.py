"""GPU tests (-m gpu) of the regression objective in the attention kernel's epilogue: ``ops.xna_mse_forward`` (naf_xna_mse_fwd),
``ops.XnaMSEFunction`` and ``naf(..., regress=t)``.  Loss and gradient are held, per element, to the bounds of tests/regress_reference.py
(derived from the kernel's one bf16 rounding of the softmax weights; no measured constant) on the smallest shapes that reach each
branch of the kernel; every case's plan is asserted through naf_xna_union_plan so that a planner change cannot silently move a case."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regress_reference as R  # noqa: E402
from test_gpu_parity import to5  # noqa: E402
from test_gpu_train_stem import rel  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_REFS = {}


def case_data(case, dev):
    """(q5, k5, v5, target view on the device, reference dict): computed once per case, never modified."""
    if case not in _REFS:
        B, heads, Dv, lr, out, ks, kind = R.CASES[case][:7]
        q, k, v, t = R.make_inputs(case)
        _REFS[case] = (to5(q, heads).to(dev), to5(k, heads).to(dev), to5(v, heads).to(dev), R.target_view(t, kind, dev),
                       R.reference(q, k, v, t, ks, heads))
    return _REFS[case]


def nchw(t5):
    B, n, H, W, D = t5.shape
    return t5.permute(0, 1, 4, 2, 3).reshape(B, n * D, H, W).double().cpu()


@pytest.mark.parametrize("case", list(R.CASES))
def test_loss_and_gradient_within_the_derived_bounds(dev, case):
    from naf_amd import ops
    B, heads, Dv, lr, out, ks, kind, wt, chunks = R.CASES[case]
    q5, k5, v5, t, ref = case_data(case, dev)
    plan = ops.xna_union_plan(q5, k5, v5, ks)
    assert plan is not None and plan["wt"] == wt, plan
    assert (plan["dvt"] == Dv) if chunks == 1 else (plan["dvt"] <= 256 and Dv // plan["dvt"] >= 2), plan
    assert ops.xna_select(q5, k5, v5, ks) == "union" and ops.xna_mse_supported(q5, k5, v5, t, ks)
    assert (t.stride(1) == 1) == kind.startswith("bf16_cl") and tuple(t.shape) == (B, heads * Dv, *out)
    loss, dout5 = ops.xna_mse_forward(q5, k5, v5, t, ks)
    torch.cuda.synchronize()
    assert loss.shape == () and loss.dtype == torch.float32 and dout5.dtype == torch.bfloat16
    assert tuple(dout5.shape) == (B, heads, *out, Dv) and dout5.permute(0, 2, 3, 1, 4).is_contiguous()
    delta = R.output_bound(ref["abs_sum"])
    err = (nchw(dout5) - ref["dout"]).abs()
    bound = R.dout_bound(ref["dout"], delta, ref["N"])
    L = R.chain_length(plan["ry"], plan["seg"], plan["dvt"], R.union_mse_waves(ks, plan["wt"]))
    lb = R.loss_bound(ref["e"], delta, ref["N"], L, ref["loss"])
    print(f"{case}: plan {plan}, L {L}; dout worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}; "
          f"loss {float(loss):.9g} ref {ref['loss']:.9g} |diff| / bound {abs(float(loss) - ref['loss']) / lb:.3f}")
    assert bool(torch.isfinite(nchw(dout5)).all())
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert abs(float(loss) - ref["loss"]) <= lb
    # loss only: the same sum
    loss_only, none = ops.xna_mse_forward(q5, k5, v5, t, ks, grad=False)
    assert none is None and torch.equal(loss_only, loss)


@pytest.mark.parametrize("case", ["b_f4_k5", "d_chunks", "e_k15", "f_k15_w16"])
def test_two_launches_are_bit_equal(dev, case):
    from naf_amd import ops
    q5, k5, v5, t, _ = case_data(case, dev)
    ks = R.CASES[case][5]
    l1, d1 = ops.xna_mse_forward(q5, k5, v5, t, ks)
    l2, d2 = ops.xna_mse_forward(q5, k5, v5, t, ks)
    assert torch.equal(l1, l2) and torch.equal(d1.view(torch.int16), d2.view(torch.int16))


def test_loss_only_launch_writes_nothing(dev):
    """``grad=False`` hands the kernel a NULL gradient pointer, so there is no buffer of the caller's it could write: what can be held is
    that the launch allocates no gradient (the allocator's peak grows by less than a gradient's bytes), that a buffer offered with
    ``out=`` is refused rather than silently ignored, and that a buffer the previous launch wrote -- poisoned and kept alive -- is still
    poisoned afterwards.  That the NULL-pointer path computes the same sum is held for every case by the parametrised test above."""
    from naf_amd import ops
    case = "b_f4_k3"
    q5, k5, v5, t, _ = case_data(case, dev)
    B, heads, Dv, lr, out, ks = R.CASES[case][:6]
    buf = torch.empty((B, *out, heads, Dv), dtype=torch.bfloat16, device=dev).permute(0, 3, 1, 2, 4)
    loss, d = ops.xna_mse_forward(q5, k5, v5, t, ks, out=buf)
    assert d is buf
    poison = torch.full_like(buf.view(torch.int16), 0x7FC1)          # a NaN pattern the kernel never produces
    buf.view(torch.int16).copy_(poison)
    with pytest.raises(ValueError, match="grad=False"):
        ops.xna_mse_forward(q5, k5, v5, t, ks, grad=False, out=buf)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss2, none = ops.xna_mse_forward(q5, k5, v5, t, ks, grad=False)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < buf.numel() * 2      # workspace and loss only: no gradient-sized allocation
    assert none is None and torch.equal(loss2, loss) and torch.equal(buf.view(torch.int16), poison)


def test_function_backward_is_xna_backward_of_the_stored_gradient(dev):
    from naf_amd import ops
    case = "a_train_small"
    q5, k5, v5, t, ref = case_data(case, dev)
    ks = R.CASES[case][5]
    _, dout5 = ops.xna_mse_forward(q5, k5, v5, t, ks)
    grads = {}
    for mul in (1.0, 4.0):
        ins = [x.clone().requires_grad_(True) for x in (q5, k5, v5)]
        loss = ops.XnaMSEFunction.apply(*ins, t, ks, None)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
        (mul * loss).backward()
        grads[mul] = [x.grad for x in ins]
    # dq has no atomics: bit-equal.  dk / dv are added with fp32 atomics whose order is not fixed (include/naf_hip.h; the precedent is
    # test_backward_scales_exactly in tests/test_gpu_input_statistics.py): five identical launches give the spread, and the function's
    # fp32 sums -- rounded once to bf16, the operands' dtype -- may differ from a launch's by twice that spread plus that one rounding
    # (2^-8 |ref|); where the five launches are bit-equal this is torch.equal.  The same for 4x: a power of two commutes with every rounding.
    runs = [ops.xna_backward(q5, k5, v5, dout5, ks) for _ in range(5)]
    dq, dk, dv = runs[0]
    assert all(torch.equal(r[0], dq) for r in runs)
    assert torch.equal(grads[1.0][0], dq) and torch.equal(grads[4.0][0], 4 * dq)
    for i, (name, ref) in enumerate((("dk", dk), ("dv", dv)), start=1):
        spread = max(float((r[i] - ref).abs().max()) for r in runs)
        g1, g4 = grads[1.0][i], grads[4.0][i]
        assert g1.dtype == torch.bfloat16 and g1.shape == ref.shape and float(ref.abs().max()) > 0
        if spread == 0.0:
            assert torch.equal(g1, ref.to(torch.bfloat16)) and torch.equal(g4, (4 * ref).to(torch.bfloat16)), name
        for g, m in ((g1, 1.0), (g4, 4.0)):
            err = (g.float() - m * ref).abs()
            assert bool((err <= m * 2 * spread + 2.0 ** -8 * (m * ref).abs()).all()), (name, m, float(err.max()), spread)
        # a dropped or misplaced factor is far outside: 4x against 1x differs by 3 |ref|
        assert float((g4.float() - ref).abs().max()) > 2 * float(ref.abs().max())
        print(f"{name}: launch-to-launch spread {spread:.3e}, max |ref| {float(ref.abs().max()):.3e}")
    with pytest.raises(ValueError, match="no gradient"):
        ops.XnaMSEFunction.apply(q5, k5, v5, t.clone().requires_grad_(True), ks, None)


def test_refusals_carry_a_message(dev):
    from naf_amd import ops, _lib
    q5, k5, v5, t, _ = case_data("a_train_small", dev)
    v8 = v5[..., :8]                                                      # Dv % 16 != 0: not this kernel's
    t8 = torch.zeros(t.shape[0], 4 * 8, *t.shape[2:], device=dev)
    assert not ops.xna_mse_supported(q5, k5, v8, t8, 3)
    with pytest.raises(_lib.NafHipError):
        ops.xna_mse_forward(q5, k5, v8, t8, 3)


def _step_kernels(fn):
    """Device kernels of ``fn`` in launch order, from the profiler's kernel table."""
    fn()                                # warm-up: code objects, index tables and plans are loaded outside the profiled step
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return [e.name for e in sorted(ev, key=lambda e: e.time_range.start)]


def _between_attention(names):
    fwd = [i for i, n in enumerate(names) if "xna_union_kernel" in n]
    bwd = [i for i, n in enumerate(names) if "xna_rows_bwd_kernel" in n or "xna_bwd2_kernel" in n or "xna_generic_bwd_kernel" in n]
    assert fwd and bwd and fwd[-1] < bwd[0], names
    return names[fwd[-1] + 1:bwd[0]]


def _torch_objective_kernels(names):
    """Kernels of a torch-side objective: the loss, casts / layout copies, elementwise arithmetic.  Fills are not among them: the
    backward's zeroed dk / dv accumulators and autograd's root gradient of one are there on every path."""
    low = [n.lower() for n in names]
    return [n for n in low if ("mse" in n and "xna_mse_finish_kernel" not in n) or "copy" in n or ("elementwise" in n and "fillfunctor" not in n) or "reduce" in n]


def test_whole_model_training_step_and_validation(dev, monkeypatch):
    """NAF() at its default width, image 64^2, features 64 x 16^2, output 32^2, window 9: the reference's training geometry
    (config/base.yaml) at the smallest feature width.  (8^2 -> 16^2 is not a valid call at window 9: NATTEN's rule, window * dilation <=
    extent, which naf_xna_select enforces, wants 9 * 2 <= 16.)"""
    from naf_amd import NAF, ops
    calls = {"n": 0}
    real = ops.xna_mse_forward

    def spy(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops, "xna_mse_forward", spy)
    torch.manual_seed(7)
    naf = NAF().to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(21)
    image = torch.randn(2, 3, 64, 64, generator=g).to(dev)
    feats = torch.randn(2, 64, 16, 16, generator=g).to(dev)
    size = (32, 32)
    naf.image_encoder.rope.cache_train_coords = True      # both arms see the same jittered RoPE coordinates
    with torch.no_grad():
        t = (naf.eval()(image, feats, size).float() + 0.5 * torch.randn(2, 64, 32, 32, generator=g).to(dev)).contiguous()
    naf.train()
    res = {}
    for path in ("auto", "composed"):
        def step():
            naf.zero_grad(set_to_none=True)
            loss = naf(image, feats, size, regress=t, regress_path=path)
            loss.backward()
            res[path] = (loss.detach(), {n: p.grad.detach().clone() for n, p in naf.named_parameters() if p.grad is not None})

        names = _step_kernels(step)
        between = _torch_objective_kernels(_between_attention(names))
        print(path, "attention kernels:", [n[:120] for n in names if "xna_" in n], "torch objective kernels between them:", [n[:80] for n in between])
        if path == "auto":
            assert calls["n"] == 2 and any("xna_mse_finish_kernel" in n for n in names)         # the profiled step and its warm-up
            assert not between, between
        else:
            assert calls["n"] == 2 and between and not any("xna_mse_finish_kernel" in n for n in names)   # the check tells the arms apart
    loss_f, gf = res["auto"]
    loss_c, gc = res["composed"]
    assert loss_f.shape == () and loss_f.dtype == torch.float32
    worst = max((rel(gf[n], gc[n]), n) for n in gc)
    print(f"whole model: loss fused {float(loss_f):.7g} composed {float(loss_c):.7g}; worst parameter gradient {worst[0]:.3e} ({worst[1]})")
    # the tolerances tests/test_gpu_train_stem.py holds two arms of the training step to: 2e-2 on the output, 6e-2 on every gradient
    assert rel(loss_f, loss_c) < 2e-2
    assert set(gf) == set(gc) and len(gc) == 36
    assert worst[0] < 6e-2, worst
    # validation: eval mode under no_grad, the loss-only launch, against the fp64 objective of the kernel's own operands
    naf.eval()
    with torch.no_grad():
        val = naf(image, feats, size, regress=t)
        val_c = naf(image, feats, size, regress=t, regress_path="composed")
        q5, k5, _ = naf.guidance_qk(image, feats.shape[-2:], size)
    assert val.shape == () and val.dtype == torch.float32 and not val.requires_grad
    to_nchw = lambda x5: x5.permute(0, 1, 4, 2, 3).reshape(x5.shape[0], -1, *x5.shape[2:4]).float().cpu()
    qn, kn, vn = to_nchw(q5), to_nchw(k5), feats.to(torch.bfloat16).float().cpu()
    ref = R.reference(qn, kn, vn, t.cpu(), 9, 4)
    v5 = to5(vn, 4).to(dev)
    plan = ops.xna_union_plan(q5, k5, v5, 9)
    L = R.chain_length(plan["ry"], plan["seg"], plan["dvt"], R.union_mse_waves(9, plan["wt"]))
    lb = R.loss_bound(ref["e"], R.output_bound(ref["abs_sum"]), ref["N"], L, ref["loss"])
    print(f"validation: loss {float(val):.7g} composed {float(val_c):.7g} fp64 {ref['loss']:.7g} |diff| / bound {abs(float(val) - ref['loss']) / lb:.3f}")
    assert abs(float(val) - ref["loss"]) <= lb
    assert rel(val, val_c) < 2e-2
    from naf_amd._lib import NafHipError
    with pytest.raises(NafHipError, match="naf_xna_mse_supported"):                  # C / heads = 15: the kernel refuses, "fused" does not fall back
        naf(image, feats[:, :60], size, regress=t[:, :60], regress_path="fused")
