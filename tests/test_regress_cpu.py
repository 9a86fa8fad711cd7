"""Host-side tests of the regression objective (``naf(..., regress=t)``): the fp64 restatement against autograd, the bounds of
tests/regress_reference.py against an emulation of the kernel's arithmetic and against four planted defects, the new C-ABI symbols, and
the argument errors of the Python entry points (raised on CPU tensors, before the device check where the order allows)."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import regress_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_CASES = ["a_train_small", "b_f4_k5", "c_ratio1"]


@pytest.fixture(scope="module")
def refs():
    """case -> (inputs, reference dict): computed once, never modified."""
    out = {}
    for case in CPU_CASES:
        q, k, v, t = R.make_inputs(case)
        heads, ks = R.CASES[case][1], R.CASES[case][5]
        out[case] = ((q, k, v, t, ks, heads), R.reference(q, k, v, t, ks, heads))
    return out


def worst(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


def inside(case_inputs, ref, L, **defect):
    """(dout inside its bound everywhere, loss inside its bound) for the emulated kernel with ``defect``."""
    q, k, v, t, ks, heads = case_inputs
    loss, dout = R.emulate_kernel(q, k, v, t, ks, heads, **defect)
    delta = R.output_bound(ref["abs_sum"])
    d_ok = worst((dout - ref["dout"]).abs(), R.dout_bound(ref["dout"], delta, ref["N"])) <= 1.0
    l_ok = abs(loss - ref["loss"]) <= R.loss_bound(ref["e"], delta, ref["N"], L, ref["loss"])
    return d_ok, l_ok


def test_restatement_equals_autograd(refs):
    for case, (_, ref) in refs.items():
        t = refs[case][0][3].double()
        out = ref["out"].clone().requires_grad_(True)
        loss = F.mse_loss(out, t)
        loss.backward()
        assert abs(float(loss.detach()) - ref["loss"]) <= 1e-14 * ref["loss"], case
        assert torch.allclose(out.grad, ref["dout"], rtol=1e-13, atol=0.0), case


def test_chain_length_is_the_codes():
    # 16 rows x 32 pixels per workgroup, 12 waves, 16 channels: 32 tiles -> 3 per wave, 1 channel tile, 4 fmaf each
    assert R.chain_length(16, 32, 16, 12) == 3 * 4 + 9
    assert R.chain_length(8, 16, 64, 12) == 1 * 4 * 4 + 9
    assert [R.union_mse_waves(k, 16) for k in (3, 9, 13, 15)] == [12, 12, 12, 8] and [R.union_mse_waves(k, 32) for k in (3, 11, 13, 15)] == [8, 8, 4, 4]
    src = open(os.path.join(ROOT, "naf_amd", "csrc", "xna_union_mse_kernel.h")).read()
    assert "return wt == 16 ? (ks >= 15 ? 8 : 12) : (ks >= 13 ? 4 : 8);" in src


@pytest.mark.parametrize("case", CPU_CASES)
def test_emulated_kernel_is_inside_the_bounds(refs, case):
    inputs, ref = refs[case]
    # the shortest chain any plan can give (one tile per lane, one channel tile): the tightest loss bound
    assert inside(inputs, ref, R.chain_length(1, 16, 16, 12)) == (True, True)


@pytest.mark.parametrize("defect", ["drop_last_pixel", "n_without_batch", "transpose_target"])
def test_planted_defects_leave_the_bounds(refs, defect):
    # b: a 14-pixel partial tile ends every row, B = 2; c: a square output for the transposed read.  The LONGEST chain a plan could give
    # (one workgroup of 4 waves owning 64 rows x 512 pixels at 256 channels): the loosest loss bound
    case = {"drop_last_pixel": "b_f4_k5", "n_without_batch": "b_f4_k5", "transpose_target": "c_ratio1"}[defect]
    inputs, ref = refs[case]
    d_ok, l_ok = inside(inputs, ref, R.chain_length(64, 512, 256, 4), **{defect: True})
    assert not d_ok and not l_ok, (defect, d_ok, l_ok)


def test_rounded_prediction_leaves_the_bounds_of_the_exact_case(refs):
    """The fourth defect -- the prediction rounded to bf16 before the subtraction, i.e. what the composed step computes.  On general
    inputs it CANNOT leave the n = 1 bounds (regress_reference, "The exact case": 2^-9 |out| + 2^-9 abs_sum < 1.25 * 2^-8 abs_sum), which
    the first assertion records; where the softmax weights are powers of two the kernel's accumulator carries fp32 error only, the bound
    follows (n = 0), the emulation is inside it and the defect is outside."""
    inputs, ref = refs["c_ratio1"]
    assert inside(inputs, ref, R.chain_length(1, 16, 16, 12), round_prediction=True)[0]
    q, k, v, t, ks, heads = R.exact_case()
    ref = R.reference(q, k, v, t, ks, heads)
    delta = R.output_bound(ref["abs_sum"], n=0, fp32_terms=ks * ks)
    L = R.chain_length(1, 16, 16, 12)
    res = {}
    for name, kw in (("kernel", {}), ("rounded", {"round_prediction": True})):
        loss, dout = R.emulate_kernel(q, k, v, t, ks, heads, **kw)
        # the store term of the dout bound would hide it again: hold the implied output, (N / 2) dout before its one rounding
        acc = S.attention_emulated(q, k, v, ks, heads).float()
        if kw:
            acc = acc.to(torch.bfloat16).float()
        res[name] = (worst((acc.double() - ref["out"]).abs(), delta) <= 1.0,
                     abs(loss - ref["loss"]) <= R.loss_bound(ref["e"], delta, ref["N"], L, ref["loss"]))
    assert res["kernel"] == (True, True) and res["rounded"] == (False, False), res


def test_new_symbols_are_exported_and_declared():
    from naf_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    for name in ("naf_xna_mse_supported", "naf_xna_mse_workspace_bytes", "naf_xna_mse_fwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\b(int|size_t)\s+%s\(const naf_xna_mse_args\*" % name, header), name
    assert re.search(r"typedef struct naf_xna_mse_args \{\s*naf_xna_args a;", header)
    assert "#define NAF_HIP_VERSION 403" in header and lib.naf_version() == 403      # detected by symbol: the version does not move
    import ctypes as C
    assert C.sizeof(_lib.XnaMSEArgs) == C.sizeof(_lib.XnaArgs) + 4 * 8 + 8 + 4 * 8
    # a host-side refusal, with a message: NULL tensors
    m = _lib.XnaMSEArgs()
    assert lib.naf_xna_mse_supported(C.byref(m)) == -1 and "NULL" in _lib.last_error()
    assert lib.naf_xna_mse_workspace_bytes(C.byref(m)) == 0


def _operands(B=1, heads=2, Dv=16, lr=(4, 4), out=(8, 8)):
    q = torch.zeros(B, heads, *out, 64, dtype=torch.bfloat16)
    k = torch.zeros(B, heads, *lr, 64, dtype=torch.bfloat16)
    v = torch.zeros(B, heads, *lr, Dv, dtype=torch.bfloat16)
    t = torch.zeros(B, heads * Dv, *out)
    return q, k, v, t


def test_ops_argument_errors_on_cpu_tensors():
    from naf_amd import ops
    q, k, v, t = _operands()
    with pytest.raises(TypeError, match="bfloat16"):
        ops.xna_mse_forward(q.float(), k, v, t, 3)
    with pytest.raises(ValueError, match="target shape"):
        ops.xna_mse_forward(q, k, v, t[:, :-1], 3)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ops.xna_mse_forward(q, k, v, t.double(), 3)
    with pytest.raises(ValueError, match="no gradient"):
        ops.xna_mse_forward(q, k, v, t.clone().requires_grad_(True), 3)
    with pytest.raises(ValueError, match="do not match"):
        ops.xna_mse_forward(q, k[:, :1], v, t, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # everything else in order: the device check
        ops.xna_mse_forward(q, k, v, t, 3)


def test_model_argument_errors_on_cpu_tensors():
    from naf_amd import NAF
    naf = NAF(kernel_size=3).eval()
    image, feats = torch.zeros(1, 3, 16, 16), torch.zeros(1, 32, 4, 4)
    t = torch.zeros(1, 32, 8, 8)
    probe = torch.nn.Conv2d(32, 5, 1)
    for kw in ({"head": probe}, {"target": torch.zeros(1, 8, 8, dtype=torch.long)}, {"predict": True}, {"confusion": True}, {"return_weights": True}):
        with pytest.raises(ValueError, match="does not combine"):
            naf(image, feats, (8, 8), regress=t, **kw)
    with pytest.raises(ValueError, match="regress_path"):
        naf(image, feats, (8, 8), regress=t, regress_path="quick")
    with pytest.raises(ValueError, match="target shape"):
        naf(image, feats, (8, 8), regress=t[:, :, :4])
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        naf(image, feats, (8, 8), regress=t.long())
    with pytest.raises(TypeError, match="must be a tensor"):
        naf(image, feats, (8, 8), regress=[1.0])
    with pytest.raises(ValueError, match="no gradient"):
        naf(image, feats, (8, 8), regress=t.clone().requires_grad_(True))
    for path in ("auto", "fused", "composed"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):    # the call no longer ignores the keyword and returns a map
            naf(image, feats, (8, 8), regress=t, regress_path=path)
