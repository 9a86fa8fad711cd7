"""GPU parity tests (-m gpu) on realistic input statistics with scale-aware, per-element bounds.

The rest of the GPU suite varies shapes, windows, kernel paths and layouts on i.i.d. unit-variance data and asserts absolute constants
sized for it.  Here the VALUES vary -- per-channel means, outlier tokens, magnitudes from 2^-10 to 2^10, smooth fields, peaked / flat /
offset scores, images that look like images (tests/input_statistics.py) -- and every element is held to a bound derived from the kernels'
rounding points, which scales with the inputs:

    |err| <= 1.25 * (n * 2^-8 * abs_sum  +  2^-8 * |ref| per bf16 store of the result)

``abs_sum`` is the contraction with absolute values (sum_j P_j |v_j| for the forward; sum_j |dS_ij||k_j|, sum_i |dS_ij||q_i|, sum_i P_ij
|dout_i| for dq, dk, dv), in fp64 from the oracle; ``n`` is the number of bf16 roundings a weight of that contraction passes through.
The quarter on top covers the fp32 accumulation order and the hardware exp2 / rcp.  tests/test_input_statistics_cpu.py shows on the host
that the reference with those roundings stays inside each bound and that two planted defects leave it.

n per kernel path, read from the sources:
  forward, out = sum_j P_j v_j                                                                                         n   stores
    cell      xna_mfma_kernel.h:625-629   s *= 1 / sum, then pf = (bf16_t) s: the normalised weight, once               1   fp32 0 / bf16 1 (:125-128)
    sliding   xna_slide_kernel.h:341-345  the same two statements                                                        1   fp32 0 / bf16 1
    union     xna_union_kernel.h:281      pf = (bf16_t)(s * inv)                                                         1   fp32 0 / bf16 1 (:310-311)
    rows      xna_rows.hip:131-133        pa = (bf16_t) e with e = weight * exp2(s - running max): rounded BEFORE the     1   fp32 0 / bf16 1 (:166)
              division by the fp32 sum of the unrounded e (:135, :158); the running-max rescale (:151) is fp32
    generic   xna_generic.hip             fp32 throughout: fp32_score_factor(q, k, window) * abs_sum instead of n * 2^-8 0   fp32 0 / bf16 1 (:102)
    rotate-on-load (cell, xna_mfma_kernel.h:255-256): the rotated query is rounded to bf16 exactly as naf_rope_pool_fwd rounds it
              (bit-equal, asserted); the reference is fed those queries, so n stays 1
  head, logit = bias + sum_g sum_j P_g,j PV_g,j
    fused     xna_head_kernel.h:287       pf = (bf16_t)(s * inv) per head; heads and bias add in fp32                     1   fp32 0 / bf16 1
  backward (include/naf_hip.h, naf_xna_bwd; P and dS are the only bf16 intermediates, dP and delta stay fp32)
    cell      xna_bwd2_kernel.h:410/:463  pkv = (bf16_t) P^T           -> dv = P^T dout                                   1   fp32 (atomics)
              xna_bwd2_kernel.h:451       dsf = (bf16_t)(scale P (dP - delta)) -> dq = dS k, dk = dS^T q                  1   dq: bf16 1 (:519-520); dk fp32
    chunked   the same kernel once per channel chunk (naf_xna_bwd_chunk_plan): each launch rounds ITS dS_c = scale P (dP_c - delta_c), so the
              abs-sums are sum_c |dS_c| (>= |dS|), and dq is read back, added to and stored as bf16 once per chunk (:506-520): the store term
              is 2^-8 * sum_c |running dq after chunk c|
    rows      xna_rows_bwd.hip:424 pa = (bf16_t) P, :426 dsa = (bf16_t)(scale P (dP - delta)); delta from pass 1 in fp32 (:369)   1   dq: bf16 1 (:484)
    generic   xna_generic.hip             fp32 throughout: input_statistics.backward_bounds("generic")                  0   dq: bf16 1 (:244)
    every path: dP (a Dv-term sum) and delta = sum_j P_j dP_j are fp32 numbers and dS is scale P times their DIFFERENCE (xna_bwd2_kernel.h:396 /
              :451, xna_rows_bwd.hip:369 / :426).  Where the softmax is peaked delta -> dP of the dominant key and the exact dS of that key is
              far below 2^-24 |dP|: no bound relative to |dS| holds for fp32 arithmetic.  dq and dk therefore carry, on top of the bf16 term,
              (Dv + kk + 8) * 2^-24 * (u_dq, u_dk) -- the abs-sums with |dP - delta| replaced by |dout|.|v| + sum_j P_j |dout|.|v|
              (input_statistics.cancellation_factor: the Dv-term sum dP, the kk-term sum delta, nothing else).  Measured before the term
              existed, peaked family: worst |err| / (1.25 * 2^-8 * (abs_sum + stored)) of dq = 4e3 .. 1e15 on the bf16 paths, at absolute
              errors of 2e-7 .. 5e-5; the fp32 scalar kernel shows the same.  The share of the term each kernel uses is in the profile
  stem
    conv0     include/naf_hip.h (naf_stem_conv0_fwd): 2^-15 * sum|x||w| for the 3x3 layer of the default width (stem_conv0.hip:267-268), fp32 for
              the 1x1 layer and the general widths (stem_generic.hip:103); one bf16 store (stem_conv0.hip:118, :416; stem_generic.hip:110)
    layer     a = SiLU(GN(x)) is rounded to bf16 once before the matrix cores (stem_generic.hip:195-196 and the hand-scheduled kernels alike):
              n = 1 against sum |w||a|, one bf16 store
    whole     tests/test_gpu_parity.py::test_stem_whole_matches_oracle's mean <= 8e-3 / max <= 1.5e-1 (GroupNorm makes the output O(1) at any image
              scale); the hot pixel: plus 1e-2 of the mean / max |ref|
  whole model: 2e-2 + 1e-2 * sum_j P_j |v_j| elementwise (the bf16 emulation holds it: tests/test_input_statistics_cpu.py)

Exact identities (no oracle, no tolerance): a power-of-two factor on the values, on the output gradient, on projected values and bias,
on the features commutes with every rounding, so the results must scale bit for bit.  Two identical launches are compared first; the
backward adds dk / dv with fp32 atomics (naf_hip.h: "the kernel adds every cell's window sums (fp32 atomics)"), whose order is not
fixed -- where identical launches differ (five are compared), the scaled launch may differ from the unscaled one by twice the largest
difference seen between them, no more.

Measured worst err / abs_sum per path and family: profiles/input_statistics.txt (NAF_INPUT_STATS_PROFILE=<file> appends the lines).
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
from input_statistics import BWD_CASES, FWD_CASES, backward_inputs, forward_bound, forward_inputs, sliding_runs  # noqa: E402
from test_gpu_parity import _load_model, to5  # noqa: E402
from test_gpu_head_objective import make_target, valid_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def record(path, family, ratio, derived, of_bound):
    line = S.profile_line(path, family, ratio, derived, of_bound)
    print(line)
    dest = os.environ.get("NAF_INPUT_STATS_PROFILE")
    if dest:
        with open(dest, "a") as f:
            f.write(line + "\n")


def nchw(t5):
    """[B, heads, H, W, D] device tensor -> fp64 [B, heads * D, H, W] on the host."""
    B, n, H, W, D = t5.shape
    return t5.permute(0, 1, 4, 2, 3).reshape(B, n * D, H, W).double().cpu()


def v5_of(v, heads, dev):
    B, C, h, w = v.shape
    return v.to(dev).to(torch.bfloat16).permute(0, 2, 3, 1).contiguous().view(B, h, w, heads, C // heads).permute(0, 3, 1, 2, 4)


# ---- forward -------------------------------------------------------------------------------------------------------------------
def test_forward_cases_cover_every_path_and_window():
    assert {c[1] for c in FWD_CASES} == {"mfma", "union", "rows", "generic"} and {c[2] for c in FWD_CASES} >= {"cell", "sliding"}
    for kernel in ("cell", "sliding", "union", "rows", "generic"):
        mine = [c for c in FWD_CASES if (c[2] or c[1]) == kernel]
        assert {3, 7, 9, 15} <= {c[7] for c in mine} | ({3} if kernel == "sliding" else set()), kernel      # the sliding kernel starts at 7 x 7
        assert any(c[9] is S.FORWARD_FAMILIES for c in mine), kernel
    assert any(c[6][0] % c[5][0] or c[6][1] % c[5][1] for c in FWD_CASES)                                  # a non-integer ratio
    assert len(S.FORWARD_FAMILIES) == 9


def kernels_run(fn):
    """Names of the device kernels ``fn`` launches, from the profiler's device activity."""
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}


_CHECKED = set()


def run_forward(dev, case, q, k, v, out_dtype):
    """The case's launch, as fp64 NCHW on the host.  The path is forced and asserted; for the two kernels behind path="mfma" the first launch
    of a (case, output type) runs under the profiler and the kernel that RAN must be the one the case is named after (xna_slide_kernel /
    xna_mfma_kernel), which must also be what the dispatch condition of xna_mfma.hip:94 (input_statistics.sliding_runs) says."""
    from naf_amd import ops
    name, path, sub, heads, Dq, lr, out_sz, ksz, C, _ = case
    q5, k5, v5 = to5(q, heads).to(dev), to5(k, heads).to(dev), v5_of(v, heads, dev)
    assert ops.xna_select(q5, k5, v5, ksz, out_dtype=out_dtype, path=path) == path
    launch = lambda: ops.xna_forward(q5, k5, v5, ksz, out_dtype=out_dtype, path=path)
    if sub is not None and (name, out_dtype) not in _CHECKED:
        _CHECKED.add((name, out_dtype))
        assert sliding_runs(ksz, lr, out_sz, out_dtype) == (sub == "sliding"), "the case does not select the kernel it is named after"
        names = kernels_run(launch)
        ran = {"sliding" if "xna_slide_kernel" in n else "cell" for n in names if "xna_slide_kernel" in n or "xna_mfma_kernel" in n}
        assert ran == {sub}, f"{name} {out_dtype}: kernels {sorted(names)}"
    return nchw(launch())


def skip_dtype(case, out_dtype):
    """bf16 output of a 7 x 7 / 9 x 9 window may take the staged cell plan: those sliding cases are fp32 by construction; from 11 x 11 up
    there is no staged plan and the sliding kernel's bf16 stores are held too."""
    return case[2] == "sliding" and out_dtype == torch.bfloat16 and sliding_runs(case[7], case[5], case[6], out_dtype) is None


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c[0])
def test_forward_per_element_bound(dev, case):
    """Every forward path on every family: |out - ref| <= the path's bound of the module docstring, all elements; fp32 and bf16 output."""
    name, path, sub = case[0], case[1], case[2]
    failures = []
    for fam in case[9]:
        q, k, v = forward_inputs(case, fam)
        ref, a = S.attention_reference(q, k, v, case[7], case[3])
        for out_dtype in (torch.float32, torch.bfloat16):
            if skip_dtype(case, out_dtype):
                continue
            out = run_forward(dev, case, q, k, v, out_dtype)
            assert bool(torch.isfinite(out).all())
            bound, derived = forward_bound(case, q, k, ref, a, out_dtype)
            err = (out - ref).abs()
            if out_dtype == torch.float32:
                record(f"forward {name} fp32", fam, S.worst_ratio(err, a), derived, S.worst_of_bound(err, bound))
            try:
                S.check(err, bound, f"forward {name} {fam} {out_dtype}")
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_forward_rotate_on_load(dev):
    """The cell kernel rotating the queries as it loads them, on peaked scores and outlier values: bit-equal to materialised queries, and
    inside the n = 1 bound against the oracle fed the SAME bf16 queries and keys (read back from naf_rope_pool_fwd)."""
    from naf_amd import ops
    heads, Dq, lr, out_sz, ksz, C = 4, 64, (8, 8), (16, 128), 7, 256
    x = S.bf16r(O.hash_normal((1, heads * Dq, *out_sz), 310) * 4.0)
    v = S.make_values((1, C, *lr), "outlier", 311)
    per = O.rope_periods(heads * Dq, heads, 100.0)
    xd = x.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ty, tx = ops.rope_tables(per.to(dev), *out_sz)
    q_mat, k5 = ops.rope_pool(xd, ty, tx, heads, lr)
    q_raw = xd.permute(0, 2, 3, 1).unflatten(3, (heads, Dq)).permute(0, 3, 1, 2, 4)
    v5 = v5_of(v, heads, dev)
    assert ops.xna_rope_fusable(q_raw, lr, C // heads, ksz, (ty, tx), out_dtype=torch.float32)
    a_ = ops.xna_forward(q_mat, k5, v5, ksz, out_dtype=torch.float32, path="mfma")
    b_ = ops.xna_forward(q_raw, k5, v5, ksz, out_dtype=torch.float32, path="mfma", rope_tables=(ty, tx))
    assert torch.equal(a_, b_)
    ref, a = S.attention_reference(nchw(q_mat).float(), nchw(k5).float(), v, ksz, heads)
    err = (nchw(b_) - ref).abs()
    record("forward cell rotate-on-load fp32", ("outlier", "peaked"), S.worst_ratio(err, a), S.U, S.worst_of_bound(err, S.bf16_bound(1, a)))
    S.check(err, S.bf16_bound(1, a), "rotate-on-load")


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c[0])
def test_forward_scales_exactly_with_the_values(dev, case):
    """out(q, k, 2^m v) == 2^m out(q, k, v), bit for bit, m = +-10, after two identical launches have been found bit-equal."""
    q, k, v = forward_inputs(case, ("chan_offset", "unit"))
    for out_dtype in (torch.float32, torch.bfloat16):
        if skip_dtype(case, out_dtype):
            continue
        base = run_forward(dev, case, q, k, v, out_dtype)
        assert torch.equal(base, run_forward(dev, case, q, k, v, out_dtype)), "two identical launches differ"
        for m in (-10, 10):
            got = run_forward(dev, case, q, k, v * 2.0 ** m, out_dtype)
            assert torch.equal(got, base * 2.0 ** m), f"{case[0]} {out_dtype}: values x 2^{m} do not scale the output exactly"


# ---- backward ------------------------------------------------------------------------------------------------------------------
def run_backward(dev, case, q, k, v, g):
    """(dq, dk, dv) fp64 NCHW on the host, and the channel-chunk plan; asserts that the case runs the kernel it is named after."""
    from naf_amd import ops
    _, path, heads, Dq, lr, out_sz, ksz, C, nchunk, _ = case
    q5, k5, v5, g5 = (to5(t, heads).to(dev) for t in (q, k, v, g))
    chunks = None
    if path == "generic":
        dq, dk, dv = ops.xna_backward(q5, k5, v5, g5, ksz, path="generic")
    else:
        assert ops.xna_backward_select(q5, k5, v5, ksz) == path, "AUTO does not pick the kernel the case is named after"
        if path == "mfma":
            chunks = [int(c) for c in ops.xna_backward_chunks(q5, k5, v5, ksz)]
            assert len(chunks) == nchunk and sum(chunks) == C // heads, chunks
        dq, dk, dv = ops.xna_backward(q5, k5, v5, g5, ksz, path=path)
    return (nchw(dq), nchw(dk), nchw(dv)), chunks


def test_backward_cases_cover_every_path():
    ids = {c[0] for c in BWD_CASES}
    assert {"cell", "cell-partial-tiles", "cell-chunked-k13", "rows-ratio1", "generic"} <= ids
    assert any(c[8] > 1 and c[6] in (13, 15) for c in BWD_CASES) and any(c[5][1] // c[4][1] == 14 for c in BWD_CASES)
    assert len(S.BACKWARD_FAMILIES) >= 6 and any(f[2] == "peaked" for f in S.BACKWARD_FAMILIES) and any(f[2] == "key_offset" for f in S.BACKWARD_FAMILIES)


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c[0])
def test_backward_per_element_bounds(dev, case):
    """dq, dk and dv of every backward path on every family, all elements, against the explicit fp64 backward (which
    tests/test_input_statistics_cpu.py holds to O.xna_backward) under input_statistics.backward_bounds: the bf16 terms of the module
    docstring plus the fp32 term of dS = scale P (dP - delta), a difference of fp32 numbers (xna_bwd2_kernel.h:396 / :451,
    xna_rows_bwd.hip:369 / :426) that no bound relative to |dS| covers where the softmax is peaked."""
    name, path, heads, Dq, lr, out_sz, ksz, C = case[:8]
    failures = []
    for fam in case[9]:
        q, k, v, g = backward_inputs(case, fam)
        (dq, dk, dv), chunks = run_backward(dev, case, q, k, v, g)
        r = S.backward_reference(q, k, v, g, ksz, heads, chunks=chunks)
        bounds = S.backward_bounds(r, q, k, heads, ksz, path)
        for n_, got in (("dq", dq), ("dk", dk), ("dv", dv)):
            assert bool(torch.isfinite(got).all()), (name, fam, n_)
            err = (got - r[n_]).abs()
            # dq: what is left of the error after one store rounding per chunk, against the abs-sum
            pure = (err - S.U * r["dq_store"]).clamp_min(0.0) if n_ == "dq" else err
            record(f"backward {name} {n_}", fam, S.worst_ratio(pure, r["a_" + n_]), S.U if path != "generic" else 0.0, S.worst_of_bound(err, bounds[n_]))
            if n_ != "dv":
                # how much of the fp32 (cancellation) term the kernel uses: what the error exceeds the rest of the bound by, against that term
                f32 = bounds["fp32_" + n_]
                record(f"backward {name} {n_} fp32 term", fam, S.worst_ratio((err - (bounds[n_] - f32)).clamp_min(0.0), r["u_" + n_]),
                       S.cancellation_factor(r["chunk"], ksz * ksz), S.worst_of_bound((err - (bounds[n_] - f32)).clamp_min(0.0), f32))
            try:
                S.check(err, bounds[n_], f"backward {name} {n_} {fam}")
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c[0])
def test_backward_scales_exactly(dev, case):
    """dout -> 2^m dout scales dq, dk and dv; v -> 2^m v scales dq and dk and leaves dv unchanged; m = +-10.  dq is written once per query:
    bit-equal.  dk / dv are sums of fp32 atomics over the cells that share a key (module docstring): where two identical launches are
    bit-equal in five launches the identity is asserted bit for bit, otherwise within twice the largest difference seen between them."""
    q, k, v, g = backward_inputs(case, ("chan_offset", "unit", "unit"))
    (dq0, dk0, dv0), _ = run_backward(dev, case, q, k, v, g)
    slack = {"dk": 0.0, "dv": 0.0}
    for _ in range(4):
        (dq1, dk1, dv1), _ = run_backward(dev, case, q, k, v, g)
        assert torch.equal(dq0, dq1), "dq of two identical launches differs"
        slack["dk"], slack["dv"] = max(slack["dk"], float((dk0 - dk1).abs().max())), max(slack["dv"], float((dv0 - dv1).abs().max()))
    print(f"backward {case[0]}: identical launches differ by at most dk {slack['dk']:.3e} (max |dk| {float(dk0.abs().max()):.3e}), dv {slack['dv']:.3e} "
          f"(max |dv| {float(dv0.abs().max()):.3e})")
    # the run-to-run difference is an fp32 reordering, nothing more: far below one bf16 rounding of the largest element
    assert slack["dk"] <= 2.0 ** -13 * float(dk0.abs().max()) and slack["dv"] <= 2.0 ** -13 * float(dv0.abs().max())
    slack = {n: 2.0 * d for n, d in slack.items()}       # the largest of four samples of a maximum, doubled: the scaled launches draw from the same distribution

    def same(name, got, want):
        d = float((got - want).abs().max())
        assert d <= slack[name], f"{case[0]}: {name} off by {d:.3e} (identical launches: {slack[name] / 2:.3e})"

    for m in (-10, 10):
        f = 2.0 ** m
        (dq, dk, dv), _ = run_backward(dev, case, q, k, v, g * f)
        assert torch.equal(dq, dq0 * f), f"dout x 2^{m}: dq"
        same("dk", dk / f, dk0)
        same("dv", dv / f, dv0)
        (dq, dk, dv), _ = run_backward(dev, case, q, k, v * f, g)
        assert torch.equal(dq, dq0 * f), f"v x 2^{m}: dq"
        same("dk", dk / f, dk0)
        same("dv", dv, dv0)


# ---- head ----------------------------------------------------------------------------------------------------------------------
def head_device_inputs(name, dev):
    q, k, pv, pvn, bias = S.make_head_inputs(name)
    heads = S.HEAD_GEOM[6]
    return (q, k, pv, pvn, bias), (to5(q, heads).to(dev), to5(k, heads).to(dev), pv.to(dev).to(torch.bfloat16), bias.to(dev))


@pytest.mark.parametrize("name", ["offset", "outlier", "logits50"])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_head_forward_per_element_bound(dev, name, out_dtype):
    """xna_head_forward(path="fused") on projected values with channel offsets, outlier tokens and logits of ~50."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, heads = S.HEAD_GEOM
    N = S.HEAD_CASES[name][0]
    (q, k, pv, pvn, bias), (q5, k5, pv5, bd) = head_device_inputs(name, dev)
    assert ops.xna_head_select(q5, (h, w), N, ksz, out_dtype=out_dtype) == "fused"
    ref, a = S.head_reference64(q, k, pvn, ksz, heads, N, bias)
    out = ops.xna_head_forward(q5, k5, pv5, bd, ksz, n_out=N, out_dtype=out_dtype, path="fused").double().cpu()
    err = (out - ref).abs()
    bound = S.head_bound(ref, a, out_dtype == torch.bfloat16)
    if out_dtype == torch.float32:
        record("head fused fp32", name, S.worst_ratio(err, a), S.U, S.worst_of_bound(err, bound))
    S.check(err, bound, f"head {name} {out_dtype}")


@pytest.mark.parametrize("name", ["logits50", "bias40", "dominant", "offset"])
def test_head_objective_on_large_logits(dev, name):
    """The CE epilogue where the logits are large: sections A and B of tests/test_gpu_head_objective.py (their tolerances scale with |lse|,
    |L[t]| and the abs-sum), with B's per-logit bound replaced by head_bound; plus the confusion matrix of the same launch."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, heads = S.HEAD_GEOM
    N, ign = S.HEAD_CASES[name][0], 255
    Ho, Wo = h * dy, w * dx
    (q, k, pv, pvn, bias), (q5, k5, pv5, bd) = head_device_inputs(name, dev)
    t = make_target(B, Ho, Wo, N, ign)
    valid = valid_of(t, ign, N)
    cm = torch.zeros(N, N, dtype=torch.int64, device=dev)
    loss, labels, g, L = ops.xna_head_objective(q5, k5, pv5, bd, ksz, n_out=N, target=t.to(dev), ignore_index=ign, want_loss=True, want_labels=True,
                                                want_dlogits=True, return_logits=True, path="fused", confusion=cm)
    loss, labels, g, L64 = loss.double().cpu(), labels.long().cpu(), g[..., :N].double().cpu(), L.double().cpu()
    # A: the launch against its own fp32 logits
    assert torch.equal(labels, L64.argmax(1))
    lse = torch.logsumexp(L64, dim=1)
    tc = torch.where(valid, t, torch.zeros_like(t))
    Lt = L64.gather(1, tc.unsqueeze(1))[:, 0]
    assert not bool(((loss - (lse - Lt)).abs() > 1e-5 * (1.0 + lse.abs() + Lt.abs()))[valid].any())
    assert float(loss[~valid].abs().sum()) == 0.0
    ref_g = ((torch.softmax(L64, dim=1) - F.one_hot(tc, N).permute(0, 3, 1, 2).double()) * valid.unsqueeze(1)).permute(0, 2, 3, 1)
    assert not bool(((g - ref_g).abs() > 2.0 ** -8 * ref_g.abs() + 1e-5).any())
    # the confusion matrix of the same launch: exactly the counts of its labels
    assert torch.equal(cm.cpu(), ops.head_confusion_from_labels(labels, t, ign, N)) and int(cm.sum()) == int(valid.sum())
    # B: against the oracle
    ref, a = S.head_reference64(q, k, pvn, ksz, heads, N, bias)
    S.check((L64 - ref).abs(), S.head_bound(ref, a), f"objective logits {name}")
    bound = S.head_bound(ref, a).amax(dim=1)
    det, share = S.share_determined(ref, bound)
    assert share >= 0.75                                      # a condition on the inputs (tests/test_input_statistics_cpu.py), before the device result
    rlse = torch.logsumexp(ref, dim=1)
    rt = ref.gather(1, tc.unsqueeze(1))[:, 0]
    tol = 2.0 * bound + 1e-5 * (1.0 + rlse.abs() + rt.abs())
    assert not bool(((loss - (rlse - rt)).abs() > tol)[valid].any())
    chosen = ref.gather(1, labels.unsqueeze(1))[:, 0]
    assert bool((chosen >= ref.amax(dim=1) - 2.0 * bound).all()) and torch.equal(labels[det], ref.argmax(1)[det])
    if name == "dominant":
        assert float((labels == S.HEAD_CASES[name][4]).double().mean()) > 0.99


def test_head_objective_is_invariant_to_a_common_bias(dev):
    """+ 40 on every class bias: the logits move by 40 (exactly, up to the fp32 addition), loss and g do not move beyond section A's fp32
    slack, the labels and the confusion matrix not at all."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, heads = S.HEAD_GEOM
    N, ign = S.HEAD_CASES["bias40"][0], 255
    t = make_target(B, h * dy, w * dx, N, ign).to(dev)
    res = {}
    for name in ("logits50", "bias40"):
        _, (q5, k5, pv5, bd) = head_device_inputs(name, dev)
        cm = torch.zeros(N, N, dtype=torch.int64, device=dev)
        loss, labels, g, L = ops.xna_head_objective(q5, k5, pv5, bd, ksz, n_out=N, target=t, ignore_index=ign, want_loss=True, want_labels=True,
                                                    want_dlogits=True, return_logits=True, path="fused", confusion=cm)
        res[name] = (loss.double().cpu(), labels.cpu(), g.double().cpu(), L.double().cpu(), cm.cpu())
    (l0, lab0, g0, L0, cm0), (l1, lab1, g1, L1, cm1) = res["logits50"], res["bias40"]
    assert float((L1 - L0 - 40.0).abs().max()) <= 2.0 ** -22 * float(L1.abs().max())
    lse0, lse1 = torch.logsumexp(L0, dim=1), torch.logsumexp(L1, dim=1)
    # each loss is within 1e-5 (1 + |lse| + |L[t]|) of its own logits' (section A); the shifted logits differ from the unshifted by fp32 roundings
    # of numbers of size |L| + 40, which move lse - L[t] by at most 4 * 2^-24 * (|L| + 40) each
    tol = 1e-5 * (2.0 + 2.0 * lse0.abs() + 2.0 * lse1.abs()) + 2.0 ** -20 * (L1.abs().amax(dim=1) + 40.0)
    assert not bool(((l1 - l0).abs() > tol).any())
    diff = (L1 - L0 - 40.0).abs().amax(dim=1)                                 # how far the two launches' logits are from a pure shift
    margin = L0.topk(2, dim=1).values
    firm = (margin[:, 0] - margin[:, 1]) > 2.0 * diff
    assert float(firm.double().mean()) > 0.999 and torch.equal(lab0[firm], lab1[firm])
    assert int((cm0 - cm1).abs().sum()) <= 2 * int((~firm).sum())
    assert not bool(((g1 - g0).abs() > 2.0 ** -7 * g0.abs() + 2e-5 + 4.0 * diff.unsqueeze(-1)).any())


def test_head_scales_exactly(dev):
    """2^m on the projected values AND the bias scales the fp32 logits bit for bit and leaves the argmax labels unchanged."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, heads = S.HEAD_GEOM
    N = S.HEAD_CASES["offset"][0]
    _, (q5, k5, pv5, bd) = head_device_inputs("offset", dev)
    run = lambda f: ops.xna_head_objective(q5, k5, (pv5.float() * f).to(torch.bfloat16), bd * f, ksz, n_out=N, want_labels=True, return_logits=True,
                                           path="fused")
    _, lab0, _, L0 = run(1.0)
    _, lab0b, _, L0b = run(1.0)
    assert torch.equal(L0, L0b) and torch.equal(lab0, lab0b)
    for m in (-10, 10):
        _, lab, _, L = run(2.0 ** m)
        assert torch.equal(L, L0 * 2.0 ** m) and torch.equal(lab, lab0)
        out = ops.xna_head_forward(q5, k5, (pv5.float() * 2.0 ** m).to(torch.bfloat16), bd * 2.0 ** m, ksz, n_out=N, out_dtype=torch.bfloat16, path="fused")
        base = ops.xna_head_forward(q5, k5, pv5, bd, ksz, n_out=N, out_dtype=torch.bfloat16, path="fused")
        assert torch.equal(out.float(), base.float() * 2.0 ** m)


# ---- stem ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", S.IMAGE_FAMILIES)
@pytest.mark.parametrize("ks,width", [(1, 128), (3, 128), (1, 96), (3, 96)])
def test_stem_conv0_and_layer_per_element_bounds(dev, fam, ks, width):
    """conv0 on the image families under conv0_bound (2^-15 sum|x||w| + 2^-8 |ref| for the 3x3 layer of the default width, fp32 otherwise),
    its GroupNorm sums relative to sum|y| and sum y^2, and one GroupNorm -> SiLU -> conv layer on top of the kernel's own output under the
    n = 1 bound against sum |w||a|."""
    from naf_amd import ops
    B, H, W = 1, 64, 80
    img = S.make_image(B, H, W, fam, 61)
    w = O.hash_normal((width, 3, ks, ks), 62, 0.3)
    b = O.hash_normal((width,), 63, 0.1)
    ref, a = S.conv0_reference(img, w, b)
    y = torch.empty((B, H, W, width), dtype=torch.bfloat16, device=dev)
    st = ops.new_stats(B, dev)
    ops.stem_conv0(img.to(dev), w.to(dev).contiguous(), b.to(dev), y, st)
    got = y.double().cpu().permute(0, 3, 1, 2)
    bound = S.conv0_bound(ref, a, ks, width)
    pre = (got - ref).abs() - S.U * ref.abs()                   # what is left for the arithmetic before the store
    record(f"stem conv0 k{ks} width {width}", fam, S.worst_ratio(pre.clamp_min(0.0), a), 2.0 ** -15 if (ks == 3 and width == 128) else (3 * ks * ks + 2) * S.F32,
           S.worst_of_bound((got - ref).abs(), bound))
    S.check((got - ref).abs(), bound, f"conv0 k{ks} width {width} {fam}")
    sums = ops.stats_total(st).cpu()
    sb = S.group_sums_bound(ref, bound)
    assert bool(((sums - S.group_sums(ref)).abs() <= sb).all()), f"GroupNorm sums {fam}: {float(((sums - S.group_sums(ref)).abs() / sb).max()):.3f} of the bound"
    # the layer on top of the stored activation
    x = got.float()
    wl = S.bf16r(O.hash_normal((width, width, ks, ks), 72, 1.0 / (width ** 0.5 * ks)))
    bl = O.hash_normal((width,), 73, 0.1)
    gw, gb = 1.0 + O.hash_normal((width,), 74, 0.1), O.hash_normal((width,), 75, 0.1)
    rl, al = S.layer_reference(x, gw, gb, wl, bl)
    st_in = ops.stats_from_total(S.group_sums(x).to(dev))
    st_out = ops.new_stats(B, dev)
    yl = torch.empty((B, H, W, width), dtype=torch.bfloat16, device=dev)
    ops.stem_conv(y, st_in, gw.to(dev), gb.to(dev), 1e-5, ops.pack_conv_weight(wl).to(dev), bl.to(dev), yl, st_out)
    gotl = yl.double().cpu().permute(0, 3, 1, 2)
    lb = S.bf16_bound(1, al, rl.abs())
    record(f"stem layer k{ks} width {width}", fam, S.worst_ratio(((gotl - rl).abs() - S.U * rl.abs()).clamp_min(0.0), al), S.U, S.worst_of_bound((gotl - rl).abs(), lb))
    S.check((gotl - rl).abs(), lb, f"layer k{ks} width {width} {fam}")
    assert bool(((ops.stats_total(st_out).cpu() - S.group_sums(rl)).abs() <= S.group_sums_bound(rl, lb)).all())


@pytest.mark.parametrize("fam", S.IMAGE_FAMILIES)
@pytest.mark.parametrize("dim", [256, 192])
def test_stem_whole_on_image_families(dev, fam, dim):
    """Both branches, five layers each, default width 128 and the general width 96, against the fp32 oracle stem: the existing mean / max
    bound (input_statistics.stem_bound; the hot pixel with its relative term)."""
    p = O.make_params(dim=dim, seed=9)
    m = _load_model(dev, p, dim=dim)
    img = S.make_image(1, 64, 80, fam, 91)
    ref = O.conv_stem(img, p)
    assert m.image_encoder._hip_stem_ok() and m.image_encoder._hip_stem_default_width() == (dim == 256)
    got = m.image_encoder._stem_hip(img.to(dev)).float().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    mean_tol, max_tol = S.stem_bound(ref, fam)
    print(f"stem width {dim // 2} {fam}: mean err {float(err.mean()):.3e} (<= {mean_tol:.3e}) max {float(err.max()):.3e} (<= {max_tol:.3e}), |ref| max {float(ref.abs().max()):.1f}")
    assert float(err.mean()) <= mean_tol and float(err.max()) <= max_tol, (float(err.mean()), float(err.max()))


# ---- whole model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,ksz", [((64, 128), 7), ((50, 70), 5)])
def test_model_on_a_natural_image_and_features_with_offsets_and_outliers(dev, size, ksz):
    """naf(image, feats, size) on a natural-like normalised image and features with channel offsets and outlier tokens, an integer ratio
    (single-call forward, rotate-on-load) and a non-integer one: every element inside 2e-2 + 1e-2 * sum_j P_j |v_j|; and naf(image, 2^m
    feats) == 2^m naf(image, feats) bit for bit."""
    p, img, ft = S.model_case()
    m = _load_model(dev, p, kernel_size=ksz)
    ref, a = S.model_reference(p, img, ft, size, ksz)
    imgd, ftd = img.to(dev), ft.to(dev)
    with torch.no_grad():
        out = m(imgd, ftd, size)
        again = m(imgd, ftd, size)
        assert torch.equal(out, again), "two identical forwards differ"
        for e in (-10, 10):
            assert torch.equal(m(imgd, ftd * 2.0 ** e, size).float(), out.float() * 2.0 ** e), f"features x 2^{e} do not scale the output exactly"
    err = (out.double().cpu() - ref).abs()
    bound = S.model_bound(a)
    record(f"model {size} k{ksz}", "natural image, offset + outlier features", S.worst_ratio(err, a), 1e-2, S.worst_of_bound(err, bound))
    S.check(err, bound, f"model {size}")


def test_model_probe_objective_on_realistic_inputs(dev):
    """naf(image, feats, size, head=probe, target=t) on the same inputs: the mean loss against fp64 cross-entropy of the probe on the oracle's
    output.  Per logit the probe turns the elementwise bound of the output into sum_c |W[n, c]| (2e-2 + 1e-2 abs_sum_c), plus the bf16 rounding
    of the projected values the fused path forms (1.25 * 2^-8 sum_c |W[n, c]| abs_sum_c); logsumexp is 1-Lipschitz and the target logit moves by
    as much: every pixel's loss within twice the largest logit bound of that pixel, the mean loss within the mean of that."""
    from test_gpu_head import _probe
    p, img, ft = S.model_case()
    size, ksz, N = (64, 128), 7, 21
    m = _load_model(dev, p, kernel_size=ksz)
    conv = _probe(128, N, 603, dev)
    t = make_target(1, *size, N, 255)
    valid = valid_of(t, 255, N)
    ref, a = S.model_reference(p, img, ft, size, ksz)
    W64, b64 = conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu()
    logits = F.conv2d(ref, W64, b64)
    ref_loss = float(F.cross_entropy(logits, t, ignore_index=255))
    lb = F.conv2d(S.model_bound(a) + S.SLACK * S.U * a, W64.abs()).amax(dim=1)
    tol = float((2.0 * lb)[valid].mean()) + 1e-5 * (1.0 + float(logits.abs().max()))
    with torch.no_grad():
        loss = float(m(img.to(dev), ft.to(dev), size, head=conv, target=t.to(dev), ignore_index=255))
        lmap = m(img.to(dev), ft.to(dev), size, head=conv, target=t.to(dev), ignore_index=255, reduction="none").double().cpu()
    print(f"probe objective: loss {loss:.6f} reference {ref_loss:.6f} (tolerance {tol:.3e})")
    assert abs(loss - ref_loss) <= tol
    # ... and pixel by pixel
    ref_map = F.cross_entropy(logits, t, ignore_index=255, reduction="none")
    ptol = 2.0 * lb + 1e-5 * (1.0 + logits.abs().amax(dim=1))
    perr = (lmap - ref_map).abs()
    print(f"    loss map: worst err / tolerance {float((perr / ptol)[valid].max()):.3f}, worst err {float(perr[valid].max()):.3e}")
    assert not bool((perr > ptol)[valid].any()) and float(lmap[~valid].abs().sum()) == 0.0
    # ... and against the model's OWN output through the probe (the stem's error drops out: both calls see the same queries and keys).  The two
    # differ by the roundings alone: P to bf16 in each (1.25 * 2^-8 sum_c |W| abs_sum_c each), the projected values W_g V_g to bf16 in the fused
    # call (2^-8 of the same sum), the bf16 store of the unfused output (2^-8 sum_c |W||out_c|).  abs_sum is taken from the oracle and raised by
    # the whole-forward bound applied to |v| (it is the forward of |v|: the device's weights move it by no more than that).
    with torch.no_grad():
        out = m(img.to(dev), ft.to(dev), size)
    own = F.conv2d(out.double().cpu(), W64, b64)
    a_up = a + S.model_bound(a)
    lself = F.conv2d((2.0 * S.SLACK + 1.0) * S.U * a_up + (S.U * out.double().cpu().abs() if out.dtype == torch.bfloat16 else 0.0), W64.abs()).amax(dim=1)
    stol = 2.0 * lself + 1e-5 * (1.0 + own.abs().amax(dim=1))
    serr = (lmap - F.cross_entropy(own, t, ignore_index=255, reduction="none")).abs()
    print(f"    against its own output: worst err / tolerance {float((serr / stol)[valid].max()):.3f}, worst err {float(serr[valid].max()):.3e}, "
          f"tolerance {float(stol[valid].min()):.2e} .. {float(stol[valid].max()):.2e}")
    assert not bool((serr > stol)[valid].any())
