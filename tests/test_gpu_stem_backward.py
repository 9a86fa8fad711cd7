"""GPU tests (-m gpu) of the training side of the conv stem -- stem_bwd.hip, stem_wgrad.hip, stem_generic_bwd.hip and rope_pool_bwd_kernel --
against the fp64 restatement of tests/stem_backward_reference.py (its docstring derives every bound, with file and line).

Tolerance part: EVERY element of dx, d gamma, d beta, dW, d bias is held to its own bound, on input families that make GroupNorm's two
correction terms O(1) (``correlated``), that cost xhat bits (``chan_offset``), that saturate SiLU and overflow exp2 (``outlier``) and on a
layer input the HIP stem itself produced (``from_stem``); at the shapes that reach each code path of stem_act_bwd_kernel.  tests/
test_gpu_train_stem.py holds the same kernels to whole-tensor norms on i.i.d. inputs, where a 10 % error of either mean is invisible
(tests/test_stem_backward_cpu.py shows both, and that the planted defects leave these bounds).

Exact part, the pixel census: integer-valued inputs whose sums stay below 2^24 make every fp32 sum exact in any order, atomics included,
so the weight gradients are compared with ``torch.equal``.  Pass (a): a == 1 and dy = the bits of the pixel's index -- every 16-byte piece
of every pixel is counted once, and the output channels that are off spell the pixel that was lost or doubled.  Pass (b): dy == 1 and a =
the bits of the column / row index -- every tap reads its own reflected pixels.  The shapes reach every branch of the launchers
(stem_backward_reference.wgrad_plan restates them from the device's CU count).

NAF_STEM_BWD_PROFILE=<file> appends the measured worst err / abs_sum and worst share of the bound per kernel and family
(profiles/stem_backward_statistics.txt)."""
import os
import sys

import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import stem_backward_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 1e-5
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def record(kernel, family, ratio, of_bound):
    line = R.profile_line(kernel, family, ratio, of_bound)
    print(line)
    dest = os.environ.get("NAF_STEM_BWD_PROFILE")
    if dest:
        with open(dest, "a") as f:
            f.write(line + "\n")


def cu_count(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def stats_of(x, dev):
    from naf_amd import ops
    return ops.stats_from_total(R.group_totals(x).to(dev).contiguous())


def family_case(dev, family, B, H, W, C, fold, seed):
    """(x, da, gamma, beta) on the host (bf16-representable fp32), the device's stats buffer and the fp64 totals it holds."""
    from naf_amd import ops
    gamma, beta = R.make_affine(C, seed, family)
    if family == "from_stem":
        img, w0, b0 = R.from_stem_case(C, B, H, W, "natural_norm", seed)
        y = torch.empty((B, H, W, C), dtype=BF, device=dev)
        stats = ops.new_stats(B, dev)
        ops.stem_conv0(img.to(dev), w0.to(dev).contiguous(), b0.to(dev), y, stats)
        x, totals = y.float().cpu(), ops.stats_total(stats).cpu()
    else:
        x = R.make_x(family, B, H, W, C, seed)
        stats, totals = stats_of(x, dev), None
    return x, R.make_grad(family, x, fold, seed), gamma, beta, stats, totals


def run_act_bwd(dev, x, da, gamma, beta, stats, fold, dx=None, sums=None):
    from naf_amd import ops
    B, H, W, C = x.shape
    if dx is None:
        dx = torch.full((B, H, W, C), float("nan"), dtype=BF, device=dev)
    s = ops.stem_act_bwd(da.to(dev).to(BF), x.to(dev).to(BF), stats, gamma.to(dev), beta.to(dev), EPS, dx, fold=fold, sums=sums)
    return dx.double().cpu(), s.cpu()


def hold(failures, err, bound, what):
    try:
        S.check(err, bound, what)
    except AssertionError as e:
        failures.append(str(e))


# ---- SiLU / GroupNorm backward -------------------------------------------------------------------------------------------------------
# (B, H, W, C): width 128 at W = 20 / 70 (16 pixel planes: one pixel per thread / the batched four-at-a-time run and its remainder loop; planes whose
# last pixel is column W - 2 and planes whose last pixel is W - 1 exist at both), the `general` path (W < 4; H = 3: rows 1 and H - 2 coincide),
# H = 2; the widths whose 8-channel chunks straddle groups (48, 240) and 16 (128 pixel planes)
ACT_SHAPES = [(2, 12, 20, 128), (1, 5, 70, 128), (1, 3, 7, 128), (2, 4, 3, 128), (1, 2, 9, 128), (2, 9, 14, 48), (1, 6, 10, 240), (2, 5, 5, 16), (1, 4, 150, 16)]


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_act_backward_per_element(dev, shape, fold):
    """ops.stem_act_bwd: dx and the per-sample {d beta, d gamma} sums, every element inside its bound, on every family."""
    B, H, W, C = shape
    chain = R.act_bwd_chain(H, W, C, cu_count(dev))
    failures = []
    for family in R.FAMILIES:
        x, da, gamma, beta, stats, totals = family_case(dev, family, B, H, W, C, fold, 100 + H + C)
        dx, sums = run_act_bwd(dev, x, da, gamma, beta, stats, fold)
        r = R.act_bwd_reference(x, da, gamma, beta, EPS, fold, totals)
        b = R.act_bwd_bounds(r, chain)
        assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(sums).all()), family
        e_dx, e_s = (dx - r["dx"]).abs(), (sums - r["sums"]).abs()
        name = f"stem_act_bwd {'fold' if fold else 'plain'} {'x'.join(map(str, shape))}"
        record(name + " dx", family, S.worst_ratio(e_dx, R.act_bwd_abs_sum(r)), S.worst_of_bound(e_dx, b["dx"]))
        record(name + " sums", family, S.worst_ratio(e_s, torch.stack([r["adz"].sum((1, 2)), (r["adz"] * r["f"]["xh"].abs()).sum((1, 2))], -1)),
               S.worst_of_bound(e_s, b["sums"]))
        hold(failures, e_dx, b["dx"], f"{name} dx {family}")
        hold(failures, e_s, b["sums"], f"{name} sums {family}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("where,pos", [("corner", (0, 0)), ("corner-far", (13, 21)), ("top edge", (0, 7)), ("bottom edge", (13, 2)), ("left edge", (5, 0)),
                                        ("right edge", (6, 21)), ("first ring", (1, 1)), ("first ring row", (1, 9)), ("first ring column", (7, 20))])
def test_act_backward_fold_impulse(dev, where, pos):
    """An impulse of da at each class of position of the padded border: the mirrored contribution must arrive at ITS pixel (same bound)."""
    B, H, W, C = 1, 12, 20, 128
    x, _, gamma, beta, stats, _ = family_case(dev, "correlated", B, H, W, C, True, 77)
    da = torch.zeros(B, H + 2, W + 2, C)
    da[0, pos[0], pos[1]] = S.bf16r(1.0 + O.hash_normal((C,), 78))
    dx, sums = run_act_bwd(dev, x, da, gamma, beta, stats, True)
    r = R.act_bwd_reference(x, da, gamma, beta, EPS, True)
    b = R.act_bwd_bounds(r, R.act_bwd_chain(H, W, C, cu_count(dev)))
    S.check((dx - r["dx"]).abs(), b["dx"], f"impulse at the {where} {pos}: dx")
    S.check((sums - r["sums"]).abs(), b["sums"], f"impulse at the {where} {pos}: sums")


def test_act_backward_strided_view_and_shared_sums(dev):
    """As _HipStem.backward passes them (naf_amd/model.py:295): dx is the interior of a zero-bordered (H + 4) x (W + 4) buffer, da the interior of the
    data-gradient buffer, the sums one layer's slice of the step's zeroed fp64 accumulator."""
    B, H, W, C = 2, 7, 37, 128
    x, da, gamma, beta, stats, _ = family_case(dev, "correlated", B, H, W, C, True, 55)
    full = torch.full((B, H + 4, W + 4, C), float("nan"), dtype=BF, device=dev)
    full[:, 1:H + 3, 1:W + 3] = da.to(dev).to(BF)
    ext = torch.zeros((B, H + 4, W + 4, C), dtype=BF, device=dev)
    acc64 = torch.zeros((2, 3, B, C, 2), dtype=torch.float64, device=dev)
    from naf_amd import ops
    s = ops.stem_act_bwd(full[:, 1:H + 3, 1:W + 3], x.to(dev).to(BF), stats, gamma.to(dev), beta.to(dev), EPS, ext[:, 2:H + 2, 2:W + 2], fold=True, sums=acc64[1, 2])
    assert s.data_ptr() == acc64[1, 2].data_ptr()
    r = R.act_bwd_reference(x, da, gamma, beta, EPS, True)
    b = R.act_bwd_bounds(r, R.act_bwd_chain(H, W, C, cu_count(dev)))
    S.check((ext[:, 2:H + 2, 2:W + 2].double().cpu() - r["dx"]).abs(), b["dx"], "strided dx")
    S.check((acc64[1, 2].cpu() - r["sums"]).abs(), b["sums"], "sums slice")
    border = ext.clone()
    border[:, 2:H + 2, 2:W + 2] = 0
    assert float(border.abs().max()) == 0.0 and float(acc64[0].abs().max()) == 0.0 and float(acc64[1, :2].abs().max()) == 0.0


# ---- weight gradient, activation computed by the loader ---------------------------------------------------------------------------------
# width 128: the simple kernel (W mod 32 = 1) and the pipelined one (two segments, the last of 4 pixels); the general widths, 144 and 256 with their
# output channels split over two workgroups
WGRAD_CASES = [(3, 2, 9, 33, 128), (1, 2, 9, 33, 128), (3, 1, 12, 36, 128), (1, 1, 12, 36, 128), (3, 2, 13, 45, 48), (1, 2, 13, 45, 48),
               (3, 1, 6, 70, 144), (1, 1, 6, 70, 144), (3, 1, 10, 18, 256), (1, 1, 10, 18, 256)]


@pytest.mark.parametrize("k,B,H,W,C", WGRAD_CASES)
def test_weight_gradient_per_element(dev, k, B, H, W, C):
    """ops.stem_wgrad with the activation computed in its loader, and the two-call sequence stem_act -> plain stem_wgrad: dW and d bias."""
    from naf_amd import ops
    if C == 128:
        assert R.wgrad_plan(k, B, H, W, cu_count(dev))["kernel"] == ("simple" if W == 33 else "pipelined")
    failures = []
    for family in ("correlated", "chan_offset", "outlier"):
        x, dy, gamma, beta, stats, _ = family_case(dev, family, B, H, W, C, False, 200 + W + k)
        xd, dyd, gd, bd = x.to(dev).to(BF), dy.to(dev).to(BF), gamma.to(dev), beta.to(dev)
        dw, db = ops.stem_wgrad(dyd, xd, stats, gd, bd, EPS, k, with_bias=True)
        a0 = ops.stem_act(xd, stats, gd, bd, EPS, pad=0)
        dw2, db2 = ops.stem_wgrad(dyd, a0, None, None, None, EPS, k, with_bias=True)
        f = R.act_forward(x, gamma, beta, EPS)
        ref, aw, rdb, adb = R.wgrad_reference(dy, f["a"], k)
        b_dw, b_db = R.wgrad_bounds(dy, aw, adb, k, f)
        for tag, got_w, got_b in (("loader", dw, db), ("two-call", dw2, db2)):
            e_w, e_b = (got_w.double().cpu() - ref).abs(), (got_b.double().cpu() - rdb).abs()
            name = f"stem_wgrad {tag} k{k} {B}x{H}x{W}x{C}"
            record(name + " dW", family, S.worst_ratio(e_w, aw), S.worst_of_bound(e_w, b_dw))
            record(name + " db", family, S.worst_ratio(e_b, adb), S.worst_of_bound(e_b, b_db))
            hold(failures, e_w, b_dw, f"{name} dW {family}")
            hold(failures, e_b, b_db, f"{name} db {family}")
    assert not failures, "\n".join(failures)


# ---- RoPE + key pooling, adjoint -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lr", [((2, 256, 32, 48), (4, 6)), ((1, 256, 23, 30), (5, 7)), ((1, 128, 16, 16), (16, 16))])
def test_rope_pool_backward_per_element(dev, shape, lr):
    """ops.rope_pool_bwd at the three geometries of test_gpu_train_stem.py::test_rope_pool_backward (divisible, overlapping windows, ratio 1), per
    element, against the fp64 adjoint fed the SAME fp32 cos / sin tables."""
    from naf_amd import ops
    B, C, H, W = shape
    heads = C // 64
    ty, tx = ops.rope_tables(O.rope_periods(C, heads, 100.0).to(dev), H, W)
    gq = S.bf16r(O.hash_normal(shape, 21) + 0.5)
    gk = O.hash_normal((B, C, *lr), 22) * float(H * W) / float(lr[0] * lr[1]) + 1.0          # a cell's gradient spreads over its window
    to5 = lambda t: t.reshape(B, heads, 64, *t.shape[-2:]).permute(0, 1, 3, 4, 2).contiguous()
    dx = ops.rope_pool_bwd(to5(gq).to(dev).to(BF), to5(gk).to(dev), ty, tx, (H, W))
    assert dx.shape == shape and dx.dtype == BF
    ref, a = R.rope_pool_bwd_reference(to5(gq), to5(gk), ty.cpu(), tx.cpu())
    err = (dx.double().cpu() - ref).abs()
    bound = R.rope_pool_bwd_bound(ref, a)
    record(f"rope_pool_bwd {shape} -> {lr}", "unit + offset", S.worst_ratio(err, a), S.worst_of_bound(err, bound))
    S.check(err, bound, f"rope_pool_bwd {shape} {lr}")
    # the tables themselves (rope_pool.hip:24-28): |angle| <= 2 pi after seven fp32 roundings, 2 pi * 7 * 2^-24 = 2.6e-6, plus sinf / cosf
    t64y, t64x = R.rope_tables64(O.rope_periods(C, heads, 100.0), H, W)
    assert float((ty.double().cpu() - t64y).abs().max()) < 3e-6 and float((tx.double().cpu() - t64x).abs().max()) < 3e-6


# ---- exact identities ------------------------------------------------------------------------------------------------------------------
def scaling_protocol(launch, scaled_launch, names, what):
    """tests/test_gpu_input_statistics.py::test_backward_scales_exactly's protocol: five identical launches first; a result that is bit-equal in all
    of them must scale bit for bit, one that is not (fp32 / fp64 atomics in an order that is not fixed) may differ by twice the largest difference
    seen between identical launches."""
    base = launch()
    slack = {n: 0.0 for n in names}
    for _ in range(4):
        again = launch()
        for n, a, b in zip(names, base, again):
            slack[n] = max(slack[n], float((a - b).abs().max()))
    print(f"{what}: identical launches differ by at most {slack}")
    for n, a in zip(names, base):
        assert slack[n] <= 2.0 ** -13 * float(a.abs().max()), (n, slack[n])
    for m in (-10, 10):
        f = 2.0 ** m
        got = scaled_launch(f)
        for n, a, g in zip(names, base, got):
            if slack[n] == 0.0:
                assert torch.equal(g, a * f), f"{what}: {n} x 2^{m} is not bit-equal"
            else:
                d = float((g / f - a).abs().max())
                assert d <= 2.0 * slack[n], f"{what}: {n} x 2^{m} off by {d:.3e} (identical launches: {slack[n]:.3e})"


# The shapes of the bit-for-bit identities.  A sum that leaves through atomics is order-independent -- and five identical launches can therefore DECIDE
# whether it is bit-equal -- exactly when an element receives at most TWO contributions: the buffer starts at zero, 0 + a is exact and a + b = b + a.
# With three or more the order of the additions is not fixed, identical launches differ in the last bit now and then, and five samples that agree
# prove nothing about the sixth.  So H = 2 and one sample where sums are compared: stem_act_bwd adds one partial sum per image row and sample
# (stem_bwd.hip:285), the weight-gradient kernels one per row band / segment range and sample (stem_wgrad.hip:212, :546, stem_generic_bwd.hip:179);
# 2 x 32 is two ranges of one segment.  dx is written once per element; it is also asserted at 12 x 20 and 5 x 70 (the interior rows' code path).
# Sums with MANY contributions are held by test_scaling_up_to_the_order_of_the_atomics below.
@pytest.mark.parametrize("fold,B,H,W,C,names", [(True, 2, 2, 70, 128, ("dx", "sums")), (False, 2, 2, 20, 128, ("dx", "sums")), (True, 1, 2, 14, 48, ("dx", "sums")),
                                                (True, 2, 12, 20, 128, ("dx",)), (False, 1, 5, 70, 128, ("dx",))])
def test_act_backward_scales_exactly(dev, fold, B, H, W, C, names):
    """da -> 2^m da scales dx (written once per element) and the GroupNorm sums (fp64 atomics of fp32 partial sums), m = +-10."""
    x, da, gamma, beta, stats, _ = family_case(dev, "correlated", B, H, W, C, fold, 300 + W)
    launch = lambda f=1.0: run_act_bwd(dev, x, da * f, gamma, beta, stats, fold)[:len(names)]
    scaling_protocol(launch, launch, names, f"stem_act_bwd fold={fold} {B}x{H}x{W}x{C}")


@pytest.mark.parametrize("k,B,H,W,C", [(3, 1, 2, 32, 128), (1, 1, 2, 32, 128), (3, 1, 2, 33, 128), (1, 1, 2, 19, 128), (3, 1, 2, 45, 48), (3, 1, 2, 70, 144), (1, 1, 2, 18, 256)])
def test_weight_gradient_scales_exactly(dev, k, B, H, W, C):
    """dy -> 2^m dy scales dW and d bias (fp32 atomics, two contributions per element), m = +-10; the activation comes from the loader.  Width 128: the
    pipelined kernel (W = 32) and the simple one."""
    from naf_amd import ops
    if C == 128:
        plan = R.wgrad_plan(k, B, H, W, cu_count(dev))
        assert plan["kernel"] == ("pipelined" if W == 32 else "simple") and plan.get("nranges", 2) <= 2
    x, dy, gamma, beta, stats, _ = family_case(dev, "correlated", B, H, W, C, False, 400 + W)
    xd, gd, bd = x.to(dev).to(BF), gamma.to(dev), beta.to(dev)

    def launch(f=1.0):
        dw, db = ops.stem_wgrad((dy * f).to(dev).to(BF), xd, stats, gd, bd, EPS, k, with_bias=True)
        return dw.double().cpu(), db.double().cpu()
    scaling_protocol(launch, launch, ("dW", "db"), f"stem_wgrad k{k} {B}x{H}x{W}x{C}")


@pytest.mark.parametrize("k,B,H,W,C", [(3, 1, 40, 36, 128), (1, 2, 64, 100, 128), (3, 1, 6, 70, 144), (3, 2, 13, 45, 48)])
def test_scaling_up_to_the_order_of_the_atomics(dev, k, B, H, W, C):
    """dy -> 2^m dy where an element of dW / d bias receives MANY atomic contributions (80 segment ranges at 40 x 36; the row bands of the general
    kernel).  A workgroup's partial sum is a fixed sequence of operations, so the scaled launch's partials are exactly 2^m times the unscaled ones;
    only the order in which n of them meet differs, and two orders of an n-term fp32 sum differ by at most 2 (n - 1) 2^-24 sum |partials| <=
    2 (n - 1) 2^-24 abs-sum.  That bound is asserted per element (1e-5 of the abs-sum at n = 80, 400 times below one bf16 rounding); the spread of
    five identical launches is printed next to it."""
    from naf_amd import ops
    cu = cu_count(dev)
    n = B * (R.wgrad_plan(k, B, H, W, cu)["nranges"] if C == 128 else R.wgradg_plan(k, B, H, C, cu)[1])
    assert n > 2
    x, dy, gamma, beta, stats, _ = family_case(dev, "correlated", B, H, W, C, False, 400 + W)
    xd, gd, bd = x.to(dev).to(BF), gamma.to(dev), beta.to(dev)

    def launch(f=1.0):
        dw, db = ops.stem_wgrad((dy * f).to(dev).to(BF), xd, stats, gd, bd, EPS, k, with_bias=True)
        return dw.double().cpu(), db.double().cpu()
    a = ops.stem_act(xd, stats, gd, bd, EPS, pad=0).float().cpu()                     # the loader's bf16 operand: only its abs-sum is used
    _, aw, _, adb = R.wgrad_reference(dy, a, k)
    allowed = {"dW": 2.0 * (n - 1) * R.F32 * aw * (1.0 + R.U), "db": 2.0 * (n - 1) * R.F32 * adb}
    base = launch()
    spread = {"dW": 0.0, "db": 0.0}
    for _ in range(4):
        for name, p0, p1 in zip(("dW", "db"), base, launch()):
            S.check((p0 - p1).abs(), allowed[name], f"identical launches, {name}")
            spread[name] = max(spread[name], float((p0 - p1).abs().max()))
    print(f"stem_wgrad k{k} {B}x{H}x{W}x{C}: {n} contributions per element; identical launches differ by at most {spread}")
    for m in (-10, 10):
        f = 2.0 ** m
        for name, p0, p1 in zip(("dW", "db"), base, launch(f)):
            S.check((p1 / f - p0).abs(), allowed[name], f"dy x 2^{m}: {name}")


# ---- one composed layer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,H,W,C", [(3, 12, 20, 128), (3, 5, 33, 128), (1, 9, 17, 128), (3, 12, 20, 48)])
def test_composed_layer_backward(dev, k, H, W, C):
    """One layer of _HipStem.backward (naf_amd/model.py:287-301): the zero-bordered gradient buffer, stem_conv_plain on the flipped / transposed
    packed weights, stem_act_bwd on the interior of its output with the fold -- dx per element against fp64 autograd's formula of
    conv(reflect_pad(SiLU(GN(x)))), bound = the two kernels' bounds (stem_backward_reference.layer_reference).  What this case is for is the plumbing
    between the two kernels (weight flip and transpose, the buffer offsets, the fold): the output gradient g correlates with x, but da = conv^T(g) through
    hash-normal weights does not, so GroupNorm's means are small here and the bound is mostly the carried bf16 error of da; the means themselves are
    held by test_act_backward_per_element on the ``correlated`` family."""
    from naf_amd import ops
    B = 2
    x, g, gamma, beta, stats, _ = family_case(dev, "correlated", B, H, W, C, False, 500 + W)
    w = S.bf16r(O.hash_normal((C, C, k, k), 501, (C * k * k) ** -0.5))
    wt = ops.pack_conv_weight(w.to(dev).flip(2, 3).transpose(0, 1))
    xd, gd, bd = x.to(dev).to(BF), gamma.to(dev), beta.to(dev)
    dx = torch.full((B, H, W, C), float("nan"), dtype=BF, device=dev)
    if k == 3:
        ext = torch.zeros((B, H + 4, W + 4, C), dtype=BF, device=dev)
        ext[:, 2:H + 2, 2:W + 2] = g.to(dev).to(BF)
        full = torch.empty_like(ext)
        ops.stem_conv_plain(ext, wt, full)
        ops.stem_act_bwd(full[:, 1:H + 3, 1:W + 3], xd, stats, gd, bd, EPS, dx, fold=True)
    else:
        da = torch.empty((B, H, W, C), dtype=BF, device=dev)
        ops.stem_conv_plain(g.to(dev).to(BF), wt, da)
        ops.stem_act_bwd(da, xd, stats, gd, bd, EPS, dx, fold=False)
    r, bound = R.layer_reference(x, g, gamma, beta, EPS, w, R.act_bwd_chain(H, W, C, cu_count(dev)))
    err = (dx.double().cpu() - r["dx"]).abs()
    record(f"composed layer k{k} {B}x{H}x{W}x{C} dx", "correlated", S.worst_ratio(err, R.act_bwd_abs_sum(r)), S.worst_of_bound(err, bound))
    S.check(err, bound, f"composed layer k{k} {H}x{W}x{C}")


# ---- the exact pixel census --------------------------------------------------------------------------------------------------------------
def census_wgrad(dev, k, B, H, W, C):
    from naf_amd import ops
    # pass (a): every piece of every pixel once
    dy, counts, nbits = R.census_dy(B, H, W, C)
    assert int(counts.max()) < 2 ** 24
    ones = torch.ones((B, H, W, C), dtype=BF, device=dev)
    dw, db = ops.stem_wgrad(dy.to(dev).to(BF), ones, None, None, None, EPS, k, with_bias=True)
    want = counts.view(C, 1, 1, 1).expand(C, C, k, k)
    got = dw.cpu().double()
    assert bool((got == got.round()).all())
    diff = got.long() - want
    assert not bool(diff.any()), f"pass (a) k{k} {B}x{H}x{W}x{C}: {R.census_decode(diff, nbits, (B, H, W))}"
    assert torch.equal(db.cpu().double().long(), counts) and torch.equal(db.cpu().double(), counts.double()), f"pass (a) k{k} {B}x{H}x{W}x{C}: d bias"
    # pass (b): every tap reads its own pixels
    a = R.census_a(B, H, W, C)
    cnt = R.census_a_counts(a, k)
    assert int(cnt.max()) < 2 ** 24
    dw, db = ops.stem_wgrad(ones, a.to(dev).to(BF), None, None, None, EPS, k, with_bias=True)
    got = dw.cpu().double()
    wrong = (got != cnt.double().view(1, C, k, k)).nonzero()
    assert wrong.numel() == 0, (f"pass (b) k{k} {B}x{H}x{W}x{C}: {wrong.shape[0]} entries wrong, first (oc, ic, ty, tx) = {wrong[0].tolist()}: "
                                f"got {float(got[tuple(wrong[0].tolist())])}, want {int(cnt[tuple(wrong[0, 1:].tolist())])}")
    assert torch.equal(db.cpu().double(), torch.full((C,), float(B * H * W), dtype=torch.float64)), "pass (b): d bias"


@pytest.mark.parametrize("k,B,H,W", R.WGRAD_CENSUS_SHAPES)
def test_weight_gradient_census(dev, k, B, H, W):
    """ops.stem_wgrad in plain mode at width 128 (stem_wgrad_kernel / stem_wgrad2_kernel), exact."""
    census_wgrad(dev, k, B, H, W, 128)


@pytest.mark.parametrize("name", list(R.WGRAD_CLASSES))
def test_weight_gradient_census_reaches(dev, name):
    """The census shapes reach this behaviour of naf_launch_stem_wgrad / stem_wgrad2_launch on THIS device (the plan depends on its CU count)."""
    plans = [R.wgrad_plan(k, B, H, W, cu_count(dev)) for k, B, H, W in R.WGRAD_CENSUS_SHAPES]
    if not any(R.WGRAD_CLASSES[name](p) for p in plans):
        # a class the device cannot reach below the pixel cap is skipped (and named); a class it CAN reach but the list misses is a gap in the list
        assert not R.wgrad_class_reachable(name, cu_count(dev)), f"{cu_count(dev)} CUs: '{name}' is reachable below the pixel cap but no census shape reaches it"
        pytest.skip(f"{cu_count(dev)} CUs: no shape below the pixel cap reaches '{name}'")


@pytest.mark.parametrize("C", [48, 96, 144, 256])
@pytest.mark.parametrize("k,B,H,W", [(3, 2, 13, 45), (1, 1, 40, 33), (3, 1, 131, 45)])
def test_weight_gradient_census_general_widths(dev, k, B, H, W, C):
    """stem_wgradg_kernel, exact; 144 and 256 split their output channels over two workgroups.  131 x 45: several rows per workgroup (the first two
    shapes give every workgroup one row) and, on 256 CUs, a last band cut short at every width (r1 = min(H, r0 + rows), stem_generic_bwd.hip:55):
    3 rows at 48 / 96 (131 = 43 * 3 + 2), 5 rows at 144 / 256 (131 = 26 * 5 + 1).  The census runs whatever the device's plan is."""
    if H == 131:
        rows, bands = R.wgradg_plan(k, B, H, C, cu_count(dev))
        print(f"width {C}: {rows} rows per workgroup, {bands} bands, last band of {H - (bands - 1) * rows} rows")
        if cu_count(dev) == 256:
            assert rows == (3 if C <= 128 else 5) and H % rows != 0
    census_wgrad(dev, k, B, H, W, C)


def small_ints(shape, seed, amp):
    return torch.round(O.hash_normal(shape, seed) * (amp / 2.0)).clamp(-amp, amp)


@pytest.mark.parametrize("image_dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [16, 128, 256])          # 16: stem_conv0_wgrad_kernel; from 32 (stem_bwd.hip:555): the matrix-pipe kernel
@pytest.mark.parametrize("k,B,H,W,amp", [(3, 2, 9, 37, 1000.0), (1, 2, 9, 37, 1000.0), (3, 1, 33, 64, 1000.0), (1, 1, 33, 64, 1000.0),
                                         (3, 2, 200, 96, 300.0), (1, 2, 200, 96, 300.0)])
def test_first_convolution_weight_gradient_census(dev, k, B, H, W, amp, C, image_dtype):
    """ops.stem_conv0_wgrad on an integer image and bit-coded dy: exact.  Integers up to 1000 need more than bf16's 8 bits, so the matrix-pipe kernel's
    lo part (stem_bwd.hip:523) carries them -- hi + lo is exact for |v| < 2^16 --; as a bf16 image they are rounded first and the reference takes the
    rounded values.  2 x 200 x 96 is 1 200 segments, more than the 3 workgroups per CU the launcher starts (asserted): the double-buffered loop
    (:498-529) runs several segments per workgroup."""
    from naf_amd import ops
    if H == 200 and C >= 32:
        assert B * H * ((W + 31) // 32) > 3 * cu_count(dev)
    img = small_ints((B, 3, H, W), 61 + H, amp).to(image_dtype).float()
    dy, counts, nbits = R.census_dy(B, H, W, C)
    dw, db = ops.stem_conv0_wgrad(dy.to(dev).to(BF), img.to(dev).to(image_dtype), k)
    ref, aw, _, _ = R.wgrad_reference(dy, img.permute(0, 2, 3, 1), k)
    assert float(aw.max()) < 2 ** 24 and float(img.abs().max()) > 256
    wrong = (dw.cpu().double() != ref).nonzero()
    assert wrong.numel() == 0, f"{wrong.shape[0]} entries wrong, first (oc, c, ty, tx) = {wrong[0].tolist()}"
    assert torch.equal(db.cpu().double(), counts.double())


@pytest.mark.parametrize("image_dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("family", ["natural_norm", "hot_pixel"])
@pytest.mark.parametrize("k,C", [(3, 16), (1, 16), (3, 128), (1, 128)])
def test_first_convolution_gradients_per_element(dev, k, C, family, image_dtype):
    """ops.stem_conv0_wgrad / stem_conv0_dgrad on images that are not integers: every element inside the fp32 accumulation bound, plus 2^-16 abs-sum
    for the bf16 hi + lo split of an fp32 image on the matrix-pipe kernel (C >= 32) -- without the lo part the error would be 2^-9 abs-sum."""
    from naf_amd import ops
    B, H, W = 2, 9, 37
    img = S.make_image(B, H, W, family, 81).to(image_dtype).float()
    dy = R.make_grad("chan_offset", torch.zeros(B, H, W, C), False, 82)
    w = O.hash_normal((C, 3, k, k), 83, (3 * k * k) ** -0.5)
    r = R.conv0_grads_reference(dy, img, w)
    b = R.conv0_bounds(r, dy, image_dtype == torch.float32, C >= 32)
    dw, db = ops.stem_conv0_wgrad(dy.to(dev).to(BF), img.to(dev).to(image_dtype), k)
    dimg = torch.full((B, 3, H, W), float("nan"), device=dev)
    ops.stem_conv0_dgrad(dy.to(dev).to(BF), w.to(dev).contiguous(), dimg)
    failures = []
    for what, got, ref, a in (("dw", dw, r["dw"], r["a_dw"]), ("db", db, r["db"], r["a_db"]), ("dimage", dimg, r["dimage"], r["a_dimage"])):
        err = (got.double().cpu() - ref).abs()
        record(f"stem_conv0 k{k} C{C} {'f32' if image_dtype == torch.float32 else 'bf16'} image {what}", family, S.worst_ratio(err, a), S.worst_of_bound(err, b[what]))
        hold(failures, err, b[what], f"conv0 {what} k{k} C{C} {family}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("C", [16, 160, 256])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("H,W", [(2, 2), (5, 6), (33, 35), (24, 100)])
def test_first_convolution_image_gradient_exact(dev, H, W, k, C):
    """ops.stem_conv0_dgrad on small-integer weights and dy: written into a NaN-filled buffer, then added to an integer-filled one; exact."""
    from naf_amd import ops
    B = 2
    w = small_ints((C, 3, k, k), 71 + C, 3.0)
    dy = small_ints((B, H, W, C), 72 + W, 4.0)
    r = R.conv0_grads_reference(dy, torch.zeros(B, 3, H, W), w)
    assert float(r["a_dimage"].max()) + 7.0 < 2 ** 24
    dimg = torch.full((B, 3, H, W), float("nan"), device=dev)
    ops.stem_conv0_dgrad(dy.to(dev).to(BF), w.to(dev).contiguous(), dimg)
    assert torch.equal(dimg.cpu().double(), r["dimage"]), "written"
    fill = small_ints((B, 3, H, W), 73, 7.0)
    dimg = fill.to(dev).clone()
    ops.stem_conv0_dgrad(dy.to(dev).to(BF), w.to(dev).contiguous(), dimg, accumulate=True)
    assert torch.equal(dimg.cpu().double(), r["dimage"] + fill.double()), "accumulated"
