"""Host-side companion of tests/test_gpu_stem_backward.py (no device): the fp64 restatement of the stem's backward equals torch autograd in
fp64; the kernels' arithmetic emulated on the host (fp32, bf16 at the kernels' rounding points) stays inside every bound of
tests/stem_backward_reference.py on every input family; planted defects leave those bounds; the exact pixel census notices one lost or
doubled 16-byte piece and names its pixel."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import input_statistics as S  # noqa: E402
import stem_backward_reference as R  # noqa: E402
from oracle import naf_oracle as O  # noqa: E402

EPS = 1e-5
HOST_FAMILIES = R.FAMILIES
ACT_SHAPES = [(2, 12, 20, 128), (2, 9, 14, 48), (1, 6, 10, 240), (2, 5, 5, 16)]


def family_inputs(family, B, H, W, C, fold, seed):
    if family == "from_stem":
        x = R.from_stem_x_host(*R.from_stem_case(C, B, H, W, "natural_norm", seed))
    else:
        x = R.make_x(family, B, H, W, C, seed)
    gamma, beta = R.make_affine(C, seed, family)
    return x, R.make_grad(family, x, fold, seed), gamma, beta


def layer64(x, gamma, beta, weight=None):
    """The reference's layer in fp64 torch: GroupNorm(8) -> SiLU (-> reflect pad -> conv), NCHW."""
    a = F.silu(F.group_norm(x.permute(0, 3, 1, 2), 8, gamma, beta, EPS))
    if weight is None:
        return a
    k = weight.shape[-1]
    return F.conv2d(F.pad(a, (k // 2,) * 4, mode="reflect") if k == 3 else a, weight)


# ---- the restatement is the operation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("B,H,W,C", [(2, 6, 7, 48), (1, 2, 2, 16), (2, 3, 5, 128)])
def test_act_backward_restatement_equals_autograd(fold, B, H, W, C):
    x, da, gamma, beta = family_inputs("correlated", B, H, W, C, fold, 3)
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a = layer64(xr, gr, br)
    if fold:
        a = F.pad(a, (1, 1, 1, 1), mode="reflect")
    a.backward(da.double().permute(0, 3, 1, 2))
    r = R.act_bwd_reference(x, da, gamma, beta, EPS, fold)
    # the restatement divides by sqrt(max(var, 0) + eps) from {sum, sum^2}, autograd from the two-pass variance: equal to fp64 rounding of the
    # statistics (the sums of squares cancel to ~1e-13 relative at these magnitudes)
    tol = lambda t: 1e-9 * float(t.abs().max())
    assert float((r["dx"] - xr.grad).abs().max()) <= tol(xr.grad)
    assert float((r["dgamma"] - gr.grad).abs().max()) <= tol(gr.grad) and float((r["dbeta"] - br.grad).abs().max()) <= tol(br.grad)


@pytest.mark.parametrize("k,B,H,W,C", [(3, 2, 5, 6, 16), (1, 1, 4, 7, 32), (3, 1, 2, 2, 16)])
def test_weight_gradient_restatement_equals_autograd(k, B, H, W, C):
    x, dy, gamma, beta = family_inputs("chan_offset", B, H, W, C, False, 5)
    w = torch.zeros(C, C, k, k, dtype=torch.float64, requires_grad=True)
    bb = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    (layer64(x.double(), gamma.double(), beta.double(), w) + bb.view(1, C, 1, 1)).backward(dy.double().permute(0, 3, 1, 2))
    f = R.act_forward(x, gamma, beta, EPS)
    dw, aw, db, adb = R.wgrad_reference(dy, f["a"], k)
    assert float((dw - w.grad).abs().max()) <= 1e-9 * float(w.grad.abs().max()) and float((db - bb.grad).abs().max()) <= 1e-12 * float(adb.max())
    assert bool((aw >= dw.abs() - 1e-12 * aw).all())


@pytest.mark.parametrize("k,H,W", [(3, 5, 6), (1, 4, 3), (3, 2, 2)])
def test_first_convolution_restatement_equals_autograd(k, H, W):
    C, B = 16, 2
    img = O.hash_normal((B, 3, H, W), 7).double().requires_grad_(True)
    w = O.hash_normal((C, 3, k, k), 8).double().requires_grad_(True)
    b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    dy = O.hash_normal((B, H, W, C), 9)
    F.conv2d(F.pad(img, (1,) * 4, mode="reflect") if k == 3 else img, w, b).backward(dy.double().permute(0, 3, 1, 2))
    r = R.conv0_grads_reference(dy, img.detach(), w.detach())
    for got, want in ((r["dw"], w.grad), (r["db"], b.grad), (r["dimage"], img.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("shape,lr", [((1, 128, 6, 8), (2, 4)), ((1, 64, 7, 10), (3, 4)), ((2, 64, 4, 4), (4, 4))])
def test_rope_pool_adjoint_restatement_equals_autograd(shape, lr):
    B, C, H, W = shape
    heads = C // 64
    per = O.rope_periods(C, heads, 100.0).double()
    x = O.hash_normal(shape, 21).double().requires_grad_(True)
    gq, gk = O.hash_normal(shape, 22).double(), O.hash_normal((B, C, *lr), 23).double()
    q = O.rope(x, per, heads)
    ((q * gq).sum() + (O.key_pool(q, lr) * gk).sum()).backward()
    to5 = lambda t: t.reshape(B, heads, 64, *t.shape[-2:]).permute(0, 1, 3, 4, 2)
    dx, a = R.rope_pool_bwd_reference(to5(gq), to5(gk), *R.rope_tables64(per, H, W))
    assert float((dx - x.grad).abs().max()) <= 1e-12 * float(a.max())


@pytest.mark.parametrize("k,H,W", [(3, 5, 6), (1, 4, 5)])
def test_composed_layer_restatement_equals_autograd(k, H, W):
    C, B = 16, 2
    x, g, gamma, beta = family_inputs("correlated", B, H, W, C, False, 31)
    w = S.bf16r(O.hash_normal((C, C, k, k), 32, (C * k * k) ** -0.5))
    xr = x.double().requires_grad_(True)
    layer64(xr, gamma.double(), beta.double(), w.double()).backward(g.double().permute(0, 3, 1, 2))
    r, bound = R.layer_reference(x, g, gamma, beta, EPS, w, R.act_bwd_chain(H, W, C))
    assert float((r["dx"] - xr.grad).abs().max()) <= 1e-9 * float(xr.grad.abs().max()) and bool((bound > 0).all())


# ---- the emulation stays inside, the defects leave ------------------------------------------------------------------------------------
def act_case(family, shape, fold, **defect):
    B, H, W, C = shape
    x, da, gamma, beta = family_inputs(family, B, H, W, C, fold, 100 + H + C)
    r = R.act_bwd_reference(x, da, gamma, beta, EPS, fold)
    b = R.act_bwd_bounds(r, R.act_bwd_chain(H, W, C))
    dx, sums = R.act_bwd_emulated(x, da, gamma, beta, EPS, fold, **defect)
    return (dx - r["dx"]).abs(), b["dx"], (sums - r["sums"]).abs(), b["sums"]


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=str)
@pytest.mark.parametrize("family", HOST_FAMILIES)
def test_act_backward_emulation_inside_every_bound(family, shape, fold):
    e_dx, b_dx, e_s, b_s = act_case(family, shape, fold)
    S.check(e_dx, b_dx, f"dx {family} {shape} fold={fold}")
    S.check(e_s, b_s, f"sums {family} {shape} fold={fold}")


def leaves(err, bound):
    return bool((err > bound).any())


@pytest.mark.parametrize("family", ["correlated", "chan_offset", "from_stem"])
def test_scaled_mean_leaves_the_bound(family):
    e, b, _, _ = act_case(family, ACT_SHAPES[0], True, m1_scale=0.9)
    assert leaves(e, b)


def test_scaled_mean_hides_in_the_norm_on_iid_inputs():
    """What the whole-tensor norm of tests/test_gpu_train_stem.py cannot see: on i.i.d. inputs the planted 10 % error of mean(dxhat) moves dx by
    less than that test's 6e-3."""
    B, H, W, C = ACT_SHAPES[0]
    x, da, gamma, beta = family_inputs("iid", B, H, W, C, False, 100 + H + C)
    r = R.act_bwd_reference(x, da, gamma, beta, EPS, False)
    dx, _ = R.act_bwd_emulated(x, da, gamma, beta, EPS, False, m1_scale=0.9)
    assert float((dx - r["dx"]).norm() / r["dx"].norm()) < 6e-3


@pytest.mark.parametrize("shape", [ACT_SHAPES[1], ACT_SHAPES[2]], ids=str)      # widths 48 and 240: a chunk of 8 channels straddles groups
@pytest.mark.parametrize("fold", [False, True])
def test_neighbouring_groups_means_leave_the_bound(shape, fold):
    e, b, _, _ = act_case("correlated", shape, fold, wrong_group=True)
    assert leaves(e, b)
    C = shape[-1]
    last = torch.arange(C) % (C // 8) == C // 8 - 1
    assert not leaves(e[..., ~last], b[..., ~last])                             # and only the channels that read the wrong means


@pytest.mark.parametrize("skip,pixel", [((0, 0), (1, 1)), ((0, 6), (1, 5)), ((5, 0), (4, 1)), ((13, 7), (10, 6))])
def test_missing_mirrored_contribution_leaves_the_bound_at_its_pixel(skip, pixel):
    """One element of the padded border not folded back: the corner pixel (1, 1) loses padded (0, 0); edge pixels lose their one mirror."""
    e, b, _, _ = act_case("correlated", ACT_SHAPES[0], True, skip=skip)
    over = (e > b).any(-1).any(0)
    assert bool(over[pixel])


@pytest.mark.parametrize("family", ["correlated", "chan_offset", "outlier", "iid"])
@pytest.mark.parametrize("k,B,H,W,C", [(3, 2, 9, 14, 48), (1, 1, 7, 19, 128), (3, 1, 6, 33, 144)])
def test_weight_gradient_emulation_inside_the_bound_and_a_shifted_tap_outside(family, k, B, H, W, C):
    x, dy, gamma, beta = family_inputs(family, B, H, W, C, False, 200 + W)
    f = R.act_forward(x, gamma, beta, EPS)
    dw, aw, db, adb = R.wgrad_reference(dy, f["a"], k)
    b_dw, b_db = R.wgrad_bounds(dy, aw, adb, k, f)
    e_dw, e_db = R.wgrad_emulated(dy, x, gamma, beta, EPS, k)
    S.check((e_dw - dw).abs(), b_dw, f"dW {family}")
    S.check((e_db - db).abs(), b_db, f"db {family}")
    if family == "correlated":
        tap = (k // 2, k - 1)
        bad, _ = R.wgrad_emulated(dy, x, gamma, beta, EPS, k, shift_tap=tap)
        err = (bad - dw).abs()
        assert leaves(err[:, :, tap[0], tap[1]], b_dw[:, :, tap[0], tap[1]])
        keep = torch.ones(k, k, dtype=torch.bool)
        keep[tap] = False
        assert not leaves(err[:, :, keep], b_dw[:, :, keep])


# ---- the exact census ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("mult", [0.0, 2.0])
def test_census_notices_one_piece_and_names_its_pixel(k, mult):
    """a == 1 and bit-coded dy: dW and d bias are pixel counts.  One 8-channel piece of ONE pixel of ``a`` dropped (x 0) or doubled (x 2) changes the
    integers, and the decode names that pixel and that piece."""
    B, H, W, C = 2, 9, 37, 128
    dy, counts, nbits = R.census_dy(B, H, W, C)
    a = torch.ones(B, H, W, C)
    want = counts.view(C, 1, 1, 1).expand(C, C, k, k)
    dw, _, db, _ = R.wgrad_reference(dy, a, k)
    assert torch.equal(dw.long(), want) and torch.equal(db.long(), counts) and float(dw.max()) < 2 ** 24
    assert R.census_decode(dw.long() - want, nbits, (B, H, W)) == "nothing lost"
    b, y, x, piece = 1, 4, 20, 5
    a[b, y, x, 8 * piece: 8 * piece + 8] = mult
    dw, _, _, _ = R.wgrad_reference(dy, a, k)
    diff = dw.long() - want
    assert bool((diff != 0).any())
    said = R.census_decode(diff, nbits, (B, H, W))
    assert f"a pixel (b {b}, y {y}, x {x})" in said and f"input [{piece}]" in said and said.startswith("lost" if mult == 0.0 else "doubled"), said


def test_census_pass_b_tells_the_taps_apart():
    """dy == 1 and a = bits of the column / row index: the nine taps of a channel differ exactly through the reflected border, so a tap that reads a
    neighbour's pixels (here: shifted by one) changes the integers."""
    B, H, W, C = 1, 9, 37, 32
    a = R.census_a(B, H, W, C)
    want = R.census_a_counts(a, 3)
    assert len({tuple(want[:, t // 3, t % 3].tolist()) for t in range(9)}) == 9
    dw, _, _, _ = R.wgrad_reference(torch.ones(B, H, W, 1), a, 3, shift_tap=(1, 2))
    assert not torch.equal(dw[0].round().long(), want)


def test_census_shapes_reach_every_class_of_the_launcher():
    plans = [R.wgrad_plan(k, B, H, W, 256) for k, B, H, W in R.WGRAD_CENSUS_SHAPES]
    for name, cond in R.WGRAD_CLASSES.items():
        assert any(cond(p) for p in plans), name
    assert all(H * W <= R.PIXEL_CAP for _, B, H, W in R.WGRAD_CENSUS_SHAPES)
    assert all(R.wgrad_class_reachable(name, 256) for name in R.WGRAD_CLASSES)
    assert not R.wgrad_class_reachable("pipelined: even segments per workgroup", 10 ** 6)   # a device with more CUs than segments: one segment each


# ---- the first convolution, the RoPE adjoint and the composed layer: host emulations inside their bounds -----------------------------------
@pytest.mark.parametrize("family", ["natural_norm", "natural_255", "hot_pixel", "unit"])
@pytest.mark.parametrize("k,mfma", [(3, True), (1, True), (3, False), (1, False)])
def test_first_convolution_emulation_inside_the_bounds(family, k, mfma):
    """fp32 sums, and for the matrix-pipe kernel the image as bf16 hi + bf16 lo: inside (B H W 2^-24 + 2^-16) abs-sum; the hi part ALONE is not."""
    B, H, W, C = 2, 9, 37, 32
    img = S.make_image(B, H, W, family, 81)
    dy = R.make_grad("chan_offset", torch.zeros(B, H, W, C), False, 82)
    w = O.hash_normal((C, 3, k, k), 83, (3 * k * k) ** -0.5)
    r = R.conv0_grads_reference(dy, img, w)
    b = R.conv0_bounds(r, dy, True, mfma)
    dw, db, dimg = R.conv0_grads_emulated(dy, img, w, mfma)
    S.check((dw - r["dw"]).abs(), b["dw"], f"dW0 {family}")
    S.check((db - r["db"]).abs(), b["db"], f"db0 {family}")
    S.check((dimg - r["dimage"]).abs(), b["dimage"], f"dimage {family}")
    if mfma and family != "natural_255":                       # integers up to 255 are bf16 hi + lo exactly; hi alone is not
        hi_only, _, _, _ = R.wgrad_reference(dy, S.bf16r(img.permute(0, 2, 3, 1)), k)
        assert leaves((hi_only - r["dw"]).abs(), b["dw"])


@pytest.mark.parametrize("shape,lr", [((1, 128, 12, 16), (3, 4)), ((1, 64, 7, 10), (3, 4))])
def test_rope_pool_adjoint_emulation_inside_the_bound(shape, lr):
    B, C, H, W = shape
    heads = C // 64
    ty, tx = (t.float() for t in R.rope_tables64(O.rope_periods(C, heads, 100.0), H, W))
    to5 = lambda t: t.reshape(B, heads, 64, *t.shape[-2:]).permute(0, 1, 3, 4, 2)
    gq, gk = to5(S.bf16r(O.hash_normal(shape, 21) + 0.5)), to5(O.hash_normal((B, C, *lr), 22) * 4.0 + 1.0)
    ref, a = R.rope_pool_bwd_reference(gq, gk, ty, tx)
    emu, _ = R.rope_pool_bwd_reference(gq, gk, ty, tx, dtype=torch.float32)
    S.check((R.r16(emu) - ref).abs(), R.rope_pool_bwd_bound(ref, a), "rope adjoint")
    wrong, _ = R.rope_pool_bwd_reference(gq, gk, ty, -tx)                      # the rotation by the POSITIVE angle along x leaves it
    assert leaves((wrong - ref).abs(), R.rope_pool_bwd_bound(ref, a))


@pytest.mark.parametrize("k,H,W,C", [(3, 12, 20, 128), (1, 9, 17, 128), (3, 5, 33, 48)])
def test_composed_layer_emulation_inside_the_bound(k, H, W, C):
    x, g, gamma, beta = family_inputs("correlated", 2, H, W, C, False, 500 + W)
    w = S.bf16r(O.hash_normal((C, C, k, k), 501, (C * k * k) ** -0.5))
    r, bound = R.layer_reference(x, g, gamma, beta, EPS, w, R.act_bwd_chain(H, W, C))
    S.check((R.layer_emulated(x, g, gamma, beta, EPS, w) - r["dx"]).abs(), bound, f"composed k{k}")
