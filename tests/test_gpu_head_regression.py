"""GPU tests (-m gpu) of the fused dense regression probe: the regression epilogue of the head-summed attention kernel
(naf_xna_head_reg_fwd: per-pixel L1 / MSE / smooth-L1 loss, its gradient and the error sums of depth evaluation, without the logits
tensor), ``ops.XnaHeadRegFunction`` and ``naf(image, feats, size, head=probe, dense_target=t, valid=m)`` end to end.

Tolerances.
  A. One launch against itself -- the same launch also stores its fp32 logits L, so nothing has to be invented:
     * L is bit-equal to naf_xna_head_fwd's fp32 logits (same accumulators);
     * the loss map against the fp64 restatement on L (tests/head_regression_reference.py): within (N + 4) * 2^-24 * sum_n term_n + 1e-30 --
       one rounding for r = z - t, at most two per term (r * r; 0.5 r r / beta: a product and a quotient), N - 1 additions.  Invalid: exactly 0;
     * g[..., :N]: L1 bit-equal to sign(L - t) in bf16; MSE bit-equal to (2 * (L - t)).bfloat16() in fp32 torch arithmetic; smooth-L1 within
       2^-8 |ref| + 1e-30 (one rounding of r, one of the quotient, one to bf16).  Pad channels and invalid pixels exactly zero.
  B. Statistics (N = 1) against the restatement on L: the count exact; the threshold counts between the restatement's counts at
     1.25^k (1 -+ 2^-20) (the kernel's ratio carries two fp32 divisions, 2^-23 relative); sums 1-4 within 72 * 2^-24 * sum |term| (a chain
     of at most 64 fp32 additions plus the per-term roundings: the kernel's chain is 6); sums 5 and 6 -- with S = |ln p| + |ln t|, each
     logarithm within 2 ulp (2^-22 |ln x|, the library's logf), d = fl(ln p - ln t) within 2^-22 S + 2^-24 |d| <= 5 * 2^-24 S of exact, a
     chain of at most 64 additions on terms |d| <= S: sum d within (5 + 64) * 2^-24 sum S, stated as 72 * 2^-24 sum S; d^2 moves by
     2 |d| * 5 * 2^-24 S + 2^-24 d^2 <= 11 * 2^-24 S^2, plus the chain: 80 * 2^-24 sum S^2.
  C. Gradients: g is held by A; given g, the backward is naf_xna_bwd with one dout shared by the heads, under
     test_ce_function_gradients_match_oracle's own bound, unchanged.
  D. Module level: the loss against the torch expression in fp64 on the parent path's logits -- the same kernel arithmetic, so what
     remains is A's per-pixel bound and the fp32 reduction of the map, bounded for ANY order of n additions by n * 2^-24 * sum |term|;
     the probe's gradients: fused error <= 2 * (error of the composed route: the torch loss on the logits call) + 2^-8 max|ref|, the
     bound of the module-level objective test.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_regression_reference as R  # noqa: E402
import layout_contract as LC  # noqa: E402
from test_gpu_parity import bf16r, oracle_xna_backward, to5  # noqa: E402
from test_gpu_head import HEAD_GEOMS, _load_model, _probe, make_pv, npad_of, xna_row_tiles_ok  # noqa: E402
from test_gpu_head_objective import CC, KSZ, LABEL_GEOM, LR, SIZE, _module_setup, make_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


BETA = 0.4
REG_CASES = [
    # (geometry, N, mask mode, channels-last target)
    ((1, 5, 5, 3, 30, 3, 256, 4), 1, "tenth", False),          # window 3, a full and a 14-pixel tile per row, one output
    ((1, 6, 7, 14, 14, 5, 192, 4), 2, "none", False),          # window 5, 14 x 14 cells: partial row tiles, no mask
    (LABEL_GEOM, 3, "row", True),                              # window 7, one image row invalid, the target a view of [B, Ho, Wo, N] memory
    ((1, 9, 9, 7, 15, 9, 1024, 4), 32, "tenth", False),        # window 9, 15-pixel rows, every channel of the two tiles
    ((1, 12, 13, 2, 16, 11, 0, 3), 17, "tenth", False),        # window 11, three heads, the second channel tile partly used
    ((1, 14, 13, 1, 16, 13, 0, 1), 3, "none", False),          # window 13, one head, one-row cells
    ((1, 16, 15, 3, 32, 15, 0, 2), 2, "tenth", False),         # window 15
    ((1, 7, 8, 32, 16, 7, 0, 6), 1, "all", False),             # 32 x 16 cells: two rounds per workgroup; every pixel invalid
    ((2, 9, 9, 14, 14, 9, 0, 12), 17, "tenth", True),          # two images, twelve heads, patch-14 cells
]


def test_cases_cover_every_window_and_tile_count():
    assert all(g in HEAD_GEOMS or g == LABEL_GEOM for g, *_ in REG_CASES) and all(xna_row_tiles_ok(g[4]) for g, *_ in REG_CASES)
    assert {c[0][5] for c in REG_CASES} == {3, 5, 7, 9, 11, 13, 15}
    assert {1, 2, 3, 17, 32} == {c[1] for c in REG_CASES}
    assert {14, 15, 30} <= {c[0][4] for c in REG_CASES}                              # partial row tiles
    assert any(c[0][3] * ((c[0][4] + 15) // 16) > 16 for c in REG_CASES)             # more tiles than a round takes
    assert (1, 7, 8, 32, 16, 7, 0, 6) in [c[0] for c in REG_CASES]
    assert {1, 2} == {c[0][0] for c in REG_CASES} and {1, 3, 12} <= {c[0][7] for c in REG_CASES}
    assert {"none", "tenth", "row", "all"} == {c[2] for c in REG_CASES}
    assert any(c[3] for c in REG_CASES)


def _case_inputs(geom, N, mode, cl, dev):
    B, h, w, dy, dx, ksz, _, heads = geom
    Ho, Wo = h * dy, w * dx
    s = sum(geom) + N
    _, dv = make_inputs(geom, N, (s + 1, s + 2, s + 3, s + 4), dev)
    t = R.dense_target(B, N, Ho, Wo, s + 5, channels_last=cl).to(dev)
    assert t.is_contiguous() != cl or N == 1
    valid = R.make_valid(B, Ho, Wo, mode)
    return dv, t, (None if valid is None else valid.to(dev))


@pytest.mark.parametrize("geom,N,mode,cl", REG_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_one_launch_against_itself(dev, geom, N, mode, cl):
    """A of the module docstring, for the three losses."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, _, heads = geom
    Ho, Wo = h * dy, w * dx
    (q5, k5, pv5, bd), t, valid = _case_inputs(geom, N, mode, cl, dev)
    fwd = ops.xna_head_forward(q5, k5, pv5, bd, ksz, n_out=N, out_dtype=torch.float32, path="fused")
    gc = ops.head_dlogits_channels(N)
    ok = torch.ones(B, Ho, Wo, dtype=torch.bool, device=dev) if valid is None else valid
    assert (int(ok.sum()) == 0) == (mode == "all")
    if mode == "row":
        assert not bool(ok[:, 5].any())
    if valid is not None:                      # what lies under an invalid pixel reaches nothing
        t = torch.where(ok.unsqueeze(1), t, torch.full_like(t, float("nan")))
    for kind in R.KINDS:
        kw = dict(n_out=N, target=t, valid=valid, kind=kind, beta=BETA, path="fused")
        loss, g, L = ops.xna_head_regression(q5, k5, pv5, bd, ksz, want_loss=True, want_dlogits=True, return_logits=True, **kw)
        assert loss.dtype == torch.float32 and tuple(loss.shape) == (B, Ho, Wo)
        assert g.dtype == torch.bfloat16 and tuple(g.shape) == (B, Ho, Wo, gc) and g.is_contiguous() and gc == 32 >= npad_of(N)
        assert L.dtype == torch.float32 and tuple(L.shape) == (B, N, Ho, Wo)
        assert torch.equal(L, fwd), "the logits of the regression launch differ from naf_xna_head_fwd's"
        ref_l, ref_mag, ref_g = R.restate(L, t, valid, kind, BETA)
        err = (loss.double() - ref_l).abs()
        tol = (N + 4) * U * ref_mag + 1e-30
        print(f"self {geom} N={N} {mode} {kind}: loss max err / tol {float((err / tol).max()):.3f}")
        assert not bool((err > tol).any()), f"{kind} loss: max err {float(err.max()):.3e}"
        if bool((~ok).any()):
            assert float(loss[~ok].abs().sum()) == 0.0
        r32 = torch.where(ok.unsqueeze(1), L - t, torch.zeros_like(L)).permute(0, 2, 3, 1)
        if kind == "l1":
            assert torch.equal(g[..., :N], torch.sign(r32).bfloat16()), "L1: g is not sign(L - t)"
        elif kind == "mse":
            assert torch.equal(g[..., :N], (2 * r32).bfloat16()), "MSE: g is not (2 * (L - t)) rounded once"
        else:
            eg = (g[..., :N].double() - ref_g).abs()
            tg = 2.0 ** -8 * ref_g.abs() + 1e-30
            print(f"    g max err / tol {float((eg / tg).max()):.3f}")
            assert not bool((eg > tg).any()), f"smooth-L1 g: max err {float(eg.max()):.3e}"
        if gc > N:
            assert float(g[..., N:].float().abs().max()) == 0.0, "pad channels of g are not zero"
        if bool((~ok).any()):
            assert float(g[~ok].float().abs().max()) == 0.0, "invalid pixels carry a gradient"
        # each output requested alone: the NULL branches change nothing
        a1 = ops.xna_head_regression(q5, k5, pv5, bd, ksz, want_loss=True, **kw)
        assert torch.equal(a1[0], loss) and a1[1] is None and a1[2] is None
        a2 = ops.xna_head_regression(q5, k5, pv5, bd, ksz, want_dlogits=True, **kw)
        assert LC.same_bits(a2[1], g) and a2[0] is None
        a3 = ops.xna_head_regression(q5, k5, pv5, bd, ksz, n_out=N, return_logits=True, path="fused")            # no target
        assert torch.equal(a3[2], L)
    # the composition has the same contract
    c = ops.xna_head_regression(q5, k5, pv5, bd, ksz, n_out=N, target=t, valid=valid, kind="smooth_l1", beta=BETA, want_loss=True,
                                want_dlogits=True, return_logits=True, path="composed")
    assert c[0].dtype == loss.dtype and c[0].shape == loss.shape and c[1].dtype == g.dtype and c[1].shape == g.shape and c[2].shape == L.shape
    assert float(c[1][..., N:].float().abs().sum()) == 0.0
    if bool((~ok).any()):
        assert float(c[0][~ok].abs().sum()) == 0.0 and float(c[1][~ok].float().abs().sum()) == 0.0
    assert bool(torch.isfinite(c[0]).all())


def test_fused_path_refuses_more_than_32_outputs_and_auto_composes(dev):
    from naf_amd import ops
    from naf_amd._lib import NafHipError
    geom, N = LABEL_GEOM, 33
    (q5, k5, pv5, bd), t, valid = _case_inputs(geom, N, "tenth", False, dev)
    with pytest.raises(NafHipError, match="N <= 32"):
        ops.xna_head_regression(q5, k5, pv5, bd, 7, n_out=N, target=t, valid=valid, want_loss=True, path="fused")
    loss, g, L = ops.xna_head_regression(q5, k5, pv5, bd, 7, n_out=N, target=t, valid=valid, kind="mse", want_loss=True, want_dlogits=True,
                                         return_logits=True)
    assert torch.equal(L, ops.xna_head_forward(q5, k5, pv5, bd, 7, n_out=N, out_dtype=torch.float32))
    ref_l, ref_mag, _ = R.restate(L, t, valid, "mse")
    assert bool(((loss.double() - ref_l).abs() <= (N + 4) * U * ref_mag + 1e-30).all())
    assert tuple(g.shape) == (1, 128, 128, 64) and float(g[..., N:].float().abs().sum()) == 0.0
    with pytest.raises(ValueError, match="one output"):
        ops.xna_head_regression(q5, k5, pv5, bd, 7, n_out=N, target=t, errors=torch.zeros(10, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="nothing asked"):
        ops.xna_head_regression(q5, k5, pv5, bd, 7, n_out=N, target=t)
    with pytest.raises(ValueError, match="need a target"):
        ops.xna_head_regression(q5, k5, pv5, bd, 7, n_out=N, want_loss=True)


# ---- B: the error statistics -----------------------------------------------------------------------------------------------------
STATS_CASES = [
    (LABEL_GEOM, "tenth"),                                     # one round per workgroup
    ((1, 7, 8, 32, 16, 7, 0, 6), "none"),                      # two rounds per workgroup: the waves' sums carry over
    ((2, 9, 9, 14, 14, 9, 0, 12), "row"),                      # partial tiles: repeated last pixels must not be counted; two images
]


@pytest.mark.parametrize("geom,mode", STATS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_error_statistics_against_the_restatement(dev, geom, mode):
    """B of the module docstring."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, _, heads = geom
    Ho, Wo = h * dy, w * dx
    s = sum(geom)
    _, (q5, k5, pv5, bd) = make_inputs(geom, 1, (s + 11, s + 12, s + 13, s + 14), dev)
    bd = torch.ones_like(bd)                           # logits around 1: on both sides of both clamp bounds
    t = R.stats_target(B, Ho, Wo, s + 15).to(dev)
    valid = R.make_valid(B, Ho, Wo, mode)
    valid = None if valid is None else valid.to(dev)
    clamp = R.STATS_CLAMP
    acc = torch.zeros(10, dtype=torch.float64, device=dev)
    kw = dict(n_out=1, target=t, valid=valid, clamp=clamp, path="fused")
    _, _, L = ops.xna_head_regression(q5, k5, pv5, bd, ksz, errors=acc, return_logits=True, **kw)
    z, tt = L[:, 0], t[:, 0]
    assert bool((z < clamp[0]).any()) and bool((z > clamp[1]).any()) and bool(((z > clamp[0]) & (z < clamp[1])).any())
    for bad in (tt == 0, tt < 0, torch.isinf(tt), torch.isnan(tt)):
        assert bool(bad.any())
    ref, mags, S1, S2 = R.error_sums(z, tt, valid, clamp)
    widths, n = R.bracket_widths(z, tt, valid, clamp)
    print(f"stats {geom} {mode}: counted {n:.0f} of {B * Ho * Wo}; bracket widths {[hi - lo for lo, hi in widths]}")
    assert 0 < n < B * Ho * Wo and all(hi - lo < 0.01 * n for lo, hi in widths), "the inputs put too many ratios on a threshold"
    got = acc.cpu()
    ref, mags = ref.cpu(), mags.cpu()
    assert float(got[0]) == float(ref[0]) == n, f"count {float(got[0])} vs {float(ref[0])}"
    for i, (lo, hi) in enumerate(widths):
        assert lo <= float(got[7 + i]) <= hi, f"threshold {i}: {float(got[7 + i])} outside [{lo}, {hi}]"
    for i in (1, 2, 3, 4):
        err, tol = abs(float(got[i] - ref[i])), 72 * U * float(mags[i])
        print(f"    sum {i}: err / tol {err / tol:.4f}")
        assert err <= tol, f"sum {i}: err {err:.3e} tol {tol:.3e}"
    for i, tol in ((5, 72 * U * float(S1)), (6, 80 * U * float(S2))):
        err = abs(float(got[i] - ref[i]))
        print(f"    sum {i}: err / tol {err / tol:.4f}")
        assert err <= tol, f"sum {i}: err {err:.3e} tol {tol:.3e}"
    # the composed route holds the same definitions
    comp = torch.zeros(10, dtype=torch.float64, device=dev)
    Lc = ops.xna_head_regression(q5, k5, pv5, bd, ksz, errors=comp, return_logits=True, **{**kw, "path": "composed"})[2]
    refc = R.error_sums(Lc[:, 0], tt, valid, clamp)[0].cpu()          # on the composition's own logits (another kernel's arithmetic)
    assert float((comp.cpu() - refc).abs().max()) <= 1e-9 * float(refc.abs().max())
    # bit-reproducible, accumulating, and untouched by a call without a counted pixel
    again = torch.zeros(10, dtype=torch.float64, device=dev)
    ops.xna_head_regression(q5, k5, pv5, bd, ksz, errors=again, **kw)
    assert torch.equal(again, acc)
    ops.xna_head_regression(q5, k5, pv5, bd, ksz, errors=again, **kw)
    assert torch.equal(again, 2 * acc)
    before = LC.bits(again).clone()
    nothing = torch.zeros(B, Ho, Wo, dtype=torch.bool, device=dev)
    ops.xna_head_regression(q5, k5, pv5, bd, ksz, errors=again, **{**kw, "valid": nothing})
    assert torch.equal(LC.bits(again), before)
    # the loss map and the statistics of one launch are those of the separate launches
    both = torch.zeros(10, dtype=torch.float64, device=dev)
    l1 = ops.xna_head_regression(q5, k5, pv5, bd, ksz, errors=both, want_loss=True, **kw)[0]
    assert torch.equal(both, acc) and LC.same_bits(l1, ops.xna_head_regression(q5, k5, pv5, bd, ksz, want_loss=True, **kw)[0])


# ---- C: the gradient to the head -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,heads,lr,out_sz,ksz,N,kind", [
    (1, 4, (8, 8), (128, 128), 7, 3, "l1"),               # the cell backward at Dv = 32
    (1, 4, (12, 10), (168, 140), 9, 17, "smooth_l1"),     # patch 14: partial row tiles
])
def test_reg_function_gradients_match_oracle(dev, B, heads, lr, out_sz, ksz, N, kind):
    """C: test_ce_function_gradients_match_oracle with the regression launch's g in the place of softmax - onehot: dPV of
    ops.XnaHeadRegFunction(reduction="sum") against the oracle's backward fed g[..., :N] read back from the kernel, under that test's bound;
    pad channels exactly 0; dbias against the fp64 sum of g; "mean" = "sum" / (valid pixels * N) within two fp32 roundings; "none"."""
    from naf_amd import ops
    npad = npad_of(N)
    q = bf16r(O.hash_normal((B, 64 * heads, *out_sz), 501))
    k = bf16r(O.hash_normal((B, 64 * heads, *lr), 502))
    pv, pvn = make_pv(B, heads, *lr, N, 503)
    t = R.dense_target(B, N, *out_sz, 506).to(dev)
    valid = R.make_valid(B, *out_sz, "row").to(dev)
    q5, k5 = to5(q, heads).to(dev), to5(k, heads).to(dev)
    pv5 = pv.to(dev).to(torch.bfloat16).requires_grad_(True)
    bias = O.hash_normal((N,), 505).to(dev).requires_grad_(True)
    loss = ops.XnaHeadRegFunction.apply(q5, k5, pv5, bias, t, valid, ksz, N, kind, BETA, "sum")
    assert loss.requires_grad and loss.dim() == 0 and loss.dtype == torch.float32 and not q5.requires_grad
    loss.backward()
    g = ops.xna_head_regression(q5, k5, pv5.detach(), bias.detach(), ksz, n_out=N, target=t, valid=valid, kind=kind, beta=BETA, want_dlogits=True)[1]
    dout = g[..., :N].float().permute(0, 3, 1, 2).cpu()
    d5 = torch.zeros(B, heads, npad, *out_sz)
    d5[:, :, :N] = dout[:, None]
    _, _, rv = oracle_xna_backward(dev, q, k, pvn, d5.reshape(B, heads * npad, *out_sz), ksz, heads)
    ref = rv.view(B, heads, npad, *lr).permute(0, 1, 3, 4, 2)
    got = pv5.grad.float().cpu()
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    print(f"reg dPV k={ksz} N={N} {kind}: max err {float(err.max()):.3e} mean {float(err.mean()):.3e} (ref max {scale:.3e})")
    assert float(err.max()) <= 2e-2 * scale + 1e-3 and float(err.mean()) <= 3e-3 * scale + 1e-4, \
        f"dPV: max err {float(err.max()):.3e} mean {float(err.mean()):.3e} (ref max {scale:.3e})"
    assert float(got[..., N:].abs().max()) == 0.0 if npad > N else True
    rb = dout.double().sum(dim=(0, 2, 3))
    eb = float((bias.grad.double().cpu() - rb).abs().max())
    nterm = B * out_sz[0] * out_sz[1]
    assert eb <= nterm * U * float(dout.abs().max()), f"dbias err {eb:.3e}"
    # "mean": the "sum" result times 1 / (valid pixels * N)
    db_sum, loss_sum = bias.grad.double().clone(), loss.detach().double()
    bias.grad = None
    pv5.grad = None
    lm = ops.XnaHeadRegFunction.apply(q5, k5, pv5, bias, t, valid, ksz, N, kind, BETA, "mean")
    lm.backward()
    count = float(valid.sum()) * N
    assert abs(float(lm.detach().double()) * count - float(loss_sum)) <= 2.0 ** -22 * abs(float(loss_sum))
    assert bool(((bias.grad.double() * count - db_sum).abs() <= 2.0 ** -22 * db_sum.abs() + 1e-30).all())
    sm = float((pv5.grad.float().cpu() * count - got).abs().max())
    assert sm <= 2e-2 * scale + 1e-3          # atomics in the backward: the two runs add in different orders, no bit equality
    # "none": a map, and a map of incoming gradients
    pv5.grad = None
    bias.grad = None
    ln = ops.XnaHeadRegFunction.apply(q5, k5, pv5, bias, t, valid, ksz, N, kind, BETA, "none")
    assert tuple(ln.shape) == (B, *out_sz) and abs(float(ln.detach().double().sum()) - float(loss_sum)) <= 1e-5 * abs(float(loss_sum))
    ln.sum().backward()
    assert float((bias.grad.double() - db_sum).abs().max()) <= nterm * U * float(dout.abs().max())


# ---- D: module level -------------------------------------------------------------------------------------------------------------
def _torch_loss(kind):
    return {"l1": F.l1_loss, "mse": F.mse_loss, "smooth_l1": lambda a, b, reduction="mean": F.smooth_l1_loss(a, b, reduction=reduction, beta=BETA)}[kind]


@pytest.mark.parametrize("N,kind", [(1, "l1"), (3, "smooth_l1"), (3, "mse")])
def test_module_regression_matches_the_torch_expression_and_trains_the_probe(dev, N, kind):
    """D of the module docstring."""
    p, img, ft, up = _module_setup()
    m = _load_model(dev, p, kernel_size=KSZ)
    conv, conv_par = _probe(CC, N, 603, dev), _probe(CC, N, 603, dev)
    t = R.dense_target(1, N, *SIZE, 640 + N)
    valid = R.make_valid(1, *SIZE, "tenth")
    sel = valid.unsqueeze(1).expand_as(t)
    fn = _torch_loss(kind)
    w64 = conv.weight.detach().cpu().double().requires_grad_(True)
    b64 = conv.bias.detach().cpu().double().requires_grad_(True)
    ref = fn(F.conv2d(up, w64, b64)[sel], t.double()[sel])
    ref.backward()
    imgd, ftd, td, vd = img.to(dev), ft.to(dev).to(torch.bfloat16), t.to(dev), valid.to(dev)
    kw = dict(head=conv, dense_target=td, valid=vd, dense_loss=kind, beta=BETA)
    loss = m(imgd, ftd, SIZE, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward()
    assert all(q.grad is None for q in m.parameters()), "the frozen upsampler received a gradient"
    seld = vd.unsqueeze(1).expand_as(td)
    par = fn(m(imgd, ftd, SIZE, head=conv_par).float()[seld], td[seld])
    par.backward()
    for name, got, parent, rf in (("loss", loss.detach().cpu().double(), par.detach().cpu().double(), ref.detach()),
                                  ("weight grad", conv.weight.grad.cpu().double(), conv_par.weight.grad.cpu().double(), w64.grad),
                                  ("bias grad", conv.bias.grad.cpu().double(), conv_par.bias.grad.cpu().double(), b64.grad)):
        e_f, e_p, scale = float((got - rf).abs().max()), float((parent - rf).abs().max()), float(rf.abs().max())
        print(f"module regression N={N} {kind} {name}: fused err {e_f:.3e}, composed-route err {e_p:.3e}, ref max {scale:.3e}")
        assert e_f <= 2.0 * e_p + 2.0 ** -8 * scale, f"{name}: fused err {e_f:.3e} vs composed {e_p:.3e} (ref max {scale:.3e})"
    # without a gradient: the three reductions against the torch expression in fp64 on the parent path's logits, and the prediction
    with torch.no_grad():
        logits = m(imgd, ftd, SIZE, head=conv)
        mean, pred = m(imgd, ftd, SIZE, predict=True, **kw)
        total = m(imgd, ftd, SIZE, reduction="sum", **kw)
        lmap = m(imgd, ftd, SIZE, reduction="none", **kw)
        g = m.guide(imgd)
        gmean, gpred = m(g, ftd, SIZE, predict=True, **kw)
    assert torch.equal(pred, logits) and pred.dtype == torch.float32 and tuple(pred.shape) == (1, N, *SIZE) and not pred.requires_grad
    assert torch.equal(gmean, mean) and torch.equal(gpred, pred), "the Guidance call differs from the image call"
    assert not mean.requires_grad and abs(float(mean) - float(loss.detach())) <= 1e-5 * (1.0 + abs(float(loss.detach())))
    ref_map, ref_mag, _ = R.restate(logits, td, vd, kind, BETA)
    assert tuple(lmap.shape) == (1, *SIZE) and float(lmap[~vd].abs().sum()) == 0.0
    assert bool(((lmap.double() - ref_map).abs() <= (N + 4) * U * ref_mag + 1e-30).all())
    n_el, n_px = float(vd.sum()) * N, SIZE[0] * SIZE[1]
    e64 = fn(logits.double()[seld], td.double()[seld], reduction="sum")
    tol = (N + 4 + n_px) * U * float(ref_mag.sum())           # A's per-pixel bound, then n_px fp32 additions in any order
    print(f"    sum err / tol {abs(float(total) - float(e64)) / tol:.4f}, mean err / tol {abs(float(mean) * n_el - float(e64)) / (tol + 2 * U * float(e64)):.4f}")
    assert abs(float(total) - float(e64)) <= tol
    assert abs(float(mean) * n_el - float(e64)) <= tol + 2 * U * abs(float(e64))          # ... one division, one rounding of the count product


def test_module_regression_routes_errors_and_edge_cases(dev):
    """D: N = 33 composes; the unfused route when the upsampler wants a gradient; ``errors=`` accumulates over batches, in place of the
    loss; an all-invalid mask; an empty batch; other float dtypes of the target."""
    p = O.make_params(seed=32)
    m = _load_model(dev, p, kernel_size=7)
    size = (96, 128)
    img, ft = O.hash_normal((2, 3, *size), 611).to(dev), O.hash_normal((2, 128, 8, 8), 612).to(dev).to(torch.bfloat16)
    valid = R.make_valid(2, *size, "tenth").to(dev)
    # N = 33: the kernel refuses, "auto" composes; the probe trains there too
    conv33 = _probe(128, 33, 613, dev)
    t33 = R.dense_target(2, 33, *size, 614).to(dev)
    sel = valid.unsqueeze(1).expand_as(t33)
    l33 = m(img, ft, size, head=conv33, dense_target=t33, valid=valid, dense_loss="mse")
    with torch.no_grad():
        z33 = m(img, ft, size, head=conv33)
    ref33 = F.mse_loss(z33.double()[sel], t33.double()[sel])
    assert abs(float(l33.detach()) - float(ref33)) <= 1e-5 * float(ref33)
    l33.backward()
    assert conv33.weight.grad is not None and float(conv33.weight.grad.abs().sum()) > 0
    # a gradient for the features: the unfused composition on forward_train, the same value up to the two paths' arithmetic
    conv = _probe(128, 1, 615, dev)
    t = R.stats_target(2, *size, 616).to(dev)
    tfin = torch.where(torch.isfinite(t), t, torch.ones_like(t))
    fr = ft.float().requires_grad_(True)
    lu = m(img, fr, size, head=conv, dense_target=tfin, valid=valid)
    lu.backward()
    assert fr.grad is not None and float(fr.grad.abs().sum()) > 0
    with torch.no_grad():
        lf = m(img, ft, size, head=conv, dense_target=tfin, valid=valid)
        assert abs(float(lu) - float(lf)) <= 0.05 * (1.0 + float(lf))
        assert torch.equal(m(img, ft, size, head=conv, dense_target=tfin.double(), valid=valid.to(torch.uint8)), lf)
        # errors: a fresh accumulator per call, or one accumulator over the batches; in place of the loss; never differentiable
        acc = torch.zeros(10, dtype=torch.float64, device=dev)
        kw = dict(head=conv, valid=valid[:1], clamp=(0.5, 3.0))
        e0 = m(img[:1], ft[:1], size, dense_target=t[:1], errors=True, **kw)
        e1 = m(img[1:], ft[1:], size, dense_target=t[1:], errors=True, **{**kw, "valid": valid[1:]})
        assert e0.dtype == torch.float64 and tuple(e0.shape) == (10,) and float(e0[0]) > 0
        out = m(img[:1], ft[:1], size, dense_target=t[:1], errors=acc, **kw)
        assert out is acc and torch.equal(acc, e0)
        out, pred = m(img[1:], ft[1:], size, dense_target=t[1:], errors=acc, predict=True, **{**kw, "valid": valid[1:]})
        assert out is acc and torch.equal(acc, e0 + e1)
        assert torch.equal(pred, m(img[1:], ft[1:], size, head=conv))
        zall = m(img, ft, size, head=conv)
    with torch.enable_grad():
        e2 = m(img[:1], ft[:1], size, dense_target=t[:1], errors=True, **kw)
    assert not e2.requires_grad and torch.equal(e2, e0)
    import naf_amd
    both = naf_amd.depth_metrics(acc)
    ref = R.metrics(R.error_sums(zall[:, 0], t[:, 0], valid, (0.5, 3.0))[0].cpu())
    for name in ("mae", "rmse", "abs_rel", "sq_rel", "rmse_log", "silog", "d1", "d2", "d3"):
        assert abs(float(getattr(both, name)) - ref[name]) <= 1e-4 * (1e-3 + abs(ref[name])), name
    with torch.no_grad():
        # all invalid: nan / 0 / zeros, as the torch expressions on an empty selection
        none = torch.zeros_like(valid)
        assert torch.isnan(m(img, ft, size, head=conv, dense_target=tfin, valid=none))
        assert float(m(img, ft, size, head=conv, dense_target=tfin, valid=none, reduction="sum")) == 0.0
        assert float(m(img, ft, size, head=conv, dense_target=tfin, valid=none, reduction="none").abs().sum()) == 0.0
        before = acc.clone()
        m(img, ft, size, head=conv, dense_target=t, valid=none, errors=acc)
        assert torch.equal(LC.bits(acc), LC.bits(before))
        # empty batch
        z = m(img[:0], ft[:0], size, head=conv, dense_target=tfin[:0], predict=True)
        assert torch.isnan(z[0]) and tuple(z[1].shape) == (0, 1, *size)
        assert m(img[:0], ft[:0], size, head=conv, dense_target=tfin[:0], reduction="none").shape == (0, *size)
        assert m(img[:0], ft[:0], size, head=conv, dense_target=tfin[:0], errors=acc) is acc and torch.equal(acc, before)


# ---- E: layout -------------------------------------------------------------------------------------------------------------------
def _reg_args(q, k, pv, bias, out, n_out, ksz, target, valid, loss, dlogits, kind="smooth_l1"):
    """(naf_xna_head_reg_args, naf_xna_head_reg_select's answer): ops.xna_head_regression's filling with the caller's buffers."""
    import ctypes as C
    from naf_amd import _lib, ops
    ky, kx = ops._ksize(ksz)
    a = _lib.XnaHeadRegArgs()
    a.head = ops._fill_xna_head(q, k, pv, bias, out if out is not None else q, n_out, ky, kx, "fused", None)
    if out is None:
        a.head.out, a.head.out_dtype = None, _lib.NAF_F32
    a.kind, a.beta, a.clamp_lo, a.clamp_hi = _lib.HEAD_REG_KINDS[kind], BETA, 1e-3, float("inf")
    a.dlogits_channels = int(dlogits.shape[-1]) if dlogits is not None else ops.head_dlogits_channels(n_out)
    a.target, a.t_stride = target.data_ptr(), ops._strides4(target, (0, 1, 2, 3))
    for t, ptr, st in ((valid, "valid", "valid_stride"), (loss, "loss", "loss_stride"), (dlogits, "dlogits", "dlogits_stride")):
        if t is not None:
            setattr(a, ptr, t.data_ptr())
            setattr(a, st, ops._strides3(t))
    return a, int(_lib.load().naf_xna_head_reg_select(C.byref(a)))


@pytest.mark.parametrize("family", ["row_gap", "crop"])
def test_outputs_inside_sentinel_arenas_and_strided_inputs(dev, family):
    """E: loss, dlogits and the logits written into windows of larger sentinel-filled buffers (tests/layout_contract.py): the views hold the
    bits of the dense launch and nothing outside them changes; a strided mask and a strided target give the bits of their contiguous copies."""
    import ctypes as C
    from naf_amd import _lib, ops
    geom, N = (2, 9, 9, 14, 14, 9, 0, 12), 17          # partial row tiles: masked lanes must store nothing
    B, h, w, dy, dx, ksz, _, heads = geom
    Ho, Wo = h * dy, w * dx
    (q5, k5, pv5, bd), t, valid = _case_inputs(geom, N, "tenth", False, dev)
    gc = ops.head_dlogits_channels(N)
    base = ops.xna_head_regression(q5, k5, pv5, bd, ksz, n_out=N, target=t, valid=valid, kind="smooth_l1", beta=BETA, want_loss=True,
                                   want_dlogits=True, return_logits=True, path="fused")
    # strided inputs: every second element of wider buffers whose other elements are NaN / 1
    wide_t = torch.full((B, N, Ho, 2 * Wo), float("nan"), device=dev)
    wide_t[..., ::2] = t
    wide_v = torch.ones(B, Ho, 2 * Wo, dtype=torch.bool, device=dev)
    wide_v[..., ::2] = valid
    wide_v[..., 1::2] = ~valid
    tcl = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    for tt, vv in ((wide_t[..., ::2], wide_v[..., ::2]), (tcl, valid.to(torch.uint8))):
        got = ops.xna_head_regression(q5, k5, pv5, bd, ksz, n_out=N, target=tt, valid=vv, kind="smooth_l1", beta=BETA, want_loss=True,
                                      want_dlogits=True, return_logits=True, path="fused")
        assert all(LC.same_bits(a, b) for a, b in zip(got, base))
    # outputs in arenas
    loss5, loss_arena, loss_mask = LC.arena_for((B, 1, Ho, Wo, 1), torch.float32, family, dev)
    g5, g_arena, g_mask = LC.arena_for((B, 1, Ho, Wo, gc), torch.bfloat16, family, dev)
    o5, o_arena, o_mask = LC.arena_for((B, 1, Ho, Wo, N), torch.float32, family, dev)
    before = [x.clone() for x in (loss_arena, g_arena, o_arena)]
    a, sel = _reg_args(q5, k5, pv5, bd, LC.hw3(o5), N, ksz, t, valid.view(torch.uint8), LC.hw2(loss5), LC.hw3(g5))
    assert sel == _lib.XNA_HEAD_FUSED, _lib.last_error()
    with torch.cuda.device(dev):
        rc = _lib.load().naf_xna_head_reg_fwd(C.byref(a), ops._stream(q5))
    _lib.check(rc, "naf_xna_head_reg_fwd")
    torch.cuda.synchronize()
    assert LC.same_bits(LC.hw2(loss5), base[0]) and LC.same_bits(LC.hw3(g5), base[1]) and LC.same_bits(LC.hw3(o5).permute(0, 3, 1, 2), base[2])
    for arena, b4, mask, what in ((loss_arena, before[0], loss_mask, "loss"), (g_arena, before[1], g_mask, "dlogits"), (o_arena, before[2], o_mask, "out")):
        assert LC.untouched(arena, b4, mask), f"{what}: {LC.outside_writes(arena, b4, mask)} elements outside the view changed"
