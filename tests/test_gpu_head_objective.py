"""GPU tests (-m gpu) of the fused probe objective: the classification epilogue of the head-summed attention kernel
(naf_xna_head_ce_fwd: per-pixel cross-entropy, argmax labels, softmax - onehot without the logits tensor), ``ops.XnaHeadCEFunction`` and
``naf(image, feats, size, head=probe, target=t / predict=True)`` end to end.

Tolerances.
  A. One launch against itself -- the same launch also stores its fp32 logits L, so nothing has to be invented:
     * L is bit-equal to naf_xna_head_fwd's fp32 logits (same accumulators), labels are bit-equal to L.argmax(1);
     * loss vs fp64 logsumexp(L) - L[t]: <= 1e-5 * (1 + |lse| + |L[t]|).  The hardware exp2 / log2 are good to about 1 ulp (2^-23), a sum of
       at most 256 positive terms adds about 10 * 2^-24 relative: under 2e-6 of |lse| + |L[t]|; 1e-5 leaves a factor five for the order
       of operations.  Ignored and out-of-range pixels: exactly 0;
     * g[..., :N] vs fp64 softmax(L) - onehot(t): <= 2^-8 |ref| + 1e-5 (one rounding to bf16 is 2^-9 relative; the absolute term is the fp32
       slack above); channels N .. Gc-1 and the rows of ignored / out-of-range pixels exactly 0.
  B. Against the oracle (test_gpu_head.head_reference: fp32 logits ``ref`` and sum_g |ref_g|): with the project's fp32-output bound per
     logit, bound[px] = max_n (G * 6e-3 + 6e-3 * sum_g |ref_g[n, px]|), logsumexp is 1-Lipschitz in the sup norm and the target logit moves by
     at most ``bound``: loss within 2 * bound + 1e-5 * (1 + |lse| + |ref[t]|); the kernel's label is a maximum of ``ref`` up to 2 * bound on EVERY
     pixel, and equal to ref.argmax where the oracle's top-2 margin exceeds 2 * bound (the share of such pixels is asserted from the oracle alone).
  C. Gradients: g is held by A; given g, the backward is naf_xna_bwd with one dout shared by the heads, under
     test_head_function_gradients_match_oracle's own bound.  Module level: fused error <= 2 * (error of the path that existed before:
     F.cross_entropy on the logits call) + 2^-8 max|ref| (the one bf16 rounding of g; the parent path rounds its dout at the same place).
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import bf16r, oracle_xna_backward, to5  # noqa: E402
from test_gpu_head import HEAD_GEOMS, _load_model, _probe, head_reference, make_pv, npad_of, xna_row_tiles_ok  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


LABEL_GEOM = (1, 8, 8, 16, 16, 7, 0, 4)       # 8 x 8 -> 128 x 128, window 7, four heads: the geometry the label shares were computed on


def make_target(B, Ho, Wo, N, ignore_index, mode="ignore"):
    """Targets from a hash of the pixel index modulo N, about a tenth of the pixels ignored.  mode "oob": image row 5 holds N + 3 (outside the
    classes, not ignore_index); "all": every pixel ignored."""
    idx = torch.arange(B * Ho * Wo, dtype=torch.int64)
    hsh = (idx * 2654435761 + 12345) & 0xFFFFFFFF
    t = ((hsh >> 9) % N).view(B, Ho, Wo)
    t[(((hsh >> 3) % 10) == 0).view(B, Ho, Wo)] = ignore_index
    if mode == "oob":
        t[:, 5] = N + 3
    if mode == "all":
        t[:] = ignore_index
    return t


def valid_of(t, ignore_index, N):
    return (t != ignore_index) & (t >= 0) & (t < N)


def make_inputs(geom, N, seeds, dev):
    B, h, w, dy, dx, ksz, _, heads = geom
    q = bf16r(O.hash_normal((B, 64 * heads, h * dy, w * dx), seeds[0]))
    k = bf16r(O.hash_normal((B, 64 * heads, h, w), seeds[1]))
    pv, pvn = make_pv(B, heads, h, w, N, seeds[2])
    bias = O.hash_normal((N,), seeds[3])
    dv = (to5(q, heads).to(dev), to5(k, heads).to(dev), pv.to(dev).to(torch.bfloat16), bias.to(dev))
    return (q, k, pvn, bias), dv


_G = {g[5]: g for g in HEAD_GEOMS if xna_row_tiles_ok(g[4])}
SELF_CASES = [
    # (geometry, N, ignore_index, mode): every window 3 .. 15, every channel-tile count (N <= 32, <= 64, <= 160, <= 256)
    ((1, 5, 5, 3, 30, 3, 256, 4), 1, 255, "ignore"),          # window 3, a full and a 14-pixel tile per row, one class
    ((1, 6, 7, 14, 14, 5, 192, 4), 2, -100, "ignore"),        # window 5, 14 x 14 cells: partial row tiles
    (LABEL_GEOM, 21, 255, "oob"),                             # window 7, one image row outside the classes
    (LABEL_GEOM, 40, 255, "ignore"),                          # four channel tiles
    ((1, 9, 9, 7, 15, 9, 1024, 4), 32, 255, "ignore"),        # window 9, 15-pixel rows
    ((1, 12, 13, 2, 16, 11, 0, 3), 151, 255, "ignore"),       # window 11, three heads, ten channel tiles
    ((1, 14, 13, 1, 16, 13, 0, 1), 160, 255, "ignore"),       # window 13, Npad = 160 -> Gc = 192 exceeds the accumulator width
    ((1, 16, 15, 3, 32, 15, 0, 2), 256, 255, "ignore"),       # window 15, 256 classes with ignore_index inside them
    ((1, 7, 8, 32, 16, 7, 0, 6), 21, 255, "all"),             # 32 x 16 cells: two rounds per workgroup; every pixel ignored
    ((2, 9, 9, 14, 14, 9, 0, 12), 151, 255, "ignore"),        # two images, twelve heads, patch-14 cells
    ((1, 10, 9, 16, 16, 7, 384, 4), 160, -100, "oob"),        # Gc = 192 with a row outside the classes
    ((1, 7, 8, 14, 28, 7, 128, 4), 65, 255, "ignore"),        # Npad = 80: ten channel tiles but Gc = 96 BELOW the accumulator width
]


def test_cases_cover_every_window_and_tile_count():
    assert all(g in HEAD_GEOMS or g == LABEL_GEOM for g, *_ in SELF_CASES) and all(xna_row_tiles_ok(g[4]) for g, *_ in SELF_CASES)
    assert {c[0][5] for c in SELF_CASES} == {3, 5, 7, 9, 11, 13, 15} == set(_G)
    assert {1, 2, 21, 32, 151, 160, 256} <= {c[1] for c in SELF_CASES}
    assert {"ignore", "oob", "all"} == {c[3] for c in SELF_CASES}


@pytest.mark.parametrize("geom,N,ign,mode", SELF_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_one_launch_against_itself(dev, geom, N, ign, mode):
    """A of the module docstring."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, _, heads = geom
    Ho, Wo = h * dy, w * dx
    s = sum(geom) + N
    _, (q5, k5, pv5, bd) = make_inputs(geom, N, (s + 1, s + 2, s + 3, s + 4), dev)
    t = make_target(B, Ho, Wo, N, ign, mode).to(dev)
    kw = dict(n_out=N, ignore_index=ign, path="fused")
    loss, labels, g, L = ops.xna_head_objective(q5, k5, pv5, bd, ksz, target=t, want_loss=True, want_labels=True, want_dlogits=True,
                                                return_logits=True, **kw)
    gc = ops.head_dlogits_channels(N)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (B, Ho, Wo)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B, Ho, Wo)
    assert g.dtype == torch.bfloat16 and tuple(g.shape) == (B, Ho, Wo, gc) and g.is_contiguous() and gc >= npad_of(N) and gc in (32, 64, 96, 128, 192, 256)
    assert L.dtype == torch.float32 and tuple(L.shape) == (B, N, Ho, Wo)
    fwd = ops.xna_head_forward(q5, k5, pv5, bd, ksz, n_out=N, out_dtype=torch.float32, path="fused")
    assert torch.equal(L, fwd), "the logits of the classification launch differ from naf_xna_head_fwd's"
    assert torch.equal(labels.long(), L.argmax(1)), "labels differ from argmax of the launch's own logits"
    valid = valid_of(t, ign, N)
    assert (int(valid.sum()) == 0) == (mode == "all")
    if mode == "oob":
        assert not bool(valid[:, 5].any())
    L64 = L.double()
    lse = torch.logsumexp(L64, dim=1)
    tc = torch.where(valid, t, torch.zeros_like(t))
    Lt = L64.gather(1, tc.unsqueeze(1))[:, 0]
    err = (loss.double() - (lse - Lt)).abs()
    tol = 1e-5 * (1.0 + lse.abs() + Lt.abs())
    print(f"self {geom} N={N} {mode}: loss max err / tol {float((err / tol)[valid].max()) if bool(valid.any()) else 0.0:.3f}")
    assert not bool((err > tol)[valid].any()), f"loss: max err {float(err[valid].max()):.3e}"
    assert float(loss[~valid].abs().sum()) == 0.0 if bool((~valid).any()) else True
    ref_g = torch.softmax(L64, dim=1) - F.one_hot(tc, N).permute(0, 3, 1, 2).double()
    ref_g = (ref_g * valid.unsqueeze(1)).permute(0, 2, 3, 1)
    eg = (g[..., :N].double() - ref_g).abs()
    tg = 2.0 ** -8 * ref_g.abs() + 1e-5
    print(f"    g max err / tol {float((eg / tg).max()):.3f}")
    assert not bool((eg > tg).any()), f"g: max err {float(eg.max()):.3e}"
    if gc > N:
        assert float(g[..., N:].float().abs().max()) == 0.0, "pad channels of g are not zero"
    if bool((~valid).any()):
        assert float(g[~valid].float().abs().max()) == 0.0, "ignored pixels carry a gradient"
    # each output requested alone: the NULL branches change nothing
    l1 = ops.xna_head_objective(q5, k5, pv5, bd, ksz, target=t, want_loss=True, **kw)
    assert torch.equal(l1[0], loss) and l1[1] is None and l1[2] is None and l1[3] is None
    l2 = ops.xna_head_objective(q5, k5, pv5, bd, ksz, want_labels=True, **kw)              # no target
    assert torch.equal(l2[1], labels) and l2[0] is None
    l3 = ops.xna_head_objective(q5, k5, pv5, bd, ksz, target=t, want_dlogits=True, **kw)
    assert torch.equal(l3[2], g)
    l4 = ops.xna_head_objective(q5, k5, pv5, bd, ksz, return_logits=True, **kw)
    assert torch.equal(l4[3], L)
    # the composition has the same contract
    c = ops.xna_head_objective(q5, k5, pv5, bd, ksz, n_out=N, ignore_index=ign, target=t, want_loss=True, want_labels=True, want_dlogits=True,
                               path="composed")
    assert c[0].dtype == loss.dtype and c[1].dtype == labels.dtype and c[2].dtype == g.dtype and c[2].shape == g.shape
    assert float(c[0][~valid].abs().sum()) == 0.0 and float(c[2][~valid].float().abs().sum()) == 0.0


def test_non_contiguous_target_and_int32(dev):
    """The target is read with element strides; the ops layer converts other integer dtypes."""
    from naf_amd import ops
    geom, N = LABEL_GEOM, 21
    _, (q5, k5, pv5, bd) = make_inputs(geom, N, (1, 2, 3, 4), dev)
    t = make_target(1, 128, 128, N, 255).to(dev)
    base = ops.xna_head_objective(q5, k5, pv5, bd, 7, n_out=N, target=t, ignore_index=255, want_loss=True, path="fused")[0]
    wide = torch.zeros(1, 128, 256, dtype=torch.int64, device=dev)
    wide[:, :, ::2] = t
    a = ops.xna_head_objective(q5, k5, pv5, bd, 7, n_out=N, target=wide[:, :, ::2], ignore_index=255, want_loss=True, path="fused")[0]
    b = ops.xna_head_objective(q5, k5, pv5, bd, 7, n_out=N, target=t.int(), ignore_index=255, want_loss=True, path="fused")[0]
    assert torch.equal(a, base) and torch.equal(b, base)
    with pytest.raises(TypeError, match="integer tensor"):
        ops.xna_head_objective(q5, k5, pv5, bd, 7, n_out=N, target=t.float(), want_loss=True)
    with pytest.raises(ValueError, match="need a target"):
        ops.xna_head_objective(q5, k5, pv5, bd, 7, n_out=N, want_loss=True)
    with pytest.raises(ValueError, match="nothing asked"):
        ops.xna_head_objective(q5, k5, pv5, bd, 7, n_out=N, target=t)


ORACLE_CASES = [
    # (geometry, N, mode, check the determined pixels?)
    (LABEL_GEOM, 2, "ignore", True),
    (LABEL_GEOM, 21, "oob", True),
    (LABEL_GEOM, 151, "ignore", True),
    (LABEL_GEOM, 256, "ignore", True),
    ((2, 9, 9, 14, 14, 9, 0, 12), 21, "ignore", False),       # twelve heads: ``bound`` grows with the head count, 0.548 determined
    ((1, 5, 5, 3, 30, 3, 256, 4), 32, "ignore", False),
]


@pytest.mark.parametrize("geom,N,mode,determined", ORACLE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_objective_matches_oracle(dev, geom, N, mode, determined):
    """B of the module docstring.  Inputs: seeds 901 / 902 / 903 / 904 of hash_normal for q / k / PV / bias."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, _, heads = geom
    Ho, Wo = h * dy, w * dx
    (q, k, pvn, bias), (q5, k5, pv5, bd) = make_inputs(geom, N, (901, 902, 903, 904), dev)
    ref, abs_sum = head_reference(q, k, pvn, ksz, heads, N, bias)
    bound = (heads * 6e-3 + 6e-3 * abs_sum).amax(dim=1).double()              # [B, Ho, Wo]
    ref64 = ref.double()
    top = ref64.topk(min(2, N), dim=1).values
    if determined:
        det = (top[:, 0] - top[:, 1]) > 2.0 * bound
        share = float(det.double().mean())
        print(f"oracle {geom} N={N}: determined share {share:.3f}")
        assert share >= 0.75, f"inputs leave only {share:.3f} of the pixels determined"      # a condition on the inputs, before the device result
    ign = 255
    t = make_target(B, Ho, Wo, N, ign, mode)
    valid = valid_of(t, ign, N)
    loss, labels, _, _ = ops.xna_head_objective(q5, k5, pv5, bd, ksz, n_out=N, target=t.to(dev), ignore_index=ign, want_loss=True,
                                                want_labels=True, path="fused")
    loss, labels = loss.double().cpu(), labels.long().cpu()
    lse = torch.logsumexp(ref64, dim=1)
    tc = torch.where(valid, t, torch.zeros_like(t))
    rt = ref64.gather(1, tc.unsqueeze(1))[:, 0]
    ref_loss = torch.where(valid, lse - rt, torch.zeros_like(lse))
    tol = 2.0 * bound + 1e-5 * (1.0 + lse.abs() + rt.abs())
    err = (loss - ref_loss).abs()
    print(f"    loss max err {float(err[valid].max()):.3e}, max err / tol {float((err / tol)[valid].max()):.3f}")
    assert not bool((err > tol)[valid].any())
    assert float(loss[~valid].abs().sum()) == 0.0
    nv = valid.sum()
    assert abs(float(loss.sum() / nv) - float(ref_loss.sum() / nv)) <= float(tol[valid].mean())
    chosen = ref64.gather(1, labels.unsqueeze(1))[:, 0]
    assert bool((chosen >= top[:, 0] - 2.0 * bound).all()), "a label is not a maximum of the oracle's logits up to the logit error"
    if determined:
        assert torch.equal(labels[det], ref64.argmax(1)[det])


@pytest.mark.parametrize("B,heads,lr,out_sz,ksz,N", [
    (1, 4, (8, 8), (128, 128), 7, 21),         # the cell backward at Dv = 32
    (2, 4, (10, 9), (80, 288), 9, 151),        # 9x9, dx = 32, Npad = 160 -> Gc = 192
    (1, 2, (15, 16), (30, 256), 15, 19),       # 15x15
    (1, 4, (12, 10), (168, 140), 9, 27),       # patch 14: partial row tiles
])
def test_ce_function_gradients_match_oracle(dev, B, heads, lr, out_sz, ksz, N):
    """C, operator level: test_head_function_gradients_match_oracle with dout := g[..., :N] read back from the kernel (bf16-representable):
    dPV of ops.XnaHeadCEFunction(reduction="sum") against the oracle's backward fed that dout, under that test's bound; pad channels exactly 0;
    dbias against the fp64 sum of g; "mean" = "sum" / count within two fp32 roundings (2^-22) for the loss and dbias (no atomics there)."""
    from naf_amd import ops
    npad = npad_of(N)
    q = bf16r(O.hash_normal((B, 64 * heads, *out_sz), 501))
    k = bf16r(O.hash_normal((B, 64 * heads, *lr), 502))
    pv, pvn = make_pv(B, heads, *lr, N, 503)
    t = make_target(B, *out_sz, N, 255, "oob").to(dev)
    q5, k5 = to5(q, heads).to(dev), to5(k, heads).to(dev)
    pv5 = pv.to(dev).to(torch.bfloat16).requires_grad_(True)
    bias = O.hash_normal((N,), 505).to(dev).requires_grad_(True)
    loss = ops.XnaHeadCEFunction.apply(q5, k5, pv5, bias, t, ksz, N, 255, "sum")
    assert loss.requires_grad and loss.dim() == 0 and loss.dtype == torch.float32 and not q5.requires_grad
    loss.backward()
    g = ops.xna_head_objective(q5, k5, pv5.detach(), bias.detach(), ksz, n_out=N, target=t, ignore_index=255, want_dlogits=True)[2]
    dout = g[..., :N].float().permute(0, 3, 1, 2).cpu()
    d5 = torch.zeros(B, heads, npad, *out_sz)
    d5[:, :, :N] = dout[:, None]
    _, _, rv = oracle_xna_backward(dev, q, k, pvn, d5.reshape(B, heads * npad, *out_sz), ksz, heads)
    ref = rv.view(B, heads, npad, *lr).permute(0, 1, 3, 4, 2)
    got = pv5.grad.float().cpu()
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    print(f"CE dPV k={ksz} N={N}: max err {float(err.max()):.3e} mean {float(err.mean()):.3e} (ref max {scale:.3e})")
    assert float(err.max()) <= 2e-2 * scale + 1e-3 and float(err.mean()) <= 3e-3 * scale + 1e-4, \
        f"dPV: max err {float(err.max()):.3e} mean {float(err.mean()):.3e} (ref max {scale:.3e})"
    assert float(got[..., N:].abs().max()) == 0.0 if npad > N else True
    rb = dout.double().sum(dim=(0, 2, 3))
    eb = float((bias.grad.double().cpu() - rb).abs().max())
    nterm = B * out_sz[0] * out_sz[1]
    assert eb <= nterm * 2.0 ** -24 * float(dout.abs().max()), f"dbias err {eb:.3e}"
    # "mean": the "sum" result times 1 / count
    db_sum, loss_sum = bias.grad.double().clone(), loss.detach().double()
    bias.grad = None
    pv5.grad = None
    lm = ops.XnaHeadCEFunction.apply(q5, k5, pv5, bias, t, ksz, N, 255, "mean")
    lm.backward()
    count = float(valid_of(t, 255, N).sum())
    assert abs(float(lm.detach().double()) * count - float(loss_sum)) <= 2.0 ** -22 * abs(float(loss_sum))
    assert bool(((bias.grad.double() * count - db_sum).abs() <= 2.0 ** -22 * db_sum.abs()).all())
    sm = float((pv5.grad.float().cpu() * count - got).abs().max())
    assert sm <= 2e-2 * scale + 1e-3          # atomics: the two runs add in different orders, no bit equality
    # "none": a map, and a map of incoming gradients
    pv5.grad = None
    bias.grad = None
    ln = ops.XnaHeadCEFunction.apply(q5, k5, pv5, bias, t, ksz, N, 255, "none")
    assert tuple(ln.shape) == (B, *out_sz) and abs(float(ln.detach().double().sum()) - float(loss_sum)) <= 1e-5 * abs(float(loss_sum))
    ln.sum().backward()
    assert float((bias.grad.double() - db_sum).abs().max()) <= nterm * 2.0 ** -24 * float(dout.abs().max())


# ---- module level -----------------------------------------------------------------------------------------------
SIZE, LR, CC, KSZ = (224, 224), (14, 14), 384, 9


@functools.lru_cache(maxsize=None)
def _module_setup():
    p = O.make_params(seed=31)
    img = O.hash_normal((1, 3, *SIZE), 601)
    ft = bf16r(O.hash_normal((1, CC, *LR), 602))
    up = O.naf_forward(p, img, ft, SIZE, kernel_size=KSZ).double()
    return p, img, ft, up


def _ref_loss_and_grads(up, wt, bs, t, ignore_index=255):
    w64 = wt.double().clone().requires_grad_(True)
    b64 = bs.double().clone().requires_grad_(True)
    loss = F.cross_entropy(F.conv2d(up, w64, b64), t, ignore_index=ignore_index)
    loss.backward()
    return float(loss), w64.grad, b64.grad


@pytest.mark.parametrize("N", [21, 151])
def test_module_objective_matches_oracle_within_the_parent_path_error(dev, N):
    """C, module level: loss, weight gradient and bias gradient of naf(..., head=conv, target=t, ignore_index=255) against fp64 autograd of
    F.cross_entropy(conv(up), t) with ``up`` the oracle's forward; the budget is twice the error of the path that existed before this change
    (F.cross_entropy on the logits call) plus 2^-8 max|ref|.  The frozen upsampler gets no gradient."""
    p, img, ft, up = _module_setup()
    m = _load_model(dev, p, kernel_size=KSZ)
    conv, conv_par = _probe(CC, N, 603, dev), _probe(CC, N, 603, dev)
    t = make_target(1, *SIZE, N, 255)
    ref_loss, ref_w, ref_b = _ref_loss_and_grads(up, conv.weight.detach().float().cpu(), conv.bias.detach().float().cpu(), t)
    imgd, ftd, td = img.to(dev), ft.to(dev).to(torch.bfloat16), t.to(dev)
    loss = m(imgd, ftd, SIZE, head=conv, target=td, ignore_index=255)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward()
    assert all(q.grad is None for q in m.parameters()), "the frozen upsampler received a gradient"
    par = F.cross_entropy(m(imgd, ftd, SIZE, head=conv_par).float(), td, ignore_index=255)
    par.backward()
    for name, got, parent, ref in (("loss", loss.detach().cpu().double(), par.detach().cpu().double(), torch.tensor(ref_loss, dtype=torch.float64)),
                                   ("weight grad", conv.weight.grad.cpu().double(), conv_par.weight.grad.cpu().double(), ref_w),
                                   ("bias grad", conv.bias.grad.cpu().double(), conv_par.bias.grad.cpu().double(), ref_b)):
        e_f, e_p, scale = float((got - ref).abs().max()), float((parent - ref).abs().max()), float(ref.abs().max())
        print(f"module objective N={N} {name}: fused err {e_f:.3e}, parent-path err {e_p:.3e}, ref max {scale:.3e}")
        assert e_f <= 2.0 * e_p + 2.0 ** -8 * scale, f"{name}: fused err {e_f:.3e} vs parent {e_p:.3e} (ref max {scale:.3e})"


def test_module_objective_unfused_route_and_training_steps(dev):
    """With m.train() and trainable parameters the call IS the unfused composition (same seed: bit equal) and trains the upsampler.  Three SGD
    steps of a probe with the fused call and with the parent path from the same start: at every step the fused loss is within the
    module-level bound of the fp64 reference sequence (twice the parent path's distance plus 2^-8 |ref|), and all three sequences decrease."""
    p, img, ft, up = _module_setup()
    m = _load_model(dev, p, kernel_size=KSZ)
    N = 21
    t = make_target(1, *SIZE, N, 255)
    imgd, ftd, td = img.to(dev), ft.to(dev).to(torch.bfloat16), t.to(dev)
    conv = _probe(CC, N, 603, dev)
    m.train()
    torch.manual_seed(5)
    a = m(imgd, ftd.float(), SIZE, head=conv, target=td, ignore_index=255)
    torch.manual_seed(5)
    b = F.cross_entropy(conv(m.forward_train(imgd, ftd.float(), SIZE)).float(), td, ignore_index=255)
    assert torch.equal(a, b)
    a.backward()
    assert any(q.grad is not None and float(q.grad.abs().sum()) > 0 for q in m.image_encoder.parameters())
    m.eval()
    fr = ftd.float().requires_grad_(True)                       # an input that requires grad, in eval mode
    c, lab = m(imgd, fr, SIZE, head=conv, target=td, ignore_index=255, predict=True)
    c.backward()
    assert fr.grad is not None and float(fr.grad.abs().sum()) > 0 and lab.dtype == torch.int64 and not lab.requires_grad
    m.zero_grad(set_to_none=True)

    conv_f, conv_p = _probe(CC, N, 603, dev), _probe(CC, N, 603, dev)
    w64 = conv_f.weight.detach().cpu().double().requires_grad_(True)
    b64 = conv_f.bias.detach().cpu().double().requires_grad_(True)
    lr = 0.5
    opts = (torch.optim.SGD(conv_f.parameters(), lr=lr), torch.optim.SGD(conv_p.parameters(), lr=lr), torch.optim.SGD([w64, b64], lr=lr))
    seq = []
    for step in range(3):
        for o in opts:
            o.zero_grad()
        lf = m(imgd, ftd, SIZE, head=conv_f, target=td, ignore_index=255)
        lp = F.cross_entropy(m(imgd, ftd, SIZE, head=conv_p).float(), td, ignore_index=255)
        lref = F.cross_entropy(F.conv2d(up, w64, b64), t, ignore_index=255)
        for l, o in zip((lf, lp, lref), opts):
            l.backward()
            o.step()
        seq.append((float(lf.detach()), float(lp.detach()), float(lref.detach())))
        print(f"probe step {step}: fused {seq[-1][0]:.6f} parent path {seq[-1][1]:.6f} fp64 reference {seq[-1][2]:.6f}")
        assert abs(seq[-1][0] - seq[-1][2]) <= 2.0 * abs(seq[-1][1] - seq[-1][2]) + 2.0 ** -8 * abs(seq[-1][2])
    for i in range(3):
        assert seq[0][i] > seq[1][i] > seq[2][i], f"sequence {i} does not decrease: {[s[i] for s in seq]}"
    assert all(q.grad is None for q in m.parameters())


def test_module_objective_table_forms_and_edge_cases(dev):
    """D: the four rows of the table (shapes, dtypes, requires_grad); predict against the logits call; head forms and a bf16 probe; a non-integer
    ratio through the composition; all-ignored targets; a row outside the classes; an empty batch."""
    from torch import nn
    p = O.make_params(seed=32)
    m = _load_model(dev, p, kernel_size=7)
    size, N = (96, 128), 19
    img, ft = O.hash_normal((2, 3, *size), 611).to(dev), O.hash_normal((2, 128, 8, 8), 612).to(dev)
    conv = _probe(128, N, 613, dev)
    t = make_target(2, *size, N, 255).to(dev)
    valid = valid_of(t, 255, N)
    with torch.no_grad():
        logits = m(img, ft, size, head=conv)
        loss = m(img, ft, size, head=conv, target=t, ignore_index=255)
        pred = m(img, ft, size, head=conv, predict=True)
        both = m(img, ft, size, head=conv, target=t, ignore_index=255, predict=True)
        lmap = m(img, ft, size, head=conv, target=t, ignore_index=255, reduction="none")
        lsum = m(img, ft, size, head=conv, target=t, ignore_index=255, reduction="sum")
    assert logits.shape == (2, N, *size) and logits.dtype == torch.float32
    assert loss.dim() == 0 and loss.dtype == torch.float32 and not loss.requires_grad
    assert pred.shape == (2, *size) and pred.dtype == torch.int64
    assert isinstance(both, tuple) and torch.equal(both[0], loss) and torch.equal(both[1], pred)
    assert lmap.shape == (2, *size) and lmap.dtype == torch.float32 and lsum.dim() == 0
    # the same kernel arithmetic on the same queries: the labels ARE the argmax of the logits call (which implies both label checks of B with
    # the logits call in the oracle's place), and the loss is F.cross_entropy of those logits up to the fp32 slack of A
    assert torch.equal(pred, logits.argmax(1))
    ref = F.cross_entropy(logits.double(), t, ignore_index=255, reduction="none")
    assert float((lmap.double() - ref).abs().max()) <= 1e-5 * (1.0 + 2.0 * float(logits.abs().max()) + float(ref.max()))
    assert abs(float(loss) - float(ref.sum() / valid.sum())) <= 1e-5 * (1.0 + float(ref.max()))
    assert abs(float(lsum) - float(ref.sum())) <= 1e-5 * float(ref.sum())
    # with a probe that requires grad the loss carries a graph to it, the labels do not
    lg, pg = m(img, ft, size, head=conv, target=t, ignore_index=255, predict=True)
    assert lg.requires_grad and not pg.requires_grad and torch.equal(pg, pred) and abs(float(lg) - float(loss)) <= 1e-5 * (1.0 + float(loss))
    assert not m(img, ft, size, head=conv, predict=True).requires_grad
    # head forms and dtypes
    lin = nn.Linear(128, N).to(dev)
    with torch.no_grad():
        lin.weight.copy_(conv.weight[:, :, 0, 0])
        lin.bias.copy_(conv.bias)
        b = m(img, ft, size, head=lin, target=t, ignore_index=255, predict=True)
        c = m(img, ft, size, head=(conv.weight.detach(), conv.bias.detach()), target=t, ignore_index=255, predict=True)
        e = m(img, ft, size, head=_probe(128, N, 613, dev, torch.bfloat16), target=t, ignore_index=255)
        i32 = m(img, ft, size, head=conv, target=t.int(), ignore_index=255)
    assert torch.equal(b[0], loss) and torch.equal(b[1], pred) and torch.equal(c[0], loss) and torch.equal(c[1], pred) and torch.equal(i32, loss)
    assert e.dtype == torch.float32 and abs(float(e) - float(loss)) <= 0.05 * (1.0 + float(loss))
    # a geometry the fused kernel does not serve (non-integer ratio) goes through the composition: same contract
    t2 = make_target(2, 50, 70, N, 255, "oob").to(dev)
    with torch.no_grad():
        f, fl = m(img, ft, (50, 70), head=conv, target=t2, ignore_index=255, predict=True)
        g = m(img, ft, (50, 70), head=conv)
    assert fl.shape == (2, 50, 70) and fl.dtype == torch.int64 and torch.equal(fl, g.argmax(1))
    t2c = torch.where(valid_of(t2, 255, N), t2, torch.full_like(t2, 255))
    assert abs(float(f) - float(F.cross_entropy(g.double(), t2c, ignore_index=255))) <= 1e-5 * (1.0 + float(f))
    # ... and trains the probe there too
    conv.zero_grad()
    m(img, ft, (50, 70), head=conv, target=t2, ignore_index=255).backward()
    assert conv.weight.grad is not None and float(conv.weight.grad.abs().sum()) > 0
    # all ignored: nan / 0 / zeros, labels still valid
    ta = torch.full_like(t, 255)
    with torch.no_grad():
        mean, lab = m(img, ft, size, head=conv, target=ta, ignore_index=255, predict=True)
        assert torch.isnan(mean) and torch.equal(lab, pred)
        assert float(m(img, ft, size, head=conv, target=ta, ignore_index=255, reduction="sum")) == 0.0
        assert float(m(img, ft, size, head=conv, target=ta, ignore_index=255, reduction="none").abs().sum()) == 0.0
        # a row outside the classes contributes nothing and the call returns normally
        to = make_target(2, *size, N, 255, "oob").to(dev)
        lo = m(img, ft, size, head=conv, target=to, ignore_index=255, reduction="none")
        toc = torch.where(valid_of(to, 255, N), to, torch.full_like(to, 255))
        assert float(lo[:, 5].abs().sum()) == 0.0
        assert abs(float(m(img, ft, size, head=conv, target=to, ignore_index=255)) - float(F.cross_entropy(logits.double(), toc, ignore_index=255))) <= 1e-5 * (1.0 + float(loss))
        # empty batch: what torch returns for empty inputs of these shapes
        z = m(img[:0], ft[:0], size, head=conv, target=t[:0], predict=True)
        assert torch.isnan(z[0]) and z[1].shape == (0, *size) and z[1].dtype == torch.int64
        assert m(img[:0], ft[:0], size, head=conv, target=t[:0], reduction="none").shape == (0, *size)
        assert float(m(img[:0], ft[:0], size, head=conv, target=t[:0], reduction="sum")) == 0.0
    with pytest.raises(ValueError, match="return_weights"):
        m(img, ft, size, return_weights=True, head=conv, target=t)
