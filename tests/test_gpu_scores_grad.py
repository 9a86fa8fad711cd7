"""Differentiable attention scores (``return_weights="differentiable"``, C ABI 0.4.3 naf_xna_bwd_scores) against fp64 autograd through the
oracle: ``loss = sum(out * dO) + sum(logits * G)``.  The reference's legacy_attention (attentions.py:16-29) returns its scores as an ordinary
autograd tensor, so a loss on them trains q and k; these tests hold the HIP backward kernels to that."""
import pytest
import torch

from oracle import naf_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bf16r(x):
    return x.to(torch.bfloat16).to(torch.float32)


def to5(x, heads):
    """[B, C, H, W] fp32 -> bf16 5-D [B, heads, H, W, D] (head-major, D contiguous)."""
    B, C, H, W = x.shape
    return x.view(B, heads, C // heads, H, W).permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)


def oracle_xna_backward(dev, q, k, v, dout, G, ksz, heads):
    """fp64 autograd through ``O.xna(..., return_logits=True)`` with loss = sum(out * dout) + sum(logits * G); large cases on the device
    (the same oracle code on ATen's fp64 kernels)."""
    B, _, Ho, Wo = q.shape
    kk = ksz * ksz if isinstance(ksz, int) else ksz[0] * ksz[1]
    on = dev if B * Ho * Wo * kk * (q.shape[1] + v.shape[1]) >= 1.5e8 else torch.device("cpu")
    qd, kd, vd = (t.detach().to(on, torch.float64).requires_grad_(True) for t in (q, k, v))
    out, lg = O.xna(qd, kd, vd, ksz, heads, return_logits=True)
    loss = (out * dout.to(on, torch.float64)).sum() + (lg * G.to(on, torch.float64)).sum()
    loss.backward()
    return tuple(t.grad.float().cpu() for t in (qd, kd, vd))


def back(t5):
    return t5.permute(0, 1, 4, 2, 3).reshape(t5.shape[0], -1, *t5.shape[2:4]).float().cpu()


def check(got, ref, name):
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    assert float(err.max()) <= 2e-2 * scale + 1e-3 and float(err.mean()) <= 3e-3 * scale + 1e-4, \
        f"{name}: max err {float(err.max()):.3e} mean {float(err.mean()):.3e} (ref max {scale:.3e})"


def inputs(B, C, lr, out_sz, ksz, heads, Dq=64, seed=0):
    ky, kx = (ksz, ksz) if isinstance(ksz, int) else ksz
    q = bf16r(O.hash_normal((B, heads * Dq, *out_sz), 601 + seed))
    k = bf16r(O.hash_normal((B, heads * Dq, *lr), 602 + seed))
    v = bf16r(O.hash_normal((B, C, *lr), 603 + seed))
    dout = bf16r(O.hash_normal((B, C, *out_sz), 604 + seed))
    G = O.hash_normal((B, heads, *out_sz, ky * kx), 605 + seed, scale=0.5)
    return q, k, v, dout, G


# (B, C, lr, out, ksz, heads, Dq, kernel with a score gradient)
CASES = [
    (1, 256, (8, 8), (128, 128), 7, 4, 64, "mfma"),
    (2, 128, (5, 6), (40, 96), 3, 4, 64, "mfma"),
    (1, 768, (7, 7), (7, 112), 7, 4, 64, "mfma"),         # one tile per cell: three dead query waves per round
    (1, 384, (10, 9), (80, 288), 9, 4, 64, "mfma"),       # 9 x 9 pad slots
    (1, 1024, (10, 11), (80, 176), 9, 4, 64, "mfma"),     # Dv 256: one P / dS buffer
    (2, 768, (9, 12), (72, 192), 7, 4, 64, "mfma"),       # G1's instantiation, runs across images and heads
    (1, 384, (12, 14), (96, 224), 11, 4, 64, "mfma"),
    (1, 1024, (12, 13), (96, 208), 11, 4, 64, "mfma"),    # two channel chunks: G enters once
    (1, 768, (13, 14), (26, 224), 13, 4, 64, "mfma"),     # three chunks
    (1, 512, (15, 16), (30, 256), 15, 4, 64, "mfma"),
    (1, 1024, (15, 16), (30, 256), 15, 4, 64, "mfma"),    # four chunks at 15 x 15, Dv 256
    (1, 384, (12, 10), (168, 140), 9, 4, 64, "mfma"),     # partial row tiles: 14-pixel cells
    (2, 768, (9, 10), (126, 280), 9, 4, 64, "mfma"),      # 14 x 28 cells
    (1, 128, (5, 6), (150, 180), 5, 4, 64, "mfma"),       # 30-pixel cells
    (1, 768, (16, 16), (32, 32), 9, 4, 64, "rows"),       # ratio 2 (the reference's training step)
    (1, 3, (32, 32), (32, 32), 15, 1, 96, "rows"),        # ratio 1, one head of Dq 96 (the denoising call)
    (1, 3, (24, 24), (24, 24), 9, 1, 256, "rows"),        # ... Dq 256
    (1, 384, (12, 12), (168, 168), 11, 4, 64, "rows"),    # patch-14 ratio at 11 x 11 (few key tiles: rows shared between waves)
    (1, 128, (13, 13), (32, 32), 7, 4, 64, "generic"),    # non-integer ratio
    (1, 64, (34, 1), (799, 1), (5, 1), 1, 64, "generic"),  # 34 -> 799 by 1, rectangular window
    (1, 128, (9, 11), (40, 52), (3, 5), 4, 32, "generic"),  # rectangular window, Dq 32
]


@pytest.mark.parametrize("B,C,lr,out_sz,ksz,heads,Dq,kern", CASES)
def test_backward_with_score_gradient_matches_oracle(dev, B, C, lr, out_sz, ksz, heads, Dq, kern):
    from naf_amd import ops
    q, k, v, dout, G = inputs(B, C, lr, out_sz, ksz, heads, Dq)
    rq, rk, rv = oracle_xna_backward(dev, q, k, v, dout, G, ksz, heads)
    q5, k5, v5, g5 = (to5(t, heads).to(dev) for t in (q, k, v, dout))
    Gd = G.to(dev)
    assert ops.xna_backward_select(q5, k5, v5, ksz, dlogits=Gd) == kern
    dq, dk, dv = ops.xna_backward(q5, k5, v5, g5, ksz, dlogits=Gd)
    for got, ref, name in ((back(dq), rq, "dq"), (back(dk), rk, "dk"), (back(dv), rv, "dv")):
        check(got, ref, name)


# one case per kernel (and the chunked cell backward): a zero score gradient is the plain backward
ZERO = [
    (1, 256, (8, 8), (128, 128), 7, 4, 64, "auto"),
    (1, 1024, (15, 16), (30, 256), 15, 4, 64, "auto"),
    (1, 384, (12, 10), (168, 140), 9, 4, 64, "auto"),
    (1, 256, (8, 8), (128, 128), 7, 4, 64, "generic"),
    (1, 128, (13, 13), (32, 32), 7, 4, 64, "generic"),
    (1, 768, (16, 16), (32, 32), 9, 4, 64, "auto"),      # row-streaming kernel
]


@pytest.mark.parametrize("B,C,lr,out_sz,ksz,heads,Dq,path", ZERO)
def test_zero_score_gradient_is_the_plain_backward(dev, B, C, lr, out_sz, ksz, heads, Dq, path):
    """dlogits = 0 adds fma(scale, 0, dS) = dS: dq (written once per query, fixed order) equals the plain backward's bit for bit; dk and dv
    are added into memory by fp32 atomics, whose order varies from run to run: to 1e-6 of their largest magnitude on the cell kernel (a few
    adds per element: one per cell column leaving the window), 2e-5 on the table-driven one (one add per (query, key) pair: hundreds
    of adds per element here)."""
    from naf_amd import ops
    q, k, v, dout, G = inputs(B, C, lr, out_sz, ksz, heads, Dq)
    q5, k5, v5, g5 = (to5(t, heads).to(dev) for t in (q, k, v, dout))
    a = ops.xna_backward(q5, k5, v5, g5, ksz, path=path)
    b = ops.xna_backward(q5, k5, v5, g5, ksz, path=path, dlogits=torch.zeros_like(G, device=dev))
    assert torch.equal(a[0], b[0])
    tol = 2e-5 if ops.xna_backward_select(q5, k5, v5, ksz) == "generic" or path == "generic" else 1e-6
    for i in (1, 2):
        assert float((a[i] - b[i]).abs().max()) <= tol * float(a[i].abs().max()), ("dk", "dv")[i - 1]


@pytest.mark.parametrize("B,C,lr,out_sz,ksz,heads,Dq,kern", [CASES[0], CASES[7], CASES[11], CASES[14], CASES[18]])
def test_scores_only_loss(dev, B, C, lr, out_sz, ksz, heads, Dq, kern):
    """dO = 0, G != 0: dv is exactly zero, dq and dk match the oracle."""
    from naf_amd import ops
    q, k, v, dout, G = inputs(B, C, lr, out_sz, ksz, heads, Dq, seed=7)
    dout = torch.zeros_like(dout)
    rq, rk, _ = oracle_xna_backward(dev, q, k, v, dout, G, ksz, heads)
    q5, k5, v5, g5 = (to5(t, heads).to(dev) for t in (q, k, v, dout))
    dq, dk, dv = ops.xna_backward(q5, k5, v5, g5, ksz, dlogits=G.to(dev))
    assert not bool(dv.any())
    check(back(dq), rq, "dq")
    check(back(dk), rk, "dk")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("mode,heads_rope", [("train", 4), ("eval", 4), ("train", 2)])
def test_model_scores_gradient_matches_oracle(dev, mode, heads_rope):
    """``model(img, ft, size, return_weights="differentiable")``: the gradients of all 36 encoder parameters and of the image under
    loss = sum(out * W) + sum(scores * H) agree with fp64 autograd through ``O.naf_forward(p, ..., return_weights=True)``.  heads_rope = 4:
    the HIP RoPE / key-pooling branch of forward_train (Dq 64); heads_rope = 2: the torch-RoPE branch."""
    from naf_amd import NAF
    ksz, size, lr = 5, (48, 64), (6, 8)
    p = O.make_params(seed=44, heads_rope=heads_rope)
    m = NAF(kernel_size=ksz, heads_rope=heads_rope).eval()
    m.load_state_dict(p, strict=True)
    m = m.to(dev)
    img = O.hash_normal((1, 3, *size), 4401)
    ft = O.hash_normal((1, 64, *lr), 4402)
    W = O.hash_normal((1, 64, *size), 4403)
    H = O.hash_normal((1, 4, *size, ksz * ksz), 4404, scale=0.1)
    im = img.to(dev).requires_grad_(True)
    ftg = ft.to(dev)
    if mode == "train":
        m.train()
        m.image_encoder.rope.rescale_coords = None
    else:
        ftg = ftg.clone().requires_grad_(True)
    out, sc = m(im, ftg, size, return_weights="differentiable")
    assert sc.grad_fn is not None and sc.dtype == torch.float32 and sc.shape == H.shape
    ((out.float() * W.to(dev)).sum() + (sc * H.to(dev)).sum()).backward()
    got = {n: t.grad.detach().double().cpu() for n, t in m.named_parameters() if t.grad is not None}

    pd = {n: t.double().requires_grad_(True) for n, t in p.items()}
    imd = img.double().requires_grad_(True)
    ro, rs = O.naf_forward(pd, imd, ft.double(), size, kernel_size=ksz, heads_rope=heads_rope, return_weights=True)
    ((ro * W.double()).sum() + (rs * H.double()).sum()).backward()
    ref = {n: t.grad for n, t in pd.items() if t.grad is not None}
    common = set(got) & set(ref)
    assert len(common) == 36, sorted(set(got) ^ set(ref))
    worst = max((rel(got[n], ref[n]), n) for n in common)
    assert worst[0] < 6e-2, worst
    assert rel(im.grad.double().cpu(), imd.grad) < 6e-2


def test_scores_only_loss_trains_the_stem_and_not_the_features(dev):
    from naf_amd import NAF
    p = O.make_params(seed=45)
    m = NAF(kernel_size=5).eval()
    m.load_state_dict(p, strict=True)
    m = m.to(dev)
    img = O.hash_normal((1, 3, 48, 64), 4501).to(dev)
    ft = O.hash_normal((1, 64, 6, 8), 4502).to(dev).requires_grad_(True)
    out, sc = m(img, ft, (48, 64), return_weights="differentiable")
    pr = torch.softmax(sc, dim=-1)
    (-(pr * torch.log(pr.clamp_min(1e-30))).sum()).backward()           # entropy of the attention maps
    assert ft.grad is not None and not bool(ft.grad.any())
    g = m.image_encoder.encoder[0].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0


def test_default_return_weights_stays_non_differentiable(dev):
    """True keeps the round-6 behaviour (scores without a gradient); "differentiable" is opt-in; outside autograd both are the same."""
    from naf_amd import NAF
    p = O.make_params(seed=46)
    m = NAF(kernel_size=5).eval()
    m.load_state_dict(p, strict=True)
    m = m.to(dev)
    img = O.hash_normal((1, 3, 48, 64), 4601).to(dev)
    ft = O.hash_normal((1, 64, 6, 8), 4602).to(dev).requires_grad_(True)
    _, lg_true = m(img, ft, (48, 64), return_weights=True)
    _, lg_diff = m(img, ft, (48, 64), return_weights="differentiable")
    assert lg_true.grad_fn is None and not lg_true.requires_grad
    assert lg_diff.grad_fn is not None and lg_diff.requires_grad
    assert torch.equal(lg_true, lg_diff.detach())
    with torch.no_grad():
        _, a = m(img, ft.detach(), (48, 64), return_weights=True)
        _, b = m(img, ft.detach(), (48, 64), return_weights="differentiable")
    assert torch.equal(a, b) and a.grad_fn is None


def test_loss_on_reduced_scores(dev):
    """A loss on ``scores.sum(dim=(2, 3))`` (a regulariser on the mean attention map) hands the backward an expanded gradient -- strides
    (.., 0, 0, 1) -- which the kernels read as it is; the gradients match fp64 autograd through the oracle."""
    from naf_amd import ops
    B, C, lr, out_sz, ksz, heads = 1, 256, (8, 8), (128, 128), 7, 4
    q, k, v, dout, _ = inputs(B, C, lr, out_sz, ksz, heads)
    w = O.hash_normal((B, heads, ksz * ksz), 611)
    q5, k5, v5 = (to5(t, heads).to(dev).requires_grad_(True) for t in (q, k, v))
    out, sc = ops.XnaFunction.apply(q5, k5, v5, ksz, None, torch.float32, "differentiable")
    (torch.log_softmax(sc.sum(dim=(2, 3)), dim=-1) * w.to(dev)).sum().backward()
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    _, lg = O.xna(qd, kd, vd, ksz, heads, return_logits=True)
    (torch.log_softmax(lg.sum(dim=(2, 3)), dim=-1) * w.double()).sum().backward()
    check(back(q5.grad), qd.grad.float(), "dq")
    check(back(k5.grad), kd.grad.float(), "dk")
    assert not bool(v5.grad.any())


def test_output_only_loss_runs_the_plain_backward(dev, monkeypatch):
    """In "differentiable" mode a loss on ``out`` alone gives the scores no gradient: the backward is the plain one (no zero dlogits)."""
    from naf_amd import ops
    seen = []
    real = ops.xna_backward

    def spy(*a, **kw):
        seen.append(kw.get("dlogits"))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "xna_backward", spy)
    q, k, v, dout, _ = inputs(1, 256, (8, 8), (128, 128), 7, 4)
    q5, k5, v5 = (to5(t, 4).to(dev).requires_grad_(True) for t in (q, k, v))
    out, sc = ops.XnaFunction.apply(q5, k5, v5, 7, None, torch.float32, "differentiable")
    out.float().square().sum().backward()
    assert seen == [None] and q5.grad is not None
