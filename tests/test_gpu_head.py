"""GPU tests (-m gpu) of the fused linear head: the head-summed attention kernel (naf_xna_head_fwd) against the CPU oracle, its
rotate-on-load, the composition that serves the geometries the kernel does not, the gradient to the head (ops.XnaHeadFunction)
and ``naf(image, feats, size, head=probe)`` end to end.

Tolerances, all derived from the project's per-head bound (tests/test_gpu_parity.py::test_xna_mfma_matches_oracle: inputs rounded to
bf16, |err| <= 6e-3 + 6e-3 |ref| with fp32 output because P is rounded to bf16 before the PV product; 1.2e-2 with bf16 output):
  * kernel, G heads:   |err| <= G * 6e-3 + 6e-3 * sum_g |ref_g|   (fp32 output: every head contributes one such error, the head sum
    itself is fp32 additions); bf16 output: G * 1.2e-2 + 1.2e-2 * sum_g |ref_g| + 2^-8 |ref| (the one rounding of the stored sum).
  * composition on geometries the table-driven kernels serve: G times the bound of the test of whichever kernel ``auto`` picks there
    (2e-5 for the scalar table-driven kernel, 6e-3 for the matrix-core ones), in the same G * tol + tol * sum_g |ref_g| form.
  * gradient to PV: ``dPV_g`` is the ``dv`` of test_xna_backward_matches_oracle with one ``dout`` shared by the heads, so its bound
    applies unchanged: max err <= 2e-2 max|ref| + 1e-3, mean err <= 3e-3 max|ref| + 1e-4.
  * module level: no invented budget -- the fused error against the oracle may be at most twice the error of the unfused product
    path ``conv(naf(image, feats, size))`` against the same reference, plus the bf16 rounding of PV (2^-8 * sum_g |PV_g|-weighted bound
    computed in the test): the two paths round at different points (features vs projected values).
"""
import os
import sys

import pytest
import torch
from torch import nn

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import GENERIC_CASES, MFMA_CASES, assert_close, bf16r, oracle_xna_backward, to5  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def npad_of(N):
    return (N + 15) // 16 * 16


def make_pv(B, heads, h, w, N, seed):
    """bf16-rounded projected values [B, heads, h, w, Npad] fp32 with zero pad channels, and their NCHW (head-major) form."""
    npad = npad_of(N)
    pv = torch.zeros(B, heads, h, w, npad)
    pv[..., :N] = bf16r(O.hash_normal((B, heads, h, w, N), seed))
    return pv, pv.permute(0, 1, 4, 2, 3).reshape(B, heads * npad, h, w)


def head_reference(q, k, pvn, ksz, heads, N, bias, general=False):
    """(ref [B, N, Ho, Wo], sum_g |ref_g|): sum over heads of the oracle's attention on PV, plus bias, fp32 on the host."""
    B, _, Ho, Wo = q.shape
    o = (O.xna(q, k, pvn, ksz, heads) if general else O.xna_lowres(q, k, pvn, ksz, heads)).view(B, heads, -1, Ho, Wo)
    ref = o.sum(1)[:, :N]
    if bias is not None:
        ref = ref + bias.view(1, N, 1, 1)
    return ref, o.abs().sum(1)[:, :N]


def assert_head_close(got, ref, abs_sum, heads, out_dtype, what, base=None):
    base = base if base is not None else (6e-3 if out_dtype == torch.float32 else 1.2e-2)
    bound = heads * base + base * abs_sum + (2.0 ** -8 * ref.abs() if out_dtype == torch.bfloat16 else 0.0)
    err = (got - ref).abs()
    print(f"{what}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}, ref absmax {float(ref.abs().max()):.3f}")
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance; max err {float(err.max()):.4e}"


NS = (1, 21, 32, 151, 256)
HEAD_GEOMS = list(MFMA_CASES) + [
    # (B, h, w, dy, dx, ksz, C (unused), heads): row-tile geometries for the windows MFMA_CASES only holds with narrow cells
    (1, 12, 13, 2, 16, 11, 0, 3),         # kernel 11, three heads
    (1, 14, 13, 1, 16, 13, 0, 1),         # kernel 13, one head, one-row cells (seven dead waves per round)
    (1, 16, 15, 3, 32, 15, 0, 2),         # kernel 15, two tiles per cell row
    (1, 7, 8, 32, 16, 7, 0, 6),           # 32 tiles per cell: two rounds per workgroup, six heads
    (2, 9, 9, 14, 14, 9, 0, 12),          # the reference's window on patch-14 cells, G1's twelve heads, two images
    (1, 16, 15, 1, 16, 15, 0, 2),         # kernel 15 with N = 151: the widest windows beside ten channel tiles
    (1, 15, 16, 2, 16, 15, 0, 1),         # kernel 15 with N = 256: the largest LDS footprint (225 slots x 16 channel tiles)
]
HEAD_CASES = []
for _i, _g in enumerate(HEAD_GEOMS):
    _dts = (torch.float32, torch.bfloat16) if _i % 2 == 0 else (torch.bfloat16, torch.float32)
    HEAD_CASES += [(_g, NS[(2 * _i) % 5], _dts[0]), (_g, NS[(2 * _i + 1) % 5], _dts[1])]


def test_cases_cover_every_window_and_width_twice():
    from collections import Counter
    wins, ns = Counter(c[0][5] for c in HEAD_CASES), Counter(c[1] for c in HEAD_CASES)
    assert all(wins[k] >= 2 for k in (3, 5, 7, 9, 11, 13, 15)) and all(ns[n] >= 2 for n in NS)


@pytest.mark.parametrize("geom,N,out_dtype", HEAD_CASES, ids=lambda v: str(v).replace(" ", "").replace("torch.", ""))
def test_head_kernel_matches_oracle(dev, geom, N, out_dtype):
    """naf_xna_head_fwd (where naf_xna_head_select grants it) and the composition against the oracle, and against each other.  A geometry
    the fused kernel does not serve is asserted to SELECT the composition, which is then held to the same bound."""
    from naf_amd import ops
    B, h, w, dy, dx, ksz, _, heads = geom
    seed = sum(geom) + N
    q = bf16r(O.hash_normal((B, 64 * heads, h * dy, w * dx), seed + 1))
    k = bf16r(O.hash_normal((B, 64 * heads, h, w), seed + 2))
    pv, pvn = make_pv(B, heads, h, w, N, seed + 3)
    bias = O.hash_normal((N,), seed + 4) if (seed % 3) else None
    ref, abs_sum = head_reference(q, k, pvn, ksz, heads, N, bias)
    q5, k5 = to5(q, heads).to(dev), to5(k, heads).to(dev)
    pv5 = pv.to(dev).to(torch.bfloat16)
    bd = None if bias is None else bias.to(dev)
    served = xna_row_tiles_ok(dx)
    assert ops.xna_head_select(q5, (h, w), N, ksz, out_dtype=out_dtype) == ("fused" if served else "composed")
    auto = ops.xna_head_forward(q5, k5, pv5, bd, ksz, n_out=N, out_dtype=out_dtype)
    assert auto.shape == (B, N, h * dy, w * dx) and auto.dtype == out_dtype
    assert auto.permute(0, 2, 3, 1).is_contiguous()           # a logical NCHW view of a dense channels-last buffer
    comp = ops.xna_head_forward(q5, k5, pv5, bd, ksz, n_out=N, out_dtype=out_dtype, path="composed").float().cpu()
    assert_head_close(comp, ref, abs_sum, heads, out_dtype, f"composed {geom} N={N}")
    auto = auto.float().cpu()
    assert torch.isfinite(auto).all()
    assert_head_close(auto, ref, abs_sum, heads, out_dtype, f"auto {geom} N={N}")
    if served:
        fused = ops.xna_head_forward(q5, k5, pv5, bd, ksz, n_out=N, out_dtype=out_dtype, path="fused").float().cpu()
        assert torch.equal(fused, auto)
        assert_head_close(fused, comp, abs_sum, heads, out_dtype, f"fused vs composed {geom} N={N}")
    else:
        from naf_amd._lib import NafHipError
        with pytest.raises(NafHipError, match="fused kernel"):
            ops.xna_head_forward(q5, k5, pv5, bd, ksz, n_out=N, out_dtype=out_dtype, path="fused")
        assert torch.equal(comp, auto)


def xna_row_tiles_ok(dx):
    pad = ((dx + 15) & ~15) - dx
    return pad * 6 <= dx


_BASE = {"generic": 2e-5, "union": 6e-3, "rows": 6e-3, "mfma": 6e-3}


@pytest.mark.parametrize("case,N", list(zip(GENERIC_CASES, (21, 1, 151, 32, 256, 19))), ids=lambda v: str(v).replace(" ", ""))
def test_composition_serves_what_the_table_kernels_serve(dev, case, N):
    """Non-integer ratios, ratio 1, tiny cells, Dq = 96: ``auto`` selects the composition (asserted, not skipped) and it matches the oracle
    at G times the bound of the kernel ``xna_forward`` picks for the projected values."""
    from naf_amd import ops
    B, Cq, heads, (Ho, Wo), (h, w), ksz, _ = case
    q = bf16r(O.hash_normal((B, Cq, Ho, Wo), 41))
    k = bf16r(O.hash_normal((B, Cq, h, w), 42))
    pv, pvn = make_pv(B, heads, h, w, N, 43)
    bias = O.hash_normal((N,), 44)
    ref, abs_sum = head_reference(q, k, pvn, ksz, heads, N, bias, general=True)
    q5, k5, pv5 = to5(q, heads).to(dev), to5(k, heads).to(dev), pv.to(dev).to(torch.bfloat16)
    assert ops.xna_head_select(q5, (h, w), N, ksz) == "composed"
    kern = ops.xna_select(q5, k5, pv5, ksz, out_dtype=torch.float32)
    out = ops.xna_head_forward(q5, k5, pv5, bias.to(dev), ksz, n_out=N, out_dtype=torch.float32).float().cpu()
    assert_head_close(out, ref, abs_sum, heads, torch.float32, f"composition ({kern}) {case} N={N}", base=_BASE[kern])


@pytest.mark.parametrize("B,heads,lr,out_sz,ksz,N,out_dtype", [
    (1, 4, (8, 8), (128, 128), 7, 21, torch.bfloat16),        # d = 16: one row tile per cell row
    (2, 4, (6, 5), (192, 160), 5, 151, torch.float32),        # d = 32: two tiles per cell row, four rounds
    (1, 12, (10, 9), (160, 144), 9, 19, torch.float32),       # G1's head count at the reference's window
    (1, 3, (6, 7), (84, 98), 5, 32, torch.bfloat16),          # patch 14: partial row tiles
    (1, 4, (5, 5), (35, 150), 3, 256, torch.float32),         # dx = 30: a full and a 14-pixel tile per row
])
def test_head_rotate_on_load_equals_materialised_queries(dev, B, heads, lr, out_sz, ksz, N, out_dtype):
    """naf_xna_head_fwd(rope_tab_*) on un-rotated guidance == naf_rope_pool_fwd queries + naf_xna_head_fwd, bit for bit (same rotation
    arithmetic and bf16 rounding), and both match the oracle's rope + attention."""
    from naf_amd import ops
    Dq = 64
    x = bf16r(O.hash_normal((B, heads * Dq, *out_sz), 310))
    pv, pvn = make_pv(B, heads, *lr, N, 311)
    bias = O.hash_normal((N,), 312)
    per = O.rope_periods(heads * Dq, heads, 100.0)
    xd = x.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ty, tx = ops.rope_tables(per.to(dev), *out_sz)
    q_mat, k5 = ops.rope_pool(xd, ty, tx, heads, lr)
    q_raw = xd.permute(0, 2, 3, 1).unflatten(3, (heads, Dq)).permute(0, 3, 1, 2, 4)
    assert ops.xna_head_select(q_raw, lr, N, ksz, out_dtype=out_dtype, rope_tables=(ty, tx)) == "fused"
    pv5, bd = pv.to(dev).to(torch.bfloat16), bias.to(dev)
    a = ops.xna_head_forward(q_mat, k5, pv5, bd, ksz, n_out=N, out_dtype=out_dtype, path="fused")
    b = ops.xna_head_forward(q_raw, k5, pv5, bd, ksz, n_out=N, out_dtype=out_dtype, path="fused", rope_tables=(ty, tx))
    assert torch.equal(a, b), f"rotate-on-load differs from materialised queries: {float((a.float() - b.float()).abs().max())}"
    ref_q = bf16r(O.rope(x, per, heads))
    ref_k = bf16r(O.key_pool(O.rope(x, per, heads), lr))
    ref, abs_sum = head_reference(ref_q, ref_k, pvn, ksz, heads, N, bias)
    # queries and keys carry one more bf16 rounding than the oracle's (the existing rotate-on-load test allows 2e-2 per head for it)
    assert_head_close(b.float().cpu(), ref, abs_sum, heads, out_dtype, "rotate-on-load vs oracle", base=2e-2)


@pytest.mark.parametrize("ksz,N", [(7, 21), (9, 151), (15, 32)])
def test_head_peaked_softmax(dev, ksz, N):
    """Large logits (|s| ~ 40): one key dominates each head.  The per-head normalisation (P scaled by 1 / sum before it is packed)
    stays finite and within the parity bound."""
    from naf_amd import ops
    B, heads, h, w, d = 1, 4, 16, 16, 16
    q = bf16r(O.hash_normal((B, 256, h * 2, w * d), 9) * 4.0)
    k = bf16r(O.hash_normal((B, 256, h, w), 10) * 4.0)
    pv, pvn = make_pv(B, heads, h, w, N, 11)
    lg = torch.einsum("bchw,bchw->bhw", q[:, :64, ::2, ::d], k[:, :64]) / 8.0
    assert float(lg.abs().max()) > 25.0
    ref, abs_sum = head_reference(q, k, pvn, ksz, heads, N, None)
    q5, k5, pv5 = to5(q, heads).to(dev), to5(k, heads).to(dev), pv.to(dev).to(torch.bfloat16)
    out = ops.xna_head_forward(q5, k5, pv5, None, ksz, n_out=N, out_dtype=torch.float32, path="fused").float().cpu()
    assert torch.isfinite(out).all()
    assert_head_close(out, ref, abs_sum, heads, torch.float32, f"peaked softmax k={ksz}")


@pytest.mark.parametrize("B,heads,lr,out_sz,ksz,N", [
    (1, 4, (8, 8), (128, 128), 7, 21),         # the cell backward at Dv = 32
    (2, 4, (10, 9), (80, 288), 9, 151),        # 9x9, dx = 32, Npad = 160 -> padded to the backward's 192
    (1, 2, (15, 16), (30, 256), 15, 19),       # 15x15
    (1, 4, (12, 10), (168, 140), 9, 27),       # patch 14: partial row tiles
])
def test_head_function_gradients_match_oracle(dev, B, heads, lr, out_sz, ksz, N):
    """ops.XnaHeadFunction: dPV against fp64 autograd through the oracle's forward with ONE dout [B, N, Ho, Wo] shared by the heads
    (test_xna_backward_matches_oracle's dv with a particular dout: its bound applies unchanged), dbias against dout.sum."""
    from naf_amd import ops
    npad = npad_of(N)
    q = bf16r(O.hash_normal((B, 64 * heads, *out_sz), 501))
    k = bf16r(O.hash_normal((B, 64 * heads, *lr), 502))
    pv, pvn = make_pv(B, heads, *lr, N, 503)
    dout = bf16r(O.hash_normal((B, N, *out_sz), 504))
    d5 = torch.zeros(B, heads, npad, *out_sz)
    d5[:, :, :N] = dout[:, None]
    _, _, rv = oracle_xna_backward(dev, q, k, pvn, d5.reshape(B, heads * npad, *out_sz), ksz, heads)
    ref = rv.view(B, heads, npad, *lr).permute(0, 1, 3, 4, 2)
    q5, k5 = to5(q, heads).to(dev), to5(k, heads).to(dev)
    pv5 = pv.to(dev).to(torch.bfloat16).requires_grad_(True)
    bias = O.hash_normal((N,), 505).to(dev).requires_grad_(True)
    out = ops.XnaHeadFunction.apply(q5, k5, pv5, bias, ksz, N, torch.float32)
    assert out.requires_grad and not q5.requires_grad
    (out * dout.to(dev)).sum().backward()
    got = pv5.grad.float().cpu()
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    print(f"dPV k={ksz} N={N}: max err {float(err.max()):.3e} mean {float(err.mean()):.3e} (ref max {scale:.3e})")
    assert float(err.max()) <= 2e-2 * scale + 1e-3 and float(err.mean()) <= 3e-3 * scale + 1e-4, \
        f"dPV: max err {float(err.max()):.3e} mean {float(err.mean()):.3e} (ref max {scale:.3e})"
    assert float(got[..., N:].abs().max()) == 0.0 if npad > N else True
    rb = dout.double().sum(dim=(0, 2, 3))
    eb = float((bias.grad.double().cpu() - rb).abs().max())
    # fp32 summation of B*Ho*Wo terms of magnitude <= max|dout|: error <= n * 2^-24 * max|dout| in the worst case
    nterm = B * out_sz[0] * out_sz[1]
    assert eb <= nterm * 2.0 ** -24 * float(dout.abs().max()), f"dbias err {eb:.3e}"


# ---- module level -----------------------------------------------------------------------------------------------
def _load_model(dev, params, **kw):
    from naf_amd import NAF
    m = NAF(**kw).eval()
    m.load_state_dict(params, strict=True)
    return m.to(dev)


def _probe(Cc, N, seed, dev, dtype=torch.float32):
    conv = nn.Conv2d(Cc, N, 1)
    with torch.no_grad():
        conv.weight.copy_(O.hash_normal((N, Cc, 1, 1), seed) * Cc ** -0.5)
        conv.bias.copy_(O.hash_normal((N,), seed + 1))
    return conv.to(dev).to(dtype)


@pytest.mark.parametrize("size,lr,Cc,ksz,N,fdt", [
    ((224, 224), (14, 14), 384, 9, 21, torch.float32),      # F5 / P1 size: fp32 features (the golden's dtype)
    ((224, 224), (14, 14), 384, 9, 151, torch.bfloat16),    # ... bf16 features, ADE's 151 classes
    ((448, 448), (28, 28), 384, 9, 21, torch.bfloat16),     # the reference's own probing point
])
def test_module_head_matches_oracle_within_the_unfused_error(dev, size, lr, Cc, ksz, N, fdt):
    """naf(image, feats, size, head=conv) against O.naf_forward(...) followed by the head in fp32.  The budget is the unfused product
    path's own error against the same reference (x 2) plus the bf16 rounding of PV."""
    p = O.make_params(seed=31)
    m = _load_model(dev, p, kernel_size=ksz)
    heads = m.upsampler.num_heads
    img = O.hash_normal((1, 3, *size), 601)
    ft = O.hash_normal((1, Cc, *lr), 602)
    if fdt == torch.bfloat16:
        ft = bf16r(ft)
    conv = _probe(Cc, N, 603, dev)
    wt, bs = conv.weight.detach().float().cpu(), conv.bias.detach().float().cpu()
    up_ref = O.naf_forward_fast(p, img, ft, size, kernel_size=ksz) if size[0] > 256 else O.naf_forward(p, img, ft, size, kernel_size=ksz)
    ref = torch.nn.functional.conv2d(up_ref, wt, bs)
    with torch.no_grad():
        fused = m(img.to(dev), ft.to(dev).to(fdt), size, head=conv)
        unfused = conv(m(img.to(dev), ft.to(dev).to(fdt), size).float())
    assert fused.shape == (1, N, *size) and fused.dtype == torch.float32 and not fused.requires_grad
    assert fused.stride() == (size[0] * size[1] * N, 1, size[1] * N, N)
    e_f = (fused.float().cpu() - ref).abs()
    e_u = (unfused.float().cpu() - ref).abs()
    # bf16 rounding of PV: every PV_g[n, cell] moves by at most 2^-8 |PV_g[n, cell]|, the attention is a convex combination per head:
    # the logit moves by at most 2^-8 * sum_g max over the grid of |PV_g[n]|
    pvf = torch.einsum("ngd,bgdhw->bgnhw", wt[:, :, 0, 0].reshape(N, heads, Cc // heads), ft.reshape(1, heads, Cc // heads, *lr))
    pv_round = 2.0 ** -8 * float(pvf.abs().amax(dim=(0, 3, 4)).sum(0).max())
    print(f"module head {size} N={N} {fdt}: fused max err {float(e_f.max()):.4e} mean {float(e_f.mean()):.4e}; "
          f"unfused max err {float(e_u.max()):.4e} mean {float(e_u.mean()):.4e}; PV rounding bound {pv_round:.4e}")
    assert float(e_f.max()) <= 2.0 * float(e_u.max()) + pv_round
    assert float(e_f.mean()) <= 2.0 * float(e_u.mean()) + pv_round


def test_module_head_forms_dtypes_and_empty_batch(dev):
    p = O.make_params(seed=32)
    m = _load_model(dev, p, kernel_size=7)
    img, ft = O.hash_normal((2, 3, 96, 128), 611).to(dev), O.hash_normal((2, 128, 8, 8), 612).to(dev)
    conv = _probe(128, 19, 613, dev)
    lin = nn.Linear(128, 19).to(dev)
    with torch.no_grad():
        lin.weight.copy_(conv.weight[:, :, 0, 0])
        lin.bias.copy_(conv.bias)
        a = m(img, ft, (96, 128), head=conv)
        b = m(img, ft, (96, 128), head=lin)
        c = m(img, ft, (96, 128), head=(conv.weight.detach(), conv.bias.detach()))
        d = m(img, ft, (96, 128), head=(conv.weight.detach()[:, :, 0, 0], None))
        e = m(img, ft, (96, 128), head=_probe(128, 19, 613, dev, torch.bfloat16))
        z = m(img[:0], ft[:0], (96, 128), head=conv)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert float((d + conv.bias.detach().view(1, -1, 1, 1) - a).abs().max()) <= 1e-5
    assert e.dtype == torch.bfloat16 and e.shape == a.shape and float((e.float() - a).abs().max()) <= 0.05 + 2.0 ** -7 * float(a.abs().max())
    assert z.shape == (0, 19, 96, 128) and z.dtype == torch.float32
    with pytest.raises(ValueError, match="return_weights"):
        m(img, ft, (96, 128), return_weights=True, head=conv)
    # a geometry the fused kernel does not serve (non-integer ratio) goes through the composition: same contract
    with torch.no_grad():
        f = m(img, ft, (50, 70), head=conv)
        g = conv(m(img, ft, (50, 70)).float())
    assert f.shape == (2, 19, 50, 70) and float((f - g).abs().max()) <= 0.05 + 1e-2 * float(g.abs().max())


def test_module_head_gradients(dev):
    """Probe training: weight and bias gradients of naf(..., head=conv).float().square().mean() against torch autograd through conv(up)
    with ``up`` the unfused product output (fp32, detached) -- both are linear maps of the same upsampled features, so the comparison
    isolates the new path.  Bound: the relative part of the operator-level one, 2e-2 max|ref| of each gradient (no absolute term: these
    gradients are small numbers).  The upsampler
    gets no gradient on this path; a call that wants one takes the unfused route, bit for bit head(naf.forward_train(...))."""
    p = O.make_params(seed=33)
    m = _load_model(dev, p, kernel_size=9)
    size, lr, Cc, N = (160, 192), (10, 12), 256, 21
    img, ft = O.hash_normal((2, 3, *size), 621).to(dev), bf16r(O.hash_normal((2, Cc, *lr), 622)).to(dev).to(torch.bfloat16)
    conv, conv_ref = _probe(Cc, N, 623, dev), _probe(Cc, N, 623, dev)
    assert not m.training and any(q.requires_grad for q in m.parameters())
    out = m(img, ft, size, head=conv)
    assert out.requires_grad and out.shape == (2, N, *size)
    out.float().square().mean().backward()
    assert all(q.grad is None for q in m.parameters()), "the frozen upsampler received a gradient"
    with torch.no_grad():
        up = m(img, ft, size).float()
    conv_ref(up).square().mean().backward()
    for name, got, ref in (("weight", conv.weight.grad, conv_ref.weight.grad), ("bias", conv.bias.grad, conv_ref.bias.grad)):
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        print(f"module head grad {name}: max err {err:.3e} (ref max {scale:.3e}, relative {err / scale:.3e})")
        assert err <= 2e-2 * scale, f"{name}: grad err {err:.3e} vs max {scale:.3e}"
    # a gradient wanted for the upsampler: the unfused composition
    m.train()
    conv.zero_grad()
    torch.manual_seed(5)
    a = m(img, ft.float(), size, head=conv)
    torch.manual_seed(5)
    b = conv(m.forward_train(img, ft.float(), size))
    assert torch.equal(a, b)
    a.float().square().mean().backward()
    assert any(q.grad is not None and float(q.grad.abs().sum()) > 0 for q in m.image_encoder.parameters())
    m.eval()
    # ... and so does an input that requires grad, in eval mode
    fr = ft.float().requires_grad_(True)
    c = m(img, fr, size, head=conv)
    c.float().square().mean().backward()
    assert fr.grad is not None and float(fr.grad.abs().sum()) > 0
