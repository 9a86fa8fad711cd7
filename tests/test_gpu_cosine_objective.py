"""GPU tests (-m gpu) of the cosine objective: naf_xna_cos_ce_fwd / ``ops.xna_cos_objective`` / ``ops.XnaCosCEFunction`` /
``naf(image, feats, size, head=E, cosine=True, target=t, loss="ce")`` against the fp64 restatement and its derived per-element bounds
(tests/cosine_objective_reference.py: nothing measured), the exact properties of the kernel (zero features, power-of-two scales, optional
outputs, repeatability, target layouts), the attention backward fed the kernel's own gradient, and the module-level rule
max |fused - ref| <= 2 max |composed - ref| + 2^-8 max |ref| with the composition measured in the same test on the same inputs.

Every fused case first asserts that ``ops.xna_cos_ce_select`` grants the kernel, so nothing is silently composed."""
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_reference as R  # noqa: E402
import cosine_objective_reference as Q  # noqa: E402
from test_gpu_parity import bf16r, oracle_xna_backward, to5  # noqa: E402

pytestmark = pytest.mark.gpu
SCALES = (10.0, 30.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _base(name, zero_block=None):
    B, heads, Dv, lr, cell, ks, N = R.CASES[name]
    q, k, v, E = R.make_inputs(name, zero_block=zero_block)
    return (q, k, v, E, ks, heads), R.reference(q, k, v, E, ks, heads, 1.0), Q.make_target(name)


@functools.lru_cache(maxsize=None)
def _case(name, ls, zero_block=None):
    """Inputs, the fp64 reference at scale ``ls`` and the objective on it: computed once per case and shared (never modified).  The
    reference at another scale is the same reference with its cosines scaled (cos = ls * num / norms)."""
    inp, r1, t = _base(name, zero_block)
    r = dict(r1, cos=r1["cos"] * ls, ls=float(ls))
    return inp, r, Q.objective(r, t), t


def _operands(q, k, v, heads, dev):
    return to5(q, heads).to(dev), to5(k, heads).to(dev), to5(v, heads).to(dev)


def _granted(q5, v5, N, ks):
    from naf_amd import ops
    assert ops.xna_cos_ce_select(q5, v5.shape[2:4], v5.shape[4], N, ks) == "fused", "the fused kernel was not granted"


def _run(dev, name, ls, t=None, **kw):
    from naf_amd import ops
    (q, k, v, E, ks, heads), r, o, tt = _case(name, float(ls) if not isinstance(ls, torch.Tensor) else float(ls.item()), kw.pop("zero_block", None))
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    _granted(q5, v5, E.shape[0], ks)
    want = dict(want_loss=True, want_labels=True, want_dlogits=True, want_dscale=True)
    want.update(kw)
    return ops.xna_cos_objective(q5, k5, v5 * want.pop("vscale", 1.0), E.to(dev), ks, target=(tt if t is None else t).to(dev), ignore_index=Q.IGNORE,
                                 logit_scale=ls, path="fused", **want)


@pytest.mark.parametrize("ls", SCALES)
@pytest.mark.parametrize("name", Q.GPU_CASES)
def test_kernel_outputs_match_the_restatement(dev, name, ls):
    """Loss, labels, g' and ds of one launch against the fp64 restatement under the derived bounds: every element, NaN counted as a miss."""
    (q, k, v, E, ks, heads), r, o, t = _case(name, ls)
    B, N = q.shape[0], E.shape[0]
    loss, labels, g, ds = _run(dev, name, ls)
    Ho, Wo = q.shape[-2:]
    assert loss.shape == ds.shape == labels.shape == (B, Ho, Wo) and g.shape == (B, Ho, Wo, Q.gc_of(N))
    assert loss.dtype == ds.dtype == torch.float32 and labels.dtype == torch.uint8 and g.dtype == torch.bfloat16
    R.check(loss.cpu(), o["loss"], Q.loss_bound(r, o), f"loss {name} s={ls}")
    Q.check_labels(labels.cpu(), r, o, f"labels {name} s={ls}")
    R.check(g[..., :N].float().cpu(), o["g"], Q.g_bound(r, o), f"g' {name} s={ls}")
    R.check(ds.cpu(), o["ds"], Q.ds_bound(r, o), f"ds {name} s={ls}")
    inv = ~o["valid"]
    gz = g.float().cpu()
    assert float(gz[..., N:].abs().max()) == 0.0 if g.shape[-1] > N else True          # pad channels, also past the accumulators
    assert float(gz[inv].abs().max()) == 0.0 and float(loss.cpu()[inv].abs().max()) == 0.0 and float(ds.cpu()[inv].abs().max()) == 0.0
    if N == 1:
        assert float(loss.abs().max()) == 0.0 and float(gz.abs().max()) == 0.0 and int(labels.max()) == 0


def test_device_scale_is_bit_equal_to_the_float(dev):
    name, ls = "a_c128_k7_n21", 10.0
    a = _run(dev, name, ls)
    b = _run(dev, name, torch.tensor([ls], device=dev))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    from naf_amd import ops
    (q, k, v, E, ks, heads), r, o, t = _case(name, ls)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    cos = ops.xna_cos_forward(q5, k5, v5, E.to(dev), ks, logit_scale=ls, path="fused")
    assert torch.equal(a[1].long(), cos.argmax(1))                     # the z of the objective are the cosines the forward stores


def test_zero_features_give_ln_n_and_a_zero_gradient(dev):
    name, ls, blk = "e_patch14_n21", 10.0, (0, 6, 0, 6)
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    (q, k, v, E, ks, heads), r, o, t = _case(name, ls, blk)
    loss, labels, g, ds = _run(dev, name, ls, zero_block=blk)
    m = R.sees_only(blk, h, w, ks).repeat_interleave(dy, 0).repeat_interleave(dx, 1).unsqueeze(0)
    mv = m & o["valid"]
    assert int(mv.sum()) >= dy * dx // 2
    R.check(loss.cpu(), o["loss"], Q.loss_bound(r, o), "zero block loss")
    assert float((loss.cpu()[mv].double() - math.log(N)).abs().max()) <= 1e-5 * (1.0 + math.log(N))
    assert float(g.float().cpu()[m.expand(B, -1, -1)].abs().max()) == 0.0 and float(ds.cpu()[m.expand(B, -1, -1)].abs().max()) == 0.0
    assert bool(torch.isfinite(g.float()).all()) and int(labels.cpu()[m.expand(B, -1, -1)].max()) == 0
    R.check(g[..., :N].float().cpu(), o["g"], Q.g_bound(r, o), "zero block g'")


@pytest.mark.parametrize("name", ["a_c128_k7_n21", "f_rows30_n151"])
def test_exact_properties_of_the_launch(dev, name):
    """Features x 2^k change no bit of loss or labels; every output alone equals the same output of the launch that stores all four; two
    launches are bit-equal; a non-contiguous and an int32 target are the same call."""
    ls = 10.0
    (q, k, v, E, ks, heads), r, o, t = _case(name, ls)
    full = _run(dev, name, ls)
    again = _run(dev, name, ls)
    assert all(torch.equal(x, y) for x, y in zip(full, again))
    for f in (4.0, 0.125):
        sc = _run(dev, name, ls, vscale=f)
        assert torch.equal(sc[0], full[0]) and torch.equal(sc[1], full[1]) and torch.equal(sc[3], full[3])
    names = ("want_loss", "want_labels", "want_dlogits", "want_dscale")
    for i, nm in enumerate(names):
        one = _run(dev, name, ls, **{n_: n_ == nm for n_ in names})
        assert torch.equal(one[i], full[i]) and all(one[j] is None for j in range(4) if j != i)
    wide = torch.full((t.shape[0], t.shape[1], t.shape[2] * 2), 7, dtype=torch.int64)
    wide[:, :, ::2] = t
    nc = wide.to(dev)[:, :, ::2]
    assert not nc.is_contiguous()
    from naf_amd import ops
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    kw = dict(ignore_index=Q.IGNORE, logit_scale=ls, path="fused", want_loss=True, want_dlogits=True)
    for tt in (nc, t.to(dev).to(torch.int32)):
        got = ops.xna_cos_objective(q5, k5, v5, E.to(dev), ks, target=tt, **kw)
        assert torch.equal(got[0], full[0]) and torch.equal(got[2], full[2])


def test_refused_instantiation_composes_under_auto(dev):
    """Window 13 with 151 embeddings has no instantiation (it would spill): select refuses it with the reason, "fused" raises, "auto"
    composes under the same contract (held to the composition's own cosine bound)."""
    from naf_amd import ops
    from naf_amd._lib import NafHipError
    name, ls = "j_k13_n21", 10.0
    B, heads, Dv, (h, w), (dy, dx), ks, _ = R.CASES[name]
    q, k, v, _ = R.make_inputs(name)
    N = 151
    E = O.hash_normal((N, heads * Dv), 5200) * 3.0
    t = torch.randint(0, N, (B, h * dy, w * dx), generator=torch.Generator().manual_seed(3))
    t[:, :2] = Q.IGNORE
    r = R.reference(q, k, v, E, ks, heads, ls)
    o = Q.objective(r, t)
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    assert ops.xna_cos_ce_select(q5, (h, w), Dv, N, ks) == "composed"
    with pytest.raises(NafHipError, match="window 13"):
        ops.xna_cos_objective(q5, k5, v5, E.to(dev), ks, target=t.to(dev), ignore_index=Q.IGNORE, logit_scale=ls, want_loss=True, path="fused")
    loss, labels, g, ds = ops.xna_cos_objective(q5, k5, v5, E.to(dev), ks, target=t.to(dev), ignore_index=Q.IGNORE, logit_scale=ls, want_loss=True,
                                                want_labels=True, want_dlogits=True, want_dscale=True)
    beta = R.composed_bound(r)[0].amax(dim=1)
    R.check(loss.cpu(), o["loss"], 2.0 * beta + 1e-5 * (1.0 + o["lse"].abs() + o["zt"].abs()), "composed loss, window 13 N = 151")
    assert g.shape[-1] == 192 and float(g[..., N:].float().abs().max()) == 0.0 and float(g[:, :2].float().abs().max()) == 0.0
    assert labels.dtype == torch.uint8 and ds.shape == loss.shape


@pytest.mark.parametrize("name", ["a_c128_k7_n21", "f_rows30_n151"])
def test_backward_kernel_gets_the_values_gradient_from_the_kernels_own_g(dev, name):
    """dPV of ops.XnaCosCEFunction(reduction="sum") against the oracle's fp64 backward FED THE KERNEL'S OWN g' (one dout shared by the heads),
    under the bound of test_gpu_head.py::test_head_function_gradients_match_oracle; pad channels exactly 0."""
    from naf_amd import ops
    ls = 10.0
    (q, k, v, E, ks, heads), r, o, t = _case(name, ls)
    B, N = q.shape[0], E.shape[0]
    Ho, Wo = q.shape[-2:]
    h, w = v.shape[-2:]
    npad = (N + 15) // 16 * 16
    q5, k5, v5 = _operands(q, k, v, heads, dev)
    _granted(q5, v5, N, ks)
    Ed = E.to(dev)
    pv5 = ops.project_cosine_values(Ed, v5).detach().requires_grad_(True)
    loss = ops.XnaCosCEFunction.apply(q5, k5, pv5, v5, Ed, ls, t.to(dev), ks, Q.IGNORE, "sum", False, "fused")
    assert loss.requires_grad and loss.dim() == 0
    loss.backward()
    _, _, g, _ = _run(dev, name, ls)
    d5 = torch.zeros(B, heads, npad, Ho, Wo)
    d5[:, :, :N] = g[..., :N].float().cpu().permute(0, 3, 1, 2)[:, None]
    pvn = pv5.detach().float().cpu().permute(0, 1, 4, 2, 3).reshape(B, heads * npad, h, w)
    _, _, rv = oracle_xna_backward(dev, q, k, pvn, d5.reshape(B, heads * npad, Ho, Wo), ks, heads)
    ref = rv.view(B, heads, npad, h, w).permute(0, 1, 3, 4, 2)
    got = pv5.grad.float().cpu()
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    print(f"dPV {name}: max err {float(err.max()):.3e} mean {float(err.mean()):.3e} (ref max {scale:.3e})")
    assert float(err.max()) <= 2e-2 * scale + 1e-3 and float(err.mean()) <= 3e-3 * scale + 1e-4
    assert float(got[..., N:].abs().max()) == 0.0 if npad > N else True
    R.check(loss.detach().cpu().reshape(1), o["loss"].sum().reshape(1), Q.loss_bound(r, o).sum().reshape(1), "summed loss")


# ---- module level -----------------------------------------------------------------------------------------------
def _load_model(dev, params, **kw):
    from naf_amd import NAF
    m = NAF(**kw).eval()
    m.load_state_dict(params, strict=True)
    return m.to(dev)


@functools.lru_cache(maxsize=None)
def _module_ref(size, lr, Cc, ksz, N, ls):
    p = O.make_params(seed=33)
    img = O.hash_normal((1, 3, *size), 901)
    ft = bf16r(O.hash_normal((1, Cc, *lr), 902))
    E = O.hash_normal((N, Cc), 903)
    t = torch.randint(0, N, (1, *size), generator=torch.Generator().manual_seed(904))
    t[:, :9, :40] = Q.IGNORE
    t[:, -1, :3] = torch.tensor([N, -2, N + 7])
    up = O.naf_forward(p, img, ft, size, kernel_size=ksz)
    return p, img, ft, E, t, Q.autograd_reference(up, E, ls, t)


GEOMS = [((128, 128), (8, 8), 128, 7, 21), ((112, 112), (8, 8), 128, 7, 21)]      # 16-pixel cells; 14-pixel cells (partial row tiles)


@pytest.mark.parametrize("size,lr,Cc,ksz,N", GEOMS)
def test_module_loss_and_gradients_within_the_composed_error(dev, size, lr, Cc, ksz, N):
    """loss, E.grad and s.grad of ``loss="ce"`` (reduction="sum") against fp64 autograd of the definition on the oracle's forward:
    max |fused - ref| <= 2 max |composed - ref| + 2^-8 max |ref|, the composition being today's route measured here on the same inputs."""
    ls = 10.0
    p, img, ft, E, t, (ref_l, ref_dE, ref_ds) = _module_ref(size, lr, Cc, ksz, N, ls)
    m = _load_model(dev, p, kernel_size=ksz)
    imgd, ftd, td = img.to(dev), ft.to(dev).to(torch.bfloat16), t.to(dev)
    res = {}
    for path in ("fused", "composed"):
        Eg = E.to(dev).requires_grad_(True)
        s = torch.tensor([ls], device=dev, requires_grad=True)
        loss = m(imgd, ftd, size, head=Eg, cosine=True, logit_scale=s, target=td, loss="ce", ignore_index=Q.IGNORE, reduction="sum", cosine_path=path)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
        loss.backward()
        res[path] = (loss.detach().cpu().double(), Eg.grad.cpu().double(), s.grad.cpu().double().reshape(()))
    Eg = E.to(dev).requires_grad_(True)
    auto = m(imgd, ftd, size, head=Eg, cosine=True, logit_scale=ls, target=td, loss="ce", ignore_index=Q.IGNORE, reduction="sum")
    assert torch.equal(auto.detach().cpu().double(), res["fused"][0])          # "auto" is the fused route here, float or tensor scale alike
    for what, i, ref in (("loss", 0, ref_l), ("E.grad", 1, ref_dE), ("s.grad", 2, ref_ds)):
        ef, ec = float((res["fused"][i] - ref).abs().max()), float((res["composed"][i] - ref).abs().max())
        print(f"module {size} {what}: fused err {ef:.4e} composed err {ec:.4e} ref max {float(ref.abs().max()):.4e}")
    for what, i, ref in (("loss", 0, ref_l), ("E.grad", 1, ref_dE), ("s.grad", 2, ref_ds)):
        ef, ec = float((res["fused"][i] - ref).abs().max()), float((res["composed"][i] - ref).abs().max())
        assert ef <= 2.0 * ec + 2.0 ** -8 * float(ref.abs().max()), f"{what}: fused err {ef:.4e}, composed err {ec:.4e}"


def test_module_routes_reductions_guidance_and_labels(dev):
    from naf_amd._lib import NafHipError
    size, lr, Cc, ksz, N = GEOMS[0]
    ls = 10.0
    p, img, ft, E, t, _ = _module_ref(size, lr, Cc, ksz, N, ls)
    m = _load_model(dev, p, kernel_size=ksz)
    imgd, ftd, td, Ed = img.to(dev), ft.to(dev).to(torch.bfloat16), t.to(dev), E.to(dev)
    call = lambda *a, **kw: m(*a, **{"head": Ed, "cosine": True, "logit_scale": ls, "target": td, "loss": "ce", "ignore_index": Q.IGNORE, **kw})
    with torch.no_grad():
        tot = call(imgd, ftd, size, reduction="sum")
        none = call(imgd, ftd, size, reduction="none")
        mean = call(imgd, ftd, size)
        assert none.shape == (1, *size) and torch.equal(none.sum(), tot)
        nvalid = int(((td != Q.IGNORE) & (td >= 0) & (td < N)).sum())
        assert torch.equal(mean, tot / nvalid) and float(none[:, :9, :40].abs().max()) == 0.0
        assert torch.equal(call(m.guide(imgd), ftd, size, reduction="none"), none)               # a Guidance call is the image call
        loss2, pred = call(imgd, ftd, size, predict=True)
        assert torch.equal(loss2, mean) and pred.dtype == torch.int64 and pred.shape == (1, *size)
        comp_l, comp_p = call(imgd, ftd, size, predict=True, cosine_path="composed")
        assert float((pred == comp_p).float().mean()) >= 0.99 and abs(float(comp_l - mean)) <= 2.0 ** -8 * float(mean)
        # the labels of the existing launch (argmax of E^ . f, before the division by the norm): the same but for near-ties
        assert float((pred == m(imgd, ftd, size, head=Ed, cosine=True, predict=True)).float().mean()) >= 0.999
    # the fused route with a gradient for E: runs under "fused"; the recorded graph is the same whatever the reduction
    Eg = Ed.clone().requires_grad_(True)
    ln, pr = call(imgd, ftd, size, head=Eg, reduction="none", predict=True, cosine_path="fused")
    assert torch.equal(pr, pred) and torch.equal(ln.detach(), none)
    ln.sum().backward()
    g_none = Eg.grad.clone()
    Eg.grad = None
    call(imgd, ftd, size, head=Eg, reduction="sum", cosine_path="fused").backward()
    assert float((g_none - Eg.grad).abs().max()) <= 2.0 ** -7 * float(Eg.grad.abs().max())       # dPV is rounded to bf16 on both
    g_sum = Eg.grad.clone()
    Eg.grad = None
    call(imgd, ftd, size, head=Eg, cosine_path="fused").backward()
    assert float((g_sum / nvalid - Eg.grad).abs().max()) <= 2.0 ** -7 * float(Eg.grad.abs().max())
    with pytest.raises(NafHipError, match="bfloat16 features"):
        call(imgd, ftd.float(), size, head=Eg, cosine_path="fused")
    with pytest.raises(NafHipError, match="integer ratio"):
        call(imgd, ftd, (100, 100), head=Eg, target=td[:, :100, :100], cosine_path="fused")
    # ... and "auto" composes both, differentiably
    l32 = call(imgd, ftd.float(), size, head=Eg)
    assert l32.requires_grad and abs(float(l32.detach() - mean)) <= 0.05 * float(mean)


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_ten_sgd_steps_decrease_the_loss(dev, path):
    """Prompt tuning with a learnable temperature: E and s = exp(t) by plain SGD, ten steps."""
    size, lr, Cc, ksz, N = GEOMS[0]
    p, img, ft, E, t, _ = _module_ref(size, lr, Cc, ksz, N, 10.0)
    m = _load_model(dev, p, kernel_size=ksz)
    imgd, ftd, td = img.to(dev), ft.to(dev).to(torch.bfloat16), t.to(dev)
    Eg = E.to(dev).requires_grad_(True)
    temp = torch.tensor([math.log(10.0)], device=dev, requires_grad=True)
    opt = torch.optim.SGD([Eg, temp], lr=0.5)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = m(imgd, ftd, size, head=Eg, cosine=True, logit_scale=temp.exp(), target=td, loss="ce", ignore_index=Q.IGNORE, cosine_path=path)
        loss.backward()
        assert Eg.grad is not None and temp.grad is not None and float(temp.grad.abs()) > 0
        opt.step()
        losses.append(float(loss))
    print(path, losses)
    assert losses[-1] < losses[0]


def test_fused_training_step_allocates_no_c_channel_tensor(dev):
    """Peak memory above the resident tensors of a training step (forward + backward for E) on a warmed ``Guidance`` (the image side is
    shared by both arms and cached): the fused step stays below the size of ONE [B, C, Ho, Wo] fp32 map, the composed step exceeds it."""
    size, lr, Cc, ksz, N = (128, 128), (8, 8), 768, 7, 21
    p = O.make_params(seed=33)
    m = _load_model(dev, p, kernel_size=ksz)
    img = O.hash_normal((1, 3, *size), 911).to(dev)
    ft = bf16r(O.hash_normal((1, Cc, *lr), 912)).to(dev).to(torch.bfloat16)
    td = torch.randint(0, N, (1, *size), generator=torch.Generator().manual_seed(5)).to(dev)
    Eg = O.hash_normal((N, Cc), 913).to(dev).requires_grad_(True)
    g = m.guide(img, size)
    map_bytes = Cc * size[0] * size[1] * 4

    def step(path):
        Eg.grad = None
        m(g, ft, size, head=Eg, cosine=True, logit_scale=10.0, target=td, loss="ce", cosine_path=path).backward()

    peak = {}
    for path in ("fused", "composed"):
        step(path)                                   # warm: the Guidance's caches, the library's tables
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(path)
        torch.cuda.synchronize()
        peak[path] = torch.cuda.max_memory_allocated() - base
    print(f"peak above resident: fused {peak['fused'] / 2 ** 20:.1f} MiB, composed {peak['composed'] / 2 ** 20:.1f} MiB, one fp32 map {map_bytes / 2 ** 20:.1f} MiB")
    assert peak["fused"] < map_bytes < peak["composed"]


def test_module_refusals_come_before_any_launch(dev):
    """Every ValueError / NafHipError of the call is raised with no kernel launched: the library's launch timer sees nothing until a call
    that runs."""
    from naf_amd import ops
    from naf_amd._lib import NafHipError
    size, lr, Cc, ksz, N = GEOMS[0]
    p, img, ft, E, t, _ = _module_ref(size, lr, Cc, ksz, N, 10.0)
    m = _load_model(dev, p, kernel_size=ksz)
    imgd, ftd, td, Ed = img.to(dev), ft.to(dev).to(torch.bfloat16), t.to(dev), E.to(dev)

    class Spy:
        def __init__(self):
            self.names = []

        def start(self, name):
            self.names.append(name)

        def stop(self, name):
            pass

    old, spy = ops.KERNEL_TIMER, Spy()
    ops.KERNEL_TIMER = spy
    try:
        for exc, kw in ((ValueError, dict(loss="mse")), (ValueError, dict(target=None)), (ValueError, dict(cosine=False)), (ValueError, dict(return_norms=True)),
                        (ValueError, dict(confusion=True)), (ValueError, dict(predict=True, logit_scale=0.0)), (ValueError, dict(reduction="x")),
                        (ValueError, dict(logit_scale=torch.ones(2, device=dev))), (ValueError, dict(target=td[:, :5])), (ValueError, dict(loss=None)),
                        (NafHipError, dict(cosine_path="fused", output_size=(100, 100), target=td[:, :100, :100])),
                        (NafHipError, dict(cosine_path="fused", features=ftd.float()))):
            kw = dict(kw)
            args = (imgd, kw.pop("features", ftd), kw.pop("output_size", size))
            with pytest.raises(exc):
                m(*args, **{"head": Ed, "cosine": True, "target": td, "loss": "ce", **kw})
        with pytest.raises(NafHipError, match="inference-only"):                 # without loss=: as before
            m(imgd, ftd, size, head=Ed.clone().requires_grad_(True), cosine=True, cosine_path="fused")
        refused = list(spy.names)
        with torch.no_grad():
            m(imgd, ftd, size, head=Ed, cosine=True, target=td, loss="ce")          # the spy does see a call that runs
        ran = list(spy.names)
    finally:
        ops.KERNEL_TIMER = old
    assert refused == [], f"a refused call launched something: {refused}"
    assert "stem" in ran and "xna_cos_ce" in ran, ran
