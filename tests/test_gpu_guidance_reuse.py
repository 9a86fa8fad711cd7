"""GPU tests of ``Guidance``: the image encoded once (``naf.guide``) and reused by every inference call of ``NAF.forward``.

A ``Guidance`` call computes nothing new: it is the composition of the operators the image call runs (``single_call = False``), with the
stem, the pooling and -- for a size and grid seen before -- the RoPE pass taken from caches.  So every result is ``torch.equal`` to that
composition, spelled out here with the public operators, and the counters on the operators show what was NOT run again.
Setup: default width, window 5, image (2, 3, 96, 128)."""
import os
import sys

import pytest
import torch
from torch import nn

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import assert_close, bf16r  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = (96, 128)
STEM_OPS = ("stem_conv0", "stem_conv", "pool_guidance", "preshrink_image", "rope_pool")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def setup(dev):
    """(params, model with single_call = False, image on the host, image on the device)."""
    from naf_amd import NAF
    p = O.make_params(seed=47)
    m = NAF(kernel_size=5).eval()
    m.load_state_dict(p, strict=True)
    m = m.to(dev)
    m.single_call = False
    img = O.hash_normal((2, 3, *SIZE), 4701)
    return p, m, img, img.to(dev)


def _features(dev):
    """A bf16 12 x 16 (8 x 8 cells: queries are materialised), B float16 6 x 8 (16 x 16 cells: rotate-on-load), C fp32 7 x 9 (non-integer ratio)."""
    fa = bf16r(O.hash_normal((2, 128, 12, 16), 4711))
    fb = O.hash_normal((2, 96, 6, 8), 4712).half().float()
    fc = O.hash_normal((2, 64, 7, 9), 4713)
    return (fa, fa.to(dev).to(torch.bfloat16)), (fb, fb.to(dev).half()), (fc, fc.to(dev))


class _Counters:
    """Call counters on the operators of the guidance pipeline (``ops.<name>`` is looked up at call time by the model)."""

    def __init__(self, monkeypatch):
        from naf_amd import ops
        self.n = {k: 0 for k in STEM_OPS}
        self.rope_pool_calls = []
        for name in STEM_OPS:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.n[name] += 1
            if name == "rope_pool":
                self.rope_pool_calls.append(bool(kw.get("write_q", True)))
            return fn(*a, **kw)
        return counted

    def take(self):
        got, self.n = self.n, {k: 0 for k in STEM_OPS}
        return got


def _unrotated(x, heads):
    return x.permute(0, 2, 3, 1).unflatten(3, (heads, x.shape[1] // heads)).permute(0, 3, 1, 2, 4)


def test_four_calls_on_one_guidance_equal_the_operators_they_stand_for(dev, setup, monkeypatch):
    from naf_amd import ops
    p, m, img, imgd = setup
    (fa, fad), (fb, fbd), (fc, fcd) = _features(dev)
    enc, heads = m.image_encoder, m.upsampler.num_heads
    # ---- what each call stands for, from the parent's operators
    want_a = m(imgd, fad, SIZE)                                           # the first call: the image call itself
    x = enc.guidance(imgd, SIZE)
    ty, tx = enc.rope.tables(*SIZE)
    assert not ops.xna_rope_fusable(_unrotated(x, heads), (12, 16), 32, 5, (ty, tx), out_dtype=torch.bfloat16)     # A materialises
    # B: 16 x 16 cells; the attention kernel rotates on load where it serves the head (24 value channels per head are not the matrix-core
    # kernel's: the guidance_qk of the image call decides, and the Guidance call decides the same)
    fus_b = ops.xna_rope_fusable(_unrotated(x, heads), (6, 8), 24, 5, (ty, tx), out_dtype=torch.float16)
    fd = O.hash_normal((2, 128, 6, 8), 4714).to(dev).half()               # D: those cells with 32 channels per head: rotate-on-load
    assert ops.xna_rope_fusable(_unrotated(x, heads), (6, 8), 32, 5, (ty, tx), out_dtype=torch.float16)
    q5, _ = ops.rope_pool(x, ty, tx, heads, (12, 16))
    _, kb = ops.rope_pool(x, ty, tx, heads, (6, 8), write_q=False)         # keys only: rotated on load, or the queries are cached by then
    want_b = m.upsampler(_unrotated(x, heads), kb, fbd, rope_tables=(ty, tx)) if fus_b else m.upsampler(q5, kb, fbd)
    _, kc = ops.rope_pool(x, ty, tx, heads, (7, 9), write_q=False)         # C: cached queries, keys only
    want_c = m.upsampler(q5, kc, fcd)
    want_d = m(imgd, fd, SIZE)
    # ---- the Guidance calls
    cnt = _Counters(monkeypatch)
    g = m.guide(imgd, SIZE)
    built = cnt.take()
    assert built["stem_conv0"] == 2 and built["stem_conv"] == 8 and built["rope_pool"] == 0     # two branches: conv0 + 4 block layers each
    assert built["pool_guidance"] == 0 and built["preshrink_image"] == 0                         # the output is the image's size
    outs = []
    for f, new_rope in ((fad, 1), (fbd, 1), (fcd, 1), (fad, 0)):
        outs.append(m(g, f, SIZE))
        n = cnt.take()
        assert n["stem_conv0"] == n["stem_conv"] == n["pool_guidance"] == n["preshrink_image"] == 0, n
        assert n["rope_pool"] == new_rope, n
    assert cnt.rope_pool_calls == [True, False, False]        # queries + keys once, then keys only (rotate-on-load; cached queries)
    torch.cuda.synchronize()
    for got, want, (ref_f, _), what in zip(outs, (want_a, want_b, want_c, want_a), ((fa, 0), (fb, 0), (fc, 0), (fa, 0)), "A B C A-again".split()):
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got, want), f"{what}: the Guidance call differs from the operators it stands for"
        assert_close(got.float().cpu(), O.naf_forward(p, img, ref_f, SIZE, kernel_size=5), 2e-2, 1e-2, f"{what} vs oracle")
    assert outs[0].dtype == torch.bfloat16 and outs[1].dtype == torch.float16 and outs[2].dtype == torch.float32
    # D on a fresh Guidance: rotate-on-load, keys from one keys-only launch, no query tensor; then on the first one: its keys are B's
    g2 = m.guide(imgd, SIZE)
    cnt.take()
    cnt.rope_pool_calls.clear()
    assert torch.equal(m(g2, fd, SIZE), want_d) and cnt.take()["rope_pool"] == 1 and cnt.rope_pool_calls == [False] and not g2._queries
    assert torch.equal(m(g, fd, SIZE), want_d) and cnt.take()["rope_pool"] == 0
    # housekeeping: the caches hold the stem output (= the pooled level here), the queries, three key sets and the tables
    stem_bytes = 2 * 256 * 96 * 128 * 2
    assert g.nbytes >= 2 * stem_bytes and g.nbytes < 2 * stem_bytes + (1 << 20)
    g.clear()
    assert g.nbytes == 0
    assert torch.equal(m(g, fad, SIZE), want_a)                            # ... and fill again on demand
    assert cnt.take()["stem_conv0"] == 2


def test_output_sizes_share_stem_outputs(dev, setup, monkeypatch):
    """Image (1, 3, 64, 96) at four output sizes: identity, pooled 4x, pooled up, pre-shrunk: each equals the image call, the stem runs twice."""
    p, m, _, _ = setup
    img = O.hash_normal((1, 3, 64, 96), 4721).to(dev)
    ft = bf16r(O.hash_normal((1, 64, 8, 12), 4722)).to(dev).to(torch.bfloat16)
    sizes = [(64, 96), (16, 24), (80, 120), (8, 12)]
    want = [m(img, ft, s) for s in sizes]
    cnt = _Counters(monkeypatch)
    g = m.guide(img)
    assert sum(cnt.take().values()) == 0                                   # lazy: nothing runs before the first call
    got = [m(g, ft, s) for s in sizes]
    n = cnt.take()
    assert n["stem_conv0"] == 2 * 2 and n["preshrink_image"] == 1 and n["pool_guidance"] == 3 and n["rope_pool"] == 4, n
    assert len(g._stem) == 2 and len(g._pooled) == 4
    for s, a, b in zip(sizes, got, want):
        assert torch.equal(a, b), f"output size {s}: the Guidance call differs from the image call"
    for s in sizes:
        m(g, ft, s)
    assert sum(cnt.take().values()) == 0                                   # everything cached


def _probe(Cc, N, seed, dev):
    conv = nn.Conv2d(Cc, N, 1)
    with torch.no_grad():
        conv.weight.copy_(O.hash_normal((N, Cc, 1, 1), seed) * Cc ** -0.5)
        conv.bias.copy_(O.hash_normal((N,), seed + 1))
    return conv.to(dev)


def test_every_inference_mode_accepts_a_guidance(dev, setup):
    p, m, img, imgd = setup
    N = 21
    ft = O.hash_normal((2, 128, 12, 16), 4731).to(dev)
    probe = _probe(128, N, 4732, dev)
    t = (O.hash_normal((2, *SIZE), 4733).abs() * 7).long().clamp(0, N - 1)
    t[:, :5] = 255
    t = t.to(dev)
    g = m.guide(imgd)
    with torch.no_grad():
        out_i, lg_i = m(imgd, ft, SIZE, return_weights=True)
        out_g, lg_g = m(g, ft, SIZE, return_weights=True)
        assert torch.equal(out_g, out_i) and torch.equal(lg_g, lg_i)
        assert torch.equal(m(g, ft, SIZE, head=probe), m(imgd, ft, SIZE, head=probe))
        assert torch.equal(m(g, ft, SIZE, head=probe, target=t, ignore_index=255), m(imgd, ft, SIZE, head=probe, target=t, ignore_index=255))
        li, pi = m(imgd, ft, SIZE, head=probe, target=t, ignore_index=255, predict=True)
        lg, pg = m(g, ft, SIZE, head=probe, target=t, ignore_index=255, predict=True)
        assert torch.equal(lg, li) and torch.equal(pg, pi)
        for red in ("sum", "none"):
            assert torch.equal(m(g, ft, SIZE, head=probe, target=t, ignore_index=255, reduction=red),
                               m(imgd, ft, SIZE, head=probe, target=t, ignore_index=255, reduction=red))
    # the accumulated confusion matrix, whatever the gradient mode
    cm_i = torch.zeros(N, N, dtype=torch.int64, device=dev)
    cm_g = torch.zeros(N, N, dtype=torch.int64, device=dev)
    for _ in range(2):
        m(imgd, ft, SIZE, head=probe, target=t, ignore_index=255, confusion=cm_i)
        assert m(g, ft, SIZE, head=probe, target=t, ignore_index=255, confusion=cm_g) is cm_g
    assert torch.equal(cm_g, cm_i) and int(cm_g.sum()) == 2 * int((t != 255).sum())
    # probe training on a frozen upsampler: the same loss and the same gradient, bit for bit
    for prm in m.parameters():
        prm.requires_grad_(False)
    try:
        grads = []
        for src in (imgd, g):
            probe.zero_grad()
            loss = m(src, ft, SIZE, head=probe, target=t, ignore_index=255)
            assert loss.requires_grad
            loss.backward()
            grads.append((loss.detach().clone(), probe.weight.grad.clone(), probe.bias.grad.clone()))
        for a, b in zip(*grads):
            assert torch.equal(a, b)
        lo_i, lo_g = m(imgd, ft, SIZE, head=probe), m(g, ft, SIZE, head=probe)
        assert lo_g.requires_grad and torch.equal(lo_g, lo_i)
    finally:
        for prm in m.parameters():
            prm.requires_grad_(True)


def test_refusals_name_their_reason(dev, setup):
    from naf_amd import NAF
    p, _, img, _ = setup
    m = NAF(kernel_size=5).eval()
    m.load_state_dict(p, strict=True)
    m = m.to(dev)
    imgd = img.to(dev).clone()
    ft = O.hash_normal((2, 64, 6, 8), 4741).to(dev)
    g = m.guide(imgd, SIZE)
    m(g, ft, SIZE)
    with pytest.raises(ValueError, match="regress"):
        m(g, ft, SIZE, regress=torch.zeros(2, 64, *SIZE, device=dev))
    with pytest.raises(ValueError, match="differentiable"):
        m(g, ft, SIZE, return_weights="differentiable")
    m.train()                                                              # trainable parameters, gradient mode: the training path
    with pytest.raises(RuntimeError, match="training path"):
        m(g, ft, SIZE)
    with pytest.raises(RuntimeError, match="training path"):
        m(g, ft, SIZE, head=_probe(64, 5, 4742, dev))
    with torch.no_grad():
        m(g, ft, SIZE)                                                     # ... which no_grad is not
    m.eval()
    with pytest.raises(RuntimeError, match="training path"):
        m(g, ft.clone().requires_grad_(True), SIZE)
    with pytest.raises(RuntimeError, match="another NAF"):
        NAF(kernel_size=5).eval().to(dev)(g, ft, SIZE)
    with pytest.raises(RuntimeError, match="ROCm"):
        m(g, ft.cpu(), SIZE)
    imgd[0, 0, 0, 0] += 1.0                                                # the image changes in place
    with pytest.raises(RuntimeError, match="stale.*image"):
        m(g, ft, SIZE)
    with pytest.raises(RuntimeError, match="stale.*image"):
        m.query(g, torch.tensor([[0, 1, 1]]), features=ft, output_size=SIZE)
    g = m.guide(imgd)
    m(g, ft, SIZE)
    with torch.no_grad():
        m.image_encoder.encoder[0].bias.add_(0.5)                          # a parameter changes in place
    with pytest.raises(RuntimeError, match="stale.*parameter"):
        m(g, ft, SIZE)
    m(m.guide(imgd), ft, SIZE)
