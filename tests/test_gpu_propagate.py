"""GPU tests of label propagation (``naf_amd.propagate_labels`` / ``pack_frame``, naf_propagate_fwd): against the fp64 restatement of
the reference's ``label_propagation`` (tests/propagate_reference.py, evaluation/eval_video_seg.py:499-561), exact checks that need no
reference, and the ways the public call accepts its frames."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import propagate_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _one_hot(labels, K):
    return torch.nn.functional.one_hot(labels, K).permute(2, 0, 1).float()        # [K, h, w]


# ---- A. against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [pytest.param(i, id=R.CASE_IDS[i]) for i in range(len(R.CASES))])
def test_matches_the_reference_on_unambiguous_pixels(dev, ci):
    """On every pixel that is not ambiguous (propagate_reference: no candidate within 0 < |s - threshold| < 4 * C * 2^-24), the kernel keeps
    the reference's set -- its scores are within delta_s = (C + 8) * 2^-24 < 4 * C * 2^-24 of the exact ones (bf16 products are exact in
    fp32, the fp32 accumulation of C terms with sum |q_i k_i| invq invk <= 1 costs at most C * 2^-24, the two inverse norms and two
    multiplies a few ulps more), and exact ties are ties on both sides (identical data through identical instructions).

    Bound, with no fitted constant: out = sum_i a_i x_i with a_i = w_i / sum_j w_j and |x_i| <= max|segs|.  Each computed weight is
    w_i (1 + e_i) with |e_i| <= eps := delta_s / T + 2^-20: the score error delta_s enters the exponent divided by T (the shift by the
    pixel's maximum cancels between numerator and denominator), and 2^-20 covers the fp32 exponential, the rounding of its argument
    and the handful of fp32 additions of the kept terms.  Then |a_i' - a_i| <= 2 eps a_i to first order, so
        |out - ref| <= 2 * (delta_s / T + 2^-20) * max|segs|.
    The excluded (ambiguous) share is capped at 3 %; tests/test_propagate_cpu.py asserts that cap from the reference alone."""
    import naf_amd
    n, C, h, w, r, topk, K, _ = R.CASES[ci]
    (target, context, segs), (ref, ambiguous, _) = R.reference(ci)
    out = naf_amd.propagate_labels(target.to(dev), [f.to(dev) for f in context], segs.to(dev), radius=r, topk=topk, temperature=R.TEMPERATURE)
    assert out.shape == (1, K, h, w) and out.dtype == torch.float32 and not out.requires_grad
    share = float(ambiguous.double().mean())
    assert share <= R.MAX_AMBIGUOUS_SHARE
    delta_s = (C + 8) * 2.0 ** -24
    bound = 2.0 * (delta_s / R.TEMPERATURE + 2.0 ** -20) * float(segs.abs().max())
    err = (out.double().cpu() - ref).abs().amax(1)[0]                              # [h, w]
    ok = ~ambiguous
    print(f"{R.CASE_IDS[ci]}: max err {float(err[ok].max()):.3e} (bound {bound:.3e}) on {int(ok.sum())} pixels; excluded {100 * share:.2f} %; "
          f"max err on excluded {float(err[ambiguous].max()) if bool(ambiguous.any()) else 0.0:.3e}")
    assert float(err[ok].max()) <= bound


@pytest.mark.parametrize("li", [pytest.param(i, id=R.LIMIT_IDS[i]) for i in range(len(R.LIMIT_CASES))])
def test_matches_the_reference_at_the_limits_of_the_served_range(dev, li):
    """LIMIT_CASES: every propagate_kernel<KSMAX>, the single-buffered key stream, topk = 16, K = 64, n = 16, kept sets above the 16 list
    slots, grids of exactly one tile and thinner than one (tests/test_propagate_cpu.py reads from naf_propagate_plan what each launches).
    The bound is the one above with one more term, propagate_reference.gpu_bound:
        |out - ref| <= 2 * (delta_s / T + 2^-20 + kept_max * 2^-24) * max|segs|
    on every non-ambiguous pixel, kept_max the reference's own largest kept set: the fp32 additions of kept_max terms, which the "handful"
    of the 2^-20 does not cover where ties keep dozens.  The lattice cases have no ambiguous pixel, so every pixel is compared."""
    import naf_amd
    n, C, h, w, r, topk, K, features = R.LIMIT_CASES[li]
    (target, context, segs), (ref, ambiguous, kept) = R.limit_reference(li)
    out = naf_amd.propagate_labels(target.to(dev), [f.to(dev) for f in context], segs.to(dev), radius=r, topk=topk, temperature=R.TEMPERATURE)
    assert out.shape == (1, K, h, w) and out.dtype == torch.float32
    share = float(ambiguous.double().mean())
    assert share <= R.MAX_AMBIGUOUS_SHARE and (features != "lattice" or share == 0.0)
    bound = R.gpu_bound(C, int(kept.max()), float(segs.abs().max()))
    err = (out.double().cpu() - ref).abs().amax(1)[0]
    ok = ~ambiguous
    worst = float(err[ok].max())
    print(f"{R.LIMIT_IDS[li]}: max err {worst:.3e} / bound {bound:.3e} = {worst / bound:.1e} on {int(ok.sum())} pixels; "
          f"kept sets up to {int(kept.max())}; excluded {100 * share:.2f} %")
    assert bool(torch.isfinite(out).all())
    assert worst <= bound


# ---- B. exact checks that need no reference -----------------------------------------------------------------------------
EMBED_BASE = (2, 64, 19, 27, 3, 5, 4)                 # n, C, h, w, radius, topk, K: lattice features with all 64 channels live (m = 64)


def _embed_inputs():
    n, C, h, w, _, _, K = EMBED_BASE
    g = torch.Generator().manual_seed(9)
    target = R.lattice_features(C, h, w, g)
    context = [R.lattice_features(C, h, w, g) for _ in range(n)]
    return target, context, R.make_labels(n, K, h, w, g)


def _embedded(x, C, seed):
    """The 64 channels of x at 64 random (sorted or not: a dot product does not care) positions among C, zeros elsewhere; one placement per
    (C, seed), shared by the target and every context frame."""
    pos = torch.randperm(C, generator=torch.Generator().manual_seed(seed))[: x.shape[0]]
    y = torch.zeros(C, *x.shape[1:], dtype=x.dtype)
    y[pos] = x
    return y


@pytest.fixture(scope="module")
def embed_base(dev):
    import naf_amd
    target, context, segs = _embed_inputs()
    _, _, _, _, r, topk, _ = EMBED_BASE
    out = naf_amd.propagate_labels(target.to(dev), [f.to(dev) for f in context], segs.to(dev), radius=r, topk=topk)
    ref, ambiguous, kept = R.windowed(target, context, segs, radius=r, topk=topk)
    assert int(ambiguous.sum()) == 0 and int(kept.max()) > topk                  # exact ties: the kept sets matter
    assert float((out.double().cpu() - ref).abs().max()) <= R.gpu_bound(64, int(kept.max()), float(segs.max()))
    return target, context, segs, out


@pytest.mark.parametrize("C", [160, 256, 416, 512, 544, 768, 800, 1024])
def test_channel_embedding_leaves_every_bit_unchanged(dev, embed_base, C):
    """The base's 64 live channels placed at random positions among C, the same for the target and every context frame, zeros elsewhere:
    the sums of squares, the integer dot products and therefore every score are exactly the base's, whichever instantiation runs and
    whichever registers hold the query fragments, so the output must be the base's bit for bit.  No reference, no tolerance."""
    import naf_amd
    from naf_amd import ops
    target, context, segs, base = embed_base
    n, _, h, w, r, topk, K = EMBED_BASE
    assert ops.propagate_plan(n, C, h, w, K, radius=r, topk=topk)["ksmax"] == {160: 8, 256: 8, 416: 16, 512: 16, 544: 24, 768: 24, 800: 32, 1024: 32}[C]
    out = naf_amd.propagate_labels(_embedded(target, C, C).to(dev), [_embedded(f, C, C).to(dev) for f in context], segs.to(dev), radius=r, topk=topk)
    assert torch.equal(out, base), f"C = {C}: {int((out != base).sum())} of {out.numel()} values differ, max |diff| {float((out - base).abs().max()):.3e}"


def test_channel_embedding_through_the_single_buffer(dev, embed_base):
    """The same at C = 1024 with K = 64 -- the four label maps followed by 60 zero channels -- which the plan runs single-buffered: the
    first four output channels are the base's bit for bit and the rest exactly 0."""
    import naf_amd
    from naf_amd import ops
    target, context, segs, base = embed_base
    n, _, h, w, r, topk, K = EMBED_BASE
    assert ops.propagate_plan(n, 1024, h, w, 64, radius=r, topk=topk)["nbuf"] == 1
    wide = torch.cat([segs, torch.zeros(n, 64 - K, h, w)], 1)
    out = naf_amd.propagate_labels(_embedded(target, 1024, 1).to(dev), [_embedded(f, 1024, 1).to(dev) for f in context], wide.to(dev), radius=r, topk=topk)
    assert out.shape == (1, 64, h, w)
    assert torch.equal(out[:, :K], base), f"{int((out[:, :K] != base).sum())} values differ, max |diff| {float((out[:, :K] - base).abs().max()):.3e}"
    assert torch.equal(out[:, K:], torch.zeros_like(out[:, K:]))


def test_a_frame_propagated_from_itself_returns_its_labels_at_every_limit(dev):
    """As below at C = 1024, K = 64, radius 15 on 17 x 33 (KSMAX 32, single-buffered, three key blocks): the only kept candidate is the pixel
    itself, and 1 * seg / 1 is exact for soft label maps too."""
    import naf_amd
    from naf_amd import ops
    g = torch.Generator().manual_seed(10)
    C, h, w, K = 1024, 17, 33, 64
    assert ops.propagate_plan(1, C, h, w, K, radius=15, topk=1) == dict(ksmax=32, nkb=3, nbuf=1, lds=132544)
    feats = torch.randn(C, h, w, generator=g).to(torch.bfloat16).to(dev)
    segs = torch.rand(1, K, h, w, generator=g).to(dev)
    out = naf_amd.propagate_labels(feats, [feats], segs, radius=15, topk=1)
    assert torch.equal(out, segs)


def test_a_frame_propagated_from_itself_returns_its_labels(dev):
    """Context = the target frame, n = 1, topk = 1: the only kept candidate is the pixel itself (cosine 1 against random neighbours), its
    weight is exp(0) = 1, and 1 * seg / 1 is exact."""
    import naf_amd
    g = torch.Generator().manual_seed(3)
    C, h, w, K = 64, 21, 37, 5
    feats = torch.randn(C, h, w, generator=g).to(torch.bfloat16).to(dev)
    segs = _one_hot(torch.randint(0, K, (h, w), generator=g), K).to(dev)
    out = naf_amd.propagate_labels(feats, [feats], [segs], radius=3, topk=1)
    assert torch.equal(out[0], segs)


def _window_reaches_exactly_its_corner(dev, r, C):
    import naf_amd
    g = torch.Generator().manual_seed(4)
    h, w, K = 35, 41, 4
    feats = torch.randn(C, h, w, generator=g).to(torch.bfloat16)
    labels = torch.randint(0, K, (h, w), generator=g)
    ctx = torch.roll(feats, shifts=(r, -r), dims=(1, 2)).to(dev)
    segs = _one_hot(torch.roll(labels, shifts=(r, -r), dims=(0, 1)), K).to(dev)
    out = naf_amd.propagate_labels(feats.to(dev), [ctx], segs[None], radius=r, topk=1)
    expect = _one_hot(labels, K).to(dev)                                           # segs rolled back by (-r, +r)
    inside = torch.zeros(h, w, dtype=torch.bool, device=dev)
    inside[: h - r, r:] = True                                                     # i + r < h and j - r >= 0: no wrap-around
    assert bool(inside.any())
    assert torch.equal(out[0][:, inside], expect[:, inside])
    if r > 1:
        short = naf_amd.propagate_labels(feats.to(dev), [ctx], segs[None], radius=r - 1, topk=1)
        assert not torch.equal(short[0][:, inside], expect[:, inside])


@pytest.mark.parametrize("r", [1, 12, 15])
def test_window_reaches_exactly_its_corner(dev, r):
    """Context = the target rolled by (+r, -r): the source of target pixel (i, j) is context pixel (i + r, j - r), the corner of its
    window.  Where that lies inside the image the output is the rolled label map bit for bit (topk = 1); with radius r - 1 the corner is
    out of reach and some such pixel must differ."""
    _window_reaches_exactly_its_corner(dev, r, 32)


@pytest.mark.parametrize("r", [1, 12, 15])
def test_window_reaches_exactly_its_corner_at_1024_channels(dev, r):
    """The same through propagate_kernel<32> (double-buffered at r = 1, single-buffered at r = 11, 12, 14 and 15)."""
    _window_reaches_exactly_its_corner(dev, r, 1024)


def test_outputs_are_convex_combinations_and_reproducible(dev):
    """One-hot label maps, topk = 5: every pixel's output lies in [0, 1] and sums to 1 over K within 1e-5; a second call is bit-equal
    (no atomics, a fixed summation order)."""
    import naf_amd
    g = torch.Generator().manual_seed(5)
    n, C, h, w, K = 3, 96, 23, 45, 6
    target = torch.randn(C, h, w, generator=g).to(torch.bfloat16).to(dev)
    context = [torch.randn(C, h, w, generator=g).to(torch.bfloat16).to(dev) for _ in range(n)]
    segs = torch.stack([_one_hot(torch.randint(0, K, (h, w), generator=g), K) for _ in range(n)]).to(dev)
    a = naf_amd.propagate_labels(target, context, segs, radius=4, topk=5)
    b = naf_amd.propagate_labels(target, context, segs, radius=4, topk=5)
    assert torch.equal(a, b)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    assert float((a.sum(1) - 1.0).abs().max()) <= 1e-5


# ---- C. the public call ---------------------------------------------------------------------------------------------
def test_every_way_of_passing_frames_gives_the_same_bits(dev):
    import naf_amd
    g = torch.Generator().manual_seed(6)
    n, C, h, w, K = 3, 64, 17, 19, 3
    target = torch.randn(C, h, w, generator=g).to(dev)                             # fp32
    context = [torch.randn(C, h, w, generator=g).to(dev) for _ in range(n)]         # separately allocated frames
    segs = torch.rand(n, K, h, w, generator=g).to(dev)
    kw = dict(radius=3, topk=5, temperature=0.07)
    base = naf_amd.propagate_labels(target.bfloat16(), [f.bfloat16() for f in context], segs, **kw)
    assert base.shape == (1, K, h, w)
    same = {
        "fp32 features (rounded to bf16 once)": naf_amd.propagate_labels(target, context, segs, **kw),
        "FrameFeatures": naf_amd.propagate_labels(naf_amd.pack_frame(target), [naf_amd.pack_frame(f) for f in context], segs, **kw),
        "stacked context": naf_amd.propagate_labels(target, torch.stack(context), segs, **kw),
        "[1, C, h, w] frames, list of segs": naf_amd.propagate_labels(target[None], [f[None] for f in context],
                                                                     [segs[0], segs[1][None], segs[2]], **kw),
        "mixed": naf_amd.propagate_labels(naf_amd.pack_frame(target), [context[0], naf_amd.pack_frame(context[1]), context[2].bfloat16()], segs, **kw),
    }
    wide = torch.randn(C, h, 2 * w, generator=g).to(dev)
    wide[:, :, ::2] = target
    same["non-contiguous NCHW"] = naf_amd.propagate_labels(wide[:, :, ::2], context, segs, **kw)
    hwc = target.bfloat16().permute(1, 2, 0).contiguous()
    same["channels-last bf16 view"] = naf_amd.propagate_labels(hwc.permute(2, 0, 1), context, segs, **kw)
    for name, out in same.items():
        assert torch.equal(out, base), name
    assert naf_amd.pack_frame(hwc.permute(2, 0, 1)).data.data_ptr() == hwc.data_ptr()
    with pytest.raises(ValueError, match="radius"):
        naf_amd.propagate_labels(target, context, segs, radius=0)


def test_inverse_norms(dev):
    import naf_amd
    g = torch.Generator().manual_seed(7)
    x = torch.randn(352, 5, 9, generator=g).to(torch.bfloat16)
    x[:, 2, 3] = 0                                                                 # F.normalize's eps: 1 / max(0, 1e-12)
    ff = naf_amd.pack_frame(x.to(dev))
    assert ff.shape == (352, 5, 9) and ff.inv_norm.shape == (5, 9) and ff.inv_norm.dtype == torch.float32
    ref = 1.0 / x.double().pow(2).sum(0).sqrt().clamp_min(1e-12)
    rel = ((ff.inv_norm.double().cpu() - ref).abs() / ref).max()
    assert float(rel) <= (352 + 8) * 2.0 ** -24                                   # fp32 sum of C exact squares, sqrt, reciprocal
    assert torch.equal(ff.data.cpu(), x.permute(1, 2, 0))


def test_the_upsampler_output_goes_in_without_a_copy(dev):
    """``naf(image, feats, size)`` on bf16 features returns a logical NCHW view of a dense channels-last bf16 buffer: pack_frame uses that
    buffer as it is, and the propagation of a frame from itself returns its labels."""
    import naf_amd
    from oracle import naf_oracle as O
    model = naf_amd.NAF(kernel_size=7).eval()
    model.load_state_dict(O.make_params(seed=11), strict=True)
    model = model.to(dev)
    img = O.hash_normal((1, 3, 64, 64), 111).to(dev)
    ft = O.hash_normal((1, 128, 8, 8), 112).to(dev).bfloat16()
    with torch.no_grad():
        up = model(img, ft, (40, 56))
    assert up.shape == (1, 128, 40, 56) and up.dtype == torch.bfloat16
    ff = naf_amd.pack_frame(up)
    assert ff.data.data_ptr() == up.data_ptr() and ff.data.shape == (40, 56, 128)
    g = torch.Generator().manual_seed(8)
    segs = torch.rand(1, 4, 40, 56, generator=g).to(dev)
    out = naf_amd.propagate_labels(up, [ff], segs, radius=2, topk=5)
    ref, ambiguous, _ = R.windowed(up[0].cpu(), [up[0].cpu()], segs.cpu(), radius=2, topk=5)
    assert out.shape == (1, 4, 40, 56) and bool(torch.isfinite(out).all())
    # upsampled neighbours are strongly correlated, so more thresholds are ambiguous here than on random features (no cap in this test);
    # everywhere the output is a convex combination of label values, and off the ambiguous pixels it meets the bound of test A
    assert float(out.min()) >= float(segs.min()) - 1e-6 and float(out.max()) <= float(segs.max()) + 1e-6
    err = (out.double().cpu() - ref).abs().amax(1)[0]
    ok = ~ambiguous
    print(f"upsampler output: {int(ambiguous.sum())} of {ambiguous.numel()} pixels ambiguous")
    assert bool(ok.any()) and float(err[ok].max()) <= 2.0 * ((128 + 8) * 2.0 ** -24 / 0.1 + 2.0 ** -20) * float(segs.max())
