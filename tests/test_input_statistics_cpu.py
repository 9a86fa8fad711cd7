"""CPU companion of tests/test_gpu_input_statistics.py (no device, small shapes): the bounds that file asserts on the kernels are
feasible for the reference alone -- the fp64 oracle with the kernels' documented rounding points (tests/input_statistics.py) stays inside
them on every input family -- and they are sensitive: two planted defects (softmax scale x 1.01; two of 64 query dims dropped from the
scores) leave them on every family on which the defect changes the exact result at all.

Measured here (9 x 10 keys -> 36 x 40, window 7, 2 heads, Dv 64; 7 x 8 -> 28 x 32, window 5, Dv 32 for the backward), worst err / abs_sum
of the emulation: forward <= 3.7e-3 (bound 1.25 * 2^-8 = 4.9e-3); dk and dv <= 2^-8; dq, whose ratio includes its bf16 store, inside
1.25 * (2^-8 abs_sum + 2^-8 stored) everywhere.

Elements over the bound with a planted defect (scale x 1.01 / two of 64 query dims dropped).
  forward, of 184 320: unit 13 130 / 156 681; channel offsets 1 176 / 65 942; outliers 59 706 / 168 703; x 2^-10 and x 2^10 as unit;
    smooth 10 152 / 151 759; peaked 18 458 / 118 330; key offset 13 247 / 156 743; flat 0 / 0.
  backward, dq of 114 688 (dk of 7 168, dv of 3 584 in brackets), under the device bound with its cancellation term:
    unit 23 744 (78, 0) / 97 369 (4 984, 2 271); peaked 40 920 (1 400, 4) / 92 773 (7 095, 3 470); key offset 2 710 (84, 0) / 54 312 (4 999,
    2 272); channel offsets 20 761 (61, 0) / 96 589 (4 864, 2 271); outliers 23 071 (1 977, 231) / 101 070 (6 651, 3 114);
    dout x 1e-4 with flat scores 811 (0, 0) / 0 (0, 0); v x 2^10, dout x 2^-10 as unit.
The flat family (q, k x 0.05: scores of 2.5e-3) cannot see a defect in the scores -- either one moves the exact fp64 forward output, and
the dropped dims the exact gradients, by less than 2^-8 of the abs-sum -- and the tests assert exactly that split: a defect that is
visible in exact arithmetic must leave the bound, on every family.  A 1 % scale error in the backward shows in dq on every family (dS
carries the scale as a factor).  The device cases come from tests/input_statistics.py: nothing here imports a device test module.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402

HEADS = 2
FWD = dict(q=(1, 128, 36, 40), k=(1, 128, 9, 10), v=(1, 128, 9, 10), ksz=7)
BWD = dict(q=(1, 128, 28, 32), k=(1, 128, 7, 8), v=(1, 64, 7, 8), g=(1, 64, 28, 32), ksz=5)


def _fwd_inputs(fam, geom=FWD, seed=20):
    q, k = S.make_qk(geom["q"], geom["k"], fam[1], seed, HEADS)
    return q, k, S.make_values(geom["v"], fam[0], seed + 2)


def _bwd_inputs(fam, seed=30):
    q, k = S.make_qk(BWD["q"], BWD["k"], fam[2], seed, HEADS)
    return q, k, S.make_values(BWD["v"], fam[0], seed + 2), S.make_values(BWD["g"], fam[1], seed + 3)


# ---- the stated conditions ---------------------------------------------------------------------------------------------------
def test_families_are_bf16_representable_deterministic_and_in_range():
    for fam in S.GRAD_FAMILIES:
        x = S.make_values((2, 24, 9, 10), fam, 5)
        assert torch.equal(x, S.bf16r(x)) and torch.equal(x, S.make_values((2, 24, 9, 10), fam, 5)) and bool(torch.isfinite(x).all())
        lim = {"unit": 3.5, "chan_offset": 32.0, "outlier": 209.0, "small": 3.5e-3, "big": 3.6e3, "smooth": 3.5, "tiny": 3.5e-4}[fam]
        assert float(x.abs().max()) <= lim, (fam, float(x.abs().max()))
        nz = x[x != 0].abs()
        assert float(nz.min()) >= 2.0 ** -40                               # far from the 2^-126 of bf16 / fp32
    for fam in S.LOGIT_FAMILIES:
        q, k = S.make_qk((1, 128, 12, 16), (1, 128, 3, 4), fam, 6, 2)
        assert torch.equal(q, S.bf16r(q)) and torch.equal(k, S.bf16r(k))
        s = torch.einsum("bnhwd,bnyxd->bnhwyx", S._heads(q, 2), S._heads(k, 2)) / 8.0
        assert float(s.abs().max()) < 1600.0
        if fam == "peaked":
            assert float(s.abs().max()) > 25.0                               # one key dominates
        if fam == "flat":
            assert float(s.abs().max()) < 0.05
        if fam == "key_offset":                                              # the offset is common to every key of a query: a large shared score
            assert float(s.mean(dim=(-1, -2)).abs().max()) > 5.0 * float((s - s.mean(dim=(-1, -2), keepdim=True)).abs().mean())
    for fam in S.IMAGE_FAMILIES:
        img = S.make_image(1, 64, 80, fam, 91)
        assert img.shape == (1, 3, 64, 80) and bool(torch.isfinite(img).all()) and float(img.abs().max()) <= 3500.0
    nat = S.make_image(1, 64, 80, "natural_01", 91)
    assert 0.0 <= float(nat.min()) and float(nat.max()) <= 1.0 and float(nat.std()) > 0.15
    # "looks like an image": neighbouring pixels are far more alike than distant ones
    assert float((nat[..., 1:] - nat[..., :-1]).abs().mean()) < 0.25 * float((nat[..., 40:] - nat[..., :-40]).abs().mean())
    assert float(S.make_image(1, 64, 80, "natural_255", 91).max()) > 200.0


def test_outlier_share():
    for h, w in ((9, 10), (7, 8), (8, 8), (28, 32), (64, 128)):
        share = float(S.outlier_mask(h, w).double().mean())
        assert 0.025 <= share <= 0.06, (h, w, share)                         # "about 4 % of keys"
        assert int(S.outlier_mask(h, w).sum()) >= 2
    v = S.make_values((1, 8, 9, 10), "outlier", 3)
    u = S.make_values((1, 8, 9, 10), "unit", 3)
    m = S.outlier_mask(9, 10)
    assert torch.equal(v[..., ~m], u[..., ~m]) and torch.equal(v[..., m], S.bf16r(O.hash_normal((1, 8, 9, 10), 3) * 60.0)[..., m])


# ---- references ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr,out,ksz", [((7, 8), (28, 32), 5), ((5, 7), (23, 30), 3)])
def test_explicit_backward_formula_equals_autograd_through_the_oracle(lr, out, ksz):
    q, k = S.make_qk((1, 128, *out), (1, 128, *lr), "unit", 10, 2)
    v, g = S.make_values((1, 48, *lr), "chan_offset", 12), S.make_values((1, 48, *out), "outlier", 13)
    r = S.backward_reference(q, k, v, g, ksz, 2)
    for name, ref in zip(("dq", "dk", "dv"), O.xna_backward(q, k, v, g, ksz, 2)):
        rel = float((r[name] - ref.double()).abs().max() / ref.abs().max())
        assert rel <= 2e-7, (name, rel)                                      # O.xna_backward returns fp32: one rounding, 6e-8
        assert bool((r["a_" + name] >= r[name].abs() * (1 - 1e-12)).all())   # an abs-sum dominates its sum
    assert bool((r["u_dq"] >= r["a_dq"] * (1 - 1e-12)).all()) and bool((r["u_dk"] >= r["a_dk"] * (1 - 1e-12)).all())
    # channel chunks: the same gradients; abs-sums that can only grow (|a + b| <= |a| + |b| per chunk)
    c = S.backward_reference(q, k, v, g, ksz, 2, chunks=[16, 8])
    for name in ("dq", "dk", "dv"):
        assert float((c[name] - r[name]).abs().max()) <= 1e-12 * float(r[name].abs().max())
    assert bool((c["a_dq"] >= r["a_dq"] * (1 - 1e-12)).all()) and bool((c["dq_store"] >= r["dq"].abs() * (1 - 1e-12)).all())


def test_attention_reference_equals_the_oracle():
    q, k, v = _fwd_inputs(("outlier", "peaked"))
    ref, a = S.attention_reference(q, k, v, 7, HEADS)
    assert float((ref - O.xna(q.double(), k.double(), v.double(), 7, HEADS)).abs().max()) == 0.0
    assert float((ref.float() - O.xna_lowres(q, k, v, 7, HEADS)).abs().max()) <= 1e-4 * float(ref.abs().max())
    assert bool((a >= ref.abs() * (1 - 1e-12)).all())
    assert float((S.attention_emulated(q, k, v, 7, HEADS, round_p=None) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# ---- feasibility: the emulation holds every bound the device test asserts --------------------------------------------------------
@pytest.mark.parametrize("fam", S.FORWARD_FAMILIES + S.FORWARD_FAMILIES_SHORT, ids=str)
def test_forward_emulation_holds_the_bound(fam):
    q, k, v = _fwd_inputs(fam)
    ref, a = S.attention_reference(q, k, v, 7, HEADS)
    for mode in ("normalised", "unnormalised"):
        for out_bf16 in ((False, True) if mode == "normalised" else (False,)):
            err = (S.attention_emulated(q, k, v, 7, HEADS, round_p=mode, out_bf16=out_bf16) - ref).abs()
            S.check(err, S.bf16_bound(1, a, ref.abs() if out_bf16 else None), f"emulation {mode} bf16-out={out_bf16} {fam}")
            if not out_bf16:
                assert S.worst_ratio(err, a) <= S.U                          # the hand-derived constant itself, before the 25 %
    # the fp32 bound of the scalar kernel is below half a bf16 rounding on every family: a bf16 intermediate would leave it
    assert S.fp32_score_factor(q, k, HEADS, 7) <= S.U / 3.0
    # a non-integer ratio (repeated taps) and a second window
    q2, k2 = S.make_qk((1, 128, 23, 27), (1, 128, 9, 10), fam[1], 40, HEADS)
    ref2, a2 = S.attention_reference(q2, k2, v, 9, HEADS)
    S.check((S.attention_emulated(q2, k2, v, 9, HEADS) - ref2).abs(), S.bf16_bound(1, a2), f"emulation, ratio 2.6 {fam}")


@pytest.mark.parametrize("fam", S.BACKWARD_FAMILIES + S.BACKWARD_FAMILIES_SHORT, ids=str)
def test_backward_emulation_holds_the_bounds(fam):
    q, k, v, g = _bwd_inputs(fam)
    for chunks in (None, [16, 16]):
        r = S.backward_reference(q, k, v, g, 5, HEADS, chunks=chunks)
        e = S.backward_reference(q, k, v, g, 5, HEADS, chunks=chunks, emulate=True)
        # the emulation is exact between its roundings, so it holds the bf16 terms alone; the device bound adds the fp32 term (backward_bounds)
        S.check((e["dq"] - r["dq"]).abs(), S.bf16_bound(1, r["a_dq"], r["dq_store"]), f"dq {fam} {chunks}")
        S.check((e["dk"] - r["dk"]).abs(), S.bf16_bound(1, r["a_dk"]), f"dk {fam} {chunks}")
        S.check((e["dv"] - r["dv"]).abs(), S.bf16_bound(1, r["a_dv"]), f"dv {fam} {chunks}")
        full = S.backward_bounds(r, q, k, HEADS, 5, "rows")
        assert all(bool((full[n] >= b).all()) for n, b in (("dq", S.bf16_bound(1, r["a_dq"], r["dq_store"])), ("dk", S.bf16_bound(1, r["a_dk"]))))
        assert S.worst_ratio((e["dk"] - r["dk"]).abs(), r["a_dk"]) <= S.U and S.worst_ratio((e["dv"] - r["dv"]).abs(), r["a_dv"]) <= S.U
    assert S.cancellation_factor(32, 25) <= S.U / 1000.0                          # (Dv + kk + 8) * 2^-24: a thousandth of one bf16 rounding
    gen = S.backward_bounds(r, q, k, HEADS, 5, "generic")
    assert bool((gen["dk"] <= full["dk"]).all()) and bool((gen["dv"] <= full["dv"]).all())      # the fp32 path's bounds are the tighter ones


def test_emulation_holds_the_bound_on_every_device_case():
    """Every geometry of tests/test_gpu_input_statistics.py (one family each here; the families are swept above on one geometry): the
    emulation with the path's rounding form is inside the bound that file asserts on that path."""
    T = S
    for case in T.FWD_CASES:
        if case[1] == "generic":
            continue                                                      # fp32 throughout: nothing to emulate
        fam = case[9][len(case[0]) % len(case[9])]
        q, k, v = T.forward_inputs(case, fam)
        ref, a = S.attention_reference(q, k, v, case[7], case[3])
        emu = S.attention_emulated(q, k, v, case[7], case[3], round_p="unnormalised" if case[1] == "rows" else "normalised")
        S.check((emu - ref).abs(), T.forward_bound(case, q, k, ref, a, torch.float32)[0], f"{case[0]} {fam}")
    for case in T.BWD_CASES:
        if case[1] == "generic":
            continue
        fam = case[9][len(case[0]) % len(case[9])]
        q, k, v, g = T.backward_inputs(case, fam)
        Dv = case[7] // case[2]
        chunks = [Dv // case[8]] * case[8] if case[8] > 1 else None
        r = S.backward_reference(q, k, v, g, case[6], case[2], chunks=chunks)
        e = S.backward_reference(q, k, v, g, case[6], case[2], chunks=chunks, emulate=True)
        bounds = S.backward_bounds(r, q, k, case[2], case[6], case[1])
        for n in ("dq", "dk", "dv"):
            S.check((e[n] - r[n]).abs(), bounds[n], f"{case[0]} {n} {fam}")


def test_key_offset_is_why_the_global_maximum_form_cannot_be_reused():
    """Under a common key offset the offset cancels exactly in dq (sum_j dS_ij = 0) and the roundings of dS do not: the emulation alone
    reaches 1.5e-2 of max|dq| -- most of tests/test_gpu_parity.py's 2e-2 -- while it sits inside the abs-sum bound like every family."""
    q, k, v, g = _bwd_inputs(("unit", "unit", "key_offset"))
    r = S.backward_reference(q, k, v, g, 5, HEADS)
    e = S.backward_reference(q, k, v, g, 5, HEADS, emulate=True)
    rel = float((e["dq"] - r["dq"]).abs().max() / r["dq"].abs().max())
    assert 8e-3 <= rel <= 2e-2, rel
    q0, k0, _, _ = _bwd_inputs(("unit", "unit", "unit"))
    r0 = S.backward_reference(q0, k0, v, g, 5, HEADS)
    e0 = S.backward_reference(q0, k0, v, g, 5, HEADS, emulate=True)
    assert float((e0["dq"] - r0["dq"]).abs().max() / r0["dq"].abs().max()) <= 5e-3


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------
DEFECTS = {"scale x 1.01": dict(scale_mul=1.01), "two of 64 query dims dropped": dict(drop_dims=2)}


@pytest.mark.parametrize("fam", S.FORWARD_FAMILIES, ids=str)
def test_forward_bound_catches_planted_defects(fam):
    q, k, v = _fwd_inputs(fam)
    ref, a = S.attention_reference(q, k, v, 7, HEADS)
    bound = S.bf16_bound(1, a)
    for name, kw in DEFECTS.items():
        over = int(((S.attention_emulated(q, k, v, 7, HEADS, **kw) - ref).abs() > bound).sum())
        visible = bool(((S.attention_emulated(q, k, v, 7, HEADS, round_p=None, **kw) - ref).abs() > 2.0 * bound).any())
        print(f"forward {fam} {name}: {over} of {ref.numel()} elements over the bound")
        assert visible == (fam[1] != "flat"), (fam, name)      # scores of 2.5e-3: neither defect changes the exact output
        assert (over > 0) == visible, (fam, name, over)
        if visible:
            assert over >= ref.numel() // 200                  # thousands of elements, not a lucky one


@pytest.mark.parametrize("fam", S.BACKWARD_FAMILIES, ids=str)
def test_backward_bounds_catch_planted_defects(fam):
    q, k, v, g = _bwd_inputs(fam)
    r = S.backward_reference(q, k, v, g, 5, HEADS)
    bounds = {n: b for n, b in S.backward_bounds(r, q, k, HEADS, 5, "rows").items() if not n.startswith("fp32")}      # what the device test asserts
    for name, kw in DEFECTS.items():
        p = S.backward_reference(q, k, v, g, 5, HEADS, emulate=True, **kw)
        x = S.backward_reference(q, k, v, g, 5, HEADS, **kw)
        over = {n: int(((p[n] - r[n]).abs() > b).sum()) for n, b in bounds.items()}
        visible = any(bool(((x[n] - r[n]).abs() > 2.0 * b).any()) for n, b in bounds.items())
        print(f"backward {fam} {name}: elements over the bound {over}")
        if name == "scale x 1.01":
            assert over["dq"] > 0, (fam, over)                # dS carries the scale as a factor: 1 % of dq on every family, flat included
        else:
            assert visible == (fam[2] != "flat") and (sum(over.values()) > 0) == visible, (fam, name, over)
            if visible:
                assert over["dq"] >= r["dq"].numel() // 200 and over["dk"] > 0 and over["dv"] > 0, (fam, name, over)


# ---- stem ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", S.IMAGE_FAMILIES)
def test_stem_emulation_holds_the_existing_bound(fam):
    p = O.make_params(seed=9)
    img = S.make_image(1, 64, 80, fam, 91)
    ref = O.conv_stem(img, p)
    err = (S.conv_stem_bf16(img, p) - ref).abs()
    mean_tol, max_tol = S.stem_bound(ref, fam)
    print(f"stem emulation {fam}: mean {float(err.mean()):.3e} max {float(err.max()):.3e} (|ref| max {float(ref.abs().max()):.1f})")
    assert float(err.mean()) <= mean_tol and float(err.max()) <= max_tol, (float(err.mean()), float(err.max()))
    if fam == "hot_pixel":                                      # ... and it needs that term: the absolute form alone fails the emulation
        assert float(err.max()) > S.STEM_MAX and float(ref.abs().max()) > 100.0


@pytest.mark.parametrize("fam", S.IMAGE_FAMILIES)
@pytest.mark.parametrize("ks,width", [(1, 128), (3, 128), (3, 96)])
def test_conv0_and_layer_bounds_are_feasible(fam, ks, width):
    img = S.make_image(1, 24, 40, fam, 61)
    w = O.hash_normal((width, 3, ks, ks), 62, 0.3)
    b = O.hash_normal((width,), 63, 0.1)
    ref, a = S.conv0_reference(img, w, b)
    y = S.bf16r(F.conv2d(F.pad(img, (ks // 2,) * 4, mode="reflect") if ks == 3 else img, w, b))      # fp32 convolution, one rounding
    bound = S.conv0_bound(ref, a, ks, width)
    S.check((y.double() - ref).abs(), bound, f"conv0 {fam}")
    assert bool(((S.group_sums(y) - S.group_sums(ref)).abs() <= S.group_sums_bound(ref, bound)).all())
    # the layer on top of it, activations rounded to bf16 before the convolution
    wl = S.bf16r(O.hash_normal((width, width, ks, ks), 72, 1.0 / (width ** 0.5 * ks)))
    bl = O.hash_normal((width,), 73, 0.1)
    gw, gb = 1.0 + O.hash_normal((width,), 74, 0.1), O.hash_normal((width,), 75, 0.1)
    rl, al = S.layer_reference(y, gw, gb, wl, bl)
    act = S.bf16r(F.silu(F.group_norm(y, 8, gw, gb, 1e-5)))
    yl = S.bf16r(S.conv_reflect64(act, wl, bl).float())
    S.check((yl.double() - rl).abs(), S.bf16_bound(1, al, rl.abs()), f"layer {fam}")


# ---- whole model and head ------------------------------------------------------------------------------------------------------------
def test_model_emulation_holds_the_whole_forward_bound():
    """bf16 stem + bf16 pooled guidance + bf16 q / k / v + bf16 P against the fp32-guidance oracle: inside 2e-2 + 1e-2 * sum_j P_j |v_j| on
    a natural-like normalised image with features that carry channel offsets AND outlier tokens (measured 0.80 / 0.71 of it), so the
    device test asserts that bound unchanged (no 1.5 x measured budget is needed)."""
    for size, ksz in (((64, 128), 7), ((50, 70), 5)):
        p, img, ft = S.model_case()
        ref, a = S.model_reference(p, img, ft, size, ksz)
        emu, _ = S.model_reference(p, img, ft, size, ksz, emulate=True)
        err = (emu - ref).abs()
        print(f"model emulation {size}: worst err / bound {float((err / S.model_bound(a)).max()):.3f}")
        S.check(err, S.model_bound(a), f"model emulation {size}")
    assert float(ft.abs().max()) > 100.0 and float(ft.mean(dim=(0, 2, 3)).abs().max()) > 10.0       # outlier tokens and channel means


@pytest.mark.parametrize("name", list(S.HEAD_CASES))
def test_head_inputs_leave_the_labels_determined(name):
    """The "determined share >= 0.75 from the oracle alone" condition of tests/test_gpu_head_objective.py for the inputs the device test
    feeds, under the scale-aware logit bound; the emulation (P rounded per head) is inside that bound."""
    B, h, w, dy, dx, ksz, heads = S.HEAD_GEOM
    N, _, mul, boff, dom = S.HEAD_CASES[name]
    q, k, pv, pvn, bias = S.make_head_inputs(name)
    assert torch.equal(pvn, S.bf16r(pvn)) and float(pv[..., N:].abs().sum()) == 0.0
    ref, a = S.head_reference64(q, k, pvn, ksz, heads, N, bias)
    bound = S.head_bound(ref, a)
    det, share = S.share_determined(ref, bound.amax(dim=1))
    print(f"head {name}: |ref| max {float(ref.abs().max()):.1f}, determined share {share:.3f}")
    assert share >= 0.75
    emu = S.attention_emulated(q, k, pvn, ksz, heads).view(B, heads, -1, h * dy, w * dx).sum(1)[:, :N] + bias.double().view(1, N, 1, 1)
    S.check((emu - ref).abs(), bound, f"head emulation {name}")
    assert torch.equal(emu.argmax(1)[det], ref.argmax(1)[det])
    if name in ("logits50", "bias40"):
        assert float(ref.abs().max()) > 30.0
    if dom is not None:
        assert float((ref.argmax(1) == dom).double().mean()) > 0.99
