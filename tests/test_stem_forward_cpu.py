"""The exact forward-stem tests without a device (tests/stem_forward_reference.py explains the constructions): (1) every construction is what it
claims -- exact in fp32 and in any order for every (kernel, shape) pair the device test runs, the alphabet's margins, rstd == 1.0f and an exactly
zero background under an fp32 restatement of the kernels' statements in both the fma and the mul + add form, representable inputs, census partial
sums below 2^24; (2) the references agree with torch fp64 of the real operation within the existing single-layer bound; (3) an fp32 / bf16
emulation of a layer reproduces the reference exactly and, with one planted defect, differs from it on every shape where the defect is reachable."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import input_statistics as S  # noqa: E402
import stem_backward_reference as R  # noqa: E402
import stem_forward_reference as X  # noqa: E402

CU = X.DEFAULT_CU
TRIPS = X.conv1x1_trips_shape(CU)


def log2e_of(kernel):
    return kernel != "generic"


def all_layer_cases():
    return X.LAYER_CASES + [("1x1", con, TRIPS, 128, 1, 0) for con in X.TRIPS_CONS]


# ---- (1) the constructions ------------------------------------------------------------------------------------------------------------------
def test_chosen_statistics_give_unit_rstd_and_a_zero_background():
    """All 16 means at every n of the device test, gamma in {+-0.5, +-1, +-2}: rstd == 1.0f, mean exact, and x = m gives z == 0 and a == 0 in the
    fma and the mul + add form, with and without the log2(e) factor."""
    sizes = sorted({(s, C) for _, _, s, C, _, _ in all_layer_cases()} | {(s, 128) for _, s, _ in X.KEYS_CASES})
    means = torch.tensor(X.MEANS, dtype=torch.float64).view(2, 8)
    for (B, H, W), C in sizes:
        n = H * W * (C // 8)
        stats16, q = X.spread_totals(X.chosen_totals(means, n))
        assert bool((q[..., 0] == n * means).all())
        assert bool((stats16 != 0).any(dim=0).sum() >= 30), "the totals must sit in all copies"
        for gm in X.GAMMAS:
            gamma = torch.full((C,), gm)
            for log2e in (False, True):
                scale, shift, rstd = X.gn_vectors32(stats16, H, W, C, gamma, torch.zeros(C), log2e)
                assert bool((rstd == 1.0).all()), (H, W, C)
                k = torch.tensor(X.LOG2E if log2e else 1.0, dtype=torch.float32)
                assert bool((scale == gm * k).all())
                x = X.per_channel(means, C).expand(2, 1, 3, C).float()
                for fma in (True, False):
                    a, z = X.act_emulated(x, scale, shift, log2e, fma)
                    assert bool((z == 0).all()) and bool((a == 0).all()), (H, W, C, gm, log2e, fma)


def test_alphabet_margins_and_stored_values():
    """Every letter keeps >= 4e-4 |SiLU| from a bf16 boundary (z = 2 and 6 do not, which is why they are left out), every (mean, gamma) keeps at
    least three usable letters, z = 1 among them, and the fp32 emulation of the kernels' activation stores the value the reference assumes."""
    for z in X.ALPHABET:
        v = float(X.silu64(z))
        assert float(X.bf16_margin(v)) >= 4e-4 * abs(v), z
    assert float(X.bf16_margin(X.silu64(2.0))) < 1e-4 * float(X.silu64(2.0)) and float(X.bf16_margin(X.silu64(6.0))) < 2e-4 * float(X.silu64(6.0))
    assert float(X.act_value(1.0)) == X.A1
    for m in X.MEANS:
        for gm in X.GAMMAS + (1.0,):
            letters = X.allowed_z(m, gm)
            assert len(letters) >= 3 and 1.0 in letters, (m, gm, letters)
            for z in letters:
                assert float(X.bf16_margin(X.silu64(z))) >= X.MARGIN_FACTOR * X.da_bound(m, gm, z)


@pytest.mark.parametrize("case", all_layer_cases(), ids=X.case_id)
def test_layer_constructions_are_exact_in_any_order(case):
    kernel, con, shape, C, k, off = case
    c = X.build_layer(con, shape, C, k, off)
    assert c.x_is_bf16, "an input is no bf16 number"
    assert c.exact_fp32, "the reference does not survive .float().double()"
    assert c.any_order, f"abs-sum {c.abs_sum_max} at lsb 2^{c.lsb} leaves 24 bits"
    if con == "A":
        assert c.lsb == -11 and c.abs_sum_max <= 466 * 2, c.abs_sum_max
    if con == "D":
        B, H, W = shape
        assert X.census_partial_max(kernel, B, H, W, C, CU) < 2 ** 24
        assert torch.equal(c.sums_ref, X.census_sums(B, H, W, C))
    if c.chosen:
        # the alphabet's margin at every hot element, from act_forward itself with the chosen statistics
        f = R.act_forward(c.x, c.gamma, c.beta, X.EPS, c.totals)
        assert bool((f["rstd"] == 1.0).all()) or float((f["rstd"] - 1.0).abs().max()) < 1e-9
        margin = X.bf16_margin(f["a"])
        assert bool((margin[c.hot] >= X.MARGIN_FACTOR * f["da_"][c.hot]).all())
        assert bool((f["a"][~c.hot] == 0).all()), "the background is not zero"


@pytest.mark.parametrize("case", X.PLAIN_CASES + [(kn, s, 128, k) for kn, s, k in X.KEYS_CASES], ids=X.case_id)
def test_plain_and_keys_constructions_are_exact_in_any_order(case):
    kernel, (B, H, W), C, k = case
    c = X.lowbit_dense(B, H, W, C, k) if case in X.PLAIN_CASES else X.binary_dense(B, H, W, C, k)
    assert c.x_is_bf16 and c.exact_fp32 and c.any_order, (c.abs_sum_max, c.lsb)
    if c.kind == "B":
        assert c.abs_sum_max * 2.0 ** -c.lsb < 2 ** 17      # "within 16 bits" plus the bias


@pytest.mark.parametrize("case", X.CONV0_CASES + [(128, 1, X.conv0_trips_shape(1, CU)), (128, 3, X.conv0_trips_shape(3, CU)), (128, 1, X.CONV0_VEC4_SHAPE)],
                         ids=X.case_id)
def test_conv0_constructions_are_exact_in_any_order(case):
    C, k, (B, H, W) = case
    c = X.conv0_lowbit(B, H, W, C, k)
    assert c.img_is_bf16 and c.w_is_bf16, "the split's middle and low parts must vanish"
    assert all(bool((p == 0).all()) for p in X.split3(c.img)[1:] + X.split3(c.w)[1:])
    assert c.exact_fp32 and c.any_order and c.abs_sum_max * 2.0 ** -c.lsb < 2 ** 15, (c.abs_sum_max, c.lsb)
    assert X.moments_bits(c) <= 48
    d = X.conv0_census(B, H, W, C, k)
    assert torch.equal(d.sums_ref, X.census_sums(B, H, W, C))
    if C == 128:
        assert X.census_partial_max("conv0", B, H, W, C, CU, k) < 2 ** 24
    else:
        assert X.census_partial_max("generic", B, H, W, C, CU) < 2 ** 24


@pytest.mark.parametrize("shape", X.E_SHAPES, ids=X.case_id)
@pytest.mark.parametrize("bits", X.E_BITS, ids=X.case_id)
@pytest.mark.parametrize("off", range(3))
def test_split_impulses_are_single_products(shape, bits, off):
    c = X.conv0_impulses(*shape, *bits, off)
    assert c.nhot > 0 and c.max_terms == 1 and c.img_fp32 and c.w_fp32
    if bits != (16, 16):
        assert c.product_fp32, "a 16 x 8 bit product must be an fp32 number"
        for terms in (3, 6):
            assert X.first_mismatch(X.conv0_split_emulated(c.img, c.w, terms), X.bf16r(c.ref), "split emulation") is None
    else:
        assert c.margin >= 2.0 ** -21
        assert X.first_mismatch(X.conv0_split_emulated(c.img, c.w, 6), X.bf16r(c.ref.float()), "split emulation") is None
    if bits[0] == 16:          # the planted defect: the image's middle part dropped
        got = X.conv0_split_emulated(c.img, c.w, 6 if bits == (16, 16) else 3, drop_middle=True)
        assert X.first_mismatch(got, X.bf16r(c.ref.float()), "dropped middle part") is not None


def test_plans_reach_what_the_shapes_are_there_for():
    p = X.conv3_plan(1, 22, 48, False, CU)
    assert p["segs_y"] == 3 and p["seg_h"] == 8 and p["last_rows"] == 6
    p = X.conv3_plan(2, 64, 64, False, CU)
    assert p["grid"] == 32 and p["xcd_remap"]
    assert X.conv3_plan(1, 5, 20, False, CU)["edge_strip"] and X.conv3_plan(2, 9, 33, False, CU)["tiles_x"] == 2
    assert X.conv1x1_plan(1, 4, 8, CU)["groups"] == 1
    p = X.conv1x1_plan(1, 8, 20, CU)
    assert p["groups"] == 5 and p["blocks"] == 2 and p["dense"]
    assert X.conv1x1_plan(1, 5, 9, CU)["partial_last"] and not X.conv1x1_plan(2, 9, 33, CU)["dense"]
    assert not X.conv1x1_plan(1, 8, 20, CU, dense_rows=False)["dense"]
    p = X.conv1x1_plan(*TRIPS, CU)
    assert p["gpw"] == 3 and p["trips"] == (3, 3) and p["dense"]
    assert X.conv0_plan(3, 1, 200, 1000, 256)["gpw"] == 3                     # the issue's example
    for k in (1, 3):
        p = X.conv0_plan(k, *X.conv0_trips_shape(k, CU), CU)
        assert p["gpw"] == 3 and p["trips"][1] == 3
    # every (pixel slot, channel) pair of the 1x1 gamma impulses occurs on the largest shape
    hc = X.hot_channel_1x1(*TRIPS, 128).flatten()
    pairs = torch.unique((torch.arange(hc.numel()) % 32) * 128 + hc)
    assert pairs.numel() == 32 * 128


# ---- (2) agreement with torch fp64 of the real operation ---------------------------------------------------------------------------------------
SMALL_CASES = [c for c in X.LAYER_CASES if c[2] != (2, 64, 64) or c[1] == "A"]


@pytest.mark.parametrize("case", SMALL_CASES, ids=X.case_id)
def test_references_agree_with_torch_fp64_and_the_emulation_reproduces_them(case):
    kernel, con, shape, C, k, off = case
    c = X.build_layer(con, shape, C, k, off)
    ref, bound, f = X.layer_torch64(c)
    S.check((c.ref.double() - ref).abs(), bound, f"{X.case_id(case)} against torch fp64")
    if not c.chosen:
        assert X.group_norm_agrees(c) < 1e-9            # the totals carry 40 bits: 2^-41 relative, on activations below 10
    want = X.bf16r(c.ref)
    for fma in (True, False):
        got = X.layer_emulated(c, log2e_of(kernel), fma)
        msg = X.first_mismatch(got, want, f"emulation (fma={fma})")
        assert msg is None, msg


@pytest.mark.parametrize("case", X.PLAIN_CASES, ids=X.case_id)
def test_plain_references_agree_with_torch(case):
    kernel, (B, H, W), C, k = case
    c = X.lowbit_dense(B, H, W, C, k)
    ref = X.conv_nhwc64(c.x.double(), c.w.double(), c.bias.double())
    assert torch.equal(ref, c.ref.double())
    assert X.first_mismatch(X.plain_emulated(c), X.bf16r(c.ref), "plain emulation") is None


# ---- (3) sensitivity ----------------------------------------------------------------------------------------------------------------------------
def _seams(kernel, shape):
    B, H, W = shape
    return X.rows_seams(B, H, W, CU) if kernel == "rows" else (X.generic_seams(H) if kernel == "generic" else [])


def reachable(defect, case):
    kernel, con, shape, C, k, off = case
    if defect in ("tap_shift", "chunk_swap", "means_swap"):
        return con == "A" and (defect != "tap_shift" or shape[2] > 1)
    if defect == "clamp_right":
        return con == "A" and k == 3
    if defect == "seam_row":
        return con == "A" and k == 3 and bool(_seams(kernel, shape))
    if defect == "gamma_swap":
        return con == "Cg" and bool(X.build_layer(con, shape, C, k, off).hot[..., :16].any())
    return False


SENSITIVITY = [(d, c) for d in X.DEFECTS[:-1] for c in SMALL_CASES if c[1] in ("A", "Cg") and reachable(d, c)]


@pytest.mark.parametrize("defect,case", SENSITIVITY, ids=lambda v: v if isinstance(v, str) else X.case_id(v))
def test_one_planted_defect_changes_at_least_one_element(defect, case):
    kernel, con, shape, C, k, off = case
    c = X.build_layer(con, shape, C, k, off)
    want = X.bf16r(c.ref)
    seams = _seams(kernel, shape) if defect == "seam_row" else [None]
    for seam in seams:
        got = X.layer_emulated(c, log2e_of(kernel), True, defect=defect, seam=seam)
        assert X.first_mismatch(got, want, defect) is not None, f"{defect} (seam {seam}) goes unseen on {X.case_id(case)}"


def test_every_defect_is_reachable_somewhere():
    seen = {d for d, _ in SENSITIVITY}
    assert seen == set(X.DEFECTS[:-1]), seen
    assert any(c[0] == "rows" for d, c in SENSITIVITY if d == "seam_row") and any(c[0] == "generic" for d, c in SENSITIVITY if d == "seam_row")


def test_reused_pipeline_buffer_changes_the_third_group():
    """The 1x1 walk at (1, 256, W*): a wave's third group (group 8 of workgroup 0) reading its first group's pixels."""
    c = X.build_layer("Cg", TRIPS, 128, 1)
    want = X.bf16r(c.ref)
    assert X.first_mismatch(X.layer_emulated(c, True, True), want, "emulation") is None
    msg = X.first_mismatch(X.layer_emulated(c, True, True, defect="pipeline_reuse"), want, "reused buffer")
    assert msg is not None and "(0, 0, 256," in msg, msg          # the first wrong pixel is index 256 = the third group's first


def test_census_notices_one_row_counted_twice():
    for kernel, con, (B, H, W), C, k, off in all_layer_cases():
        if con == "D":
            good = X.census_sums(B, H, W, C)
            assert bool((X.census_sums(B, H, W, C, twice_row=H // 2) != good).all())
            assert bool((good == torch.round(good)).all()) and float(good.max()) < 2.0 ** 53
