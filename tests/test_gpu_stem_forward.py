"""The forward conv stem, bit for bit: every forward instantiation of stem_conv_rows_kernel, stem_conv1x1_kernel, stem_convg_kernel<KS, WIDE> and the
conv0 kernels on inputs for which every fp32 partial sum is exactly representable (tests/stem_forward_reference.py derives the constructions and
says why accumulation order, MFMA shape and scheduling cannot change such a result; tests/test_stem_forward_cpu.py checks those claims and the
sensitivity to planted defects without a device).

  A  binary dense     x = m + {0, 1} under CHOSEN GroupNorm totals spread over all 16 copies of stats_in: every (tap, channel, pixel) takes part
  B  low-bit dense    the PLAIN layers and conv0 (f32, bf16 and strided bf16 images, NAF_CONV0_EXACT on and off, statistics-only launches)
  C  affine mapping   gamma impulses (one hot (pixel, channel), gamma_c in {+-0.5, +-1, +-2}) and the beta constant field (gamma = 0)
  D  census           w = 0, bias = group + 1: the GroupNorm sums are the integers (g + 1) n and (g + 1)^2 n, compared with torch.equal
  E  bf16 split       single products of 16 x 8, 8 x 16 and (NAF_CONV0_EXACT) 16 x 16 significant bits through stem_conv0_split_kernel

Outputs are compared with ``!=`` at EVERY element against the one bf16 rounding of the exact reference; a failure names the first differing
(b, y, x, oc) and the count.  GroupNorm sums of A, B and C are held to the any-order bound of an n-term fp32 sum, n 2^-24 sum |y| and (n + 1)
2^-24 sum y^2 (no measured constant).  conv0_moments_kernel + conv0_moment_sums_kernel work in fp64 on dyadic inputs of at most 48 bits: their
sums must EQUAL the fp64 sums of the exact outputs (bound 0).  The launchers' plans are restated in the helper and the property each shape is
there for is asserted from the device's own CU count; the kernel that ran is read from the profiler once per instantiation."""
import os
import re
import sys

import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stem_forward_reference as X  # noqa: E402
from test_gpu_input_statistics import kernels_run  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu_count(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---- which kernel ran -------------------------------------------------------------------------------------------------------------------------
_SEEN = set()


def template_args(name, base):
    """The template arguments of kernel ``base`` in a profiler name, as "a,b,c" -- or None.  The profiler demangles what its demangler knows and
    leaves the Itanium name otherwise (a __bf16 argument, DF16b); integers, booleans, float and __bf16 are all these kernels take."""
    m = re.search(r"(?:^|[\s:])" + re.escape(base) + r"<([^>]*)>", name)
    if m:
        return m.group(1).replace(" ", "")
    m = re.search(r"\d+" + re.escape(base) + r"I((?:Li\d+E|Lb[01]E|f|DF16b)+)E", name)
    if not m:
        return None
    tok = re.findall(r"Li(\d+)E|Lb([01])E|(f)|(DF16b)", m.group(1))
    return ",".join(i if i else (("true" if b == "1" else "false") if b else ("float" if f else "__bf16")) for i, b, f, h in tok)


def run_checked(fn, base, targs):
    """Run ``fn``; the first time an instantiation (base name, template arguments) is expected, run it under the profiler and require that a kernel
    of that name with those arguments was launched."""
    key = (base, targs)
    if key in _SEEN:
        fn()
        return
    names = kernels_run(fn)
    ran = {template_args(nm, base) for nm in names}
    assert targs in ran, f"expected {base}<{targs}>, the launch ran {sorted(names)}"
    _SEEN.add(key)


def layer_kernel(kernel, C, k, dense=True, plain=False, keys=False):
    b = lambda v: "true" if v else "false"
    if kernel == "rows":
        return "stem_conv_rows_kernel", f"0,{b(plain)},{b(keys)}"
    if kernel == "1x1":
        return "stem_conv1x1_kernel", f"false,float,{b(dense)},{b(plain)},{b(keys)}"
    return "stem_convg_kernel", f"{k},{b(C >= 128)}"


# ---- launches ---------------------------------------------------------------------------------------------------------------------------------
def place(t, layout, dev):
    """A bf16 device view of t's shape [B, H, W, C] for a launch to read or write, and the sentinel-filled canvas it lies in: dense, the lower /
    upper channel half of a buffer twice as wide, or a crop of a canvas whose rows are three pixels longer."""
    B, H, W, C = t.shape
    if layout == "dense":
        canvas = torch.full((B, H, W, C), SENTINEL, dtype=torch.bfloat16, device=dev)
        view = canvas
    elif layout in ("half_lo", "half_hi"):
        canvas = torch.full((B, H, W, 2 * C), SENTINEL, dtype=torch.bfloat16, device=dev)
        view = canvas[..., :C] if layout == "half_lo" else canvas[..., C:]
    else:
        canvas = torch.full((B, H, W + 3, C), SENTINEL, dtype=torch.bfloat16, device=dev)
        view = canvas[:, :, 2:2 + W]
    return view, canvas


def untouched(canvas, view):
    """Everything of the canvas outside the view still holds the sentinel."""
    mask = torch.ones(canvas.shape, dtype=torch.bool, device=canvas.device)
    if view.shape[-1] != canvas.shape[-1]:
        off = (view.data_ptr() - canvas.data_ptr()) // 2
        mask[..., off:off + view.shape[-1]] = False
    elif view.shape[2] != canvas.shape[2]:
        mask[:, :, 2:2 + view.shape[2]] = False
    else:
        return True
    return bool((canvas[mask] == SENTINEL).all())


def run_layer(dev, c, kernel, layout=("dense", "dense"), keys=False):
    """One forward layer on the case's inputs -> (y fp32 on the host, GroupNorm totals or None)."""
    from naf_amd import ops
    assert c.x_is_bf16 and c.exact_fp32 and c.any_order, "the construction is not exact in any order"
    B, H, W, C = c.B, c.H, c.W, c.C
    xv, xc = place(c.x, layout[0], dev)
    xv.copy_(c.x.to(torch.bfloat16))
    yv, yc = place(c.x, layout[1], dev)
    st_in = c.stats16.to(dev).contiguous()
    st_out = None if keys else ops.new_stats(B, dev)
    kk = None
    if keys:
        ty, tx = ops.rope_tables(O.rope_periods(256, 4, 100.0).to(dev), H, W)
        kbuf = torch.zeros((B, H // 16, W // 16, 128), dtype=torch.bfloat16, device=dev)
        kk = (kbuf, ty, tx)
    args = (xv, st_in, c.gamma.to(dev), c.beta.to(dev), X.EPS32, ops.pack_conv_weight(c.w).to(dev), c.bias.to(dev), yv, st_out)
    dense = layout == ("dense", "dense") and (H * W) % 32 == 0
    base, targs = layer_kernel(kernel, C, c.k, dense=dense, keys=keys)
    run_checked(lambda: ops.stem_conv(*args, keys=kk), base, targs)
    torch.cuda.synchronize()
    assert untouched(xc, xv) and untouched(yc, yv), "the launch wrote outside its output view"
    assert torch.equal(xv.float().cpu(), c.x), "the launch changed its input"
    return yv.float().cpu(), (None if keys else ops.stats_total(st_out).cpu())


def check_output(got, c, what):
    msg = X.first_mismatch(got, X.bf16r(c.ref.float()), what)
    assert msg is None, msg


def check_sums(sums, c, what, exact=False):
    if exact:
        assert torch.equal(sums, c.sums_ref), f"{what}: GroupNorm sums {sums.tolist()} != {c.sums_ref.tolist()}"
        return
    bound = X.sums_bound(c.sums_ref, c.sum_abs, c.n)
    err = (sums - c.sums_ref).abs()
    print(f"{what}: sums err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), f"{what}: GroupNorm sums off by {err.tolist()} against the any-order bound {bound.tolist()}"


def assert_plan(dev, kernel, shape):
    """The property the shape is there for, from the device's CU count."""
    cu = cu_count(dev)
    B, H, W = shape
    if kernel == "rows":
        p = X.conv3_plan(B, H, W, False, cu)
        if shape == (1, 22, 48):
            assert p["segs_y"] == 3 and p["last_rows"] == 6, p
        if shape == (2, 64, 64):
            assert p["grid"] % 8 == 0 and p["xcd_remap"], p
        if shape in ((1, 5, 20), (1, 7, 48), (2, 9, 33)):
            assert p["edge_strip"], p
    if kernel == "1x1":
        p = X.conv1x1_plan(B, H, W, cu)
        assert p["gpw"] == 1, p
        if shape == (1, 4, 8):
            assert p["groups"] == 1
        if shape == (1, 8, 20):
            assert p["groups"] == 5 and p["blocks"] == 2, p
        if shape in X.C1_SPARSE_SHAPES:
            assert p["partial_last"] and not p["dense"], p


# ---- forward layers: A, C, D --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.LAYER_CASES, ids=X.case_id)
def test_forward_layer_bit_exact(dev, case):
    kernel, con, shape, C, k, off = case
    assert_plan(dev, kernel, shape)
    c = X.build_layer(con, shape, C, k, off)
    got, sums = run_layer(dev, c, kernel)
    check_output(got, c, X.case_id(case))
    check_sums(sums, c, X.case_id(case), exact=con == "D")


@pytest.mark.parametrize("con", ["A", "D"])
def test_rows_layer_on_channel_halves_of_wider_buffers(dev, con):
    """x the lower and y the upper channel half of 256-wide buffers; the other halves keep their sentinel."""
    c = X.build_layer(con, X.ROWS_STRIDED_SHAPE, 128, 3)
    got, sums = run_layer(dev, c, "rows", layout=("half_lo", "half_hi"))
    check_output(got, c, f"rows {con} on channel halves")
    check_sums(sums, c, f"rows {con} on channel halves", exact=con == "D")


@pytest.mark.parametrize("con", ["A", "Cg", "D"])
def test_1x1_layer_on_a_crop_of_a_wider_canvas(dev, con):
    """Rows of stride (W + 3) C on both sides: the kernel that is not DENSE although H W is a multiple of 32."""
    c = X.build_layer(con, X.C1_CROP_SHAPE, 128, 1)
    got, sums = run_layer(dev, c, "1x1", layout=("crop", "crop"))
    check_output(got, c, f"1x1 {con} on a crop")
    check_sums(sums, c, f"1x1 {con} on a crop", exact=con == "D")


@pytest.mark.parametrize("con", X.TRIPS_CONS)
def test_1x1_layer_three_groups_per_wave(dev, con):
    """(1, 256, W*) with W* from the CU count: every wave takes three trips through the in-wave pipeline (an odd count: both buffers turn over)."""
    cu = cu_count(dev)
    shape = X.conv1x1_trips_shape(cu)
    p = X.conv1x1_plan(*shape, cu)
    assert p["gpw"] == 3 and p["trips"] == (3, 3) and p["dense"], p
    c = X.build_layer(con, shape, 128, 1)
    got, sums = run_layer(dev, c, "1x1")
    check_output(got, c, f"1x1 {con} {shape}")
    check_sums(sums, c, f"1x1 {con} {shape}", exact=con == "D")


@pytest.mark.parametrize("case", X.KEYS_CASES, ids=X.case_id)
def test_keys_layer_output_bit_exact(dev, case):
    """The key-pooling instantiations: the layer's own output (the pooled keys stay with tests/test_gpu_keys.py and test_gpu_stem_rows_shape.py)."""
    kernel, (B, H, W), k = case
    c = X.binary_dense(B, H, W, 128, k)
    got, _ = run_layer(dev, c, kernel, keys=True)
    check_output(got, c, X.case_id(case))


# ---- PLAIN layers: B ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.PLAIN_CASES, ids=X.case_id)
def test_plain_layer_bit_exact(dev, case):
    from naf_amd import ops
    kernel, (B, H, W), C, k = case
    c = X.lowbit_dense(B, H, W, C, k)
    assert c.x_is_bf16 and c.exact_fp32 and c.any_order
    xd = c.x.to(torch.bfloat16).to(dev)
    y = torch.full_like(xd, SENTINEL)
    base, targs = layer_kernel(kernel, C, k, dense=(H * W) % 32 == 0, plain=True)
    run_checked(lambda: ops.stem_conv_plain(xd, ops.pack_conv_weight(c.w).to(dev), y, bias=c.bias.to(dev)), base, targs)
    check_output(y.float().cpu(), c, X.case_id(case))


# ---- first convolution: B, D ------------------------------------------------------------------------------------------------------------------------
def conv0_image(img, dtype, strided, dev):
    if not strided:
        return img.to(dtype).to(dev)
    B, _, H, W = img.shape
    canvas = torch.full((B, 3, H + 3, 2 * W + 10), SENTINEL, dtype=dtype, device=dev)
    view = canvas[:, :, 2:2 + H, 3:3 + 2 * W:2]
    view.copy_(img.to(dtype))
    return view


def conv0_kernel(C, k, dtype, exact, stores):
    t = "float" if dtype == torch.float32 else "__bf16"
    if C != 128:
        return "stem_conv0_generic_kernel", f"{k},{t}"
    if k == 3:
        return "stem_conv0_split_kernel", f"{t},{0 if exact else 3}"
    return ("stem_conv0_kernel", f"1,{t}") if stores else ("conv0_moments_kernel", t)


def run_conv0(dev, c, dtype=torch.float32, strided=False, exact=False, stores=True):
    from naf_amd import ops
    B, H, W, C = c.B, c.H, c.W, c.C
    img = conv0_image(c.img, dtype, strided, dev)
    y = torch.full((B, H, W, C), SENTINEL, dtype=torch.bfloat16, device=dev) if stores else None
    st = ops.new_stats(B, dev)
    base, targs = conv0_kernel(C, c.k, dtype, exact, stores)
    w, bias = c.w.to(dev).contiguous(), c.bias.to(dev)
    if exact:
        run_checked(lambda: ops.stem_conv0(img, w, bias, y, st, exact=True), base, targs)
    else:
        run_checked(lambda: ops.stem_conv0(img, w, bias, y, st), base, targs)
    torch.cuda.synchronize()
    return (y.float().cpu() if stores else None), ops.stats_total(st).cpu(), img


def conv0_variants(C, k, shape):
    """(image dtype, strided, exact) of a conv0 case: f32 and bf16 images, the strided bf16 image at (1, 37, 70), NAF_CONV0_EXACT for the split kernel."""
    out = [(torch.float32, False, False), (torch.bfloat16, shape == (1, 37, 70), False)]
    if C == 128 and k == 3:
        out += [(dt, st, True) for dt, st, _ in out]
    return out


@pytest.mark.parametrize("case", X.CONV0_CASES, ids=X.case_id)
def test_conv0_bit_exact_and_census(dev, case):
    C, k, (B, H, W) = case
    c, d = X.conv0_lowbit(B, H, W, C, k), X.conv0_census(B, H, W, C, k)
    assert c.img_is_bf16 and c.w_is_bf16 and c.exact_fp32 and c.any_order
    for dtype, strided, exact in conv0_variants(C, k, (B, H, W)):
        what = f"conv0 {X.case_id(case)} {dtype} strided={strided} exact={exact}"
        got, sums, _ = run_conv0(dev, c, dtype, strided, exact)
        check_output(got, c, what)
        check_sums(sums, c, what)
        got, sums, _ = run_conv0(dev, d, dtype, strided, exact)
        check_output(got, d, what + " census")
        check_sums(sums, d, what + " census", exact=True)


@pytest.mark.parametrize("case", X.CONV0_CASES + [(128, 1, X.CONV0_VEC4_SHAPE)], ids=X.case_id)
def test_conv0_statistics_only(dev, case):
    """y == NULL.  k = 1, width 128: conv0_moments_kernel (scalar path; four-pixel path at (2, 12, 40)) and conv0_moment_sums_kernel add and combine
    dyadic numbers of at most 48 bits in fp64 -- every product and sum is exact, so the sums EQUAL the fp64 sums of the exact outputs.  Otherwise
    the convolution kernel runs without its stores: the any-order bound of its fp32 sums."""
    C, k, (B, H, W) = case
    c, d = X.conv0_lowbit(B, H, W, C, k), X.conv0_census(B, H, W, C, k)
    moments = C == 128 and k == 1
    assert X.moments_bits(c) <= 48
    for dtype, strided, exact in conv0_variants(C, k, (B, H, W)):
        what = f"conv0 sums only {X.case_id(case)} {dtype} strided={strided} exact={exact}"
        _, sums, img = run_conv0(dev, c, dtype, strided, exact, stores=False)
        if moments:
            assert X.moments_vec4(img) == ((B, H, W) == X.CONV0_VEC4_SHAPE), "the shape does not take the path it is there for"
        check_sums(sums, c, what, exact=moments)
        _, sums, _ = run_conv0(dev, d, dtype, strided, exact, stores=False)
        check_sums(sums, d, what + " census", exact=True)


@pytest.mark.parametrize("k", [1, 3])
def test_conv0_three_segments_per_wave(dev, k):
    """(1, H*, 1000) with H* from the CU count: the waves of stem_conv0_kernel<1> / stem_conv0_split_kernel<T, 3> and <T, 0> walk three segments (the
    next segment's taps are in flight while the current one is multiplied), every row ends in a partial segment."""
    cu = cu_count(dev)
    shape = X.conv0_trips_shape(k, cu)
    p = X.conv0_plan(k, *shape, cu)
    assert p["gpw"] == 3 and p["trips"][1] == 3, p
    c, d = X.conv0_lowbit(*shape, 128, k), X.conv0_census(*shape, 128, k)
    assert c.exact_fp32 and c.any_order
    for exact in ([False, True] if k == 3 else [False]):
        what = f"conv0 k{k} {shape} exact={exact}"
        got, sums, _ = run_conv0(dev, c, exact=exact)
        check_output(got, c, what)
        check_sums(sums, c, what)
        got, sums, _ = run_conv0(dev, d, exact=exact)
        check_output(got, d, what + " census")
        check_sums(sums, d, what + " census", exact=True)


# ---- the bf16 split: E --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", X.E_SHAPES, ids=X.case_id)
@pytest.mark.parametrize("bits", X.E_BITS, ids=X.case_id)
def test_conv0_split_products(dev, shape, bits):
    """16 x 8 bits = x0 w0 + x1 w0 and 8 x 16 = x0 w0 + x0 w1 must come out exact with three and with six terms; 16 x 16 with six terms is within fp32
    roundings of x w, and no product of the chosen inputs lies within 2^-21 relative of a bf16 boundary: the stored value is bf16(float32(x w))."""
    for off in range(3):
        c = X.conv0_impulses(*shape, *bits, off)
        assert c.nhot > 0 and c.max_terms == 1 and c.img_fp32 and c.w_fp32
        if bits == (16, 16):
            assert c.margin >= 2.0 ** -21 > 2.0 ** -24
        else:
            assert c.product_fp32
        for exact in ([True] if bits == (16, 16) else [False, True]):
            got, _, _ = run_conv0(dev, c, exact=exact)
            check_output(got, c, f"split {bits} bits {shape} offset {off} exact={exact}")
