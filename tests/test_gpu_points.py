"""GPU tests of the point queries (naf_xna_points, ``ops.xna_points``, ``NAF.query``): for N points the scores, the softmax weights and the
feature vectors of the attention, without its dense tensors.

What is held, on the geometries of tests/points_reference.py (the smallest at which the index arithmetic can go wrong):
  * scores and features are BIT-equal to the pixel of ``ops.xna_forward(..., path="generic", out_dtype=float32, return_logits=True)`` (half
    values: after the same final rounding to half) -- the kernel restates that kernel's loops for one query;
  * the un-rotated-guidance form (the kernel rotates the vectors it reads) is bit-equal to the rotated-query form;
  * against the fp64 gather, features are within fp32_score_factor * sum P|v| and weights within that factor relative to P
    (tests/input_statistics.py::fp32_weight_factor: the bound of an all-fp32 softmax);
  * a point outside the grid gets NaN rows and changes no other row; nothing outside the N rows is written (guard bands, the technique of
    tests/test_gpu_layout_contract.py); strided k_lr / v_lr give the dense result; N = 1, 4m + 1 and 0.
"""
import os
import sys

import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import layout_contract as LC  # noqa: E402
import points_reference as PR  # noqa: E402
from test_gpu_parity import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_dense_cache = {}


def _operands(dev, name, B=1, half=False):
    """Device operands of a case (dense head-major 5-D) and the generic kernel's dense result for them, computed once per case."""
    from naf_amd import ops
    key = (name, B, half)
    if key not in _dense_cache:
        c = PR.CASES[name]
        q, k, v = PR.inputs(name, B, half)
        q5, k5 = LC.to5(q, c["heads"]).to(dev), LC.to5(k, c["heads"]).to(dev)
        v5 = None if v is None else LC.to5(v, c["heads"], torch.float16 if half else torch.bfloat16).to(dev)
        vv = v5 if v5 is not None else torch.zeros((B, c["heads"], *c["lr"], 16), dtype=torch.bfloat16, device=dev)
        odt = torch.float16 if half else torch.float32
        out5, logits = ops.xna_forward(q5, k5, vv, c["ksz"], path="generic", out_dtype=odt, return_logits=True)
        _dense_cache[key] = (q5, k5, v5, (out5 if v5 is not None else None), logits)
    return _dense_cache[key]


def _pixels(t5, pts):
    """[B, heads, Ho, Wo, D] at the points -> [N, heads, D]."""
    b, y, x = pts[:, 0].long(), pts[:, 1].long(), pts[:, 2].long()
    return t5[b, :, y, x]


@pytest.mark.parametrize("name,B,half,N", [("a", 1, False, 21), ("a", 1, False, 1), ("a", 1, True, 21), ("a", 2, False, 29),
                                           ("b", 1, False, 17), ("c", 1, False, 21), ("c", 1, False, 1)])
def test_points_equal_the_generic_kernels_pixels_and_meet_the_fp32_bound(dev, name, B, half, N):
    from naf_amd import ops
    c = PR.CASES[name]
    heads, ksz = c["heads"], c["ksz"]
    q5, k5, v5, out5, logits5 = _operands(dev, name, B, half)
    pts = PR.make_points(B, *c["out"], N)
    if B == 2:
        assert set(pts[:, 0].tolist()) == {0, 1} and len({tuple(p) for p in pts.tolist()}) < N       # both images, unsorted, duplicates
    pd = pts.to(dev, torch.int32)
    out, lg, pr = ops.xna_points(q5, k5, v5, pd, ksz, want_logits=True, want_probs=True)
    assert lg.shape == (N, heads, ksz * ksz) and lg.dtype == torch.float32 and pr.shape == lg.shape
    assert torch.equal(lg, _pixels(logits5, pd)), "scores differ from the generic kernel's pixel"
    if v5 is None:
        assert out is None
    else:
        assert out.shape == (N, c["C"]) and out.dtype == torch.float32
        want = _pixels(out5, pd).reshape(N, c["C"])
        if half:
            assert torch.equal(out.half(), want), "features differ from the generic kernel's pixel after its rounding to half"
        else:
            assert torch.equal(out, want), "features differ from the generic kernel's pixel"
    # against the fp64 gather: the bound of an all-fp32 softmax
    q, k, v = PR.inputs(name, B, half)
    r_lg, r_pr, r_out, abs_sum, _, _ = PR.point_query(q, k, v, pts, ksz, heads)
    f = S.fp32_score_factor(q, k, heads, ksz)
    e_p = (pr.double().cpu() - r_pr).abs()
    print(f"points {name} B={B} half={half} N={N}: factor {f:.3e}; weights worst err/P {float((e_p / r_pr).max()):.3e}")
    assert bool((e_p <= f * r_pr).all()), f"weights: worst err / P {float((e_p / r_pr).max()):.3e} > {f:.3e}"
    if v is not None:
        e_o = (out.double().cpu() - r_out).abs()
        print(f"  features worst err / sum P|v| {float((e_o / abs_sum).max()):.3e}")
        assert bool((e_o <= f * abs_sum).all()), f"features: worst err / sum P|v| {float((e_o / abs_sum).max()):.3e} > {f:.3e}"


def test_single_outputs_and_no_points(dev):
    """Each output alone is the bits it has among the others; N = 0 launches nothing and returns empty tensors."""
    from naf_amd import ops
    c = PR.CASES["a"]
    q5, k5, v5, _, _ = _operands(dev, "a")
    pd = PR.make_points(1, *c["out"], 9).to(dev, torch.int32)
    out, lg, pr = ops.xna_points(q5, k5, v5, pd, c["ksz"], want_logits=True, want_probs=True)
    o1, l1, p1 = ops.xna_points(q5, k5, v5, pd, c["ksz"], want_logits=False)
    assert l1 is None and p1 is None and torch.equal(o1, out)
    o2, l2, p2 = ops.xna_points(q5, k5, None, pd, c["ksz"])
    assert o2 is None and p2 is None and torch.equal(l2, lg)
    o3, l3, p3 = ops.xna_points(q5, k5, None, pd, c["ksz"], want_logits=False, want_probs=True)
    assert o3 is None and l3 is None and torch.equal(p3, pr)
    assert float((pr.sum(-1) - 1).abs().max()) <= 1e-5
    o0, l0, p0 = ops.xna_points(q5, k5, v5, pd[:0], c["ksz"], want_probs=True)
    assert o0.shape == (0, c["C"]) and l0.shape == (0, c["heads"], 25) and p0.shape == l0.shape


@pytest.mark.parametrize("name", ["a", "c"])
def test_unrotated_guidance_form_equals_rotated_queries(dev, name):
    """q = the un-rotated guidance + the RoPE tables: the kernel rotates the vectors it reads with naf_rope_pool_fwd's arithmetic and rounding."""
    from naf_amd import ops
    c = PR.CASES[name]
    heads, Dq, ksz, B = c["heads"], c["Dq"], c["ksz"], 2
    x = S.bf16r(O.hash_normal((B, heads * Dq, *c["out"]), 4400 + Dq)).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ty, tx = ops.rope_tables(O.rope_periods(heads * Dq, heads, 100.0).to(dev), *c["out"])
    q5, k5 = ops.rope_pool(x, ty, tx, heads, c["lr"])
    xq5 = x.permute(0, 2, 3, 1).unflatten(3, (heads, Dq)).permute(0, 3, 1, 2, 4)
    assert not torch.equal(xq5, q5)
    _, _, v = PR.inputs(name, B)
    v5 = LC.to5(v, heads).to(dev)
    pd = PR.make_points(B, *c["out"], 25).to(dev, torch.int32)
    rot = ops.xna_points(q5, k5, v5, pd, ksz, want_probs=True)
    raw = ops.xna_points(xq5, k5, v5, pd, ksz, want_probs=True, rope_tables=(ty, tx))
    for a, b, what in zip(rot, raw, ("features", "scores", "weights")):
        assert torch.equal(a, b), f"{what}: rotate-on-read differs from rotated queries"
    # ... and the rotated form is the generic kernel's pixel for these queries too
    out5, logits5 = ops.xna_forward(q5, k5, v5, ksz, path="generic", out_dtype=torch.float32, return_logits=True)
    assert torch.equal(raw[1], _pixels(logits5, pd)) and torch.equal(raw[0], _pixels(out5, pd).reshape(25, -1))


def test_points_outside_the_grid_get_nan_rows_and_change_nothing_else(dev):
    from naf_amd import ops
    c = PR.CASES["a"]
    Ho, Wo = c["out"]
    q5, k5, v5, _, _ = _operands(dev, "a", 2)
    good = PR.make_points(2, Ho, Wo, 13)
    bad = torch.tensor([[-1, 0, 0], [2, 3, 3], [0, -1, 5], [1, Ho, 0], [0, 2, -1], [1, 2, Wo], [0, 2 ** 31 - 1, 0], [0, 0, -2 ** 31],
                        [2 ** 30, 2 ** 30, 2 ** 30]])
    mixed = torch.empty(22, 3, dtype=torch.int64)
    where_bad = [0, 3, 4, 8, 11, 12, 16, 20, 21]
    where_good = [i for i in range(22) if i not in where_bad]
    mixed[where_bad], mixed[where_good] = bad, good
    clean = ops.xna_points(q5, k5, v5, good.to(dev, torch.int32), c["ksz"], want_probs=True)
    got = ops.xna_points(q5, k5, v5, mixed.to(dev, torch.int32), c["ksz"], want_probs=True)
    torch.cuda.synchronize()
    for a, b, what in zip(got, clean, ("features", "scores", "weights")):
        assert bool(torch.isnan(a[where_bad]).all()), f"{what}: a point outside the grid did not get NaN"
        assert torch.equal(a[where_good], b), f"{what}: rows of the points inside changed"


@pytest.mark.parametrize("N", [1, 21])
def test_nothing_is_written_outside_the_rows(dev, N):
    """Outputs inside guard bands of sentinels: the N rows are written in full, not one byte around them."""
    from naf_amd import ops
    c = PR.CASES["a"]
    q5, k5, v5, _, _ = _operands(dev, "a")
    pts = PR.make_points(1, *c["out"], N)
    pts[N // 2] = torch.tensor([0, c["out"][0], 0])                      # one point outside: its NaN rows stay inside as well
    pd = pts.to(dev, torch.int32)
    want = ops.xna_points(q5, k5, v5, pd, c["ksz"], want_probs=True)
    kk = c["ksz"] ** 2
    bufs = [LC.banded(s, torch.float32, dev) for s in ((N, c["C"]), (N, c["heads"], kk), (N, c["heads"], kk))]
    before = [a.clone() for _, a, _ in bufs]
    ops.xna_points(q5, k5, v5, pd, c["ksz"], out=bufs[0][0], logits=bufs[1][0], probs=bufs[2][0])
    torch.cuda.synchronize()
    for (t, arena, mask), b, w, what in zip(bufs, before, want, ("features", "scores", "weights")):
        assert LC.untouched(arena, b, mask), f"{what}: {LC.outside_writes(arena, b, mask)} elements outside the rows were written"
        assert LC.same_bits(t, w), f"{what}: the banded buffer holds other bits"
        assert not bool((LC.bits(t) == LC.SENT32).any()), f"{what}: an element of the rows was not written"


@pytest.mark.parametrize("family", ["channels_last", "head_major", "crop", "expanded"])
def test_strided_keys_and_values_give_the_dense_result(dev, family):
    from naf_amd import ops
    c = PR.CASES["a"]
    B = 2
    q5, k5, v5, _, _ = _operands(dev, "a", B)
    if family == "expanded":        # batch stride 0: both images read image 0's keys and values
        k5, v5 = k5[:1].expand(B, -1, -1, -1, -1).contiguous(), v5[:1].expand(B, -1, -1, -1, -1).contiguous()
    pd = PR.make_points(B, *c["out"], 21).to(dev, torch.int32)
    want = ops.xna_points(q5, k5, v5, pd, c["ksz"], want_probs=True)
    # q is a placed operand too (naf_xna_points takes q_stride[4]).  The queries differ between the images, so where the family is the
    # stride-0 one they sit in the crop: a batch stride of their own next to keys and values that have none
    placed = [LC.embed(q5, "crop" if family == "expanded" else family), LC.embed(k5, family), LC.embed(v5, family)]
    before = [a.clone() for _, a, _ in placed]
    if family == "expanded":
        assert placed[1][0].stride(0) == 0 and placed[2][0].stride(0) == 0
    got = ops.xna_points(placed[0][0], placed[1][0], placed[2][0], pd, c["ksz"], want_probs=True)
    torch.cuda.synchronize()
    for a, b, what in zip(got, want, ("features", "scores", "weights")):
        assert LC.same_bits(a, b), f"{what}: {family} operands give other bits than dense ones"
    for (_, arena, _), b in zip(placed, before):
        assert LC.unchanged(arena, b), "an input arena changed"


def test_query_end_to_end_against_the_oracle(dev):
    """``naf.query(g, points, features=f)`` at the pixels of O.naf_forward, within the project's forward-versus-oracle tolerance; the windows
    are the oracle's table rows; [N, 2] points for a batch of one; weights only with lr_size."""
    from naf_amd import NAF
    p = O.make_params(seed=41)
    m = NAF(kernel_size=5).eval()
    m.load_state_dict(p, strict=True)
    m = m.to(dev)
    img = O.hash_normal((2, 3, 96, 128), 4501)
    ft = O.hash_normal((2, 64, 7, 9), 4502)
    size = (96, 128)
    ref, ref_lg = O.naf_forward(p, img, ft, size, kernel_size=5, return_weights=True)
    pts = PR.make_points(2, *size, 25)
    g = m.guide(img.to(dev))
    r = m.query(g, pts, features=ft.to(dev), output_size=size, weights="both")          # points on the host, int64
    assert len(g._queries) == 0                                                          # no query tensor was written for 25 points
    b, y, x = pts[:, 0], pts[:, 1], pts[:, 2]
    assert r.features.shape == (25, 64) and r.features.dtype == torch.float32 and r.logits.shape == (25, 4, 25)
    assert_close(r.features.cpu(), ref[b, :, y, x], 2e-2, 1e-2, "query features")
    print(f"query scores vs oracle: max err {float((r.logits.cpu() - ref_lg[b, :, y, x]).abs().max()):.3e}, absmax {float(ref_lg.abs().max()):.3f}")
    assert float((r.probs.sum(-1) - 1).abs().max()) <= 1e-5
    iy, ix = O.axis_index_table(96, 7, 5), O.axis_index_table(128, 9, 5)
    assert r.window_y.dtype == torch.int32 and r.window_y.cpu().tolist() == iy[y.numpy()].tolist()
    assert r.window_x.cpu().tolist() == ix[x.numpy()].tolist()
    # the same rows as the dense scores of the Guidance call (another kernel: the same tolerance, not the same bits)
    _, dense_lg = m(g, ft.to(dev), size, return_weights=True)
    assert_close(r.logits.cpu(), dense_lg[b.to(dev), :, y.to(dev), x.to(dev)].cpu(), 2e-2, 1e-2, "query scores vs return_weights")
    # weights only, a batch of one with (y, x) points, a point outside
    g1 = m.guide(img[:1].to(dev))
    p2 = torch.cat([pts[pts[:, 0] == 0][:, 1:], torch.tensor([[96, 0]])])
    r1 = m.query(g1, p2.to(dev), output_size=size, lr_size=(7, 9), weights="softmax")
    assert r1.features is None and r1.logits is None and r1.probs.shape == (len(p2), 4, 25)
    assert bool(torch.isnan(r1.probs[-1]).all()) and r1.window_y[-1].tolist() == [-1] * 5 and r1.window_x[-1].tolist() == [-1] * 5
    # cached rotated queries (a dense materialising call came first) give the same bits as rotate-on-read
    m(g1, ft[:1].to(dev), size)
    assert (96, 128) in g1._queries
    r2 = m.query(g1, p2.to(dev), output_size=size, lr_size=(7, 9), weights="softmax")
    assert torch.equal(r2.probs[:-1], r1.probs[:-1])
