"""CPU self-tests of tests/rope_pool_reference.py: the restatement agrees with the oracle, the exact construction IS exact at every case of the table, the
restated launch plan reaches the instance each case is there for, every planted defect changes the exact result (the counts are printed), and the
derived float bound holds for an fp32 emulation of the kernel's order while a one-row shift of the table at the slowest period leaves it.  Nothing
here checks which kernel ran: tests/test_gpu_rope_pool.py reads that from the profiler."""
import os
import sys

import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import rope_pool_reference as R  # noqa: E402


@pytest.mark.parametrize("name", ["B", "F", "H", "N"])
def test_restatement_agrees_with_the_oracle(name):
    c = R.CASE[name]
    x = O.hash_normal(c.shape(), 31 + c.Cq).double()
    per = O.rope_periods(c.Cq, c.heads, 100.0)
    ty, tx = R.tables64(per, *c.out)
    q, k, _, _ = R.rope_pool_reference(x, ty, tx, c.heads, c.lr)
    rq = O.rope(x, per, c.heads)
    rk = O.key_pool(rq, c.lr)
    assert float((R.nchw(q) - rq).abs().max()) <= 1e-12 and float((R.nchw(k) - rk).abs().max()) <= 1e-12


@pytest.mark.parametrize("c", R.CASES + [R.PRODUCTION], ids=repr)
def test_exact_equals_fp64_rounded_once(c):
    """The preconditions hold (rope_pool_exact asserts them) and the bits are those of the fp64 reference rounded once -- and of an fp32 evaluation."""
    for seed in (1, 2):
        x, ty, tx = c.exact_inputs(seed)
        assert float(x.abs().max()) <= R.X_MAX and float(ty.abs().max()) <= R.TAB_MAX and float(tx.abs().max()) <= R.TAB_MAX
        q, k = R.rope_pool_exact(x, ty, tx, c.heads, c.lr)
        q64, k64, _, _ = R.rope_pool_reference(x, ty, tx, c.heads, c.lr)
        assert torch.equal(q.double(), q64), "a query is not a bf16 number"
        assert R.first_mismatch(k, k64.to(torch.bfloat16), f"{c} keys against fp64 rounded once") is None
        q32, k32, _, _ = R.rope_pool_reference(x, ty, tx, c.heads, c.lr, torch.float32, inv32=True)
        assert torch.equal(q32.double(), q64) and torch.equal(k32.to(torch.bfloat16), k)
    assert not torch.equal(c.exact_inputs(1)[1], c.exact_inputs(2)[1]), "the two table sets are one"


@pytest.mark.parametrize("c", R.CASES, ids=repr)
def test_plan_reaches_the_instance_the_case_is_there_for(c):
    p = c.plan()
    assert p["status"] == "ok"
    for key, want in c.expect.items():
        assert p[key] == want, (c, key, p[key], want)
    pk = c.plan(write_q=False)
    assert pk["kernel"] == (c.keys_expect or c.expect["kernel"]), (c, pk)
    if c.name == "M":
        assert 16 * 1024 + 34848 > R.LDS_TABLE_BUDGET and p["lds"] == 16 * 1024
    if c.name == "L":
        assert c.plan(aligned=True)["VEC"] == 8, "only the offset makes L scalar"


def test_table_reaches_every_instance_and_the_refused_case_is_refused():
    seen = {c.plan()["kernel"] for c in R.CASES} | {c.plan(write_q=False)["kernel"] for c in R.CASES}
    assert seen == R.EXPECTED_INSTANCES
    assert {c.plan()["tab_lds"] for c in R.CASES if c.plan()["VEC"] == 8 and not c.plan()["multi"]} == {True, False}
    p = R.REFUSED.plan()
    assert p["status"] == "unsupported" and p["nchunk"] == 512 and p["VEC"] == 1


# (defect, the cases the construction must catch it at, the outputs it must show in)
PLANTED = [("row_shift_last", "B"), ("row_shift_last", "F"), ("col_shift_last", "B"), ("col_shift_last", "F"), ("col_for_row", "H"), ("angle_off_by_one", "N"),
           ("sin_sign", "A"), ("halves_swapped", "A"), ("head_next", "D"), ("floor_end", "B"), ("neighbour_divisor", "F"), ("neighbour_divisor", "K"),
           ("cell_decode_swapped", "E"), ("cell_decode_swapped", "K"), ("drop_last_cell", "C"), ("drop_last_cell", "E"), ("drop_trip_pixel", "B")]


@pytest.mark.parametrize("defect,name", PLANTED, ids=lambda v: str(v))
def test_planted_defect_changes_the_exact_result(defect, name):
    """Each defect changes at least one element of the exact q or k, with BOTH table sets."""
    c = R.CASE[name]
    for seed in (1, 2):
        x, ty, tx = c.exact_inputs(seed)
        q, k = R.rope_pool_exact(x, ty, tx, c.heads, c.lr)
        dq, dk, _, _ = R.rope_pool_reference(x, ty, tx, c.heads, c.lr, torch.float64, defect, inv32=True)
        nq, nk = int((dq.float().to(torch.bfloat16) != q).sum()), int((dk.float().to(torch.bfloat16) != k).sum())
        print(f"planted {defect:<20s} case {name} tables {seed}: {nq} of {q.numel()} queries, {nk} of {k.numel()} keys differ")
        assert nq + nk > 0
        if defect in ("row_shift_last", "col_shift_last", "floor_end", "neighbour_divisor", "drop_trip_pixel"):
            assert nk > 0, "a defect of the pooling must show in the keys"


def test_queries_of_the_whole_window_are_a_benign_race():
    """A cell that stored the queries of its whole window, not of its owned range, would store the SAME bits as the neighbour that owns the shared row /
    column (same pixel, same table rows): no value changes, at case F or anywhere.  What holds the owned-range test of rope_pool.hip:200 is that
    the ranges partition the image (asserted here) and the guard bands of the GPU test; the count of changed elements is 0 by construction."""
    c = R.CASE["F"]
    x, ty, tx = c.exact_inputs(1)
    q, k = R.rope_pool_exact(x, ty, tx, c.heads, c.lr)
    dq, dk = R.rope_pool_exact(x, ty, tx, c.heads, c.lr, "q_whole_window")
    print(f"planted q_whole_window       case F: {int((dq != q).sum())} queries, {int((dk != k).sum())} keys differ (the stores of both cells are equal)")
    assert torch.equal(dq, q) and torch.equal(dk, k)
    for L, n in ((c.out[0], c.lr[0]), (c.out[1], c.lr[1])):
        owned = [R.window(i, L, n) for i in range(n)]
        assert owned[0][0] == 0 and owned[-1][2] == L and all(owned[i][2] == owned[i + 1][0] for i in range(n - 1))
        assert any(owned[i][1] > owned[i][2] for i in range(n)), "windows overlap at this case"


def test_one_bf16_rounding_is_not_bounded_by_2_to_minus_9():
    """The unit roundoff of bf16 is 2^-8: 1 + 2^-8 lies half way between 1 and 1 + 2^-7 and rounds to 1 (even), an error of 2^-8 = 0.996 2^-8 |v|."""
    v = torch.tensor(1.0 + 2.0 ** -8)
    err = float((v.to(torch.bfloat16).float() - v).abs())
    assert err == 2.0 ** -8 and err > 2.0 ** -9 * float(v) and err <= S.U * float(v)


@pytest.mark.parametrize("name", ["A", "B", "F", "production"])
def test_float_bound_holds_the_emulation_and_not_a_shifted_row(name):
    """True tables (fp32, from the fp64 tables rounded once): the fp32 emulation of the kernel's order stays inside the derived bound at every element;
    with row y + 1 of tab_y used for y at the SLOWEST period only (the last angle index) elements leave it."""
    c = R.PRODUCTION if name == "production" else R.CASE[name]
    per = O.rope_periods(c.Cq, c.heads, 100.0)
    ty, tx = (t.float() for t in R.tables64(per, *c.out))
    for fam in ("unit", "chan_offset", "outlier"):
        x = S.make_values(c.shape(), fam, 77 + c.out[1])
        q, k, qa, ka = R.rope_pool_reference(x, ty, tx, c.heads, c.lr)
        bq, bk = R.float_bounds(q, k, qa, ka, c.lr)
        lanes = c.plan()["ppc"] if c.plan()["multi"] else c.plan()["planes"]
        eq, ek = R.rope_pool_emulated(x, ty, tx, c.heads, c.lr, lanes)
        S.check((eq.double() - q).abs(), bq, f"{name} {fam} emulated q")
        S.check((ek.double() - k).abs(), bk, f"{name} {fam} emulated k")
        bad = ty.clone()
        bad[:-1, :, -1] = ty[1:, :, -1]
        dq, dk = R.rope_pool_emulated(x, bad, tx, c.heads, c.lr, lanes)
        nq, nk = int(((dq.double() - q).abs() > bq).sum()), int(((dk.double() - k).abs() > bk).sum())
        print(f"{name} {fam}: emulated worst share q {S.worst_of_bound((eq.double() - q).abs(), bq):.3f} k {S.worst_of_bound((ek.double() - k).abs(), bk):.3f}; "
              f"row shift at the slowest period: {nq} queries, {nk} keys over the bound")
        assert nq > 0 and nk > 0


def test_epilogue_bound_catches_a_row_shift_under_integer_tables():
    """naf_stem_conv_keys_fwd's check: bf16 layer outputs (not integers), integer tables that differ from row to row.  A reference evaluated in fp32
    stays inside ``epilogue_key_bound``; one shifted row of tab_y, one shifted column of tab_x, a neighbouring angle index each leave it."""
    B, H, W = 1, 32, 32
    y = S.bf16r(O.hash_normal((B, 128, H, W), 5) * 1.5 + 0.3)
    ty, tx = R.integer_tables(H, W, 16, 9)
    q, k, qa, ka = R.rope_pool_reference(y, ty, tx, 2, (2, 2))
    bound = R.epilogue_key_bound(k, ka)
    k32 = R.rope_pool_reference(y, ty, tx, 2, (2, 2), torch.float32, inv32=True)[1]
    S.check((S.bf16r(k32).double() - k).abs(), bound, "fp32 evaluation")
    sy, sx = ty.clone(), tx.clone()
    sy[7] = ty[8]
    sx[20] = tx[21]
    for what, (a, b) in {"row": (sy, tx), "column": (ty, sx), "angle index": (ty.roll(1, -1), tx)}.items():
        kd = R.rope_pool_reference(y, a, b, 2, (2, 2))[1]
        over = (kd - k).abs() > bound
        print(f"epilogue keys, shifted {what}: {int(over.sum())} of {k.numel()} keys over the bound, worst {float(((kd - k).abs() / bound).max()):.0f} x")
        assert int(over.sum()) > 0 and float(((kd - k).abs() / bound).max()) > 10
