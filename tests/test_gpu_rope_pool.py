"""The RoPE and key-pooling forward on the device: every instance of rope_pool_kernel<T, VEC, MULTI>, rope_pool_keys_kernel, rope_tables_kernel and the
key epilogue of the last stem layers (tests/rope_pool_reference.py derives the constructions and the bounds; tests/test_rope_pool_cpu.py checks
them and their sensitivity to planted defects without a device).

  exact    integer guidance in [-8, 8] and integer tables in [-15, 15] (two sets per case): every fp32 partial sum is exactly representable, so q
           and k are compared with ``!=`` at EVERY element against ``rope_pool_exact``; a failure names the first differing (b, head, y, x, d) and
           the count.  Each case asserts the property it is there for from the restated launch plan, and the kernel that RAN (name and template
           arguments) is read from the profiler at every case, with and without q.  ``tab_lds`` is a launch parameter, not part of a kernel's
           name: it is asserted from the plan.
  layout   x, q and k in sentinel-filled arenas (tests/layout_contract.py): bit-equal views, nothing written outside them, inputs unchanged,
           outputs finite; the layouts that are not vectorisable must run the VEC = 1 instance and give the same bits.
  float    the tables of ops.rope_tables and input_statistics' value families against the fp64 reference fed the SAME device tables, inside the
           derived per-element bounds; the worst share of each bound is printed.
  epilogue naf_stem_conv_keys_fwd under integer tables: keys of the layer's own bf16 output inside the any-order bound of the 256-term sum."""
import ctypes as C
import os
import sys

import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import layout_contract as L  # noqa: E402
import rope_pool_reference as R  # noqa: E402
import stem_backward_reference as SB  # noqa: E402
from test_gpu_input_statistics import kernels_run  # noqa: E402
from test_gpu_keys import _layer_inputs  # noqa: E402
from test_gpu_stem_forward import layer_kernel, template_args  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def spellings(base, targs):
    """The names a profiler may give rope_pool_kernel<targs>: the Itanium name, and what the C++ runtime's own demangler makes of it.  Demanglers
    that predate __bf16 (DF16b) leave the name as it is or misread it (<__bf16, 1, false> comes out as <bool _Accum, int, E, false>), so the name is
    not parsed: it is compared with what THIS host's demangler answers for the expected instance."""
    t, v, m = targs.split(",")
    mangled = f"_Z{len(base)}{base}I{'DF16b' if t == '__bf16' else 'f'}Li{v}ELb{1 if m == 'true' else 0}EEv14RopePoolParams"
    out = {mangled}
    try:
        cxx = C.CDLL("libstdc++.so.6")
        cxx.__cxa_demangle.restype = C.c_void_p
        status = C.c_int()
        ptr = cxx.__cxa_demangle(mangled.encode(), None, None, C.byref(status))
        if status.value == 0 and ptr:
            out.add(C.string_at(ptr).decode())
    except OSError:
        pass
    return out


def assert_ran(fn, kernel):
    """Run ``fn`` under the profiler and require a launch of ``kernel`` = (base name, template arguments or None)."""
    base, targs = kernel
    names = kernels_run(fn)
    if targs is None:
        assert any(base in nm for nm in names), f"expected {base}, the launch ran {sorted(names)}"
    elif base == "rope_pool_kernel":
        want = spellings(base, targs)
        assert any(template_args(nm, base) == targs or any(w in nm for w in want) for nm in names), f"expected {base}<{targs}>, the launch ran {sorted(names)}"
    else:
        assert targs in {template_args(nm, base) for nm in names}, f"expected {base}<{targs}>, the launch ran {sorted(names)}"


def record(what, family, err, a, bound):
    print(SB.profile_line(what, family, S.worst_ratio(err, a), S.worst_of_bound(err, bound)))


_EXACT = {}


def exact_case(c, seed, expanded=False):
    """(x, ty, tx, q, k) of the case's exact construction on the host, computed once."""
    key = (c.name, seed, expanded)
    if key not in _EXACT:
        x, ty, tx = c.exact_inputs(seed)
        if expanded:
            x = x[:1].expand_as(x).contiguous()
        _EXACT[key] = (x, ty, tx) + R.rope_pool_exact(x, ty, tx, c.heads, c.lr)
    return _EXACT[key]


def out_buffers(c, dev, write_q=True):
    """Dense outputs filled with NaN: q head-major, k channels-last (what ops.rope_pool allocates)."""
    (Ho, Wo), (h, w) = c.out, c.lr
    q = torch.full((c.B, c.heads, Ho, Wo, c.Dh), float("nan"), dtype=BF, device=dev) if write_q else None
    k = torch.full((c.B, h, w, c.heads, c.Dh), float("nan"), dtype=BF, device=dev).permute(0, 3, 1, 2, 4)
    return q, k


def launch(a, x):
    from naf_amd import _lib
    _lib.check(R.rope_pool_launch(a, x), "naf_rope_pool_fwd")


# ---- 3.1 exact, per instance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=repr)
def test_every_element_bit_exact(dev, c):
    from naf_amd import ops
    plan, plan_k = c.plan(), c.plan(write_q=False)
    for key, want in c.expect.items():
        assert plan[key] == want, (c, key, plan[key], want)
    assert plan_k["kernel"] == (c.keys_expect or c.expect["kernel"])
    for seed in (1, 2):
        x, ty, tx, q_ref, k_ref = exact_case(c, seed)
        xd, tyd, txd = R.place_x(c, x, dev), ty.to(dev), tx.to(dev)
        assert (xd.data_ptr() % 16 == 0) == (c.offset == 0) and (xd.stride(1) == 1) == c.nhwc
        for write_q, p in ((True, plan), (False, plan_k)):
            q, k = out_buffers(c, dev, write_q)
            a = R.rope_pool_args(xd, q, k, tyd, txd, c.heads)
            assert c.Dh % 32 != 0 or R.args_aligned(a, xd.element_size()) == (c.offset == 0)
            if seed == 1:
                assert_ran(lambda: launch(a, xd), p["kernel"])
            else:
                launch(a, xd)
            torch.cuda.synchronize()
            what = f"case {c} tables {seed} {'q and k' if write_q else 'keys only'} ({p['kernel']}, tab_lds={p['tab_lds']})"
            if write_q:
                msg = R.first_mismatch(q.cpu(), q_ref, what + ": q")
                assert msg is None, msg
            msg = R.first_mismatch(k.cpu(), k_ref, what + ": k")
            assert msg is None, msg
        if c.offset == 0:                                  # the public function, both query layouts and keys only
            for layout in ("head_major", "channels_last"):
                q, k = ops.rope_pool(xd, tyd, txd, c.heads, c.lr, q_layout=layout)
                assert R.first_mismatch(q.cpu(), q_ref, f"ops.rope_pool {layout} case {c}: q") is None
                assert R.first_mismatch(k.cpu(), k_ref, f"ops.rope_pool {layout} case {c}: k") is None
            _, k = ops.rope_pool(xd, tyd, txd, c.heads, c.lr, write_q=False)
            assert R.first_mismatch(k.cpu(), k_ref, f"ops.rope_pool keys only case {c}") is None
        assert torch.equal(xd.float().cpu(), x), "the launch changed its input"


def test_scalar_path_refuses_1024_channels(dev):
    """Cq = 1024 with x offset by 4 elements: the scalar path would need 512 pair-chunks per pixel.  Asked, not launched."""
    from naf_amd import _lib
    c = R.REFUSED
    assert c.plan()["status"] == "unsupported"
    xd = R.place_x(c, torch.zeros(c.shape()), dev)
    q, k = out_buffers(c, dev)
    ty, tx = (t.to(dev) for t in R.integer_tables(*c.out, c.Dh // 4, 3))
    before = k.clone()
    rc = R.rope_pool_launch(R.rope_pool_args(xd, q, k, ty, tx, c.heads), xd)
    torch.cuda.synchronize()
    assert rc == 2, rc                                     # NAF_ERR_UNSUPPORTED
    assert "512" in _lib.last_error() and "256" in _lib.last_error(), _lib.last_error()
    assert L.same_bits(k, before), "a refused call wrote"


# ---- 3.2 layout and guard bands -----------------------------------------------------------------------------------------------------------------
X_FAMILIES = ("channels_last", "pixel_gap", "row_gap", "crop", "head_gap", "batch_inner", "transposed")     # of the guidance as [B, 1, Ho, Wo, Cq]


def layout_plans(c):
    """[(label, {x, q, k: family})]: every operand in one family; each alone in ``crop``; the production mix; x expanded; x planar."""
    x0 = "channels_last" if c.nhwc else "planar"
    fx = lambda f: (f if f in X_FAMILIES else "channels_last") if c.nhwc else "planar"
    plans = [(f"all-{f}", dict(x=fx(f), q=f, k=f)) for f in L.VECTOR_FAMILIES]
    plans += [(f"{o}-crop", {p: ("crop" if p == o and (p != "x" or c.nhwc) else (x0 if p == "x" else "head_major")) for p in ("x", "q", "k")}) for o in ("x", "q", "k")]
    plans.append(("production", dict(x=x0, q="head_major", k="channels_last")))
    plans.append(("x-expanded", dict(x="expanded" if c.nhwc else "planar_expanded", q="head_major", k="head_major")))
    plans.append(("x-planar", dict(x="planar", q="head_major", k="head_major")))
    return plans


def place_operands(c, fam, x, dev, write_q=True):
    """x, q and k in arenas of the families named: (Placed, x as a logical [B, Cq, Ho, Wo] view, q, k)."""
    P = L.Placed()
    (Ho, Wo), (h, w) = c.out, c.lr
    xt = x.to(c.dtype)
    if fam["x"] == "planar":
        xv = P.add("x", L.planar(xt, device=dev))
    elif fam["x"] == "planar_expanded":
        v, arena, mask = L.planar(xt[:1], device=dev)
        xv = P.add("x", (v.expand(c.B, -1, -1, -1), arena, mask))
    else:
        x5 = xt.permute(0, 2, 3, 1).unsqueeze(1)                    # [B, 1, Ho, Wo, Cq]: the channels contiguous in every family
        xv = P.add("x", L.embed(x5, fam["x"], device=dev))[:, 0].permute(0, 3, 1, 2)
    q = P.add("q", L.arena_for((c.B, c.heads, Ho, Wo, c.Dh), BF, fam["q"], dev), output=True) if write_q else None
    k = P.add("k", L.arena_for((c.B, c.heads, h, w, c.Dh), BF, fam["k"], dev), output=True)
    P.snapshot()
    return P, xv, q, k


def check_launch(P, q, k, q_ref, k_ref, what):
    torch.cuda.synchronize()
    if q is not None:
        msg = R.first_mismatch(q.cpu(), q_ref, what + ": q")
        assert msg is None, msg
        assert bool(torch.isfinite(q.float()).all())
    msg = R.first_mismatch(k.cpu(), k_ref, what + ": k")
    assert msg is None, msg
    assert bool(torch.isfinite(k.float()).all())
    assert not P.problems(), f"{what}: {P.problems()}"


@pytest.mark.parametrize("name,write_q", [("A", True), ("E", True), ("F", True), ("H", True), ("K", True), ("M", True), ("A", False), ("F", False), ("M", False)],
                         ids=lambda v: {True: "q", False: "keys"}.get(v, v))
def test_strides_and_guard_bands(dev, name, write_q):
    c = R.CASE[name]
    kernel = c.plan(write_q)["kernel"]
    for label, fam in layout_plans(c):
        x, ty, tx, q_ref, k_ref = exact_case(c, 1, expanded="expanded" in fam["x"])
        tyd, txd = ty.to(dev), tx.to(dev)
        P, xv, q, k = place_operands(c, fam, x, dev, write_q)
        a = R.rope_pool_args(xv, q, k, tyd, txd, c.heads)
        # every family here is vectorisable where the case's head dim is: the instance is the case's, whatever the strides
        assert c.Dh % 32 != 0 or R.args_aligned(a, xv.element_size()), (label, fam)
        now = launch_kernel(c, a, xv, write_q)
        assert now == (c.plan(True)["kernel"] if fam["x"].startswith("planar") else kernel), (label, fam, now)     # the keys kernel reads contiguous channels only
        launch(a, xv)
        check_launch(P, q, k, q_ref, k_ref, f"case {c} {label} {fam}")


def launch_kernel(c, a, xv, write_q):
    """The plan of the args as they are filled (alignment from the pointers and strides, channel stride from x)."""
    return R.launch_plan(c.B, c.Cq, c.heads, *c.out, *c.lr, c.dtype, int(a.x_stride[1]) == 1, R.args_aligned(a, xv.element_size()), write_q)["kernel"]


@pytest.mark.parametrize("name", ["A", "E", "F", "M"])
def test_unaligned_operands_take_the_scalar_instance(dev, name):
    """q with an x stride of C + 4 or 4 elements off, x 4 elements off, a table one float off: Dh is a multiple of 32 and the call still runs
    rope_pool_kernel<__bf16, 1, .> (the profiler), with the same bits and nothing written outside the views."""
    c = R.CASE[name]
    assert c.Dh % 32 == 0 and c.plan()["VEC"] == 8
    x, ty, tx, q_ref, k_ref = exact_case(c, 1)
    scalar = c.plan(aligned=False)["kernel"]
    assert scalar[1].startswith("__bf16,1,")
    tyd = ty.to(dev)
    txo = torch.zeros(tx.numel() + 4, dtype=torch.float32, device=dev)[1:1 + tx.numel()].view(tx.shape)
    txo.copy_(tx)
    assert txo.data_ptr() % 16 == 4
    routes = [("q-odd_stride", dict(x="channels_last", q="odd_stride", k="head_major"), tx.to(dev)),
              ("q-odd_offset", dict(x="channels_last", q="odd_offset", k="head_major"), tx.to(dev)),
              ("x-odd_offset", dict(x="odd_offset", q="head_major", k="head_major"), tx.to(dev)),
              ("x-odd_stride", dict(x="odd_stride", q="head_major", k="head_major"), tx.to(dev)),
              ("table-one-float-off", dict(x="channels_last", q="head_major", k="head_major"), txo)]
    for label, fam, txd in routes:
        P, xv, q, k = place_operands(c, fam, x, dev)
        a = R.rope_pool_args(xv, q, k, tyd, txd, c.heads)
        assert not R.args_aligned(a, 2), label
        assert_ran(lambda: launch(a, xv), scalar)
        check_launch(P, q, k, q_ref, k_ref, f"case {c} {label}")


# ---- 3.3 true tables, scale-aware ---------------------------------------------------------------------------------------------------------------
TABLE_SHAPES = [(37, 50, 16), (5, 7, 3), (1, 1, 24), (16, 16, 16), (33, 9, 8)]      # Ho * np: 592, 15, 24, 256 (one whole workgroup), 264


@pytest.mark.parametrize("Ho,Wo,P", TABLE_SHAPES)
def test_rope_tables(dev, Ho, Wo, P):
    """naf_rope_tables against the fp64 tables: |angle| <= 2 pi after seven fp32 roundings, 2 pi * 7 * 2^-24 = 2.6e-6, plus sinf / cosf (the bound
    argued at tests/test_gpu_stem_backward.py); guard-banded buffers: nothing beyond row Ho / Wo is written."""
    from naf_amd import _lib, ops
    per = O.rope_periods(4 * P, 1, 100.0)
    assert per.numel() == P
    perd = per.to(dev)
    ty, ay, my = L.banded((Ho, 2, P), torch.float32, dev)
    tx, ax, mx = L.banded((Wo, 2, P), torch.float32, dev)
    by, bx = ay.clone(), ax.clone()

    def run():
        with torch.cuda.device(dev):
            _lib.check(_lib.load().naf_rope_tables(ty.data_ptr(), tx.data_ptr(), perd.data_ptr(), P, Ho, Wo, ops._stream(perd)), "naf_rope_tables")
    assert_ran(run, ("rope_tables_kernel", None))
    torch.cuda.synchronize()
    assert L.untouched(ay, by, my) and L.untouched(ax, bx, mx), "wrote beyond the tables"
    t64y, t64x = R.tables64(per, Ho, Wo)
    ey, ex = float((ty.double().cpu() - t64y).abs().max()), float((tx.double().cpu() - t64x).abs().max())
    print(f"rope tables {Ho} x {Wo}, {P} periods: max err {max(ey, ex):.3e} of 3e-6")
    assert ey < 3e-6 and ex < 3e-6
    oy, ox = ops.rope_tables(perd, Ho, Wo)
    assert L.same_bits(oy, ty) and L.same_bits(ox, tx)


@pytest.mark.parametrize("name", ["A", "B", "F", "M", "production"])
def test_true_tables_inside_the_derived_bounds(dev, name):
    from naf_amd import ops
    c = R.PRODUCTION if name == "production" else R.CASE[name]
    ty, tx = ops.rope_tables(O.rope_periods(c.Cq, c.heads, 100.0).to(dev), *c.out)
    tyh, txh = ty.cpu(), tx.cpu()
    failures = []
    for fam in ("unit", "chan_offset", "outlier"):
        x = S.make_values(c.shape(), fam, 77 + c.out[1])
        q_ref, k_ref, qa, ka = R.rope_pool_reference(x, tyh, txh, c.heads, c.lr)
        bq, bk = R.float_bounds(q_ref, k_ref, qa, ka, c.lr)
        xd = R.place_x(c, x, dev)
        for write_q in (True, False):
            q, k = ops.rope_pool(xd, ty, tx, c.heads, c.lr, write_q=write_q)
            what = f"rope_pool {name} {'q+k' if write_q else 'keys'} {c.plan(write_q)['kernel'][0][10:]}"
            pairs = [("k", k, k_ref, ka, bk)] + ([("q", q, q_ref, qa, bq)] if write_q else [])
            for tag, got, ref, a, bound in pairs:
                err = (got.double().cpu() - ref).abs()
                assert bool(torch.isfinite(err).all())
                record(f"{what} {tag}", fam, err, a, bound)
                try:
                    S.check(err, bound, f"{what} {tag} {fam}")
                except AssertionError as e:
                    failures.append(str(e))
    assert not failures, "\n".join(failures)


# ---- 3.4 the key epilogue of the last stem layers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("shape", [(1, 32, 32), (2, 48, 64), (3, 16, 160)])
def test_stem_key_epilogue_under_integer_tables(dev, ks, shape):
    """naf_stem_conv_keys_fwd on both kernels with CHOSEN integer tables (|cos|, |sin| <= 15, different from row to row): the keys must be
    ``rope_pool_reference`` of the layer's own bf16 output inside ``epilogue_key_bound``; a wrong row, column, angle index or pair half is 10 to
    10^4 bounds away (tests/test_rope_pool_cpu.py).  The key slice lives in a guard-banded [B, h, w, 256] buffer: the other branch's channels
    and the band stay as they were."""
    from naf_amd import ops
    B, H, W = shape
    h, w = H // 16, W // 16
    xd, st_in, gw, gb, wp, bias = _layer_inputs(dev, B, H, W, ks, 1200 + 10 * ks)
    base, targs = layer_kernel("1x1" if ks == 1 else "rows", 128, ks, dense=True, keys=True)
    for seed, branch in ((1, 0), (2, 1)):
        ty, tx = (t.to(dev) for t in R.integer_tables(H, W, 16, 50 * seed + H))
        y = torch.full((B, H, W, 128), float("nan"), dtype=BF, device=dev)
        keys, arena, _ = L.banded((B, h, w, 256), BF, dev)
        ksl = keys[..., 128 * branch:128 * branch + 128]
        inside = L.view_mask(arena.numel(), (ksl.data_ptr() - arena.data_ptr()) // 2, (B, h, w, 128), (h * w * 256, w * 256, 256), dev)
        before = arena.clone()
        run = lambda: R.stem_keys_launch(xd, st_in, gw, gb, 1e-5, wp, bias, y, ksl, ty, tx)
        if seed == 1:
            assert_ran(run, (base, targs))
        else:
            run()
        torch.cuda.synchronize()
        assert L.untouched(arena, before, inside), "wrote outside its key slice"
        yh = y.float().cpu().permute(0, 3, 1, 2).contiguous()
        assert bool(torch.isfinite(yh).all())
        _, k_ref, _, ka = R.rope_pool_reference(yh, ty.cpu(), tx.cpu(), 2, (h, w))
        got = ksl.contiguous().double().cpu().view(B, h, w, 2, 64).permute(0, 3, 1, 2, 4)
        err, bound = (got - k_ref).abs(), R.epilogue_key_bound(k_ref, ka)
        record(f"stem keys ks={ks} {shape} tables {seed}", "integer tables", err, ka, bound)
        S.check(err, bound, f"stem keys ks={ks} {shape} tables {seed}")
