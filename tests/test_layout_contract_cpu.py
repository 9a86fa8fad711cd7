"""The layout contract of the attention entries without a device (tests/layout_contract.py has the contract and the technique).

1. The helper checks itself: a view holds the dense tensor's values, the mask counts its elements, strides and alignment are what the
   family claims, the margins hold, everything else of the arena is the sentinel.
2. The contract as a table.  Host pointers that nothing dereferences (the precedent is
   tests/test_head_cpu.py::test_select_refuses_misaligned_and_null): for every case of tests/test_gpu_layout_contract.py and every
   family, what naf_xna_select, naf_xna_bwd_supported, naf_xna_head_select / naf_xna_head_ce_select, naf_xna_cos_select /
   naf_xna_cos_ce_select and naf_xna_mse_supported answer.
   The vectorisable families get the kernel of the dense layout.  ``odd_offset`` / ``odd_stride`` on one operand get, under AUTO, a
   kernel whose eligibility test (restated in layout_contract.*_admits, with the source lines) admits that layout -- the dense layout's
   kernel where it still does -- and -NAF_ERR_UNSUPPORTED where the dense layout's kernel is insisted on and does not.
3. Teeth: three defects emulated in torch on an arena -- a writer that stores all 16 lanes of a partial tile, a reader that takes
   W * x_stride for the row stride, a writer of the cosine head's norm map that takes its strides from `out`'s -- and what ``untouched``
   and the equality checks say about each; on the dense layouts the rest of the suite uses, the last two are invisible.  And the inputs
   of the cosine cases: the fp64 definition on values (keys) read from the wrong image, head, channel, row or column leaves twice the
   bound the canonical launch is held to.
4. ops.xna_forward(out=...) refuses a wrong-shaped buffer before anything else happens.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_reference as CR  # noqa: E402
import input_statistics as S  # noqa: E402
import layout_contract as LC  # noqa: E402
import regress_reference as R  # noqa: E402

INVALID = -1           # -NAF_ERR_INVALID
UNSUPPORTED = -2       # -NAF_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib(built_lib):
    from naf_amd import _lib
    return _lib.load()


# ---- 1. the helper ---------------------------------------------------------------------------------------------------------------
SHAPE = (2, 3, 4, 5, 16)       # B, heads, H, W, D


def _dense(shape, dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.uint8], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("family", LC.FAMILIES)
def test_embed_gives_the_view_the_family_claims(family, dtype):
    B, n, H, W, D = SHAPE
    Cc = n * D
    x = (torch.arange(B * n * H * W * D) % 251).to(torch.uint8).view(SHAPE) if dtype == torch.uint8 else _dense(SHAPE, dtype)
    if family == "expanded":
        x = x[:1].expand(SHAPE).contiguous()
    if family == "expanded_head":
        x = x[:, :1].expand(SHAPE).contiguous()
    view, arena, mask = LC.embed(x, family)
    it = x.element_size()
    assert view.shape == x.shape and view.dtype == x.dtype and LC.same_bits(view, x) and view.stride(4) == 1
    sb, sh, sy, sx = view.stride()[:4]
    unique = x.numel() // (B if family == "expanded" else n if family == "expanded_head" else 1)
    assert int(mask.sum()) == unique and mask.numel() == arena.numel()
    # the strides of the family, written out once more
    want = {"head_major": (n * H * W * D, H * W * D, W * D, D), "channels_last": (H * W * Cc, D, W * Cc, Cc),
            "pixel_gap": (H * W * (Cc + 8), D, W * (Cc + 8), Cc + 8), "row_gap": (H * (W * Cc + 24), D, W * Cc + 24, Cc),
            "crop": ((H + 5) * (W + 7) * (Cc + 24), D, (W + 7) * (Cc + 24), Cc + 24), "head_gap": (H * W * 2 * Cc, 2 * D, W * 2 * Cc, 2 * Cc),
            "batch_inner": (D, H * W * B * D, W * B * D, B * D), "transposed": (n * W * H * D, W * H * D, D, H * D),
            "expanded": (0, H * W * D, W * D, D), "expanded_head": (H * W * D, 0, W * D, D),
            "odd_offset": (n * H * W * D, H * W * D, W * D, D), "odd_stride": (H * W * (Cc + 4), D, W * (Cc + 4), Cc + 4)}[family]
    assert (sb, sh, sy, sx) == want
    if family == "transposed":
        assert sy < sx
    # alignment
    ptr = view.data_ptr()
    if family == "crop":
        assert ptr % 32 == 16
    elif family == "odd_offset":
        assert ptr % 32 == (4 * it) % 32
    else:
        assert ptr % 32 == 0
    if it == 2:
        assert LC.vec_ok(view) == (family not in LC.ROUTING_FAMILIES)
    # the margins, and the sentinel everywhere else
    inside = mask.nonzero().flatten()
    m = LC.margin((sb, sh, sy, sx))
    assert m == 2 * sy + 16 * sx + 16
    assert int(inside.min()) >= m and arena.numel() - 1 - int(inside.max()) >= m
    assert bool((LC.bits(arena)[~mask] == LC.sentinel(dtype)).all())
    if dtype in (torch.bfloat16, torch.float16, torch.float32):
        assert bool(torch.isnan(arena[~mask]).all())
    assert LC.untouched(arena, arena.clone(), mask) and LC.unchanged(arena, arena.clone())


def test_crop_is_a_window_of_a_larger_batch_canvas_and_channel_axis():
    B, n, H, W, D = SHAPE
    x = _dense(SHAPE, torch.bfloat16)
    view, arena, mask = LC.embed(x, "crop")
    _, off, extent = LC.layout(SHAPE, "crop")
    start = int(mask.nonzero().min())
    wide = arena[start - off: start - off + extent].view(B + 1, H + 5, W + 7, n * D + 24)
    win = wide[1:, 2:2 + H, 3:3 + W, 8:8 + n * D].unflatten(3, (n, D)).permute(0, 3, 1, 2, 4)
    assert win.data_ptr() == view.data_ptr() and win.stride() == view.stride() and LC.same_bits(win, x)


def test_banded_and_untouched():
    t, arena, mask = LC.banded((3, 7), torch.float32, inside=0.0)
    assert t.is_contiguous() and float(t.abs().sum()) == 0.0 and int(mask.sum()) == 21 and t.data_ptr() % 64 == 0
    before = arena.clone()
    t += 1.0
    assert LC.untouched(arena, before, mask) and not LC.unchanged(arena, before)
    arena[int(mask.nonzero().max()) + 1] = 0.0          # one element past the end
    assert not LC.untouched(arena, before, mask) and LC.outside_writes(arena, before, mask) == 1
    # bit-level: a NaN with another payload is a change, the same NaN is not
    ws, wa, wm = LC.banded((16,), torch.uint8)
    assert ws.numel() == 16 and bool((wa == LC.SENT8).all())


def test_launch_plans_cover_the_issue_s_sets():
    plans = dict(LC.launch_plans(("q", "k", "v"), ("out",), expandable=("k", "v")))
    assert {f"all-{f}" for f in LC.VECTOR_FAMILIES} <= set(plans) and {"q-crop", "k-crop", "v-crop", "out-crop", "production", "expanded"} <= set(plans)
    assert plans["production"] == {"q": "head_major", "k": "head_major", "v": "channels_last", "out": "channels_last"}
    assert plans["v-crop"] == {"q": "head_major", "k": "head_major", "v": "crop", "out": "head_major"}
    assert plans["expanded"]["k"] == "expanded" and plans["expanded"]["out"] == "head_major"
    assert len(LC.FWD_RUNS) == len({LC.run_id(r) for r in LC.FWD_RUNS}) == 19


# ---- 2. the contract as a table ----------------------------------------------------------------------------------------------------
def _fake(shape, dtype, family):
    """A host tensor in the family's layout: pointer and strides only, never dereferenced by the queries."""
    return LC.arena_for(shape, dtype, family, mask=False)[:2]


def _fwd_operands(run):
    name, out_dtype, variant = run
    _, path, sub, heads, Dq, lr, out_sz, ksz, Cc, _ = LC.fwd_case(name)
    Dv = Cc // heads
    shapes = {"q": (LC.B2, heads, *out_sz, Dq), "k": (LC.B2, heads, *lr, Dq), "v": (LC.B2, heads, *lr, Dv), "out": (LC.B2, heads, *out_sz, Dv)}
    dtypes = {"q": torch.bfloat16, "k": torch.bfloat16, "v": torch.float16 if variant == "half" else torch.bfloat16, "out": out_dtype}
    return path, ksz, shapes, dtypes


@pytest.mark.parametrize("run", LC.FWD_RUNS, ids=LC.run_id)
def test_forward_select_table(lib, run):
    from naf_amd import _lib, ops
    path, ksz, shapes, dtypes = _fwd_operands(run)
    variant = run[2]
    keep = []
    extra = {}
    if variant == "logits":
        extra["logits"] = torch.empty(8)
    if variant == "rope":
        Ho, Wo, Dq = shapes["q"][2], shapes["q"][3], shapes["q"][4]
        extra["rope_tables"] = (torch.zeros(Ho, 2, Dq // 4), torch.zeros(Wo, 2, Dq // 4))

    def select(plan, p):
        t = {}
        for o in shapes:
            t[o], arena = _fake(shapes[o], dtypes[o], plan[o])
            keep.append(arena)
        return t, LC.forward_args(t["q"], t["k"], t["v"], t["out"], ksz, p, **extra)[1]

    dense = {o: LC.CANONICAL for o in shapes}
    assert select(dense, path)[1] == ops._PATH[path], "the case does not reach the kernel it is named after"
    auto_dense = select(dense, "auto")[1]
    assert auto_dense > 0
    for label, plan in LC.launch_plans(("q", "k", "v"), ("out",), expandable=("k", "v")):
        assert select(plan, path)[1] == ops._PATH[path], label
        assert select(plan, "auto")[1] == auto_dense, label
    for fam in LC.ROUTING_FAMILIES:
        for o in shapes:
            plan = dict(dense, **{o: fam})
            t, sel = select(plan, "auto")
            admits = lambda kern: LC.forward_admits(kern, t["q"], t["k"], t["v"], t["out"])
            if variant == "rope":          # rotate-on-load lives in the cell kernel alone: no other kernel to route to
                assert sel == (_lib.XNA_MFMA if admits("mfma") else UNSUPPORTED), (fam, o, sel)
            else:
                assert sel > 0 and admits(ops._PATH_NAME[sel]), (fam, o, sel)
                assert (sel == auto_dense) == admits(ops._PATH_NAME[auto_dense]), (fam, o, sel)
            if variant == "logits" and not admits("mfma"):
                assert sel == _lib.XNA_GENERIC          # the scores come from the cell kernel or the scalar one
            _, forced = select(plan, path)
            assert forced == (ops._PATH[path] if admits(path) else UNSUPPORTED), (fam, o, forced)


@pytest.mark.parametrize("name", LC.BWD_RUNS)
def test_backward_supported_table(lib, name):
    from naf_amd import _lib, ops
    _, path, heads, Dq, lr, out_sz, ksz, Cc, nchunk, _ = LC.bwd_case(name)
    Dv = Cc // heads
    shapes = {"q": (LC.B2, heads, *out_sz, Dq), "k": (LC.B2, heads, *lr, Dq), "v": (LC.B2, heads, *lr, Dv), "dout": (LC.B2, heads, *out_sz, Dv),
              "dq": (LC.B2, heads, *out_sz, Dq)}
    dk = torch.empty(8)
    keep = []
    code = {"mfma": _lib.XNA_MFMA, "rows": _lib.XNA_ROWS, "generic": _lib.XNA_GENERIC}
    kname = {v: k for k, v in code.items()}

    def select(plan, p):
        t = {}
        for o in shapes:
            t[o], arena = _fake(shapes[o], torch.bfloat16, plan[o])
            keep.append(arena)
        return t, LC.backward_args(t["q"], t["k"], t["v"], t["dout"], t["dq"], dk, dk, ksz, p)[1]

    dense = {o: LC.CANONICAL for o in shapes}
    assert select(dense, path)[1] == code[path]
    auto_dense = select(dense, "auto")[1]
    if path != "generic":
        assert auto_dense == code[path], "AUTO does not pick the kernel the case is named after"
    for label, plan in LC.launch_plans(("q", "k", "v", "dout"), ("dq",), expandable=("k", "v", "dout"), head_expandable=("dout",)):
        assert select(plan, path)[1] == code[path] and select(plan, "auto")[1] == auto_dense, label
    for fam in LC.ROUTING_FAMILIES:
        for o in shapes:
            plan = dict(dense, **{o: fam})
            t, sel = select(plan, "auto")
            admits = lambda kern: LC.backward_admits(kern, t["q"], t["k"], t["v"], t["dout"], t["dq"])
            assert sel > 0 and admits(kname[sel]), (fam, o, sel)
            assert (sel == auto_dense) == admits(kname[auto_dense]), (fam, o, sel)
            _, forced = select(plan, path)
            assert forced == (code[path] if admits(path) else UNSUPPORTED), (fam, o, forced)


def test_head_geometries_are_the_suite_s_and_a_partial_tile_one():
    assert LC.HEAD_GEOMS["tiles16"] == (LC.B2,) + tuple(S.HEAD_GEOM[1:]) and LC.HEAD_GEOMS["patch14"][4] == 14


def _head_shapes(gname):
    B, h, w, dy, dx, ksz, heads = LC.HEAD_GEOMS[gname]
    N = LC.HEAD_N
    npad = (N + 15) // 16 * 16
    Ho, Wo = h * dy, w * dx
    return ksz, N, {"q": (B, heads, Ho, Wo, 64), "k": (B, heads, h, w, 64), "pv": (B, heads, h, w, npad), "out": (B, 1, Ho, Wo, N),
                    "loss": (B, 1, Ho, Wo, 1), "labels": (B, 1, Ho, Wo, 1), "dlogits": (B, 1, Ho, Wo, 32)}


HEAD_DTYPES = {"q": torch.bfloat16, "k": torch.bfloat16, "pv": torch.bfloat16, "out": torch.float32, "loss": torch.float32, "labels": torch.uint8,
               "dlogits": torch.bfloat16}


@pytest.mark.parametrize("gname", list(LC.HEAD_GEOMS))
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_head_select_table(lib, out_dtype, gname):
    """The head's `out` (and the loss map and labels of the classification entry) are stored element by element: any alignment, any
    strides.  q / k_lr / pv_lr and dlogits that are not vectorisable are refused under AUTO and FUSED alike -- the caller composes."""
    from naf_amd import _lib
    ksz, N, shapes = _head_shapes(gname)
    keep = []
    bias = torch.zeros(N)
    target = torch.zeros(shapes["loss"][0], shapes["loss"][2], shapes["loss"][3], dtype=torch.int64)

    def select(plan, p, ce):
        t = {}
        for o in shapes:
            t[o], arena = _fake(shapes[o], out_dtype if o == "out" and not ce else HEAD_DTYPES[o], plan[o])
            keep.append(arena)
        if ce:
            return t, LC.head_ce_args(t["q"], t["k"], t["pv"], bias, LC.hw3(t["out"]), N, ksz, target, LC.hw2(t["loss"]), LC.hw2(t["labels"]),
                                      LC.hw3(t["dlogits"]), 255, p)[1]
        return t, LC.head_args(t["q"], t["k"], t["pv"], bias, LC.hw3(t["out"]), N, ksz, p)[1]

    dense = {o: LC.CANONICAL for o in shapes}
    for ce in (False, True):
        if ce and out_dtype != torch.float32:
            continue
        outs = ("out", "loss", "labels", "dlogits") if ce else ("out",)
        for p in ("auto", "fused"):
            assert select(dense, p, ce)[1] == _lib.XNA_HEAD_FUSED
            for label, plan in LC.launch_plans(("q", "k", "pv"), outs, expandable=("k", "pv")):
                assert select(dict(dense, **plan), p, ce)[1] == _lib.XNA_HEAD_FUSED, label
            for fam in LC.ROUTING_FAMILIES:
                for o in ("q", "k", "pv") + outs:
                    t, sel = select(dict(dense, **{o: fam}), p, ce)
                    ok = LC.head_admits(t["q"], t["k"], t["pv"], LC.hw3(t["dlogits"]) if ce else None)
                    assert ok == (o in ("out", "loss", "labels"))
                    assert sel == (_lib.XNA_HEAD_FUSED if ok else UNSUPPORTED), (fam, o, sel)


@pytest.mark.parametrize("gname", list(LC.COS_GEOMS))
def test_cos_select_table(lib, gname):
    """naf_xna_cos_select / naf_xna_cos_ce_select against layout_contract.cos_admits: q / k_lr / pv_lr / v_lr (and dlogits) that are not
    vectorisable are -NAF_ERR_UNSUPPORTED under AUTO and FUSED alike; out, norms, target, loss, labels and dscale take any strides and any
    alignment of their element size; an `out` row shorter than N and a dlogits row shorter than dlogits_channels are -NAF_ERR_INVALID."""
    from naf_amd import _lib
    ksz, N, shapes = LC.cos_shapes(gname)
    B, heads, Dv, lr, cell, _, _ = LC.COS_GEOMS[gname]
    assert Dv != shapes["pv"][4], "pv_lr and v_lr would have the same strides in every family"
    keep = []

    def select(plan, p, ce):
        t = {}
        for o in shapes:
            t[o], arena = _fake(shapes[o], LC.COS_DTYPES[o], plan[o])
            keep.append(arena)
        if ce:
            return t, LC.cos_ce_args(t["q"], t["k"], t["pv"], t["v"], LC.hw3(t["out"]), LC.hw2(t["norms"]), N, ksz, LC.hw2(t["target"]), LC.hw2(t["loss"]),
                                     LC.hw2(t["labels"]), LC.hw3(t["dlogits"]), LC.hw2(t["dscale"]), path=p)[1]
        return t, LC.cos_args(t["q"], t["k"], t["pv"], t["v"], LC.hw3(t["out"]), LC.hw2(t["norms"]), N, ksz, path=p)[1]

    dense = {o: LC.CANONICAL for o in shapes}
    for ce in (False, True):
        ins, outs = (LC.COS_CE_INPUTS, LC.COS_CE_OUTPUTS) if ce else (LC.COS_INPUTS, LC.COS_OUTPUTS)
        vector = LC.COS_INPUTS + (("dlogits",) if ce else ())          # the operands read / written in 16-byte chunks
        for p in ("auto", "fused"):
            assert select(dense, p, ce)[1] == _lib.XNA_HEAD_FUSED
            for label, plan in LC.launch_plans(ins, outs, expandable=("k", "pv", "v") + (("target",) if ce else ()), head_expandable=("k", "pv", "v")):
                assert select(dict(dense, **plan), p, ce)[1] == _lib.XNA_HEAD_FUSED, label
            for fam in LC.FAMILIES:
                for o in vector:
                    t, sel = select(dict(dense, **{o: fam}), p, ce)
                    ok = LC.cos_admits(t["q"], t["k"], t["pv"], t["v"], LC.hw3(t["dlogits"]) if ce else None)
                    assert ok == (fam not in LC.ROUTING_FAMILIES), (fam, o)
                    assert sel == (_lib.XNA_HEAD_FUSED if ok else UNSUPPORTED), (fam, o, p, sel)
            for fam in LC.ROUTING_FAMILIES:                            # element by element: still the fused kernel's
                for o in tuple(ins[4:]) + tuple(x for x in outs if x != "dlogits"):
                    assert select(dict(dense, **{o: fam}), p, ce)[1] == _lib.XNA_HEAD_FUSED, (fam, o, p)
            # rows too short for what is stored in them: arguments no kernel could serve
            t, _ = select(dense, p, ce)
            out, g = LC.hw3(t["out"]), LC.hw3(t["dlogits"])
            short = out.as_strided(out.shape, (out.stride(0), out.stride(1), N - 1, 1), out.storage_offset())
            gshort = g.as_strided(g.shape, (g.stride(0), g.stride(1), g.shape[3] - 8, 1), g.storage_offset())
            if ce:
                args = (LC.hw2(t["target"]), LC.hw2(t["loss"]), LC.hw2(t["labels"]))
                assert LC.cos_ce_args(t["q"], t["k"], t["pv"], t["v"], short, None, N, ksz, *args, g, LC.hw2(t["dscale"]), path=p)[1] == INVALID
                assert LC.cos_ce_args(t["q"], t["k"], t["pv"], t["v"], out, None, N, ksz, *args, gshort, LC.hw2(t["dscale"]), path=p)[1] == INVALID
            else:
                assert LC.cos_args(t["q"], t["k"], t["pv"], t["v"], short, None, N, ksz, path=p)[1] == INVALID


@functools.lru_cache(maxsize=None)
def _cos_reference(gname):
    """Inputs of a cosine geometry, their fp64 reference and its bound: once, shared, never modified."""
    B, heads, Dv, lr, cell, ks, N = LC.COS_GEOMS[gname]
    q, k, v, E = LC.cos_inputs(gname)
    r = CR.reference(q, k, v, E, ks, heads)
    return (q, k, v, E), r, CR.bound(r)


@pytest.mark.parametrize("gname", list(LC.COS_GEOMS))
def test_cos_inputs_show_a_misplaced_read(gname):
    """Teeth of the inputs test_gpu_layout_contract.py runs the cosine entries on: a kernel that read v_lr (or k_lr) from another image,
    head, channel group, row or column would compute the definition on other inputs.  The fp64 reference of each such misread leaves
    TWICE the derived bound of the true reference at every pixel (for at least one embedding) and at no less than 0.9 of all elements,
    so no such misread can hide inside the bound the canonical launch is held to.  The per-channel offsets of the values do that."""
    B, heads, Dv, (h, w), cell, ks, N = LC.COS_GEOMS[gname]
    (q, k, v, E), r, bnd = _cos_reference(gname)
    v5 = v.view(B, heads, Dv, h, w)
    misreads = {"v of the other image": (k, v.flip(0)), "v of the next head": (k, v5.roll(-1, 1).reshape(v.shape)),
                "v shifted by 8 channels inside a head": (k, v5.roll(-8, 2).reshape(v.shape)), "v shifted by one low-res row": (k, v.roll(-1, 2)),
                "v shifted by one low-res column": (k, v.roll(-1, 3)), "k of the other image": (k.flip(0), v)}
    assert float(r["norms"].min()) > 1.0
    for what, (km, vm) in misreads.items():
        off = (CR.reference(q, km, vm, E, ks, heads)["cos"] - r["cos"]).abs() > 2.0 * bnd
        px, el = float(off.any(dim=1).double().mean()), float(off.double().mean())
        print(f"{gname}: {what}: leaves twice the bound at {px:.3f} of the pixels, {el:.3f} of the elements")
        assert px == 1.0 and el >= 0.9, (gname, what, px, el)


def test_mse_supported_table(lib):
    B, heads, Dv, lr, out_sz, ks, kind = R.CASES[LC.MSE_CASE][:7]
    assert B == LC.B2
    shapes = {"q": (B, heads, *out_sz, R.DQ), "k": (B, heads, *lr, R.DQ), "v": (B, heads, *lr, Dv), "out": (B, heads, *out_sz, Dv)}
    target = torch.zeros(B, heads * Dv, *out_sz)
    keep = []

    def supported(plan):
        t = {}
        for o in shapes:
            t[o], arena = _fake(shapes[o], torch.bfloat16, plan[o])
            keep.append(arena)
        return t, LC.mse_args(t["q"], t["k"], t["v"], target, t["out"], ks)[1]

    dense = {o: LC.CANONICAL for o in shapes}
    assert supported(dense)[1] == 1
    for label, plan in LC.launch_plans(("q", "k", "v"), ("out",), expandable=("k", "v")):
        assert supported(plan)[1] == 1, label
    for fam in LC.ROUTING_FAMILIES:
        for o in shapes:
            t, ok = supported(dict(dense, **{o: fam}))
            assert ok == (1 if LC.forward_admits("union", t["q"], t["k"], t["v"], t["out"]) else UNSUPPORTED), (fam, o, ok)


# ---- 3. teeth --------------------------------------------------------------------------------------------------------------------
def _tile_writer(view, arena, mask, values, lanes):
    """A kernel's row-tile store emulated on the arena: for every (b, head, y) one tile of 16 lanes, lane l -> pixel x = l, of which the
    first ``lanes`` are stored (a correct kernel: W of them).  A masked lane carries the clamped pixel's values, as the kernels' do."""
    B, n, H, W, D = view.shape
    sb, sh, sy, sx = view.stride()[:4]
    start = int(mask.nonzero().min())
    for b in range(B):
        for g in range(n):
            for y in range(H):
                for lane in range(lanes):
                    at = start + b * sb + g * sh + y * sy + lane * sx
                    arena[at:at + D] = values[b, g, y, min(lane, W - 1)]


@pytest.mark.parametrize("family", ["head_major", "row_gap", "crop", "transposed"])
def test_a_writer_that_ignores_the_partial_tile_mask_is_reported(family):
    shape = (2, 2, 3, 14, 8)                     # 14 of a tile's 16 lanes hold a pixel
    x = _dense(shape, torch.bfloat16)
    view, arena, mask = LC.arena_for(shape, torch.bfloat16, family)
    before = arena.clone()
    _tile_writer(view, arena, mask, x, lanes=14)
    assert LC.same_bits(view, x) and LC.untouched(arena, before, mask)
    view2, arena2, mask2 = LC.arena_for(shape, torch.bfloat16, family)
    _tile_writer(view2, arena2, mask2, x, lanes=16)
    # the two extra lanes land in the next row (overwritten by its own store later, except after the last row), in a gap or in the margin:
    # always inside the arena, and never unseen
    assert not LC.untouched(arena2, before, mask2)
    assert LC.outside_writes(arena2, before, mask2) >= 2 * shape[4]
    if family in ("row_gap", "crop"):            # every row's overshoot lands in a gap of its own, not only the last row's
        assert LC.outside_writes(arena2, before, mask2) > 2 * shape[4] * shape[0] * shape[1]


@pytest.mark.parametrize("family", LC.VECTOR_FAMILIES)
def test_a_reader_that_derives_the_row_stride_is_reported(family):
    """y stride taken as W * x_stride.  Invisible on the dense layouts (and on every layout whose rows ARE W pixels apart, which is why the
    suite never saw it); on row_gap and crop the reader lands in the gaps and returns the sentinel, on transposed it returns other pixels."""
    shape = (2, 2, 4, 5, 8)
    x = _dense(shape, torch.bfloat16)
    view, arena, mask = LC.embed(x, family)
    sb, sh, sy, sx = view.stride()[:4]
    got = arena.as_strided(shape, (sb, sh, shape[3] * sx, sx, 1), view.storage_offset())
    visible = family in ("row_gap", "crop", "transposed")
    assert (shape[3] * sx != sy) == visible
    assert LC.same_bits(got, x) == (not visible)
    if family in ("row_gap", "crop"):
        assert not bool(torch.isfinite(got.float()).all())


def _norms_writer(view, arena, values, strides):
    """The cosine kernel's store of the norm map emulated on the arena: pixel (b, y, x) of the [B, 1, H, W, 1] view goes to
    start + b * s_b + y * s_y + x * s_x for ``strides`` = {b, y, x} (a correct kernel: the norm map's own)."""
    B, _, H, W, _ = view.shape
    sb, sy, sx = strides
    start = view.storage_offset()
    for b in range(B):
        for y in range(H):
            for x in range(W):
                arena[start + b * sb + y * sy + x * sx] = values[b, y, x]


@pytest.mark.parametrize("family", LC.VECTOR_FAMILIES)
def test_a_norms_writer_that_takes_its_strides_from_out_is_reported(family):
    """norms [B, Ho, Wo] addressed by `out`'s {b, y, x} strides (out is [B, Ho, Wo, N]; in pixels, i.e. divided by N, which is what the
    norm map's strides ARE whenever both are dense, so no test on dense buffers sees it).  Where the two operands' gaps differ the
    writer leaves the view: ``untouched`` says so, and the view keeps sentinels where nothing was stored."""
    B, H, W, N = 2, 3, 14, 21
    x = _dense((B, H, W), torch.float32)
    out = LC.arena_for((B, 1, H, W, N), torch.float32, family, mask=False)[0]
    os_ = tuple(int(s) // N for s in LC.hw3(out).stride()[:3])
    view, arena, mask = LC.arena_for((B, 1, H, W, 1), torch.float32, family)
    own = tuple(int(s) for s in LC.hw2(view).stride())
    before = arena.clone()
    _norms_writer(view, arena, x, own)
    assert LC.same_bits(LC.hw2(view), x) and LC.untouched(arena, before, mask)
    view2, arena2, mask2 = LC.arena_for((B, 1, H, W, 1), torch.float32, family)
    _norms_writer(view2, arena2, x, os_)
    visible = family in ("pixel_gap", "row_gap", "crop")
    assert (os_ != own) == visible
    assert LC.untouched(arena2, before, mask2) == (not visible)
    assert LC.same_bits(LC.hw2(view2), x) == (not visible)
    if visible:
        assert LC.outside_writes(arena2, before, mask2) >= H and not bool(torch.isfinite(LC.hw2(view2)).all())


# ---- 4. ops.xna_forward(out=...) ---------------------------------------------------------------------------------------------------
def test_xna_forward_refuses_a_wrong_out_before_anything_else():
    from naf_amd import ops
    q = torch.zeros(2, 2, 8, 8, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 4, 4, 64, dtype=torch.bfloat16)
    v = torch.zeros(2, 2, 4, 4, 16, dtype=torch.bfloat16)
    good = torch.zeros(2, 8, 8, 2, 16, dtype=torch.bfloat16).permute(0, 3, 1, 2, 4)
    for bad in (torch.zeros(2, 2, 8, 8, 32, dtype=torch.bfloat16),          # Dv of another call
                torch.zeros(1, 2, 8, 8, 16, dtype=torch.bfloat16),          # one image short
                torch.zeros(2, 2, 4, 4, 16, dtype=torch.bfloat16),          # the low-res grid
                torch.zeros(2, 8, 8, 2, 16, dtype=torch.bfloat16),          # channels-last memory passed without the permute
                torch.zeros(2, 2, 8, 16, 8, dtype=torch.bfloat16).transpose(3, 4),      # Dv not contiguous
                torch.zeros(2 * 2 * 8 * 8 * 16, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="out must be a"):
            ops.xna_forward(q, k, v, 3, out=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # a well-formed out gets as far as the device check
        ops.xna_forward(q, k, v, 3, out=good)
