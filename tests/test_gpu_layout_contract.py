"""GPU tests (-m gpu) of the layout contract of the attention entries: naf_xna_fwd, naf_xna_head_fwd, naf_xna_head_ce_fwd, naf_xna_cos_fwd,
naf_xna_cos_ce_fwd, naf_xna_mse_fwd and naf_xna_bwd take every operand as a pointer plus four element strides; the kernels must honour
each stride of each operand on its own, write nothing but their outputs and let nothing that lies next to an input reach a result.
tests/layout_contract.py describes the families, the arenas and the sentinels; tests/test_layout_contract_cpu.py holds the host side
(what the eligibility checks answer for every case and family here) and shows that the technique reports three planted defects.

Every case runs at B = 2 (no per-element bound test of the suite has a batch stride that is multiplied by anything but 0) on the
geometries tests/input_statistics.py uses to reach each kernel, the kernel that runs is asserted -- naf_xna_select /
naf_xna_bwd_supported / naf_xna_head_select on the very arguments of every launch, cell versus sliding from the profiler's kernel names
as tests/test_gpu_input_statistics.py does -- and only layouts the host checks accept are launched.  The head runs on
input_statistics.HEAD_GEOM (whole 16-pixel row tiles) and on 14-pixel cells, where its epilogues mask two lanes of every tile.

The cosine head (naf_xna_cos_fwd, naf_xna_cos_ce_fwd) runs on layout_contract.COS_GEOMS: whole 16-pixel row tiles, 14-pixel cells and
151 embeddings (ten channel tiles), with one, one and a half and two 64-channel value chunks per head and Dv != Npad everywhere, so
that pv_lr's strides and v_lr's differ in every family; the value channels carry offsets of their own
(test_layout_contract_cpu.py::test_cos_inputs_show_a_misplaced_read: a head, channel, row, column or image read from the wrong place
leaves twice the bound).  q, k_lr, pv_lr, v_lr and the int64 target are input arenas; the cosines, the norm map, the loss map, the
labels, dlogits and dscale are output arenas, each with strides of its own.  The canonical launch is held to the derived bounds of
tests/cosine_reference.py / cosine_objective_reference.py (the objective's cosines and norms: bit for bit naf_xna_cos_fwd's), every
other launch to the canonical bits -- the kernel has no atomics.  Beyond the launch set below: head stride 0 on k_lr, pv_lr and v_lr,
batch stride 0 on the target, rotate-on-load on the 14-pixel cells (its canonical launch is bit for bit the launch on materialised
queries), outputs handed over as NULL (the others keep their bits, the NULL ones' arenas are not written), and the logit scale as a
device value.  The header's routing rules for the two entries: the element-wise operands (out, norms, loss, labels, dscale, target) in
``odd_offset`` / ``odd_stride`` still run the fused kernel, bit-equal; q, k_lr, pv_lr, v_lr or dlogits there are refused with
-NAF_ERR_UNSUPPORTED under AUTO and FUSED alike, and ops.xna_cos_forward / xna_cos_objective (path="auto") then return the
composition inside cosine_reference.composed_bound.

Launch set per case (layout_contract.launch_plans): (a) every operand in one family, for each of the eight vectorisable families; (b)
each operand in turn in ``crop`` and the rest head-major; (c) q, k head-major and everything else channels-last, what the model hands
over; (d) ``expanded`` (batch stride 0) on k, v / pv and dout, and dout with head stride 0 -- on inputs whose images (heads) are equal,
against a canonical launch of their own.

Per launch:
  1. the output view is bit-equal to the same kernel's output on the canonical dense head-major layout (forward, scores, head logits,
     labels, loss map, dlogits, dq, the MSE's dout): plain stores, and two canonical launches are compared first.  No layout-dependent
     arithmetic was found in these kernels: the one documented branch of that kind, `tvec` of xna_union_mse.hip:108, depends on the
     TARGET's layout, which is the same in every launch here;
  2. dk, dv (fp32 atomics) and the MSE loss: five canonical launches give d = the largest pairwise difference; a strided launch differs
     from a canonical one by at most 2 d, elementwise, and is bit-equal where d == 0;
  3. the canonical result lies inside the per-element fp64 bounds of input_statistics.forward_bound / backward_bounds / head_bound,
     half_reference.half_bound and regress_reference (the oracle is evaluated once per case);
  4. every output arena is bit-unchanged outside its view -- the dense-by-contract dk_lr, dv_lr, scores, loss and the row-streaming
     backward's workspace of exactly naf_xna_bwd_workspace_bytes sit between guard bands;
  5. every input arena is bit-unchanged;
  6. the outputs are finite: the gaps and margins hold NaN, and so does every output element before the launch.

Recorded per case: the kernel and the spread d of (2); printed, and appended to the file NAF_LAYOUT_PROFILE names
(profiles/layout_contract.txt).
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_objective_reference as CQ  # noqa: E402
import cosine_reference as CR  # noqa: E402
import half_reference as HR  # noqa: E402
import input_statistics as S  # noqa: E402
import layout_contract as LC  # noqa: E402
import regress_reference as R  # noqa: E402
from test_gpu_head_objective import make_target, valid_of  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def record(line):
    print(line)
    dest = os.environ.get("NAF_LAYOUT_PROFILE")
    if dest:
        with open(dest, "a") as f:
            f.write(line + "\n")


def nchw(t5):
    B, n, H, W, D = t5.shape
    return t5.permute(0, 1, 4, 2, 3).reshape(B, n * D, H, W).double().cpu()


def kernels_run(fn):
    """Names of the device kernels ``fn`` launches, from the profiler's device activity."""
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}


def equal_images(t):
    return t[:1].expand_as(t).contiguous()


def equal_heads(t):
    return t[:, :1].expand_as(t).contiguous()


def spread(results):
    """Largest pairwise difference between fp32 results of identical launches."""
    d = 0.0
    for i in range(len(results)):
        for j in range(i + 1, len(results)):
            d = max(d, float((results[i] - results[j]).abs().max()))
    return d


def within_spread(got, canon, d, what, failures):
    """Rule (2) of the module docstring."""
    if d == 0.0:
        if not LC.same_bits(got, canon):
            failures.append(f"{what}: not bit-equal to the canonical launch (identical canonical launches are)")
    else:
        e = float((got - canon).abs().max())
        if not e <= 2.0 * d:
            failures.append(f"{what}: differs from the canonical launch by {e:.3e}, identical launches by at most {d:.3e}")


def finite(t):
    return bool(torch.isfinite(t.float()).all())


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def forward_data(run, dev):
    """Dense device operands of a run and what the oracle needs: dict(q, k, v, [tables, q_mat], host = (q, k, v) fp32 NCHW)."""
    from naf_amd import ops
    name, out_dtype, variant = run
    case = LC.fwd_case(name)
    _, path, sub, heads, Dq, lr, out_sz, ksz, Cc, _ = case
    half = variant == "half"
    q, k, v = LC.forward_inputs(case, half)
    d = {"q": LC.to5(q, heads).to(dev), "k": LC.to5(k, heads).to(dev), "v": LC.to5(v, heads, torch.float16 if half else BF16).to(dev), "tables": None}
    if variant == "rope":
        # the un-rotated guidance is q; keys and the materialised queries (for the reference) come from naf_rope_pool_fwd
        x = S.bf16r(O.hash_normal((LC.B2, heads * Dq, *out_sz), 310) * 4.0)
        xd = x.to(dev).to(BF16).contiguous(memory_format=torch.channels_last)
        ty, tx = ops.rope_tables(O.rope_periods(heads * Dq, heads, 100.0).to(dev), *out_sz)
        q_mat, k5 = ops.rope_pool(xd, ty, tx, heads, lr)
        d["q"] = xd.permute(0, 2, 3, 1).unflatten(3, (heads, Dq)).permute(0, 3, 1, 2, 4).contiguous()
        d["k"], d["q_mat"], d["tables"] = k5.contiguous(), q_mat, (ty, tx)
        q, k = nchw(q_mat).float(), nchw(k5).float()
    d["host"] = (q, k, v)
    return d


def forward_once(run, d, plan, dev, path):
    """One launch with the operands in the families of ``plan``: (out as a dense tensor, scores or None, problems)."""
    from naf_amd import ops
    name, out_dtype, variant = run
    ksz = LC.fwd_case(name)[7]
    P = LC.Placed()
    q = P.add("q", LC.embed(d["q"], plan["q"]))
    k = P.add("k", LC.embed(d["k"], plan["k"]))
    v = P.add("v", LC.embed(d["v"], plan["v"]))
    out = P.add("out", LC.arena_for((*q.shape[:4], v.shape[4]), out_dtype, plan["out"], dev), output=True)
    logits = None
    if variant == "logits":
        logits = P.add("logits", LC.banded((*q.shape[:4], ksz * ksz), F32, dev), output=True)
    P.snapshot()
    a, sel = LC.forward_args(q, k, v, out, ksz, path, logits, d["tables"])
    assert sel == ops._PATH[path], f"{plan}: naf_xna_select gives {sel}, the case is {path}"
    keep = LC.forward_launch(a, sel, q)
    torch.cuda.synchronize()
    del keep
    return out.contiguous(), (None if logits is None else logits.clone()), P.problems()


def compare_forward(label, got, canon, failures):
    out, lg, problems = got
    failures += [f"{label}: {p}" for p in problems]
    if not LC.same_bits(out, canon[0]):
        failures.append(f"{label}: out differs from the canonical launch in {int((LC.bits(out) != LC.bits(canon[0])).sum())} elements")
    if lg is not None and not LC.same_bits(lg, canon[1]):
        failures.append(f"{label}: the scores differ from the canonical launch")
    if not finite(out) or (lg is not None and not finite(lg)):
        failures.append(f"{label}: non-finite output")


def scores_reference(q, k, ksz, heads):
    """fp64 scaled scores [B, heads, Ho, Wo, kk] and sum_d |q_d||k_d| * scale, for the bound of an fp32 dot product."""
    iy, ix = S._tables(q, k, ksz)
    iyt, ixt = torch.from_numpy(iy.copy()), torch.from_numpy(ix.copy())
    qh, kh = S._heads(q, heads), S._heads(k, heads)
    kg = S._gather(kh, iyt, ixt)
    scale = qh.shape[-1] ** -0.5
    return torch.einsum("bnrwd,bnrwkd->bnrwk", qh, kg) * scale, torch.einsum("bnrwd,bnrwkd->bnrwk", qh.abs(), kg.abs()) * scale


@pytest.mark.parametrize("run", LC.FWD_RUNS, ids=LC.run_id)
def test_forward_layouts(dev, run):
    name, out_dtype, variant = run
    case = LC.fwd_case(name)
    _, path, sub, heads, Dq, lr, out_sz, ksz, Cc, _ = case
    d = forward_data(run, dev)
    dense = {o: LC.CANONICAL for o in ("q", "k", "v", "out")}
    canon = forward_once(run, d, dense, dev, path)
    again = forward_once(run, d, dense, dev, path)
    assert LC.same_bits(canon[0], again[0]) and (canon[1] is None or LC.same_bits(canon[1], again[1])), "two canonical launches differ"
    assert not canon[2] and finite(canon[0]), canon[2]
    ran = path
    if sub is not None:        # the two kernels behind path="mfma": the one that RAN must be the one the case is named after
        names = kernels_run(lambda: forward_once(run, d, dense, dev, path))
        kinds = {"sliding" if "xna_slide_kernel" in n else "cell" for n in names if "xna_slide_kernel" in n or "xna_mfma_kernel" in n}
        # half output stores 16 bits like bf16: where the plan may stage them (7 x 7 / 9 x 9) the cell kernel serves a "sliding" geometry,
        # as tests/test_gpu_half_features.py notes; everywhere else the answer is known in advance
        want = S.sliding_runs(ksz, lr, out_sz, BF16 if variant == "half" else out_dtype, logits=variant == "logits")
        assert len(kinds) == 1 and (want is None or kinds == {"sliding" if want else "cell"}), f"{LC.run_id(run)}: kernels {sorted(names)}"
        assert kinds == {sub} or (variant == "half" and want is None), f"{LC.run_id(run)}: kernels {sorted(names)}"
        ran = next(iter(kinds))
    record(f"forward  {LC.run_id(run):<34s} kernel {ran}")
    # (3) the canonical result against the oracle, every element
    q, k, v = d["host"]
    ref, a = S.attention_reference(q, k, v, ksz, heads)
    got = nchw(canon[0])
    if variant == "half":
        bound = HR.half_bound(case, q, k, v, ref, a)
    elif variant == "rope":
        # rotating on load is bit-equal to the materialised queries of naf_rope_pool_fwd, which the reference was fed
        mat = forward_once((name, out_dtype, None), dict(d, q=d["q_mat"].contiguous(), tables=None), dense, dev, path)
        assert LC.same_bits(canon[0], mat[0]), "rotate-on-load differs from materialised queries"
        bound = S.bf16_bound(1, a, ref.abs() if out_dtype == BF16 else None)
    else:
        bound = S.forward_bound(case, q, k, ref, a, out_dtype)[0]
    S.check((got - ref).abs(), bound, f"forward {LC.run_id(run)} canonical, B = {LC.B2}")
    if variant == "logits":
        sref, sabs = scores_reference(q, k, ksz, heads)
        S.check((canon[1].double().cpu() - sref).abs(), (Dq + 3) * S.F32 * sabs, "scores")
    # (a), (b), (c)
    failures = []
    for label, plan in LC.launch_plans(("q", "k", "v"), ("out",)):
        compare_forward(label, forward_once(run, d, plan, dev, path), canon, failures)
    # (d) batch stride 0 on k and v
    de = dict(d, k=equal_images(d["k"]), v=equal_images(d["v"]))
    canon_e = forward_once(run, de, dense, dev, path)
    assert not canon_e[2] and finite(canon_e[0])
    compare_forward("expanded", forward_once(run, de, dict(dense, k="expanded", v="expanded"), dev, path), canon_e, failures)
    assert not failures, "\n".join(failures)


# ---- backward --------------------------------------------------------------------------------------------------------------------
def backward_once(case, d, plan, dev, path):
    """(dq dense, dk, dv, problems, selected kernel, naf_xna_bwd_args)."""
    from naf_amd import _lib
    _, _, heads, Dq, lr, out_sz, ksz, Cc, _, _ = case
    P = LC.Placed()
    t = {o: P.add(o, LC.embed(d[o], plan[o])) for o in ("q", "k", "v", "dout")}
    dq = P.add("dq", LC.arena_for(d["q"].shape, BF16, plan["dq"], dev), output=True)
    dk = P.add("dk", LC.banded((LC.B2, *lr, heads, Dq), F32, dev, inside=0.0), output=True)
    dv = P.add("dv", LC.banded((LC.B2, *lr, heads, Cc // heads), F32, dev, inside=0.0), output=True)
    a, sel = LC.backward_args(t["q"], t["k"], t["v"], t["dout"], dq, dk, dv, ksz, path)
    assert sel > 0, f"{plan}: naf_xna_bwd_supported gives {sel}"
    ws = None
    if sel == _lib.XNA_ROWS:
        ws = P.add("workspace", LC.banded((LC.backward_workspace_bytes(a),), torch.uint8, dev), output=True)
    P.snapshot()
    keep = LC.backward_launch(a, sel, t["q"], ws)
    torch.cuda.synchronize()
    del keep
    return dq.contiguous(), dk.clone(), dv.clone(), P.problems(), sel, a


def canonical_backward(case, d, dev, path, code):
    """Five canonical launches: (the first, spread of dk, spread of dv)."""
    dense = {o: LC.CANONICAL for o in ("q", "k", "v", "dout", "dq")}
    runs = [backward_once(case, d, dense, dev, path) for _ in range(5)]
    for r in runs:
        assert r[4] == code, f"naf_xna_bwd_supported gives {r[4]}, the case is {path}"
        assert not r[3], r[3]
        assert LC.same_bits(r[0], runs[0][0]), "dq of two canonical launches differs"
        assert finite(r[0]) and finite(r[1]) and finite(r[2])
    return runs[0], spread([r[1] for r in runs]), spread([r[2] for r in runs])


def compare_backward(label, got, canon, ddk, ddv, code, failures):
    dq, dk, dv, problems, sel, _ = got
    failures += [f"{label}: {p}" for p in problems]
    if sel != code:
        failures.append(f"{label}: kernel {sel} instead of {code}")
    if not LC.same_bits(dq, canon[0]):
        failures.append(f"{label}: dq differs from the canonical launch in {int((LC.bits(dq) != LC.bits(canon[0])).sum())} elements")
    within_spread(dk, canon[1], ddk, f"{label}: dk", failures)
    within_spread(dv, canon[2], ddv, f"{label}: dv", failures)
    if not (finite(dq) and finite(dk) and finite(dv)):
        failures.append(f"{label}: non-finite gradient")


@pytest.mark.parametrize("name", LC.BWD_RUNS)
def test_backward_layouts(dev, name):
    from naf_amd import _lib
    case = LC.bwd_case(name)
    _, path, heads, Dq, lr, out_sz, ksz, Cc, nchunk, _ = case
    code = {"mfma": _lib.XNA_MFMA, "rows": _lib.XNA_ROWS, "generic": _lib.XNA_GENERIC}[path]
    q, k, v, g = LC.backward_inputs(case)
    d = {"q": LC.to5(q, heads).to(dev), "k": LC.to5(k, heads).to(dev), "v": LC.to5(v, heads).to(dev), "dout": LC.to5(g, heads).to(dev)}
    canon, ddk, ddv = canonical_backward(case, d, dev, path, code)
    chunks = None
    if path == "mfma":
        buf = (C.c_int32 * 16)()
        n = _lib.load().naf_xna_bwd_chunk_plan(C.byref(canon[5]), buf, 16)
        chunks = [int(buf[i]) for i in range(n)]
        assert len(chunks) == nchunk and sum(chunks) == Cc // heads, chunks
    record(f"backward {name:<34s} kernel {path}{'' if not chunks else ' chunks ' + str(chunks)}; identical launches differ by at most dk {ddk:.3e} "
           f"(max |dk| {float(canon[1].abs().max()):.3e}), dv {ddv:.3e} (max |dv| {float(canon[2].abs().max()):.3e})")
    # (3)
    r = S.backward_reference(q, k, v, g, ksz, heads, chunks=chunks)
    bounds = S.backward_bounds(r, q, k, heads, ksz, path)
    for n_, got in (("dq", nchw(canon[0])), ("dk", nchw(canon[1].permute(0, 3, 1, 2, 4))), ("dv", nchw(canon[2].permute(0, 3, 1, 2, 4)))):
        S.check((got - r[n_]).abs(), bounds[n_], f"backward {name} {n_} canonical, B = {LC.B2}")
    # (a), (b), (c)
    failures = []
    for label, plan in LC.launch_plans(("q", "k", "v", "dout"), ("dq",)):
        compare_backward(label, backward_once(case, d, plan, dev, path), canon, ddk, ddv, code, failures)
    # (d) batch stride 0 on k, v and dout; head stride 0 on dout (what naf_xna_head_ce_fwd's dlogits is to this entry)
    dense = {o: LC.CANONICAL for o in ("q", "k", "v", "dout", "dq")}
    de = dict(d, k=equal_images(d["k"]), v=equal_images(d["v"]), dout=equal_images(d["dout"]))
    ce, ek, ev = canonical_backward(case, de, dev, path, code)
    compare_backward("expanded", backward_once(case, de, dict(dense, k="expanded", v="expanded", dout="expanded"), dev, path), ce, ek, ev, code, failures)
    dh = dict(d, dout=equal_heads(d["dout"]))
    ch, hk, hv = canonical_backward(case, dh, dev, path, code)
    compare_backward("expanded-head", backward_once(case, dh, dict(dense, dout="expanded_head"), dev, path), ch, hk, hv, code, failures)
    assert not failures, "\n".join(failures)


# ---- head ------------------------------------------------------------------------------------------------------------------------
HEAD_GEOMS = LC.HEAD_GEOMS
_HEAD = {}


def head_data(dev, gname):
    """Device operands and the oracle's (ref, abs_sum) of a geometry: once."""
    if gname not in _HEAD:
        B, h, w, dy, dx, ksz, heads = HEAD_GEOMS[gname]
        assert S.HEAD_CASES["offset"][0] == LC.HEAD_N
        q, k, pv, pvn, bias = S.make_head_inputs("offset", geom=HEAD_GEOMS[gname])
        d = {"q": LC.to5(q, heads).to(dev), "k": LC.to5(k, heads).to(dev), "pv": pv.to(dev).to(BF16), "bias": bias.to(dev), "geom": HEAD_GEOMS[gname]}
        _HEAD[gname] = (d, S.head_reference64(q, k, pvn, ksz, heads, LC.HEAD_N, bias))
    return _HEAD[gname]


def head_once(d, plan, dev, out_dtype, ce=None):
    """One launch of naf_xna_head_fwd, or (``ce`` = the int64 target) of naf_xna_head_ce_fwd: ({output name: dense tensor}, problems)."""
    from naf_amd import _lib
    B, h, w, dy, dx, ksz, heads = d["geom"]
    Ho, Wo, N = h * dy, w * dx, LC.HEAD_N
    P = LC.Placed()
    t = {o: P.add(o, LC.embed(d[o], plan[o])) for o in ("q", "k", "pv")}
    outs = {"out": LC.hw3(P.add("out", LC.arena_for((B, 1, Ho, Wo, N), out_dtype, plan["out"], dev), output=True))}
    if ce is not None:
        outs["loss"] = LC.hw2(P.add("loss", LC.arena_for((B, 1, Ho, Wo, 1), F32, plan["loss"], dev), output=True))
        outs["labels"] = LC.hw2(P.add("labels", LC.arena_for((B, 1, Ho, Wo, 1), torch.uint8, plan["labels"], dev), output=True))
        outs["dlogits"] = LC.hw3(P.add("dlogits", LC.arena_for((B, 1, Ho, Wo, 32), BF16, plan["dlogits"], dev), output=True))
    P.snapshot()
    if ce is None:
        a, sel = LC.head_args(t["q"], t["k"], t["pv"], d["bias"], outs["out"], N, ksz)
    else:
        a, sel = LC.head_ce_args(t["q"], t["k"], t["pv"], d["bias"], outs["out"], N, ksz, ce, outs["loss"], outs["labels"], outs["dlogits"], 255)
    assert sel == _lib.XNA_HEAD_FUSED, f"{plan}: the head's select gives {sel}"
    LC.head_launch(a, sel, t["q"], ce is not None)
    torch.cuda.synchronize()
    return {n: o.contiguous() for n, o in outs.items()}, P.problems()


def compare_head(label, got, canon, failures):
    outs, problems = got
    failures += [f"{label}: {p}" for p in problems]
    for n, o in outs.items():
        if not LC.same_bits(o, canon[0][n]):
            failures.append(f"{label}: {n} differs from the canonical launch in {int((LC.bits(o) != LC.bits(canon[0][n])).sum())} elements")
        if o.dtype != torch.uint8 and not finite(o):
            failures.append(f"{label}: {n} is not finite")


@pytest.mark.parametrize("gname", list(HEAD_GEOMS))
@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["f32", "bf16"])
def test_head_layouts(dev, out_dtype, gname):
    d, (ref, a) = head_data(dev, gname)
    names = ("q", "k", "pv", "out")
    dense = {o: LC.CANONICAL for o in names}
    canon = head_once(d, dense, dev, out_dtype)
    assert LC.same_bits(canon[0]["out"], head_once(d, dense, dev, out_dtype)[0]["out"]), "two canonical launches differ"
    assert not canon[1], canon[1]
    record(f"head     {gname + ' logits ' + str(out_dtype).split('.')[-1]:<34s} kernel fused")
    got = canon[0]["out"].permute(0, 3, 1, 2).double().cpu()
    S.check((got - ref).abs(), S.head_bound(ref, a, out_dtype == BF16), f"head canonical {out_dtype}, B = {LC.B2}")
    failures = []
    for label, plan in LC.launch_plans(("q", "k", "pv"), ("out",)):
        compare_head(label, head_once(d, plan, dev, out_dtype), canon, failures)
    de = dict(d, k=equal_images(d["k"]), pv=equal_images(d["pv"]))
    canon_e = head_once(de, dense, dev, out_dtype)
    assert not canon_e[1] and finite(canon_e[0]["out"])
    compare_head("expanded", head_once(de, dict(dense, k="expanded", pv="expanded"), dev, out_dtype), canon_e, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("gname", list(HEAD_GEOMS))
def test_head_objective_layouts(dev, gname):
    """naf_xna_head_ce_fwd with the logits, the loss map, the labels and dlogits each in an arena with strides of its own.  The canonical
    launch is anchored as tests/test_gpu_input_statistics.py::test_head_objective_on_large_logits anchors it: its logits are bit for bit
    naf_xna_head_fwd's and inside head_bound; labels, loss and dlogits against those logits in fp64."""
    d, (ref, a) = head_data(dev, gname)
    B, h, w, dy, dx, ksz, heads = d["geom"]
    N, ign = LC.HEAD_N, 255
    t = make_target(B, h * dy, w * dx, N, ign)
    valid = valid_of(t, ign, N)
    td = t.to(dev)
    names = ("q", "k", "pv", "out", "loss", "labels", "dlogits")
    dense = {o: LC.CANONICAL for o in names}
    canon = head_once(d, dense, dev, F32, ce=td)
    again = head_once(d, dense, dev, F32, ce=td)
    assert all(LC.same_bits(canon[0][n], again[0][n]) for n in canon[0]), "two canonical launches differ"
    assert not canon[1], canon[1]
    record(f"head     {gname + ' objective':<34s} kernel fused (logits, loss map, labels, dlogits)")
    plain = head_once(d, {o: LC.CANONICAL for o in ("q", "k", "pv", "out")}, dev, F32)
    assert LC.same_bits(canon[0]["out"], plain[0]["out"]), "the objective's logits are not naf_xna_head_fwd's"
    L64 = canon[0]["out"].permute(0, 3, 1, 2).double().cpu()
    S.check((L64 - ref).abs(), S.head_bound(ref, a), f"objective logits canonical, B = {B}")
    loss, labels, g = canon[0]["loss"].double().cpu(), canon[0]["labels"].long().cpu(), canon[0]["dlogits"].double().cpu()
    assert torch.equal(labels, L64.argmax(1))
    lse = torch.logsumexp(L64, dim=1)
    tc = torch.where(valid, t, torch.zeros_like(t))
    Lt = L64.gather(1, tc.unsqueeze(1))[:, 0]
    assert not bool(((loss - (lse - Lt)).abs() > 1e-5 * (1.0 + lse.abs() + Lt.abs()))[valid].any()) and float(loss[~valid].abs().sum()) == 0.0
    ref_g = ((torch.softmax(L64, dim=1) - F.one_hot(tc, N).permute(0, 3, 1, 2).double()) * valid.unsqueeze(1)).permute(0, 2, 3, 1)
    assert not bool(((g[..., :N] - ref_g).abs() > 2.0 ** -8 * ref_g.abs() + 1e-5).any()) and float(g[..., N:].abs().sum()) == 0.0
    failures = []
    for label, plan in LC.launch_plans(("q", "k", "pv"), ("out", "loss", "labels", "dlogits")):
        compare_head(label, head_once(d, plan, dev, F32, ce=td), canon, failures)
    de = dict(d, k=equal_images(d["k"]), pv=equal_images(d["pv"]))
    canon_e = head_once(de, dense, dev, F32, ce=td)
    assert not canon_e[1]
    compare_head("expanded", head_once(de, dict(dense, k="expanded", pv="expanded"), dev, F32, ce=td), canon_e, failures)
    assert not failures, "\n".join(failures)


# ---- the cosine head ---------------------------------------------------------------------------------------------------------------
_COS = {}


def cos_data(dev, gname):
    """Device operands of a COS_GEOMS geometry and the fp64 reference at the geometry's logit scale: once, shared, never modified."""
    if gname not in _COS:
        from naf_amd import ops
        B, heads, Dv, lr, cell, ks, N = LC.COS_GEOMS[gname]
        q, k, v, E = LC.cos_inputs(gname)
        v5 = LC.to5(v, heads).to(dev)
        d = {"q": LC.to5(q, heads).to(dev), "k": LC.to5(k, heads).to(dev), "v": v5, "pv": ops.project_cosine_values(E.to(dev), v5), "E": E.to(dev),
             "geom": LC.COS_GEOMS[gname], "ls": LC.COS_SCALE[gname], "tables": None}
        assert d["pv"].shape[4] == ops.head_npad(N) != Dv
        _COS[gname] = (d, CR.reference(q, k, v, E, ks, heads, d["ls"]))
    return _COS[gname]


def cos_once(d, plan, dev, ce=None, null=(), scale_ptr=None):
    """One launch of naf_xna_cos_fwd, or (``ce`` = the int64 device target [B, Ho, Wo]) of naf_xna_cos_ce_fwd, every operand in the family
    ``plan`` gives it: ({output name: dense tensor}, problems).  ``null``: outputs handed over as NULL -- their arenas exist all the same
    and must come back bit-unchanged.  ``scale_ptr``: the logit scale as a device value."""
    from naf_amd import _lib, ops
    B, heads, Dv, (h, w), (dy, dx), ks, N = d["geom"]
    Ho, Wo = h * dy, w * dx
    P = LC.Placed()
    t = {o: P.add(o, LC.embed(d[o], plan[o])) for o in LC.COS_INPUTS}
    if ce is not None:
        t["target"] = LC.hw2(P.add("target", LC.embed(ce.view(B, 1, Ho, Wo, 1), plan["target"])))
    channels = {"out": N, "dlogits": ops.head_dlogits_channels(N)}
    outs = {}
    for o in (LC.COS_CE_OUTPUTS if ce is not None else LC.COS_OUTPUTS):
        view = P.add(o, LC.arena_for((B, 1, Ho, Wo, channels.get(o, 1)), LC.COS_DTYPES[o], plan[o], dev), output=True)
        outs[o] = LC.hw3(view) if o in channels else LC.hw2(view)
    P.snapshot()
    given = {o: (None if o in null else v) for o, v in outs.items()}
    if ce is None:
        a, sel = LC.cos_args(t["q"], t["k"], t["pv"], t["v"], given["out"], given["norms"], N, ks, d["ls"], rope_tables=d["tables"])
    else:
        a, sel = LC.cos_ce_args(t["q"], t["k"], t["pv"], t["v"], given["out"], given["norms"], N, ks, t["target"], given["loss"], given["labels"],
                                given["dlogits"], given["dscale"], LC.COS_IGNORE, d["ls"], scale_ptr=scale_ptr, rope_tables=d["tables"])
    assert sel == _lib.XNA_HEAD_FUSED, f"{plan}: the cosine head's select gives {sel}"
    LC.cos_launch(a, sel, t["q"], ce is not None)
    torch.cuda.synchronize()
    problems = P.problems() + [f"{o}: handed over as NULL and written all the same" for o in null if not LC.unchanged(P.arenas[o], P.before[o])]
    return {n: o.contiguous() for n, o in outs.items() if n not in null}, problems


def cos_stride0_sets(d, dense, dev, failures, ce=None, heads_too=True):
    """``expanded`` on k, pv, v (and the target) with their images made equal, ``expanded_head`` on k, pv, v with their heads made equal:
    each against a canonical launch of its own."""
    names = ("k", "pv", "v")
    de, plan = dict(d, **{o: equal_images(d[o]) for o in names}), dict(dense, **{o: "expanded" for o in names})
    te = None
    if ce is not None:
        te, plan["target"] = equal_images(ce), "expanded"
    canon_e = cos_once(de, dense, dev, te)
    assert not canon_e[1] and all(finite(o) for o in canon_e[0].values()), canon_e[1]
    compare_head("expanded", cos_once(de, plan, dev, te), canon_e, failures)
    if heads_too:
        dh = dict(d, **{o: equal_heads(d[o]) for o in names})
        canon_h = cos_once(dh, dense, dev, ce)
        assert not canon_h[1] and all(finite(o) for o in canon_h[0].values()), canon_h[1]
        compare_head("expanded-head", cos_once(dh, dict(dense, **{o: "expanded_head" for o in names}), dev, ce), canon_h, failures)


@pytest.mark.parametrize("gname", list(LC.COS_GEOMS))
def test_cos_layouts(dev, gname):
    """naf_xna_cos_fwd with q, k_lr, pv_lr, v_lr, the cosines and the norm map each in an arena with strides of its own (pv_lr and v_lr
    have other last dims, so their strides differ in every family).  The canonical launch is held to the derived bounds of
    tests/cosine_reference.py against the fp64 definition at B = 2; every other launch to its bits.  On the 14-pixel cells the same with
    rotate-on-load, whose canonical launch is bit for bit the launch on materialised queries."""
    from naf_amd import ops
    d, r = cos_data(dev, gname)
    B, heads, Dv, (h, w), (dy, dx), ks, N = d["geom"]
    dense = {o: LC.CANONICAL for o in LC.COS_INPUTS + LC.COS_OUTPUTS}
    canon = cos_once(d, dense, dev)
    again = cos_once(d, dense, dev)
    assert all(LC.same_bits(canon[0][n], again[0][n]) for n in canon[0]), "two canonical launches differ"
    assert not canon[1] and finite(canon[0]["out"]) and finite(canon[0]["norms"]), canon[1]
    record(f"cos      {gname + ' cosines, norms':<34s} kernel fused")
    CR.check(canon[0]["out"].permute(0, 3, 1, 2).cpu(), r["cos"], CR.bound(r), f"cosines {gname} canonical, B = {B}")
    CR.check(canon[0]["norms"].cpu(), r["norms"], CR.norms_bound(r), f"norms {gname} canonical, B = {B}")
    failures = []
    for label, plan in LC.launch_plans(LC.COS_INPUTS, LC.COS_OUTPUTS):
        compare_head(label, cos_once(d, plan, dev), canon, failures)
    cos_stride0_sets(d, dense, dev, failures)
    compare_head("norms = NULL", cos_once(d, dense, dev, null=("norms",)), canon, failures)
    if gname == "patch14":
        # rotate-on-load: q is the un-rotated guidance, the keys and the materialised queries come from naf_rope_pool_fwd
        x = S.bf16r(O.hash_normal((B, heads * 64, h * dy, w * dx), 310) * 4.0)
        xd = x.to(dev).to(BF16).contiguous(memory_format=torch.channels_last)
        ty, tx = ops.rope_tables(O.rope_periods(heads * 64, heads, 100.0).to(dev), h * dy, w * dx)
        q_mat, k5 = ops.rope_pool(xd, ty, tx, heads, (h, w))
        dr = dict(d, q=xd.permute(0, 2, 3, 1).unflatten(3, (heads, 64)).permute(0, 3, 1, 2, 4).contiguous(), k=k5.contiguous(), tables=(ty, tx))
        canon_r = cos_once(dr, dense, dev)
        assert not canon_r[1] and finite(canon_r[0]["out"]) and finite(canon_r[0]["norms"]), canon_r[1]
        mat = cos_once(dict(dr, q=q_mat.contiguous(), tables=None), dense, dev)
        assert all(LC.same_bits(canon_r[0][n], mat[0][n]) for n in mat[0]), "rotate-on-load differs from materialised queries"
        record(f"cos      {gname + ' cosines, norms, rope':<34s} kernel fused")
        for label, plan in LC.launch_plans(LC.COS_INPUTS, LC.COS_OUTPUTS):
            compare_head(f"rope {label}", cos_once(dr, plan, dev), canon_r, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("gname", list(LC.COS_GEOMS))
def test_cos_objective_layouts(dev, gname):
    """naf_xna_cos_ce_fwd with the cosines, the norm map, the loss map, the labels, dlogits and dscale each in an arena with strides of its
    own, and the int64 target in an input arena.  The canonical launch is anchored: its cosines and norms are bit for bit
    naf_xna_cos_fwd's at the same scale; loss, labels, dlogits and dscale lie inside the derived bounds of
    tests/cosine_objective_reference.py; pad channels and ignored pixels are exactly zero."""
    d, r = cos_data(dev, gname)
    B, heads, Dv, (h, w), (dy, dx), ks, N = d["geom"]
    t = make_target(B, h * dy, w * dx, N, LC.COS_IGNORE, "oob")          # about a tenth ignored, image row 5 outside [0, N)
    valid = valid_of(t, LC.COS_IGNORE, N)
    assert bool(((t != LC.COS_IGNORE) & ~valid).any()) and bool(valid.any())
    td = t.to(dev)
    o = CQ.objective(r, t, LC.COS_IGNORE)
    dense = {n: LC.CANONICAL for n in LC.COS_CE_INPUTS + LC.COS_CE_OUTPUTS}
    canon = cos_once(d, dense, dev, td)
    again = cos_once(d, dense, dev, td)
    assert all(LC.same_bits(canon[0][n], again[0][n]) for n in canon[0]), "two canonical launches differ"
    assert not canon[1], canon[1]
    record(f"cos      {gname + ' objective':<34s} kernel fused (cosines, norms, loss map, labels, dlogits, dscale; logit scale {d['ls']:g})")
    plain = cos_once(d, {n: LC.CANONICAL for n in LC.COS_INPUTS + LC.COS_OUTPUTS}, dev)
    assert LC.same_bits(canon[0]["out"], plain[0]["out"]), "the objective's cosines are not naf_xna_cos_fwd's"
    assert LC.same_bits(canon[0]["norms"], plain[0]["norms"]), "the objective's norms are not naf_xna_cos_fwd's"
    loss, labels, g, ds = canon[0]["loss"].cpu(), canon[0]["labels"].cpu(), canon[0]["dlogits"].float().cpu(), canon[0]["dscale"].cpu()
    CR.check(loss, o["loss"], CQ.loss_bound(r, o), f"loss {gname} canonical, B = {B}")
    CQ.check_labels(labels, r, o, f"labels {gname} canonical, B = {B}")
    CR.check(g[..., :N], o["g"], CQ.g_bound(r, o), f"dlogits {gname} canonical, B = {B}")
    CR.check(ds, o["ds"], CQ.ds_bound(r, o), f"dscale {gname} canonical, B = {B}")
    assert g.shape[-1] > N and float(g[..., N:].abs().max()) == 0.0
    assert float(loss[~valid].abs().max()) == 0.0 and float(g[~valid].abs().max()) == 0.0 and float(ds[~valid].abs().max()) == 0.0
    failures = []
    for label, plan in LC.launch_plans(LC.COS_CE_INPUTS, LC.COS_CE_OUTPUTS):
        compare_head(label, cos_once(d, plan, dev, td), canon, failures)
    cos_stride0_sets(d, dense, dev, failures, td, heads_too=False)
    compare_head("out = norms = NULL", cos_once(d, dense, dev, td, null=("out", "norms")), canon, failures)
    compare_head("logit scale on the device", cos_once(d, dense, dev, td, scale_ptr=torch.tensor([d["ls"]], dtype=F32, device=dev)), canon, failures)
    assert not failures, "\n".join(failures)


def test_cos_element_wise_outputs_take_any_layout(dev):
    """out, norms, loss, labels, dscale and the target in ``odd_offset`` (pointer + 4 elements) and ``odd_stride`` (x stride C + 4), on the
    14-pixel cells: the header has them read and stored element by element, so both selects still answer FUSED (asserted in cos_once), the
    results are the canonical launch's bits and the guard bands stay."""
    gname = "patch14"
    d, r = cos_data(dev, gname)
    B, heads, Dv, (h, w), (dy, dx), ks, N = d["geom"]
    td = make_target(B, h * dy, w * dx, N, LC.COS_IGNORE, "oob").to(dev)
    failures = []
    for ce, ins, outs in ((None, LC.COS_INPUTS, LC.COS_OUTPUTS), (td, LC.COS_CE_INPUTS, LC.COS_CE_OUTPUTS)):
        dense = {n: LC.CANONICAL for n in ins + outs}
        canon = cos_once(d, dense, dev, ce)
        assert not canon[1], canon[1]
        for fam in LC.ROUTING_FAMILIES:
            plan = {n: (fam if n in ("out", "norms", "loss", "labels", "dscale", "target") else LC.CANONICAL) for n in ins + outs}
            compare_head(f"{'objective' if ce is not None else 'cosines'} {fam}", cos_once(d, plan, dev, ce), canon, failures)
            record(f"cos      {gname + (' objective ' if ce is not None else ' cosines ') + fam:<34s} kernel fused (element-wise operands in {fam})")
    assert not failures, "\n".join(failures)


def test_cos_refuses_layouts_that_are_not_vectorisable(dev):
    """q, k_lr, pv_lr or v_lr (and dlogits, for the objective) in ``odd_offset`` / ``odd_stride``: both selects answer -NAF_ERR_UNSUPPORTED,
    not INVALID, under AUTO and FUSED alike, and nothing is launched.  ops.xna_cos_forward / xna_cos_objective (path="auto") then compose:
    the plain forward on the strided queries, normalised in torch, inside the composition's own derived bound."""
    from naf_amd import ops
    gname = "patch14"
    d, r = cos_data(dev, gname)
    B, heads, Dv, (h, w), (dy, dx), ks, N = d["geom"]
    _, _, shapes = LC.cos_shapes(gname)
    for fam in LC.ROUTING_FAMILIES:
        for o in LC.COS_INPUTS + ("dlogits",):
            t = {n: LC.arena_for(shapes[n], LC.COS_DTYPES[n], fam if n == o else LC.CANONICAL, dev, mask=False)[0] for n in shapes}
            for p in ("auto", "fused"):
                if o != "dlogits":
                    assert LC.cos_args(t["q"], t["k"], t["pv"], t["v"], LC.hw3(t["out"]), LC.hw2(t["norms"]), N, ks, path=p)[1] == -2, (fam, o, p)
                sel = LC.cos_ce_args(t["q"], t["k"], t["pv"], t["v"], LC.hw3(t["out"]), LC.hw2(t["norms"]), N, ks, LC.hw2(t["target"]), LC.hw2(t["loss"]),
                                     LC.hw2(t["labels"]), LC.hw3(t["dlogits"]), LC.hw2(t["dscale"]), path=p)[1]
                assert sel == -2, (fam, o, p, sel)
    # the Python entries on such a q: a 5-D view whose pixel stride is no multiple of 8

    class Spy:
        def __init__(self):
            self.names = []

        def start(self, name):
            self.names.append(name)

        def stop(self, name):
            pass

    q = LC.embed(d["q"], "odd_stride")[0]
    assert q.stride(3) % 8 != 0 and q.dim() == 5
    t = make_target(B, h * dy, w * dx, N, LC.COS_IGNORE, "oob")
    old, spy = ops.KERNEL_TIMER, Spy()
    ops.KERNEL_TIMER = spy
    try:
        cos, nrm = ops.xna_cos_forward(q, d["k"], d["v"], d["E"], ks, logit_scale=d["ls"], return_norms=True, path="auto")
        loss, labels, g, ds = ops.xna_cos_objective(q, d["k"], d["v"], d["E"], ks, target=t.to(dev), ignore_index=LC.COS_IGNORE, logit_scale=d["ls"],
                                                    want_loss=True, want_labels=True, want_dlogits=True, want_dscale=True, path="auto")
        torch.cuda.synchronize()
    finally:
        ops.KERNEL_TIMER = old
    assert "xna_cos_composed" in spy.names and "xna_cos_ce_composed" in spy.names and "xna_cos" not in spy.names and "xna_cos_ce" not in spy.names, spy.names
    cb, cnb = CR.composed_bound(r)
    CR.check(cos.cpu(), r["cos"], cb, "composed cosines, q with an odd pixel stride")
    CR.check(nrm.cpu(), r["norms"], cnb, "composed norms, q with an odd pixel stride")
    o = CQ.objective(r, t, LC.COS_IGNORE)
    CR.check(loss.cpu(), o["loss"], 2.0 * cb.amax(dim=1) + 1e-5 * (1.0 + o["lse"].abs() + o["zt"].abs()), "composed loss, q with an odd pixel stride")
    assert labels.shape == ds.shape == loss.shape and g.shape[-1] == ops.head_dlogits_channels(N) and float(g[..., N:].float().abs().max()) == 0.0
    assert float(g.float().cpu()[~o["valid"]].abs().max()) == 0.0 and float(ds.cpu()[~o["valid"]].abs().max()) == 0.0


# ---- the regression objective ------------------------------------------------------------------------------------------------------
def mse_once(d, plan, dev, target, ks):
    """(dout dense, loss [1] clone, problems, naf_xna_mse_args)."""
    P = LC.Placed()
    t = {o: P.add(o, LC.embed(d[o], plan[o])) for o in ("q", "k", "v")}
    dout = P.add("dout", LC.arena_for((*t["q"].shape[:4], t["v"].shape[4]), BF16, LC.CANONICAL, dev), output=True)
    loss = P.add("loss", LC.banded((1,), F32, dev), output=True)
    m, ok = LC.mse_args(t["q"], t["k"], t["v"], target, dout, ks)
    assert ok == 1, f"{plan}: naf_xna_mse_supported gives {ok}"
    ws = P.add("workspace", LC.banded((LC.mse_workspace_bytes(m),), torch.uint8, dev), output=True)
    P.snapshot()
    keep = LC.mse_launch(m, ok, t["q"], ws, loss)
    torch.cuda.synchronize()
    del keep
    return dout.contiguous(), loss.clone(), P.problems(), m


def test_mse_layouts(dev):
    """naf_xna_mse_fwd on one table-driven geometry of tests/test_gpu_regress.py (B = 2, a 14-pixel partial tile) with q, k and v in
    the families; the target kinds have tests of their own there.  The gradient is bit-equal to the canonical launch's, the loss follows
    rule (2), and loss, workspace and gradient sit between guard bands."""
    from naf_amd import ops
    case = LC.MSE_CASE
    B, heads, Dv, lr, out_sz, ks, kind, wt, chunks = R.CASES[case]
    q, k, v, tt = R.make_inputs(case)
    d = {"q": LC.to5(q, heads).to(dev), "k": LC.to5(k, heads).to(dev), "v": LC.to5(v, heads).to(dev)}
    target = R.target_view(tt, kind, dev)
    dense = {o: LC.CANONICAL for o in ("q", "k", "v")}
    runs = [mse_once(d, dense, dev, target, ks) for _ in range(5)]
    for r_ in runs:
        assert not r_[2], r_[2]
        assert LC.same_bits(r_[0], runs[0][0]), "the gradient of two canonical launches differs"
    dl = spread([r_[1] for r_ in runs])
    canon = runs[0]
    record(f"mse      {case:<34s} kernel union; identical launches differ by at most loss {dl:.3e} (loss {float(canon[1]):.6e})")
    # (3): tests/test_gpu_regress.py's bounds
    ref = R.reference(q, k, v, tt, ks, heads)
    plan = ops.xna_union_plan(d["q"], d["k"], d["v"], ks)
    delta = R.output_bound(ref["abs_sum"])
    S.check((nchw(canon[0]) - ref["dout"]).abs(), R.dout_bound(ref["dout"], delta, ref["N"]), "mse dout canonical")
    L = R.chain_length(plan["ry"], plan["seg"], plan["dvt"], R.union_mse_waves(ks, plan["wt"]))
    assert abs(float(canon[1]) - ref["loss"]) <= R.loss_bound(ref["e"], delta, ref["N"], L, ref["loss"])
    failures = []

    def compare(label, got, base, spread_):
        failures.extend(f"{label}: {p}" for p in got[2])
        if not LC.same_bits(got[0], base[0]) or not finite(got[0]):
            failures.append(f"{label}: the gradient differs from the canonical launch")
        within_spread(got[1], base[1], spread_, f"{label}: loss", failures)

    for label, plan_ in LC.launch_plans(("q", "k", "v"), ()):
        compare(label, mse_once(d, plan_, dev, target, ks), canon, dl)
    de = dict(d, k=equal_images(d["k"]), v=equal_images(d["v"]))
    runs_e = [mse_once(de, dense, dev, target, ks) for _ in range(5)]
    compare("expanded", mse_once(de, dict(dense, k="expanded", v="expanded"), dev, target, ks), runs_e[0], spread([r_[1] for r_ in runs_e]))
    assert not failures, "\n".join(failures)


# ---- routing under AUTO, on the device ---------------------------------------------------------------------------------------------
def test_auto_routes_layouts_that_are_not_vectorisable(dev):
    """``odd_offset`` (pointer + 4 elements) and ``odd_stride`` (x stride C + 4) on q, on v and on the output, one forward and one backward
    case under AUTO.  The library must pick a kernel whose eligibility test admits the layout (layout_contract.forward_admits /
    backward_admits restate them) -- never the dense layout's kernel where that one does not -- and the run meets that kernel's bound
    against the oracle with the guard bands intact.  What that is, per operand: a q that is not vectorisable leaves only the scalar
    table-driven kernel; values, `out` and dq are read and written element by element by the row-streaming kernels too (xna_rows.hip:149 /
    :169, xna_rows_bwd.hip:453 / :484), so with few value channels those serve; an `out` whose strides are multiples of 4 is still the
    matrix-core kernels' (xna_mfma.hip:23, xna_union.hip:129)."""
    from naf_amd import _lib, ops
    failures = []
    # forward: cell-k7's geometry, bf16 out
    run = ("cell-k7", BF16, None)
    case = LC.fwd_case("cell-k7")
    _, _, _, heads, Dq, lr, out_sz, ksz, Cc, _ = case
    d = forward_data(run, dev)
    q, k, v = d["host"]
    ref, a = S.attention_reference(q, k, v, ksz, heads)
    names = ("q", "k", "v", "out")
    dense = {o: LC.CANONICAL for o in names}
    P0 = {o: LC.arena_for(d[o].shape if o != "out" else (*d["q"].shape[:4], d["v"].shape[4]), BF16, LC.CANONICAL, dev, mask=False)[0] for o in names}
    auto_dense = LC.forward_args(P0["q"], P0["k"], P0["v"], P0["out"], ksz, "auto")[1]
    for fam in LC.ROUTING_FAMILIES:
        for o in ("q", "v", "out"):
            plan = dict(dense, **{o: fam})
            P = LC.Placed()
            t = {n: P.add(n, LC.embed(d[n], plan[n])) for n in ("q", "k", "v")}
            out = P.add("out", LC.arena_for(P0["out"].shape, BF16, plan["out"], dev), output=True)
            P.snapshot()
            args, sel = LC.forward_args(t["q"], t["k"], t["v"], out, ksz, "auto")
            kern = ops._PATH_NAME.get(sel)
            admits = lambda kn: LC.forward_admits(kn, t["q"], t["k"], t["v"], out)
            assert sel > 0 and admits(kern) and (sel == auto_dense) == admits(ops._PATH_NAME[auto_dense]), (fam, o, sel)
            if o == "q":
                assert kern == "generic"
            keep = LC.forward_launch(args, sel, t["q"])
            torch.cuda.synchronize()
            del keep
            record(f"routing  forward cell-k7 {o}={fam:<12s} kernel {kern} (dense: {ops._PATH_NAME[auto_dense]})")
            failures += [f"forward {o}={fam}: {p}" for p in P.problems()]
            pcase = (case[0], kern) + tuple(case[2:])
            err = (nchw(out.contiguous()) - ref).abs()
            try:
                S.check(err, S.forward_bound(pcase, q, k, ref, a, BF16)[0], f"forward {o}={fam} ({kern})")
            except AssertionError as e:
                failures.append(str(e))
    # backward: the cell case
    bcase = LC.bwd_case("cell")
    _, _, heads, Dq, lr, out_sz, ksz, Cc, _, _ = bcase
    q, k, v, g = LC.backward_inputs(bcase)
    d = {"q": LC.to5(q, heads).to(dev), "k": LC.to5(k, heads).to(dev), "v": LC.to5(v, heads).to(dev), "dout": LC.to5(g, heads).to(dev)}
    r = S.backward_reference(q, k, v, g, ksz, heads)
    kname = {_lib.XNA_MFMA: "mfma", _lib.XNA_ROWS: "rows", _lib.XNA_GENERIC: "generic"}
    names = ("q", "k", "v", "dout", "dq")
    dense = {o: LC.CANONICAL for o in names}
    for fam in LC.ROUTING_FAMILIES:
        for o in ("q", "v", "dq"):
            dq, dk, dv, problems, sel, args = backward_once(bcase, d, dict(dense, **{o: fam}), dev, "auto")
            kern = kname[sel]
            assert kern != "mfma", (fam, o)          # xna_bwd.hip:60-62 asks all five operands to be vectorisable
            if o == "q":
                assert kern == "generic"
            record(f"routing  backward cell {o}={fam:<12s} kernel {kern} (dense: mfma)")
            failures += [f"backward {o}={fam}: {p}" for p in problems]
            bounds = S.backward_bounds(r, q, k, heads, ksz, kern)
            for n_, got in (("dq", nchw(dq)), ("dk", nchw(dk.permute(0, 3, 1, 2, 4))), ("dv", nchw(dv.permute(0, 3, 1, 2, 4)))):
                try:
                    S.check((got - r[n_]).abs(), bounds[n_], f"backward {o}={fam} ({kern}) {n_}")
                except AssertionError as e:
                    failures.append(str(e))
    assert not failures, "\n".join(failures)


# ---- teeth, on the device, without touching a kernel --------------------------------------------------------------------------------
def test_the_checker_reports_another_row_stride_on_the_output_and_on_an_input(dev):
    """One launch whose `out` the kernel gets with the row stride of ``row_gap`` while the checker is told ``channels_last`` at the same
    start: both layouts are legal and inside the arena, and the kernel is right -- so, seen through the checker's layout, it writes
    outside the view.  ``untouched`` must say so, the view must differ from the canonical result and hold NaN where nothing was written."""
    run = ("union-k7", BF16, None)
    case = LC.fwd_case("union-k7")
    ksz = case[7]
    d = forward_data(run, dev)
    dense = {o: LC.CANONICAL for o in ("q", "k", "v", "out")}
    canon = forward_once(run, d, dense, dev, "union")
    q, k, v = (LC.embed(d[o], LC.CANONICAL)[0] for o in ("q", "k", "v"))
    shape = (*q.shape[:4], v.shape[4])
    given, arena, mask_given = LC.arena_for(shape, BF16, "row_gap", dev)
    sb, sh, sy, sx = given.stride()[:4]
    told_strides = (sb, sh, shape[3] * sx, sx)                      # channels-last rows, the images where row_gap has them
    told = arena.as_strided(shape, told_strides + (1,), given.storage_offset())
    mask_told = LC.view_mask(arena.numel(), given.storage_offset(), shape, told_strides, dev)
    before = arena.clone()
    a, sel = LC.forward_args(q, k, v, given, ksz, "union")
    keep = LC.forward_launch(a, sel, q)
    torch.cuda.synchronize()
    del keep
    assert LC.untouched(arena, before, mask_given) and LC.same_bits(given, canon[0])          # the kernel did what it was told
    assert not LC.untouched(arena, before, mask_told)                                         # ... which the wrong description exposes
    assert LC.outside_writes(arena, before, mask_told) >= 24 and not LC.same_bits(told, canon[0]) and not finite(told)
    # The reading side: q lives in ``row_gap`` and the kernel is handed rows W pixels apart (legal, inside the arena) -- what a kernel that
    # derives the row stride would read.  The gaps' NaN reach the output: the equality and the finiteness checks both say so.
    qv, qarena, _ = LC.embed(d["q"], "row_gap")
    sb, sh, sy, sx = qv.stride()[:4]
    q_wrong = qarena.as_strided(qv.shape, (sb, sh, qv.shape[3] * sx, sx, 1), qv.storage_offset())
    out2, arena2, mask2 = LC.arena_for(shape, BF16, LC.CANONICAL, dev)
    before2 = arena2.clone()
    a, sel = LC.forward_args(q_wrong, k, v, out2, ksz, "union")
    keep = LC.forward_launch(a, sel, q_wrong)
    torch.cuda.synchronize()
    del keep
    assert LC.untouched(arena2, before2, mask2) and not LC.same_bits(out2, canon[0]) and not finite(out2)


def test_xna_forward_checks_out_before_launching(dev):
    """ops.xna_forward(out=...): a buffer of another shape, with a strided last dim or on another device is refused with ValueError and is
    not written; a well-formed strided one is filled and returned."""
    from naf_amd import ops
    case = LC.fwd_case("union-k7")
    _, path, _, heads, Dq, lr, out_sz, ksz, Cc, _ = case
    d = forward_data(("union-k7", BF16, None), dev)
    shape = (*d["q"].shape[:4], d["v"].shape[4])
    small, arena, mask = LC.arena_for((shape[0], shape[1], shape[2] - 1, shape[3], shape[4]), BF16, "channels_last", dev)
    before = arena.clone()
    for bad in (small, torch.empty(shape, dtype=BF16), torch.empty((*shape[:3], shape[4], shape[3]), dtype=BF16, device=dev).transpose(3, 4)):
        with pytest.raises(ValueError, match="out must be a"):
            ops.xna_forward(d["q"], d["k"], d["v"], ksz, out=bad, path=path)
    torch.cuda.synchronize()
    assert LC.unchanged(arena, before)
    good, arena, mask = LC.arena_for(shape, BF16, "pixel_gap", dev)
    before = arena.clone()
    got = ops.xna_forward(d["q"], d["k"], d["v"], ksz, out=good, path=path)
    torch.cuda.synchronize()
    assert got is good and LC.untouched(arena, before, mask) and finite(good)
    assert LC.same_bits(good, ops.xna_forward(d["q"], d["k"], d["v"], ksz, path=path))
