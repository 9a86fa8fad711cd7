"""float16 features through the attention forward kernels, on the device (tests/half_reference.py: families, bound, emulations;
tests/test_half_features_cpu.py: why the bound tells the native route from the bf16 one).

C. ops.pack_values of float16: a float16 tensor, bit-equal to the permuted input (strided views too).
D. Exact gather through every arm: one-hot attention on integer values up to 2047 -- any wrong lane map, V fragment or store shows as a
   wrong integer, and bf16 cannot hold the integers above 256 at all.
E. Per-element parity: |out - ref| <= half_reference.half_bound on every element of every FWD_CASES entry and family, plus rotate-on-load.
F. Module level: dtype, strides, peak memory, whole-forward bound, the one-call plan, graph capture, no cached plan across dtypes.
"""
import os
import re
import sys

import pytest
import torch

from oracle import naf_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_reference as H  # noqa: E402
import input_statistics as S  # noqa: E402
from input_statistics import FWD_CASES  # noqa: E402
from test_gpu_parity import _load_model, to5  # noqa: E402

pytestmark = pytest.mark.gpu
F16 = torch.float16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from naf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def nchw(t5):
    B, n, Hh, Ww, D = t5.shape
    return t5.permute(0, 1, 4, 2, 3).reshape(B, n * D, Hh, Ww).double().cpu()


def v5_half(v, heads, dev):
    """fp16-representable fp32 [B, C, h, w] -> float16 5-D [B, heads, h, w, Dv] view of a channels-last buffer."""
    B, C, h, w = v.shape
    vh = v.to(dev).to(F16)
    assert torch.equal(vh.float().cpu(), v)
    return vh.permute(0, 2, 3, 1).contiguous().view(B, h, w, heads, C // heads).permute(0, 3, 1, 2, 4)


def kernels_run(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}


# ---- C -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 40, 5, 7), (1, 33, 3, 11)])
def test_pack_values_half_is_an_exact_copy(dev, shape):
    from naf_amd import ops
    B, C, h, w = shape
    v = (O.hash_normal(shape, 61) * 50.0).to(dev).to(F16)
    v.view(-1)[:4] = torch.tensor([6.0e-8, -6.1e-5, 65504.0, -0.0], dtype=F16, device=dev)       # a subnormal, the smallest normal, the largest
    big = torch.zeros((B, h + 2, w + 3, C + 5), dtype=F16, device=dev)
    big[:, 1:1 + h, 2:2 + w, 3:3 + C] = v.permute(0, 2, 3, 1)
    views = {"contiguous": v, "channels-last crop": big[:, 1:1 + h, 2:2 + w, 3:3 + C].permute(0, 3, 1, 2),
             "every other channel": torch.stack([v, v], dim=2).flatten(1, 2)[:, ::2]}
    for name, x in views.items():
        got = ops.pack_values(x)
        assert got.dtype == F16 and got.is_contiguous() and tuple(got.shape) == (B, h, w, C), name
        assert torch.equal(got.view(torch.int16), x.permute(0, 2, 3, 1).contiguous().view(torch.int16)), name
    assert ops.pack_values(v.float()).dtype == torch.bfloat16 and ops.pack_values(v.bfloat16()).dtype == torch.bfloat16


# ---- D -------------------------------------------------------------------------------------------------------------------------
# (id, path, heads, Dq, (h, w), (Ho, Wo), C, return_logits, kernel that must have run -- None: whatever the bf16 call of the geometry runs)
# Dv = 48 is three channel tiles: a pair stored as 16 bytes per lane plus a single one (xna_store4).  A 48-channel tile cannot be staged
# (staged stores want a multiple of 32), so without logits that geometry is served by the sliding kernel; Dv = 64 is the staged cell plan.
GATHER_CASES = [
    ("cell-staged", "mfma", 2, 64, (9, 10), (144, 160), 128, False, "xna_mfma_kernel"),
    ("cell-dv48", "mfma", 2, 64, (9, 10), (144, 160), 96, False, None),
    ("cell-unstaged-logits", "mfma", 2, 64, (9, 10), (144, 160), 96, True, "xna_mfma_kernel"),
    ("union", "union", 2, 64, (9, 10), (23, 27), 96, False, "xna_union_kernel"),
    ("rows", "rows", 1, 96, (16, 18), (16, 18), 3, False, "xna_rows_kernel"),
    ("generic", "generic", 2, 64, (9, 10), (23, 27), 96, False, "xna_generic_kernel"),
    ("sliding", "mfma", 2, 64, (9, 10), (18, 160), 96, False, "xna_slide_kernel"),
]


@pytest.mark.parametrize("case", GATHER_CASES, ids=lambda c: c[0])
def test_exact_gather_through_every_arm(dev, case):
    from naf_amd import ops
    name, path, heads, Dq, lr, out_sz, C, logits, kernel = case
    q, k, v, want = H.gather_inputs(heads, Dq, lr, out_sz, 7, C)
    assert float(v.max()) > 1024 and not torch.equal(v, S.bf16r(v))                       # bf16 cannot carry these values
    q5, k5, v5 = to5(q, heads).to(dev), to5(k, heads).to(dev), v5_half(v, heads, dev)
    assert ops.xna_select(q5, k5, v5, 7, out_dtype=F16, return_logits=logits, path=path) == path \
        == ops.xna_select(q5, k5, v5.bfloat16(), 7, out_dtype=torch.bfloat16, return_logits=logits, path=path)
    res, names = kernels_run(lambda: ops.xna_forward(q5, k5, v5, 7, out_dtype=F16, path=path, return_logits=logits))
    out = res[0] if logits else res
    assert out.dtype == F16
    if kernel is not None:
        assert any(kernel in n for n in names), sorted(names)
        if name == "cell-staged":      # xna_mfma_kernel<KS, DVT, OutT, STG, ...>: mangled "ILi7ELi64EDF16_Lb1E", demangled "<7, 64, _Float16, true,"
            stg = [re.search(r"xna_mfma_kernel(?:ILi\d+ELi\d+E[A-Za-z0-9_]+?Lb([01])E|<\d+, \d+, [^,]+, (true|false),)", n) for n in names if "xna_mfma_kernel" in n]
            assert stg and all(m_ is not None and (m_.group(1) == "1" or m_.group(2) == "true") for m_ in stg), sorted(names)
    else:
        _, names16 = kernels_run(lambda: ops.xna_forward(q5, k5, v5.bfloat16(), 7, out_dtype=torch.bfloat16, path=path))
        family = lambda ns: {m_.group(0) for m_ in (re.search(r"xna_[a-z]+_kernel", n) for n in ns) if m_ is not None}
        assert family(names) == family(names16) != set(), (sorted(names), sorted(names16))
    got = nchw(out)
    bad = got != want.double()
    assert not bool(bad.any()), f"{name}: {int(bad.sum())}/{bad.numel()} wrong; first at {tuple(bad.nonzero()[0].tolist())}: " \
                                f"got {float(got[bad][0])}, want {float(want.double()[bad][0])}"
    if logits:
        lg = res[1]
        assert lg.dtype == torch.float32 and float(lg.max()) == 32.0 and float(lg.min()) == 0.0
        assert bool(((lg == 32.0).sum(-1) >= 1).all())


# ---- E -------------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(case, fam):
    key = (case[0], fam)
    if key not in _REF:
        q, k, v = H.half_inputs(case, fam)
        ref, a = S.attention_reference(q, k, v, case[7], case[3])
        _REF[key] = (q, k, v, ref, a, H.half_bound(case, q, k, v, ref, a))
    return _REF[key]


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c[0])
def test_half_forward_per_element_bound(dev, case):
    from naf_amd import ops
    name, path, sub, heads, _, lr, out_sz, ksz = case[:8]
    failures = []
    for fam in case[9]:
        q, k, v, ref, _, bound = reference(case, fam)
        q5, k5, v5 = to5(q, heads).to(dev), to5(k, heads).to(dev), v5_half(v, heads, dev)
        assert ops.xna_select(q5, k5, v5, ksz, out_dtype=F16, path=path) == path
        out = ops.xna_forward(q5, k5, v5, ksz, out_dtype=F16, path=path)
        assert out.dtype == F16 and bool(torch.isfinite(out).all())
        err = (nchw(out) - ref).abs()
        print(f"half forward {name:<22s} {str(fam):<34s} worst err / bound {S.worst_of_bound(err, bound):.3f}")
        try:
            S.check(err, bound, f"half forward {name} {fam}")
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    if sub == "sliding" and ksz >= 11:                  # no staged plan from 11 x 11 up: the sliding kernel's half instantiation ran
        _, names = kernels_run(lambda: ops.xna_forward(q5, k5, v5, ksz, out_dtype=F16, path=path))
        assert any("xna_slide_kernel" in n for n in names), sorted(names)


def test_half_forward_rotate_on_load(dev):
    """The cell kernel rotating the queries as it loads them, half values: bit-equal to materialised queries and inside the bound."""
    from naf_amd import ops
    heads, Dq, lr, out_sz, ksz, C = 4, 64, (8, 8), (16, 128), 7, 256
    case = ("rope", "mfma", "cell", heads, Dq, lr, out_sz, ksz, C, None)
    x = S.bf16r(O.hash_normal((1, heads * Dq, *out_sz), 310) * 4.0)
    v = H.make_half_values((1, C, *lr), "outlier", 311)
    per = O.rope_periods(heads * Dq, heads, 100.0)
    xd = x.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ty, tx = ops.rope_tables(per.to(dev), *out_sz)
    q_mat, k5 = ops.rope_pool(xd, ty, tx, heads, lr)
    q_raw = xd.permute(0, 2, 3, 1).unflatten(3, (heads, Dq)).permute(0, 3, 1, 2, 4)
    v5 = v5_half(v, heads, dev)
    assert ops.xna_rope_fusable(q_raw, lr, C // heads, ksz, (ty, tx), out_dtype=F16)
    a_ = ops.xna_forward(q_mat, k5, v5, ksz, out_dtype=F16, path="mfma")
    b_ = ops.xna_forward(q_raw, k5, v5, ksz, out_dtype=F16, path="mfma", rope_tables=(ty, tx))
    assert b_.dtype == F16 and torch.equal(a_, b_)
    qf, kf = nchw(q_mat).float(), nchw(k5).float()
    ref, a = S.attention_reference(qf, kf, v, ksz, heads)
    S.check((nchw(b_) - ref).abs(), H.half_bound(case, qf, kf, v, ref, a), "half rotate-on-load")


def test_half_and_other_dtypes_never_mix(dev):
    from naf_amd import ops
    q = torch.zeros(1, 1, 8, 8, 64, dtype=torch.bfloat16, device=dev)
    k = q[:, :, :4, :4].contiguous()
    vh = torch.zeros(1, 1, 4, 4, 16, dtype=F16, device=dev)
    for v, od in ((vh, torch.bfloat16), (vh, torch.float32), (vh.bfloat16(), F16)):
        with pytest.raises(TypeError, match="float16 values go with out_dtype=torch.float16"):
            ops.xna_forward(q, k, v, 3, out_dtype=od)
    with pytest.raises(TypeError, match="only with it"):
        ops.xna_forward(q, k, vh, 3, out_dtype=F16, out=torch.empty(1, 8, 8, 1, 16, dtype=torch.bfloat16, device=dev).permute(0, 3, 1, 2, 4))
    with pytest.raises(TypeError, match="must be bfloat16"):
        ops.xna_forward(q.half(), k, vh, 3, out_dtype=F16)
    assert ops.xna_forward(q, k, vh, 3, out_dtype=F16).dtype == F16


# ---- F -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def module_case(dev):
    p = O.make_params(seed=83)
    img = O.hash_normal((1, 3, 256, 256), 8301)
    ft = H.f16r(O.hash_normal((1, 128, 16, 16), 8302))
    ref = O.naf_forward(p, img, ft, (256, 256), kernel_size=7)
    return _load_model(dev, p, kernel_size=7), img.to(dev), ft.to(dev), ref


def test_module_half_features_native(dev, module_case):
    m, img, ft, ref = module_case
    fh, fb = ft.half(), ft.bfloat16()
    size = (256, 256)
    before16, before32 = m(img, fb, size).clone(), m(img, ft, size).clone()
    out = m(img, fh, size)
    assert out.dtype == F16 and tuple(out.shape) == (1, 128, 256, 256)
    assert out.stride() == before16.stride() and out.permute(0, 2, 3, 1).is_contiguous()
    plan = m._forward_plan(img, fh, size)
    assert plan is not None and plan.out_dtype == F16, "float16 features must run through the one-call plan"
    err = (out.double().cpu() - ref.double()).abs()
    bound = 2e-2 + 1e-2 * ref.double().abs()
    S.check(err, bound, "module, float16 features")
    # no cached plan leaks across dtypes: the other dtypes return the bits they returned before the float16 call, and it its own
    assert torch.equal(m(img, fb, size), before16) and torch.equal(m(img, ft, size), before32)
    assert torch.equal(m(img, fh, size), out)
    assert m(img, fb, size).dtype == torch.bfloat16 and m(img, ft, size).dtype == torch.float32
    # the multi-call route (no plan; its stem launches differ, so not the same bits) serves them natively too
    m.single_call = False
    try:
        multi = m(img, fh, size)
    finally:
        m.single_call = True
    assert multi.dtype == F16 and multi.stride() == out.stride()
    S.check((multi.double().cpu() - ref.double()).abs(), bound, "module, float16 features, multi-call route")
    g = m.capture(img, fh, size)
    assert g().dtype == F16 and torch.equal(g(), out)


def test_module_half_features_peak_memory(dev, module_case):
    """No fp32 map and no cast pass: the float16 call's peak is the bf16 call's (before: + the 33.5 MB fp32 map and the cast's output)."""
    m, img, ft, _ = module_case
    fh, fb = ft.half(), ft.bfloat16()
    size = (256, 256)
    peaks = {}
    for name, f in (("bf16", fb), ("fp16", fh)):
        m(img, f, size)                               # plan, workspace and tables of this dtype exist
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        o = m(img, f, size)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(dev) - base
        del o
    print(f"peak bytes above the baseline: {peaks}")
    assert peaks["fp16"] - peaks["bf16"] <= 1 << 20, peaks
