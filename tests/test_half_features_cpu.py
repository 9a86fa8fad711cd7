"""float16 features through the attention forward, the part that needs no device (tests/half_reference.py has the bound and the
emulations; tests/test_gpu_half_features.py runs the kernels).

A. Discrimination: over every input_statistics.FWD_CASES entry and family, the NATIVE route (P * 2^8 rounded to half with worst-case
   flushing of every operand below 2^-14, half values, half store) stays inside half_bound on every element, and the route the library
   served float16 callers by before (values and P rounded to bf16, an fp32 map cast to half) leaves it -- so the device test that asserts
   half_bound cannot pass on that route.  Where it must: one rounding of a value to bf16 moves it by up to 2^-9 of itself and one of P
   likewise, four times the 2^-11 the bound allows, unless the errors of many window taps average out (a flat softmax over a 15 x 15
   window) or the bound's absolute 2^-14 dominates (the "small" family: |v| <= 3.4e-3, where 2^-9 |v| < 2^-17).  Asserted: "small" stays
   inside on either route in every case; every other (case, family) of the five cases that sweep all nine families leaves the bound on
   the bf16 route; and every value family but "small" leaves it in at least three quarters of the cases it appears in.
B. Host logic: naf_dtype_supported, naf_xna_select with NAF_F16, mixed dtypes, header / binding / exports, the version, CPU tensors.
"""
import ctypes as C
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_reference as H  # noqa: E402
import input_statistics as S  # noqa: E402
from input_statistics import FWD_CASES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RATIOS = {}


def _ratios(case):
    """{family: (native worst err / bound, bf16-route worst err / bound)} of a case, computed once."""
    if case[0] not in _RATIOS:
        out = {}
        for fam in case[9]:
            q, k, v = H.half_inputs(case, fam)
            ref, a = S.attention_reference(q, k, v, case[7], case[3])
            bound = H.half_bound(case, q, k, v, ref, a)
            fp32 = case[1] == "generic"
            native = (H.attention_half_emulated(q, k, v, case[7], case[3], "native", p_fp32=fp32) - ref).abs()
            old = (H.attention_half_emulated(q, k, v, case[7], case[3], "bf16", p_fp32=fp32) - ref).abs()
            S.check(native, bound, f"native emulation {case[0]} {fam}")
            out[fam] = (S.worst_of_bound(native, bound), S.worst_of_bound(old, bound))
            print(f"{case[0]:<22s} {str(fam):<34s} native {out[fam][0]:.3f}  bf16 route {out[fam][1]:.3f} of the bound")
        _RATIOS[case[0]] = out
    return _RATIOS[case[0]]


def test_half_values_are_half_numbers_with_eleven_bits():
    for fam in S.VALUE_FAMILIES:
        v = H.make_half_values((1, 16, 9, 10), fam, 5)
        assert torch.equal(v, H.f16r(v)) and float(v.abs().max()) < 65504.0
        if fam != "small":
            assert not torch.equal(v, S.bf16r(v)), fam            # more significand than bf16 holds
    assert H.U16 == 2.0 ** -11 and S.SLACK == 1.25


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c[0])
def test_native_route_inside_the_bound_and_the_bf16_route_outside(case):
    r = _ratios(case)
    for fam, (native, old) in r.items():
        assert native <= 1.0
        if fam[0] == "small":
            assert old <= 1.0, f"{case[0]} {fam}: the 2^-14 allowance should dominate"
        elif case[9] is S.FORWARD_FAMILIES:
            assert old > 1.0, f"{case[0]} {fam}: the bf16 route stays inside half_bound ({old:.3f}): the bound does not tell the routes apart"


def test_every_value_family_but_small_tells_the_routes_apart():
    seen = {}
    for case in FWD_CASES:
        for fam, (_, old) in _ratios(case).items():
            seen.setdefault(fam[0], []).append(old > 1.0)
    assert set(seen) == set(S.VALUE_FAMILIES)
    for vf, hits in seen.items():
        if vf == "small":
            assert not any(hits)
        else:
            assert sum(hits) >= 0.75 * len(hits), (vf, hits)


# ---- B: host logic -------------------------------------------------------------------------------------------------------------
def _xna_args(case, out_dtype, path=0, logits=False):
    from naf_amd._lib import I64x4, XnaArgs
    _, _, _, heads, Dq, (h, w), (Ho, Wo), k, Cc, _ = case
    a = XnaArgs()
    Dv = Cc // heads
    a.q = a.k_lr = a.v_lr = a.out = 0x1000           # host logic only: never dereferenced
    a.logits = 0x1000 if logits else None
    a.B, a.heads, a.Ho, a.Wo, a.h, a.w, a.Dq, a.Dv, a.ky, a.kx = 1, heads, Ho, Wo, h, w, Dq, Dv, k, k
    a.out_dtype, a.path, a.scale = out_dtype, path, 0.0
    a.q_stride = I64x4(Ho * Wo * heads * Dq, Dq, Wo * heads * Dq, heads * Dq)
    a.k_stride = I64x4(h * w * heads * Dq, Dq, w * heads * Dq, heads * Dq)
    a.v_stride = I64x4(h * w * heads * Dv, Dv, w * heads * Dv, heads * Dv)
    a.o_stride = I64x4(Ho * Wo * heads * Dv, Dv, Wo * heads * Dv, heads * Dv)
    return a


def test_dtype_supported_answers_as_documented(built_lib):
    from naf_amd import _lib
    lib = _lib.load()
    assert (_lib.NAF_BF16, _lib.NAF_F32, _lib.NAF_F16) == (0, 1, 2)
    sup = lambda what: [lib.naf_dtype_supported(what, d) for d in (_lib.NAF_BF16, _lib.NAF_F32, _lib.NAF_F16, 3, -1)]
    assert sup(_lib.DT_XNA_VALUES) == [1, 0, 1, 0, 0]          # values are 16-bit: bf16 or half
    for what in (_lib.DT_XNA_OUT, _lib.DT_PACK_SRC, _lib.DT_FWD_FEAT, _lib.DT_FWD_OUT):
        assert sup(what) == [1, 1, 1, 0, 0], what
    assert sup(5) == [0] * 5 and sup(-1) == [0] * 5


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c[0])
def test_select_picks_for_half_what_it_picks_for_bf16(built_lib, case):
    from naf_amd import _lib
    lib = _lib.load()
    names = {"mfma": _lib.XNA_MFMA, "union": _lib.XNA_UNION, "rows": _lib.XNA_ROWS, "generic": _lib.XNA_GENERIC}
    for path in (_lib.XNA_AUTO, names[case[1]]):
        for logits in (False, True):
            want = lib.naf_xna_select(C.byref(_xna_args(case, _lib.NAF_BF16, path, logits)))
            got = lib.naf_xna_select(C.byref(_xna_args(case, _lib.NAF_F16, path, logits)))
            assert got == want, (case[0], path, logits, _lib.last_error())
    assert lib.naf_xna_select(C.byref(_xna_args(case, _lib.NAF_F16, names[case[1]]))) == names[case[1]]
    assert lib.naf_xna_select(C.byref(_xna_args(case, 3))) == -1 and "out_dtype 3" in _lib.last_error()


def test_forward_rejects_mixed_dtypes_with_a_message(built_lib):
    """naf_forward: half features go with half output and only with it."""
    from naf_amd import _lib
    lib = _lib.load()
    a = _lib.ForwardArgs()
    a.image = a.features = a.out = a.tab_y = a.tab_x = 0x1000          # host logic only: never dereferenced
    a.nlayer, a.B, a.H, a.W, a.h, a.w, a.C, a.heads, a.ksize = 2, 1, 64, 64, 8, 8, 128, 4, 7
    for br in range(2):
        b = a.branch[br]
        b.conv0_weight = b.conv0_bias = 0x1000
        b.conv0_ksize, b.ksize = (1, 1) if br else (3, 3)
        for l in range(2):
            b.gn_weight[l] = b.gn_bias[l] = b.conv_bias[l] = 0x1000
            b.conv_weight_packed[l] = 0x1000
    for feat, out, ok in ((_lib.NAF_BF16, _lib.NAF_BF16, True), (_lib.NAF_F32, _lib.NAF_F32, True), (_lib.NAF_F16, _lib.NAF_F16, True),
                          (_lib.NAF_F16, _lib.NAF_BF16, False), (_lib.NAF_F16, _lib.NAF_F32, False), (_lib.NAF_BF16, _lib.NAF_F16, False),
                          (_lib.NAF_F32, _lib.NAF_F16, False)):
        a.image_dtype, a.feat_dtype, a.out_dtype = _lib.NAF_F32, feat, out
        rc = lib.naf_forward_supported(C.byref(a))
        if ok:
            assert rc == 1, (feat, out, _lib.last_error())
        else:
            assert rc == -1 and "half features go with half output" in _lib.last_error(), (feat, out, rc)
    # the workspace does not depend on the value type: 2 bytes per element either way
    a.feat_dtype = a.out_dtype = _lib.NAF_BF16
    n16 = lib.naf_forward_workspace_bytes(C.byref(a))
    a.feat_dtype = a.out_dtype = _lib.NAF_F16
    assert lib.naf_forward_workspace_bytes(C.byref(a)) == n16 > 0


def test_header_binding_exports_and_version(built_lib):
    from naf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert re.search(r"enum naf_dtype \{ NAF_BF16 = 0, NAF_F32 = 1, NAF_F16 = 2 \};", txt)
    assert re.search(r"^int naf_dtype_supported\(int what, int dtype\);", txt, flags=re.M)
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == 403 == _lib.HEADER_VERSION
    assert _lib.SIGNATURES["naf_dtype_supported"] == (C.c_int, [C.c_int, C.c_int])
    raw = C.CDLL(built_lib)
    assert hasattr(raw, "naf_dtype_supported")
    raw.naf_version.restype = C.c_int
    assert raw.naf_version() == 403
    enum = re.search(r"enum naf_dtype_arg \{(.*?)\};", txt, flags=re.S).group(1)
    vals = dict((n, int(v)) for n, v in re.findall(r"(NAF_DT_[A-Z_]+) = (\d+)", enum))
    assert vals == {"NAF_DT_XNA_VALUES": _lib.DT_XNA_VALUES, "NAF_DT_XNA_OUT": _lib.DT_XNA_OUT, "NAF_DT_PACK_SRC": _lib.DT_PACK_SRC,
                    "NAF_DT_FWD_FEAT": _lib.DT_FWD_FEAT, "NAF_DT_FWD_OUT": _lib.DT_FWD_OUT}


def test_value_dtype_map_is_separate():
    """float16 is a value / output dtype of the attention forward only: the map that gates images, targets and every other entry has not grown."""
    from naf_amd import _lib, ops
    assert ops._DT == {torch.bfloat16: _lib.NAF_BF16, torch.float32: _lib.NAF_F32}
    assert ops._DT_VALUES == {**ops._DT, torch.float16: _lib.NAF_F16}


def test_cpu_tensors_still_have_no_fallback():
    from naf_amd import NAF, ops
    v = torch.zeros(1, 16, 4, 4, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_values(v)
    q = torch.zeros(1, 1, 8, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.xna_forward(q, q[:, :, :4, :4], torch.zeros(1, 1, 4, 4, 16, dtype=torch.float16), 3, out_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NAF(kernel_size=3)(torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 4, 4, dtype=torch.float16), (16, 16))
