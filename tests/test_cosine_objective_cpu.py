"""CPU tests of the cosine objective's yardstick (tests/cosine_objective_reference.py) and of its host-side surface: the fp64 restatement
against F.cross_entropy and torch autograd, the emulated kernel against the bounds, planted defects, what naf_xna_cos_ce_select grants, the
struct layout and the refusals of ``naf(..., cosine=True, loss="ce")`` that need no device."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_reference as R  # noqa: E402
import cosine_objective_reference as Q  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = "b_whole_grid_n1", "e_patch14_n21", "f_rows30_n151"
_REFS = {}


def _ref(name, ls=10.0, **kw):
    """(inputs, reference, objective, target), computed once per (case, scale, inputs) and left unchanged."""
    key = (name, ls, tuple(sorted(kw.items())))
    if key not in _REFS:
        B, heads, Dv, lr, cell, ks, N = R.CASES[name]
        q, k, v, E = R.make_inputs(name, **kw)
        r = R.reference(q, k, v, E, ks, heads, logit_scale=ls)
        t = Q.make_target(name)
        _REFS[key] = ((q, k, v, E, ks, heads), r, Q.objective(r, t), t)
    return _REFS[key]


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name", SMALL)
def test_restatement_equals_cross_entropy_and_autograd(name):
    """loss == F.cross_entropy on cosine_from_features64; dE^ = sum_px g' f and ds_total = sum_px ds == fp64 autograd; <= 1e-9 relative."""
    (q, k, v, E, ks, heads), r, o, t = _ref(name)
    N = E.shape[0]
    z, _ = R.cosine_from_features64(r["f"], E, r["ls"])
    tgt = torch.where(Q.valid_of(t, Q.IGNORE, N), t, torch.full_like(t, -100))
    want = F.cross_entropy(z, tgt, ignore_index=-100, reduction="none")
    assert float((o["loss"] - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))
    assert torch.equal(o["labels"], z.argmax(1))
    total, d_ehat, ds_total = Q.autograd_reference(r["f"], r["e_hat"], r["ls"], t, normalized=True)
    assert abs(float(o["loss"].sum() - total)) <= 1e-9 * max(1.0, abs(float(total)))
    got = torch.einsum("bhwn,bchw->nc", o["g"], r["f"])
    if N > 1:
        assert _rel(got, d_ehat) <= 1e-9
        assert abs(float(o["ds"].sum() - ds_total)) <= 1e-9 * max(1.0, abs(float(ds_total)))
    else:       # one class: the loss is identically 0
        assert float(got.abs().max()) == 0.0 and float(d_ehat.abs().max()) <= 1e-12 and float(o["loss"].abs().max()) == 0.0
    # ignored pixels: no loss, no gradient; the target generator plants a block and out-of-range values
    inv = ~o["valid"]
    assert int(inv.sum()) > 4 and int((t == Q.IGNORE).sum()) > 0 and int(((t < 0) | (t >= N)).sum()) >= 4 * t.shape[0]
    assert float(o["loss"][inv].abs().max()) == 0.0 and float(o["g"][inv].abs().max()) == 0.0 and float(o["ds"][inv].abs().max()) == 0.0


@pytest.mark.parametrize("name", Q.SHARE_CASES)
def test_labels_are_decided_on_half_the_pixels(name):
    """From the reference alone (it does not depend on the scale: margin and bound are both linear in it)."""
    shares = []
    for ls in (10.0, 30.0):
        _, r, o, _ = _ref(name, ls)
        shares.append(float(Q.decided(r, o).double().mean()))
    print(name, shares)
    assert min(shares) >= 0.5


@pytest.mark.parametrize("ls", (10.0, 30.0))
def test_emulated_kernel_is_inside_the_bounds(ls):
    for name in SMALL:
        (q, k, v, E, ks, heads), r, o, t = _ref(name, ls)
        N = E.shape[0]
        z, nrm = R.emulate(q, k, v, E, ks, heads, ls)
        loss, labels, g, ds = Q.emulate_objective(z, nrm, ls, t)
        R.check(loss, o["loss"], Q.loss_bound(r, o), f"emulated loss {name}")
        Q.check_labels(labels, r, o, f"emulated labels {name}")
        R.check(g[..., :N], o["g"], Q.g_bound(r, o), f"emulated g' {name}")
        assert float(g[..., N:].abs().max()) == 0.0 and g.shape[-1] == Q.gc_of(N)
        R.check(ds, o["ds"], Q.ds_bound(r, o), f"emulated ds {name}")


def test_planted_defects_leave_the_bounds():
    name, ls = "e_patch14_n21", 10.0
    (q, k, v, E, ks, heads), r, o, t = _ref(name, ls)
    N = E.shape[0]
    z, nrm = R.emulate(q, k, v, E, ks, heads, ls)
    nvalid = int(o["valid"].sum())
    # g' not multiplied by 1 / norm.  Input: the features of the case have norms ~ sqrt(C) * 0.3, far from 1
    _, _, g, _ = Q.emulate_objective(z, nrm, ls, t, no_inv=True)
    assert R.outside(g[..., :N], o["g"], Q.g_bound(r, o)) > 0.5 * nvalid * N
    # ds on the scaled cosines: a factor s = 10
    _, _, _, ds = Q.emulate_objective(z, nrm, ls, t, ds_on_scaled=True)
    assert R.outside(ds, o["ds"], Q.ds_bound(r, o)) > 0.9 * nvalid
    # the onehot subtracted on an ignored pixel: every ignored pixel's row is softmax - onehot(0) instead of zero
    _, _, g, ds = Q.emulate_objective(z, nrm, ls, t, onehot_on_ignored=True)
    bad = (~((g[..., :N] - o["g"]).abs() <= Q.g_bound(r, o))).any(dim=3)
    assert bool(bad[~o["valid"]].all()) and not bool(bad[o["valid"]].any())
    assert R.outside(ds, o["ds"], Q.ds_bound(r, o)) >= 0.9 * int((~o["valid"]).sum())
    # a non-zero pad channel
    _, _, g, _ = Q.emulate_objective(z, nrm, ls, t, pad_value=2.0 ** -20)
    assert float(g[..., N:].abs().max()) > 0.0


def test_zero_norm_row_is_zero_and_keeping_it_leaves_the_bound():
    """Input: a block of zero features as wide as the window plus one (cosine_reference's zero_block): loss ln N, g' and ds exactly 0."""
    name, ls, blk = "e_patch14_n21", 10.0, (0, 6, 0, 6)
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    (q, k, v, E, ks, heads), r, o, t = _ref(name, ls, zero_block=blk)
    m = R.sees_only(blk, h, w, ks).repeat_interleave(dy, 0).repeat_interleave(dx, 1)
    mv = m.unsqueeze(0) & o["valid"]
    assert int(mv.sum()) >= dy * dx // 2
    assert float((o["loss"][mv] - math.log(N)).abs().max()) <= 1e-12
    assert float(o["g"][m.unsqueeze(0).expand_as(o["valid"])].abs().max()) == 0.0 and float(o["ds"][mv].abs().max()) == 0.0
    assert float(Q.g_bound(r, o)[mv].max()) == 0.0            # exact zero is asked for there
    z, nrm = R.emulate(q, k, v, E, ks, heads, ls)
    loss, _, g, ds = Q.emulate_objective(z, nrm, ls, t)
    R.check(g[..., :N], o["g"], Q.g_bound(r, o), "zero block g'")
    R.check(loss, o["loss"], Q.loss_bound(r, o), "zero block loss")
    _, _, bad, _ = Q.emulate_objective(z, nrm, ls, t, keep_zero_norm=True)
    assert R.outside(bad[..., :N], o["g"], Q.g_bound(r, o)) >= int(mv.sum()) * N
    # the autograd of the definition agrees: the zero-feature pixels contribute nothing to dE
    _, dE, _ = Q.autograd_reference(r["f"], E, ls, t)
    _, dE_wo, _ = Q.autograd_reference(r["f"], E, ls, torch.where(m.unsqueeze(0), torch.full_like(t, Q.IGNORE), t))
    assert _rel(dE, dE_wo) <= 1e-12


def test_composed_objective_has_the_same_contract():
    """ops.cosine_objective_from_features on the fp64 reference's feature map (CPU, fp32 torch ops): inside the same bounds, zero rows where
    the feature is zero or the pixel is ignored."""
    from naf_amd import ops
    name, ls, blk = "e_patch14_n21", 10.0, (0, 6, 0, 6)
    B, heads, Dv, (h, w), (dy, dx), ks, N = R.CASES[name]
    (q, k, v, E, ks, heads), r, o, t = _ref(name, ls, zero_block=blk)
    loss, labels, g, ds = ops.cosine_objective_from_features(r["f"].float(), ops.normalize_embeddings(E), ls, t, Q.IGNORE, want_loss=True,
                                                             want_labels=True, want_dlogits=True, want_dscale=True)
    R.check(loss, o["loss"], Q.loss_bound(r, o), "composed loss")
    Q.check_labels(labels, r, o, "composed labels")
    assert g.dtype == torch.bfloat16 and g.shape[-1] == ops.head_dlogits_channels(N) == Q.gc_of(N) and labels.dtype == torch.uint8
    R.check(g[..., :N], o["g"], Q.g_bound(r, o), "composed g'")
    R.check(ds, o["ds"], Q.ds_bound(r, o), "composed ds")
    m = R.sees_only(blk, h, w, ks).repeat_interleave(dy, 0).repeat_interleave(dx, 1).unsqueeze(0)
    assert float(g[..., N:].float().abs().max()) == 0.0 and float(g[m.expand(B, -1, -1)].float().abs().max()) == 0.0
    s_t = torch.tensor([ls])
    again = ops.cosine_objective_from_features(r["f"].float(), ops.normalize_embeddings(E), s_t, t, Q.IGNORE, want_loss=True, want_dlogits=True)
    assert torch.equal(again[0], loss) and torch.equal(again[2], g) and again[1] is None and again[3] is None


# ---- the host-side surface --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from naf_amd import _lib
    return _lib.load()


def _select(name_or_geom, N=None):
    from naf_amd import ops
    B, heads, dv, (h, w), (dy, dx), ks, n = R.CASES[name_or_geom] if isinstance(name_or_geom, str) else name_or_geom
    qp = torch.empty((B, h * dy, w * dx, heads, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    return ops.xna_cos_ce_select(qp, (h, w), dv, N or n, ks)


def test_select_grants_the_gpu_case_list_and_refuses_the_rest(lib):
    from naf_amd import _lib, ops
    assert all(_select(n) == "fused" for n in Q.GPU_CASES), [n for n in Q.GPU_CASES if _select(n) != "fused"]
    served = {(ks, nct) for ks in R.WINDOWS for nct, n in ((2, 21), (4, 40), (10, 151), (16, 256))
              if _select((1, 2, 32, (16, 16), (1, 16), ks, n)) == "fused"}
    # the pairs behind G1 (window 7) and the reference's probing point (window 9), N = 21 and 151
    assert {(7, 2), (7, 10), (9, 2), (9, 10)} <= served
    assert {(ks, nct) for ks in R.WINDOWS for nct in (2, 4, 10, 16)} - served == {(13, 10), (13, 16), (15, 10), (15, 16)}
    assert _select((1, 2, 32, (16, 16), (1, 16), 13, 151)) == "composed" and "window 13" in _lib.last_error()
    assert {R.NCT_OF(R.CASES[n][6]) for n in Q.GPU_CASES} == {2, 4, 10, 16}
    qp = torch.empty((1, 64, 64, 4, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    assert ops.xna_cos_ce_select(qp, (28, 28), 96, 21, 7) == "composed" and "integer ratio" in _lib.last_error()
    assert ops.xna_cos_ce_select(qp, (8, 8), 96, 21, 7, value_dtype=torch.float16) == "composed"
    assert ops.xna_cos_ce_select(qp, (8, 8), 24, 21, 7) == "composed" and "multiple of 16" in _lib.last_error()


def test_c_entry_validates_its_arguments(lib):
    """naf_xna_cos_ce_select on hand-filled structs with host pointers (nothing is dereferenced): the cosine entry's checks plus the head
    objective's for the new operands; naf_xna_cos_ce_fwd refuses the same before any launch."""
    from naf_amd import _lib

    def args(cos=None, **kw):
        a = _lib.XnaCosCEArgs()
        c = a.cos
        c.q = c.k_lr = c.pv_lr = c.v_lr = 4096
        c.B, c.heads, c.Ho, c.Wo, c.h, c.w, c.Dq, c.Dv, c.N, c.ky, c.kx = 1, 2, 128, 128, 8, 8, 64, 32, 21, 7, 7
        c.logit_scale = 1.0
        c.q_stride = _lib.I64x4(128 * 128 * 128, 64, 128 * 128, 128)
        c.k_stride = _lib.I64x4(8 * 8 * 128, 64, 8 * 128, 128)
        c.pv_stride = _lib.I64x4(2 * 8 * 8 * 32, 8 * 8 * 32, 8 * 32, 32)
        c.v_stride = _lib.I64x4(8 * 8 * 64, 32, 8 * 64, 64)
        a.target = a.loss = a.dlogits = a.dscale = 4096
        a.dlogits_channels = 32
        a.t_stride = a.loss_stride = a.dscale_stride = _lib.I64x3(128 * 128, 128, 1)
        a.dlogits_stride = _lib.I64x3(128 * 128 * 32, 128 * 32, 32)
        for k_, v_ in (cos or {}).items():
            setattr(c, k_, v_)
        for k_, v_ in kw.items():
            setattr(a, k_, v_)
        return a

    assert lib.naf_xna_cos_ce_select(C.byref(args())) == _lib.XNA_HEAD_FUSED           # cos.out is NULL here
    assert lib.naf_xna_cos_ce_select(C.byref(args(labels=4096, labels_stride=_lib.I64x3(128 * 128, 128, 1), logit_scale_ptr=4096))) == _lib.XNA_HEAD_FUSED
    assert lib.naf_xna_cos_ce_select(C.byref(args(target=None, loss=None, dlogits=None, dscale=None, labels=4096))) == _lib.XNA_HEAD_FUSED
    for bad in (dict(target=None), dict(target=None, loss=None, dlogits=None), dict(target=None, loss=None, dlogits=None, dscale=None),
                dict(dlogits_channels=28), dict(dlogits_channels=16), dict(dlogits_channels=264), dict(reserved=1), dict(loss=4098),
                dict(logit_scale_ptr=4097), dict(dlogits_stride=_lib.I64x3(128 * 128 * 32, 128 * 32, 24)), dict(cos=dict(v_lr=None)),
                dict(cos=dict(N=0)), dict(cos=dict(N=257)), dict(cos=dict(logit_scale=float("nan"))), dict(cos=dict(ky=8, kx=8))):
        assert lib.naf_xna_cos_ce_select(C.byref(args(**bad))) == -1, bad
        assert lib.naf_xna_cos_ce_fwd(C.byref(args(**bad)), None) == 1, bad
    assert lib.naf_xna_cos_ce_select(C.byref(args(dlogits=4104))) == -2 and "aligned" in _lib.last_error()
    assert lib.naf_xna_cos_ce_select(C.byref(args(dlogits_stride=_lib.I64x3(128 * 128 * 36, 128 * 36, 36)))) == -2
    assert lib.naf_xna_cos_ce_select(C.byref(args(cos=dict(ky=13, kx=13, N=151, h=16, w=16, Ho=256, Wo=256, pv_stride=_lib.I64x4(2 * 16 * 16 * 160, 16 * 16 * 160, 16 * 160, 160)),
                                                   dlogits_channels=192, dlogits_stride=_lib.I64x3(128 * 128 * 192, 128 * 192, 192)))) == -2
    assert "window 13" in _lib.last_error()


def test_header_declares_and_library_exports_the_entries(lib):
    from naf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    raw = C.CDLL(os.path.join(ROOT, "naf_amd", "csrc", "libnaf_hip.so"))
    for sym in ("naf_xna_cos_ce_select", "naf_xna_cos_ce_fwd"):
        assert f"int {sym}(const naf_xna_cos_ce_args* a" in txt
        assert getattr(raw, sym) is not None and sym in _lib.SIGNATURES


def test_struct_layout_matches_the_header(tmp_path):
    from naf_amd import _lib
    fields = ["cos", "target", "loss", "labels", "dlogits", "dscale", "logit_scale_ptr", "ignore_index", "dlogits_channels", "reserved", "t_stride",
              "loss_stride", "labels_stride", "dlogits_stride", "dscale_stride"]
    body = ('printf("%zu %zu", sizeof(naf_xna_cos_ce_args), sizeof(naf_xna_cos_args));' +
            "".join(f'printf(" %zu", offsetof(naf_xna_cos_ce_args, {f}));' for f in fields))
    src = tmp_path / "layout.c"
    src.write_text('#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.XnaCosCEArgs), C.sizeof(_lib.XnaCosArgs)] + [getattr(_lib.XnaCosCEArgs, f).offset for f in fields]


def test_objective_calls_are_refused_before_any_device_work():
    """Every new refusal on CPU tensors (they come before the 'runs only on a ROCm device' error, so nothing was launched), and the old
    ones still raised without ``loss=``."""
    from naf_amd import NAF
    m = NAF(kernel_size=7).eval()
    img, ft = torch.zeros(1, 3, 128, 128), torch.zeros(1, 128, 8, 8, dtype=torch.bfloat16)
    E = torch.randn(5, 128)
    t = torch.zeros(1, 128, 128, dtype=torch.long)
    call = lambda **kw: m(img, ft, (128, 128), **{"head": E, "cosine": True, "target": t, "loss": "ce", **kw})
    with pytest.raises(ValueError, match="loss must be None or 'ce'"):
        call(loss="mse")
    with pytest.raises(ValueError, match="needs target"):
        call(target=None)
    with pytest.raises(ValueError, match="cosine=True as well"):
        call(cosine=False)
    with pytest.raises(ValueError, match="cosine=True as well"):
        m(img, ft, (128, 128), loss="ce")
    with pytest.raises(ValueError, match="return_norms"):
        call(return_norms=True)
    with pytest.raises(ValueError, match="confusion"):
        call(confusion=True)
    for s in (0.0, -2.0):
        with pytest.raises(ValueError, match="logit_scale > 0"):
            call(predict=True, logit_scale=s)
    with pytest.raises(ValueError, match="reduction"):
        call(reduction="avg")
    with pytest.raises(ValueError, match="1-element float32"):
        call(logit_scale=torch.ones(2))
    with pytest.raises(ValueError, match="finite"):
        call(logit_scale=float("inf"))
    with pytest.raises(TypeError, match="integer tensor"):
        call(target=t.float())
    with pytest.raises(ValueError, match=r"\[B, Ho, Wo\]"):
        call(target=t[:, :64])
    with pytest.raises(ValueError, match="no bias"):
        call(head=(E, torch.zeros(5)))
    with pytest.raises(ValueError, match="cosine_path"):
        call(cosine_path="quick")
    for ok in (dict(), dict(predict=True), dict(logit_scale=torch.ones(1, requires_grad=True)), dict(reduction="none"), dict(logit_scale=-1.0)):
        with pytest.raises(RuntimeError, match="ROCm device"):      # a valid call gets as far as the device check, and no further
            call(**ok)
    # without loss=: what was refused is refused as before
    with pytest.raises(ValueError, match="confusion"):
        call(loss=None)
    with pytest.raises(ValueError, match="needs logit_scale > 0"):
        call(loss=None, target=None, predict=True, logit_scale=0.0)
    with pytest.raises(RuntimeError, match="ROCm device"):
        call(loss=None, target=None)
