"""CPU tests of the peak search (``naf.locate`` / ``ops.xna_cos_peaks`` / ``ops.peaks_topk``): the reference functions against brute-force
loops, the host restatement of the kernel's merge order with planted defects (each test names the input on which the defect shows), the
host-side surface (select, refusals, struct layout) and the compiler's figures of the served instantiations.  Nothing here needs a GPU."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_peak_reference as P  # noqa: E402
import cosine_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the cases tests/test_gpu_cosine_peaks.py runs (cosine_reference.CASES), with the kernel feature each exercises
GPU_CASES = ("a_c128_k7_n21", "b_whole_grid_n1", "c_dv192_n151", "d_dv256_n256", "e_patch14_n21", "f_rows30_n151", "j_k13_n21", "k_k15_n40",
             "l_two_rounds_n21")


def _map(shape, seed, levels=None):
    g = torch.Generator().manual_seed(seed)
    if levels:      # few distinct values: many ties
        return torch.randint(0, levels, shape, generator=g).float() / levels - 0.5
    return torch.rand(shape, generator=g) * 2 - 1


# ---- the reference functions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [None, 3])
def test_cell_peaks_match_the_pixel_loop(levels):
    cos = _map((2, 3, 6, 28), 11, levels)
    cos[0, 0] = 0.0
    for h, w in ((3, 2), (6, 28), (1, 1), (2, 7)):
        peak, where = P.cell_peaks(cos, h, w)
        lp, lw = P.cell_peaks_loop(cos, h, w)
        assert torch.equal(peak, lp) and torch.equal(where, lw) and where.dtype == torch.int32
    assert torch.equal(P.cell_peaks(cos, 3, 2)[1][0, 0], torch.tensor([[0, 14], [56, 70], [112, 126]], dtype=torch.int32))   # ties: the cell's first pixel


def test_ops_definition_is_the_reference():
    from naf_amd import ops
    cos = _map((2, 4, 8, 30), 12, 4)
    peak, where = ops.peaks_from_cosines(cos, (4, 2))
    rp, rw = P.cell_peaks(cos, 4, 2)
    assert torch.equal(peak, rp) and torch.equal(where, rw) and where.dtype == torch.int32
    with pytest.raises(ValueError, match="integer ratio"):
        ops.peaks_from_cosines(cos, (3, 2))


@pytest.mark.parametrize("levels", [None, 2])
def test_topk_reference_matches_the_sorted_list(levels):
    peak = _map((2, 3, 5, 7), 13, levels)
    where = torch.randperm(35, generator=torch.Generator().manual_seed(3)).view(1, 1, 5, 7).expand(2, 3, 5, 7).to(torch.int32) * 3
    for k in (1, 5, 35):
        v, i = P.topk_reference(peak, where, k)
        lv, li = P.topk_loop(peak, where, k)
        assert torch.equal(v, lv) and torch.equal(i, li)


# ---- the kernel's merge order, with planted defects ----------------------------------------------------------
def _emulated(c, ls, h, w, tpw, defect=None):
    return P.emulate(c, ls, h, w, tpw, defect)


def _definition(c, ls, h, w):
    z = (torch.tensor(ls, dtype=torch.float32) * c.float())[None, None]
    peak, where = P.cell_peaks(z, h, w)
    return peak[0, 0], where[0, 0]


@pytest.mark.parametrize("geom", [((8, 8), (16, 16), 2), ((6, 7), (14, 14), 2), ((5, 5), (3, 30), 2), ((14, 13), (1, 16), 2), ((16, 15), (1, 16), 1),
                                   ((7, 8), (32, 16), 2), ((8, 8), (16, 16), 1), ((3, 2), (40, 16), 2)])
@pytest.mark.parametrize("ls", [1.0, -3.5])
def test_merge_order_is_the_definition(geom, ls):
    """Without a defect the emulation equals the definition on random maps, on maps full of ties and on the all-zero map, for the cell
    shapes of the GPU cases (one and two tiles per wave, partial tiles, one-row cells, two and three rounds)."""
    (h, w), (dy, dx), tpw = geom
    for levels in (None, 3, 1):
        c = _map((h * dy, w * dx), 21 + dy, levels) if levels != 1 else torch.zeros(h * dy, w * dx)
        peak, where = _emulated(c, ls, h, w, tpw)
        dp, dw = _definition(c, ls, h, w)
        assert torch.equal(peak, dp) and torch.equal(where, dw)


def _differs(c, ls, h, w, tpw, defect):
    good, bad = _emulated(c, ls, h, w, tpw), _emulated(c, ls, h, w, tpw, defect)
    assert torch.equal(good[0], _definition(c, ls, h, w)[0]) and torch.equal(good[1], _definition(c, ls, h, w)[1])
    return not (torch.equal(good[0], bad[0]) and torch.equal(good[1], bad[1]))


def test_defect_tie_to_the_highest_index():
    """Input: the all-zero map (every pixel ties): the defect reports each cell's last pixel."""
    assert _differs(torch.zeros(32, 32), 1.0, 2, 2, 2, "tie_high")


def test_defect_out_of_cell_lane_counted():
    """Input: 14-pixel cells (two idle lanes per tile), the map rising with x: the neighbouring cell's first pixels beat the cell's own."""
    c = torch.arange(28, dtype=torch.float32).repeat(14, 1) / 28
    assert _differs(c, 1.0, 1, 2, 2, "ghost_lane")


def test_defect_dead_tile_counted():
    """Input: one-row cells (seven of eight waves have no live tile), the map rising with y: the rows below the cell win."""
    c = (torch.arange(4, dtype=torch.float32).view(4, 1) / 4).expand(4, 16).contiguous()
    assert _differs(c, 1.0, 4, 1, 2, "dead_tile")


def test_defect_second_round_replaces_the_first():
    """Input: a 32-row cell (two rounds of sixteen tiles), the maximum in row 0, which round one holds."""
    c = _map((32, 16), 5) * 0.5
    c[0, 3] = 0.9
    assert _differs(c, 1.0, 1, 1, 2, "round_replace")


def test_defect_one_wave_dropped():
    """Input: a 16-row cell, the maximum in row 7, the tile of the last wave."""
    c = _map((16, 16), 6) * 0.5
    c[7, 9] = 0.9
    assert _differs(c, 1.0, 1, 1, 2, "drop_wave")


def test_defect_index_in_cell_coordinates():
    """Input: any map with more than one cell per row: the cell's own coordinates are not the output's."""
    assert _differs(_map((32, 32), 7), 1.0, 2, 2, 2, "cell_coords")


def test_defect_y_and_x_swapped():
    """Input: a map whose maximum is off the diagonal."""
    c = _map((16, 32), 8) * 0.5
    c[3, 20] = 0.9
    assert _differs(c, 1.0, 1, 2, 2, "swap_yx")


def test_defect_maximum_before_scaling():
    """Input: any non-constant map under a negative scale: the maximum of z = s * c is the minimum of c."""
    assert _differs(_map((16, 16), 9), -2.0, 1, 1, 2, "max_before_scale")
    assert not _differs(_map((16, 16), 9), 2.0, 1, 1, 2, "max_before_scale")      # a positive power of two commutes with the maximum


# ---- the host-side surface --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from naf_amd import _lib
    return _lib.load()


def _select(name_or_geom, N=None, **kw):
    from naf_amd import ops
    B, heads, dv, (h, w), (dy, dx), ks, n = R.CASES[name_or_geom] if isinstance(name_or_geom, str) else name_or_geom
    qp = torch.empty((B, h * dy, w * dx, heads, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    return ops.xna_cos_peaks_select(qp, (h, w), dv, N or n, ks, **kw)


def test_select_grants_the_gpu_case_list_and_refuses_the_rest(lib):
    from naf_amd import _lib, ops
    assert all(_select(n) == "fused" for n in GPU_CASES), [n for n in GPU_CASES if _select(n) != "fused"]
    assert {R.NCT_OF(R.CASES[n][6]) for n in GPU_CASES} == {2, 4, 10, 16}
    served = {(ks, nct) for ks in R.WINDOWS for nct, n in ((2, 21), (4, 40), (10, 151), (16, 256))
              if _select((1, 2, 32, (16, 16), (1, 16), ks, n)) == "fused"}
    assert {(ks, nct) for ks in R.WINDOWS for nct in (2, 4, 10, 16)} - served == {(13, 10), (13, 16), (15, 10), (15, 16)}
    assert _select((1, 2, 32, (16, 16), (1, 16), 13, 151)) == "composed" and "window 13" in _lib.last_error()
    qp = torch.empty((1, 64, 64, 4, 64), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
    assert ops.xna_cos_peaks_select(qp, (28, 28), 96, 21, 7) == "composed" and "integer ratio" in _lib.last_error()
    assert ops.xna_cos_peaks_select(qp, (8, 8), 96, 21, 7, value_dtype=torch.float16) == "composed"
    assert ops.xna_cos_peaks_select(qp, (8, 8), 96, 300, 7) == "composed"
    assert ops.xna_cos_peaks_select(qp, (8, 8), 24, 21, 7) == "composed" and "multiple of 16" in _lib.last_error()


def _args(cos=None, **kw):
    from naf_amd import _lib
    a = _lib.XnaCosPeaksArgs()
    c = a.cos
    c.q = c.k_lr = c.pv_lr = c.v_lr = 4096
    c.B, c.heads, c.Ho, c.Wo, c.h, c.w, c.Dq, c.Dv, c.N, c.ky, c.kx = 1, 2, 128, 128, 8, 8, 64, 32, 21, 7, 7
    c.logit_scale = 1.0
    c.q_stride = _lib.I64x4(128 * 128 * 128, 64, 128 * 128, 128)
    c.k_stride = _lib.I64x4(8 * 8 * 128, 64, 8 * 128, 128)
    c.pv_stride = _lib.I64x4(2 * 8 * 8 * 32, 8 * 8 * 32, 8 * 32, 32)
    c.v_stride = _lib.I64x4(8 * 8 * 64, 32, 8 * 64, 64)
    a.peak = a.where = 4096
    a.peak_stride = a.where_stride = _lib.I64x3(8 * 8 * 21, 8 * 21, 21)
    for k_, v_ in (cos or {}).items():
        setattr(c, k_, v_)
    for k_, v_ in kw.items():
        setattr(a, k_, v_)
    return a


def test_c_entry_validates_its_arguments(lib):
    """naf_xna_cos_peaks_select on hand-filled structs with host pointers (nothing is dereferenced): the cosine entry's checks plus the new
    operands'; naf_xna_cos_peaks_fwd refuses the same before any launch."""
    from naf_amd import _lib
    assert lib.naf_xna_cos_peaks_select(C.byref(_args())) == _lib.XNA_HEAD_FUSED           # cos.out is NULL here
    assert lib.naf_xna_cos_peaks_select(C.byref(_args(cos=dict(out=4096, o_stride=_lib.I64x3(128 * 128 * 21, 128 * 21, 21))))) == _lib.XNA_HEAD_FUSED
    assert lib.naf_xna_cos_peaks_select(None) == -1
    for bad in (dict(peak=None), dict(where=None), dict(peak=4098), dict(where=4097), dict(peak_stride=_lib.I64x3(8 * 8 * 20, 8 * 20, 20)),
                dict(where_stride=_lib.I64x3(8 * 8 * 21, 8 * 21, 16)), dict(reserved=(C.c_int64 * 2)(0, 1)), dict(cos=dict(v_lr=None)),
                dict(cos=dict(N=0)), dict(cos=dict(N=257)), dict(cos=dict(logit_scale=float("inf"))), dict(cos=dict(ky=8, kx=8)),
                dict(cos=dict(out=4096, o_stride=_lib.I64x3(128 * 128 * 20, 128 * 20, 20))), dict(cos=dict(Ho=65536, Wo=32768, h=4096, w=2048))):
        assert lib.naf_xna_cos_peaks_select(C.byref(_args(**bad))) == -1, bad
        assert lib.naf_xna_cos_peaks_fwd(C.byref(_args(**bad)), None) == 1, bad
    assert "int32 flat index" in _lib.last_error()
    assert lib.naf_xna_cos_peaks_select(C.byref(_args(cos=dict(ky=13, kx=13, N=151, h=16, w=16, Ho=256, Wo=256,
                                                               pv_stride=_lib.I64x4(2 * 16 * 16 * 160, 16 * 16 * 160, 16 * 160, 160)),
                                                      peak_stride=_lib.I64x3(16 * 16 * 151, 16 * 151, 151), where_stride=_lib.I64x3(16 * 16 * 151, 16 * 151, 151)))) == -2
    assert "window 13" in _lib.last_error()
    assert lib.naf_xna_cos_peaks_select(C.byref(_args(cos=dict(q=4100)))) == -2 and "aligned" in _lib.last_error()


def test_topk_entry_validates_its_arguments(lib):
    from naf_amd import _lib
    st = (C.c_int64 * 2)(35 * 3, 3)
    call = lambda **kw: lib.naf_peaks_topk(*[{**dict(peak=4096, where=4096, values=4096, index=4096, B=2, N=3, n_cells=35, k=5, ps=st, ws=st), **kw}[n]
                                             for n in ("peak", "where", "values", "index", "B", "N", "n_cells", "k", "ps", "ws")], None)
    for bad in (dict(peak=None), dict(index=None), dict(ps=None), dict(k=0), dict(k=36), dict(k=65, n_cells=100), dict(B=0), dict(N=0),
                dict(n_cells=0), dict(ps=(C.c_int64 * 2)(35 * 2, 2))):
        assert call(**bad) == 1, bad
    assert call(k=65, n_cells=100) == 1 and "min(cells, 64)" in _lib.last_error()


def test_header_declares_and_library_exports_the_entries(lib):
    from naf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    raw = C.CDLL(os.path.join(ROOT, "naf_amd", "csrc", "libnaf_hip.so"))
    for sym in ("naf_xna_cos_peaks_select", "naf_xna_cos_peaks_fwd"):
        assert f"int {sym}(const naf_xna_cos_peaks_args* a" in txt
        assert getattr(raw, sym) is not None and sym in _lib.SIGNATURES
    assert "int naf_peaks_topk(const float* peak, const int32_t* where, float* values, int32_t* index" in txt
    assert raw.naf_peaks_topk is not None and "naf_peaks_topk" in _lib.SIGNATURES
    assert "#define NAF_HIP_VERSION 403" in txt and lib.naf_version() == 403


def test_struct_layout_matches_the_header(tmp_path):
    from naf_amd import _lib
    fields = ["cos", "peak", "where", "peak_stride", "where_stride", "reserved"]
    body = ('printf("%zu %zu", sizeof(naf_xna_cos_peaks_args), sizeof(naf_xna_cos_args));' +
            "".join(f'printf(" %zu", offsetof(naf_xna_cos_peaks_args, {f}));' for f in fields))
    src = tmp_path / "layout.c"
    src.write_text('#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.XnaCosPeaksArgs), C.sizeof(_lib.XnaCosArgs)] + [getattr(_lib.XnaCosPeaksArgs, f).offset for f in fields]
    assert _lib.XnaCosPeaksArgs.cos.offset == 0        # naf_xna_cos_args, unchanged, is the first member


def test_calls_are_refused_before_any_device_work():
    """Every refusal on CPU tensors (they come before the 'runs only on a ROCm device' error, so nothing was launched)."""
    from naf_amd import NAF, ops
    m = NAF(kernel_size=7).eval()
    img, ft = torch.zeros(1, 3, 128, 128), torch.zeros(1, 128, 8, 8, dtype=torch.bfloat16)
    E = torch.randn(5, 128)
    call = lambda **kw: m.locate(*[{**dict(image=img, features=ft, size=(128, 128), E=E), **kw}[n] for n in ("image", "features", "size", "E")],
                                 **{k_: v_ for k_, v_ in kw.items() if k_ in ("topk", "logit_scale", "path")})
    with pytest.raises(ValueError, match="path must be"):
        call(path="quick")
    with pytest.raises(ValueError, match="integer ratio"):
        call(size=(100, 128))
    with pytest.raises(ValueError, match="finite"):
        call(logit_scale=float("nan"))
    for k in (0, 65, 2.5):
        with pytest.raises(ValueError, match="topk"):
            call(topk=k)
    with pytest.raises(ValueError, match="topk"):
        m.locate(img, ft[:, :, :3, :3].repeat(1, 1, 1, 1), (96, 96), E, topk=10)      # nine cells
    with pytest.raises(ValueError, match="no bias"):
        call(E=(E, torch.zeros(5)))
    with pytest.raises(ValueError, match="channels"):
        call(E=E[:, :-1])
    with pytest.raises(ValueError, match="expected image"):
        call(features=ft[0])
    for ok in (dict(), dict(topk=64), dict(logit_scale=-1.0), dict(path="fused"), dict(path="composed")):
        with pytest.raises(RuntimeError, match="ROCm device"):      # a valid call gets as far as the device check, and no further
            call(**ok)
    with pytest.raises(TypeError, match="Guidance"):
        m.match(img, ft, torch.zeros(1, 2, dtype=torch.long), img, ft, (128, 128))
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.peaks_topk(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2, dtype=torch.int32), 1)


def test_served_instantiations_have_no_scratch():
    """The compiler's resource report of the library's own instantiations (no -DNAF_XNA_COS_ALL): every pair the peak entry serves is there
    and free of scratch, and so are the cosine and objective instantiations of the same translation units.  Compiles only."""
    import cosine_peaks_time as T
    rows = T.resource_rows(all_pairs=False)
    peaks = {(r["window"], r["nct"]): r for r in rows if r["epilogue"] == "peaks"}
    print({k_: (r["vgprs"], r["scratch"]) for k_, r in sorted(peaks.items())})
    want = {(ks, nct) for ks in R.WINDOWS for nct in (2, 4, 10, 16)} - {(13, 10), (13, 16), (15, 10), (15, 16)}
    assert set(peaks) == want
    assert all(r["scratch"] == 0 for r in rows), [(r["epilogue"], r["window"], r["nct"], r["scratch"]) for r in rows if r["scratch"]]
    assert {(r["window"], r["nct"]) for r in rows if r["epilogue"] == "cosine"} == want
    for (ks, nct) in want:
        assert T.cos_lds(ks, nct) + T.peak_lds(nct) <= 160 * 1024
