"""CPU tests of the frame preparation (``naf_amd.prepare_views`` / naf_image_prep): the yardstick of the GPU tests held against itself
(tests/image_prep_reference.py: ``literal32`` against ``exact`` within the blend bound, ATen's own CPU kernels against ``exact`` within blend +
coordinate term, on every GPU case), the recipes' geometry against the reference's formulas, every limit the library names, and the header
against its ctypes mirror.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_prep_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(built_lib):
    from naf_amd import _lib
    return _lib.load()


# ---- A. the yardstick against itself -----------------------------------------------------------------------------------------------------
def test_the_rounding_count_is_the_documented_one():
    import naf_amd
    full = R.view_spec(naf_amd.PrepView((12, 10), "bilinear", R.BACKBONE_MEAN, R.BACKBONE_STD, then=((5, 14), "bicubic")), 7, 9)
    assert R.roundings(torch.uint8, full) == 1 + 6 + 2 + 24 == 33
    assert R.roundings(torch.float32, full) == 32
    assert R.roundings(torch.float32, R.view_spec(naf_amd.PrepView(), 7, 9)) == 0
    assert R.roundings(torch.uint8, R.view_spec(naf_amd.PrepView(mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD), 7, 9)) == 3


@pytest.mark.parametrize("name", R.CASES)
def test_literal32_is_within_the_blend_bound_of_exact(name):
    src = R.source(name)
    for k, (spec, (lit, value, S, _, wterm)) in enumerate(zip(R.specs(name), R.reference(name))):
        assert lit.dtype == spec[-1] and tuple(lit.shape) == value.shape == (value.shape[0], 3, *spec[4])
        ratio, err, bound = R.check_against_exact(lit, src.dtype, spec, value, S, wterm)
        print(f"{name}[{k}]: r = {R.roundings(src.dtype, spec)}, max |literal32 - exact| = {err / R.U:.2f} x 2^-24, "
              f"largest bound {bound / R.U:.1f} x 2^-24, worst err / bound {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("name", R.CASES)
def test_atens_cpu_kernels_are_within_blend_and_coordinate_term_of_exact(name):
    """The stated semantics are ATen's: F.interpolate, subtract and divide on the CPU against ``exact``."""
    src = R.source(name)
    for k, (spec, (_, value, S, coord, wterm)) in enumerate(zip(R.specs(name), R.reference(name))):
        got = R.torch_composition(src, spec)
        ratio, err, bound = R.check_against_exact(got, src.dtype, spec, value, S, wterm, extra=coord)
        print(f"{name}[{k}]: max |torch - exact| = {err / R.U:.1f} x 2^-24, coordinate term up to {float(np.max(coord)) / R.U:.1f} x 2^-24, "
              f"worst err / bound {ratio:.3f}")
        assert ratio <= 1.0


def test_equal_size_and_none_views_return_the_source_bits():
    import naf_amd
    src = R._f32((2, 3, 9, 13), 21)
    for v in (naf_amd.PrepView(), naf_amd.PrepView((9, 13), "bilinear"), naf_amd.PrepView((9, 13), "bicubic"),
              naf_amd.PrepView((9, 13), "bilinear", then=((9, 13), "bicubic")), naf_amd.PrepView(then=((9, 13), "bilinear"))):
        assert torch.equal(R.literal32(src, R.view_spec(v, 9, 13)), src), v
    flipped = R.literal32(src, R.view_spec(naf_amd.PrepView(), 9, 13), hflip=True)
    assert torch.equal(flipped, torch.flip(src, dims=[-1]))


def test_uint8_is_exactly_u_over_255():
    import naf_amd
    u = torch.arange(256, dtype=torch.uint8).repeat(3).view(3, 16, 16).permute(1, 2, 0).contiguous()      # [16, 16, 3], every byte value
    want = (u.permute(2, 0, 1)[None].double() / 255).float()                                              # fp64 quotient rounded once
    for v in (naf_amd.PrepView(), naf_amd.PrepView((16, 16), "bicubic")):
        got = R.literal32(u, R.view_spec(v, 16, 16))
        assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(want, u.permute(2, 0, 1)[None].float().div(255))                                   # ToTensor on the host


# ---- B. the recipes hold the reference's geometry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [14, 16])
@pytest.mark.parametrize("ups_factor", [1, 8])
def test_davis_frame_views_geometry(ps, ups_factor):
    """evaluation/eval_video_seg.py:579-595: size=[v // ps * ps for v in frame], hr_size=[v * ups_factor for v in lr_feats.shape[-2:]]."""
    import naf_amd
    frame = (480, 854)
    views, lr_grid, hr_size = naf_amd.davis_frame_views(frame, ps, ups_factor, R.BACKBONE_MEAN, R.BACKBONE_STD)
    first = tuple(v // ps * ps for v in frame)
    assert lr_grid == tuple(v // ps for v in first) and hr_size == tuple(v * ups_factor for v in lr_grid)
    assert first == {14: (476, 854 // 14 * 14), 16: (480, 848)}[ps]
    bck, ups = views
    assert (bck.size, bck.mode, bck.then, bck.dtype) == (first, "bilinear", None, torch.float32)
    assert tuple(bck.mean) == R.BACKBONE_MEAN and tuple(bck.std) == R.BACKBONE_STD
    assert (ups.size, ups.mode, ups.then) == (first, "bilinear", (hr_size, "bicubic"))
    assert tuple(ups.mean) == R.IMAGENET_MEAN and tuple(ups.std) == R.IMAGENET_STD


@pytest.mark.parametrize("img,ps", [(512, 16), (448, 14)])
def test_training_views_geometry(img, ps):
    """train.py:115-126 and utils/training.py:44-47 at the fixed down factor 0.5."""
    import naf_amd
    hr_grid = (img // ps, img // ps)
    lr = naf_amd.lr_image_size(img, img, 0.5, ps)
    assert lr == (ps * round(img * 0.5 / ps),) * 2 == {16: (256, 256), 14: (224, 224)}[ps]
    bck, low, ups = naf_amd.training_views(img, hr_grid, lr, R.BACKBONE_MEAN, R.BACKBONE_STD)
    assert (bck.size, bck.mode, bck.then) == ((img, img), "bilinear", None)
    assert (low.size, low.mode, low.then) == ((img, img), "bilinear", (lr, "bilinear"))
    assert tuple(low.mean) == tuple(bck.mean) == R.BACKBONE_MEAN and tuple(low.std) == tuple(bck.std) == R.BACKBONE_STD
    want = tuple(min(224, v * 4) for v in hr_grid)
    assert want == {16: (128, 128), 14: (128, 128)}[ps]
    assert (ups.size, ups.mode, ups.then) == ((img, img), "bilinear", (want, "bilinear"))
    assert tuple(ups.mean) == R.IMAGENET_MEAN and tuple(ups.std) == R.IMAGENET_STD
    capped = naf_amd.training_views(1024, (64, 60), 512, R.BACKBONE_MEAN, R.BACKBONE_STD)[2]
    assert capped.then == ((224, 224), "bilinear")
    probe = naf_amd.probing_views(R.BACKBONE_MEAN, R.BACKBONE_STD)
    assert [(v.size, v.mode, v.then) for v in probe] == [(None, None, None)] * 2
    assert tuple(probe[0].mean) == R.BACKBONE_MEAN and tuple(probe[1].mean) == R.IMAGENET_MEAN and tuple(probe[1].std) == R.IMAGENET_STD


def test_lr_image_size_is_round_to_nearest_multiple():
    import naf_amd

    def ref(value, multiple):
        return multiple * round(value / multiple)

    for H, W, factor, ps in ((512, 512, 0.25, 16), (512, 512, 0.5, 16), (512, 512, 0.6, 16), (448, 448, 0.25, 14), (448, 448, 0.5, 14),
                             (448, 448, 0.6, 14), (480, 854, 0.6, 16), (80, 48, 0.5, 16)):
        assert naf_amd.lr_image_size(H, W, factor, ps) == (ref(H * factor, ps), ref(W * factor, ps))
    assert naf_amd.lr_image_size(512, 512, 0.6, 16) == (304, 304)             # 19.2 -> 19
    assert naf_amd.lr_image_size(448, 448, 0.6, 14) == (266, 266)             # 19.2 -> 19
    assert naf_amd.lr_image_size(80, 48, 0.5, 16) == (32, 32)                 # 2.5 -> 2 and 1.5 -> 2: halves go to the even multiple


# ---- C. the C ABI's limits ---------------------------------------------------------------------------------------------------------------
def _args(n_views=2, B=1, H=480, W=854, src_dtype=3, **first):
    from naf_amd import _lib
    a = _lib.ImagePrepArgs()
    a.src_dtype, a.B, a.H, a.W, a.n_views = src_dtype, B, H, W, n_views
    for i in range(min(max(n_views, 0), _lib.IMAGE_PREP_MAX_VIEWS)):
        v = a.view[i]
        v.out_dtype, v.h1, v.w1, v.mode1, v.normalise, v.h2, v.w2, v.mode2 = _lib.NAF_F32, 480, 848, _lib.PREP_BILINEAR, 1, 240, 424, _lib.PREP_BICUBIC
        v.mean, v.std = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25)
    for k, val in first.items():
        setattr(a.view[0], k, val)
    return a


def test_select_accepts_and_refuses_at_each_limit(lib):
    from naf_amd import _lib
    sel = lambda a: (lib.naf_image_prep_select(C.byref(a)), _lib.last_error())   # noqa: E731
    assert lib.naf_image_prep_select(None) == 1
    assert sel(_args())[0] == 0
    assert sel(_args(n_views=1))[0] == 0 and sel(_args(n_views=4))[0] == 0
    assert sel(_args(n_views=1, H=1, W=1, h1=1, w1=1, h2=1, w2=1))[0] == 0
    assert sel(_args(n_views=1, H=16384, W=16384, h1=16384, w1=16384, h2=16384, w2=16384))[0] == 0
    assert sel(_args(B=7, h2=16384, w2=16384))[0] == 0                        # 7 * 2^28 pixels: below 2^31
    rc, msg = sel(_args(n_views=5))
    assert rc == 2 and "1 <= views <= 4" in msg
    rc, msg = sel(_args(n_views=0))
    assert rc == 1 and "1 <= views <= 4" in msg
    for kw in (dict(H=16385), dict(W=16385), dict(h1=16385), dict(w1=16385), dict(h2=16385), dict(w2=16385)):
        rc, msg = sel(_args(**kw))
        assert rc == 2 and "every size <= 16384" in msg, (kw, msg)
    for kw in (dict(B=0), dict(H=0), dict(W=-2), dict(h1=0), dict(w1=0), dict(h2=0), dict(w2=-1)):
        rc, msg = sel(_args(**kw))
        assert rc == 1 and "at least 1" in msg, (kw, msg)
    rc, msg = sel(_args(B=8, h2=16384, w2=16384))
    assert rc == 2 and "below 2^31 per view" in msg
    for kw in (dict(mode1=_lib.PREP_NONE), dict(mode2=_lib.PREP_NONE), dict(mode1=_lib.PREP_NONE, h1=480, w1=853)):
        rc, msg = sel(_args(**kw))
        assert rc == 1 and "mode none requires equal sizes" in msg, (kw, msg)
    assert sel(_args(mode1=_lib.PREP_NONE, h1=480, w1=854))[0] == 0 and sel(_args(mode2=_lib.PREP_NONE, h2=480, w2=848))[0] == 0
    for c in range(3):
        std = [0.25, 0.25, 0.25]
        std[c] = 0.0
        rc, msg = sel(_args(std=(C.c_float * 3)(*std)))
        assert rc == 1 and "std != 0" in msg
        assert sel(_args(std=(C.c_float * 3)(*std), normalise=0))[0] == 0      # the statistics of a view that does not normalise are not read
    rc, msg = sel(_args(mean=(C.c_float * 3)(0.5, float("nan"), 0.5)))
    assert rc == 1 and "NaN" in msg
    for kw, named in ((dict(src_dtype=2), "src_dtype"), (dict(src_dtype=4), "src_dtype"), (dict(out_dtype=2), "out_dtype"), (dict(out_dtype=3), "out_dtype"),
                      (dict(mode1=3), "mode"), (dict(mode2=-1), "mode"), (dict(normalise=2), "normalise")):
        rc, msg = sel(_args(**kw))
        assert rc == 1 and named in msg, (kw, msg)
    for dt in (_lib.NAF_BF16, _lib.NAF_F32, _lib.IMAGE_PREP_U8):
        assert sel(_args(src_dtype=dt))[0] == 0
    a = _args()
    a.hflip = 2
    assert sel(a)[0] == 1 and "hflip" in _lib.last_error()
    a = _args()
    a.reserved[1] = 1
    assert sel(a)[0] == 1 and "reserved" in _lib.last_error()
    a = _args()
    a.view[1].reserved[0] = 7
    assert sel(a)[0] == 1 and "reserved" in _lib.last_error()
    a = _args(n_views=1)
    a.view[1].h1 = -5                                                          # a view beyond n_views is not read
    assert sel(a)[0] == 0


def test_the_call_refuses_bad_pointers_before_any_device_work(lib):
    from naf_amd import _lib
    a = _args(src_dtype=_lib.NAF_F32)
    assert lib.naf_image_prep(C.byref(a), None) == 1 and "NULL source" in _lib.last_error()
    a.src = 4096
    assert lib.naf_image_prep(C.byref(a), None) == 1 and "NULL output" in _lib.last_error()
    a.view[0].out, a.view[1].out = 4096, 4098
    assert lib.naf_image_prep(C.byref(a), None) == 1 and "view 1" in _lib.last_error() and "aligned" in _lib.last_error()
    a.view[1].out, a.src = 4096, 4098
    assert lib.naf_image_prep(C.byref(a), None) == 1 and "source must be aligned" in _lib.last_error()
    a.src_dtype, a.src = _lib.NAF_BF16, 4097
    assert lib.naf_image_prep(C.byref(a), None) == 1 and "source must be aligned" in _lib.last_error()
    a.src_dtype, a.view[0].out_dtype, a.view[0].out = _lib.IMAGE_PREP_U8, _lib.NAF_BF16, 4097
    assert lib.naf_image_prep(C.byref(a), None) == 1 and "view 0" in _lib.last_error() and "aligned" in _lib.last_error()
    a.n_views = 5
    assert lib.naf_image_prep(C.byref(a), None) == 2


def test_header_and_mirror_agree(lib):
    import subprocess
    import tempfile
    from naf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert int(re.search(r"#define\s+NAF_HIP_VERSION\s+(\d+)", txt).group(1)) == _lib.HEADER_VERSION == lib.naf_version()
    for name, value in (("MAX_VIEWS", _lib.IMAGE_PREP_MAX_VIEWS), ("MAX_SIZE", _lib.IMAGE_PREP_MAX_SIZE), ("U8", _lib.IMAGE_PREP_U8)):
        assert int(re.search(rf"#define\s+NAF_IMAGE_PREP_{name}\s+(\d+)", txt).group(1)) == value
    modes = re.search(r"enum naf_prep_mode \{(.*?)\}", txt, re.S).group(1)
    assert [m.strip() for m in modes.split(",")] == ["NAF_PREP_NONE = 0", "NAF_PREP_BILINEAR = 1", "NAF_PREP_BICUBIC = 2"]
    assert (_lib.PREP_NONE, _lib.PREP_BILINEAR, _lib.PREP_BICUBIC) == (0, 1, 2) and _lib.IMAGE_PREP_U8 not in (_lib.NAF_BF16, _lib.NAF_F32, _lib.NAF_F16)
    for cname, ct in (("naf_image_prep_view", _lib.ImagePrepView), ("naf_image_prep_args", _lib.ImagePrepArgs)):
        body = re.search(rf"typedef struct {cname} \{{(.*?)\}} {cname};", txt, re.S).group(1)
        names = [n.split("[")[0] for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in
                 re.sub(r"^\s*(const\s+)?\w+\s*\**", "", decl.strip()).replace(" ", "").split(",") if n]
        assert names == [f[0] for f in ct._fields_], cname
    assert C.sizeof(_lib.ImagePrepView) == 8 + 32 + 8 * 4 + 6 * 4 + 8 == 104
    assert C.sizeof(_lib.ImagePrepArgs) == 8 + 32 + 8 * 4 + 4 * 104 == 488
    src = ('#include "naf_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(naf_image_prep_view), '
           'sizeof(naf_image_prep_args), offsetof(naf_image_prep_view, mean), offsetof(naf_image_prep_args, n_views), '
           'offsetof(naf_image_prep_args, view));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        sizes = [int(v) for v in subprocess.check_output([os.path.join(d, "p")]).split()]
    assert sizes == [C.sizeof(_lib.ImagePrepView), C.sizeof(_lib.ImagePrepArgs), _lib.ImagePrepView.mean.offset, _lib.ImagePrepArgs.n_views.offset,
                     _lib.ImagePrepArgs.view.offset]
    assert {"naf_image_prep_select", "naf_image_prep"} <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "naf_image_prep_select") and hasattr(raw, "naf_image_prep")


def test_public_names_and_host_checks(lib):
    import naf_amd
    V = naf_amd.PrepView
    assert {"PrepView", "prepare_views", "davis_frame_views", "training_views", "probing_views", "lr_image_size"} <= set(naf_amd.__all__)
    frame, img = R.source("small")[0], R._f32((3, 8, 8), 1)
    stats = dict(mean=R.BACKBONE_MEAN, std=R.BACKBONE_STD)
    with pytest.raises(ValueError, match="std != 0"):
        naf_amd.prepare_views(frame, [V(mean=(0.5, 0.5, 0.5), std=(0.2, 0.0, 0.2))])
    with pytest.raises(ValueError, match="1 <= views <= 4"):
        naf_amd.prepare_views(frame, [])
    with pytest.raises(ValueError, match="1 <= views <= 4"):
        naf_amd.prepare_views(frame, [V()] * 5)
    with pytest.raises(ValueError, match="at least 1"):
        naf_amd.prepare_views(frame, [V((0, 4), "bilinear")])
    with pytest.raises(ValueError, match="every size <= 16384"):
        naf_amd.prepare_views(frame, [V((4, 16385), "bicubic")])
    with pytest.raises(ValueError, match="every size <= 16384"):
        naf_amd.prepare_views(frame, [V(then=((16385, 4), "bicubic"))])
    with pytest.raises(ValueError, match="mode none requires equal sizes"):
        naf_amd.prepare_views(frame, [V((4, 4), None)])
    with pytest.raises(ValueError, match="mode none requires equal sizes"):
        naf_amd.prepare_views(frame, [V(then=((4, 4), None))])
    with pytest.raises(ValueError, match="3 channels"):
        naf_amd.prepare_views(torch.zeros(7, 9, 4, dtype=torch.uint8), [V()])
    with pytest.raises(ValueError, match="3 channels"):
        naf_amd.prepare_views(torch.zeros(1, 4, 7, 9), [V()])
    with pytest.raises(ValueError, match="uint8, float32 or bfloat16"):
        naf_amd.prepare_views(torch.zeros(7, 9, 3, dtype=torch.int32), [V()])
    with pytest.raises(ValueError, match="uint8, float32 or bfloat16"):
        naf_amd.prepare_views(img.double(), [V()])
    with pytest.raises(ValueError, match="'bilinear', 'bicubic' or None"):
        naf_amd.prepare_views(img, [V((4, 4), "nearest")])
    with pytest.raises(ValueError, match="both `mean` and `std`"):
        naf_amd.prepare_views(img, [V(mean=R.BACKBONE_MEAN)])
    with pytest.raises(ValueError, match="three numbers"):
        naf_amd.prepare_views(img, [V(mean=(0.5, 0.5), std=(0.2, 0.2))])
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        naf_amd.prepare_views(img, [V(dtype=torch.float16)])
    with pytest.raises(ValueError, match="PrepView"):
        naf_amd.prepare_views(img, [dict(size=(4, 4))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # a served request on the CPU: no torch fallback
        naf_amd.prepare_views(frame, [V((12, 10), "bilinear", **stats, then=((5, 14), "bicubic"))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        naf_amd.prepare_views(img, naf_amd.probing_views(R.BACKBONE_MEAN, R.BACKBONE_STD), hflip=True)
