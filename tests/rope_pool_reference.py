"""RoPE + query write + key pooling forward (naf_amd/csrc/rope_pool.hip), restated: reference arithmetic with the TABLES as inputs, the exact
construction, the launcher's plan, the argument builders and the case table of tests/test_rope_pool_cpu.py and tests/test_gpu_rope_pool.py.
Plain helper module: no test in it.

Arithmetic (rope_pool.hip:1-16).  Inside a head of Dh channels, channel t < Dh/2 is paired with t + Dh/2; angle index t < Dh/4 reads row y of
tab_y [Ho, 2, Dh/4] (cos then sin), t >= Dh/4 reads column x of tab_x [Wo, 2, Dh/4] at index t - Dh/4:
    o1 = a c - b s        o2 = b c + a s                  (a = x[t], b = x[t + Dh/2])
The query of a pixel is bf16(o).  The key of cell (i, j) is bf16(sum over the window [floor(i Ho/h), ceil((i+1) Ho/h)) x [floor(j Wo/w),
ceil((j+1) Wo/w)) of o, times fl(1 / npix)).  A cell WRITES the queries of its owned range [floor(i Ho/h), floor((i+1) Ho/h)) x [...]: the
owned ranges partition the image, the windows overlap by a row / column where Ho % h != 0.

The exact construction.  Both entries take the tables as arguments, so a test can choose them: integer tables with |cos|, |sin| <= 15 and integer
guidance with |x| <= 8 make every product (<= 120), every fused multiply-add (<= 240, an 8-bit integer: a bf16 number), and every window sum
(<= 33 x 33 x 240 < 2^24) an exactly representable fp32 number in ANY order of accumulation.  The query is then the integer itself and the key is
bf16(fl32(sum * fl32(1 / npix))), which torch restates on the host bit for bit: ``rope_pool_exact``.  With random integer tables that differ from
row to row, column to column, angle index to angle index and between cos and sin, a dense launch is a census of every table index, every
pixel-to-cell assignment, every divisor and every head / channel mapping, compared with ``!=`` at every element.

Float bound of the true-table runs (``float_bounds``), per element, nothing measured.  U = 2^-8 is the unit roundoff of bf16 (input_statistics.U):
round-to-nearest onto 8 significant bits moves v by at most half a spacing, 2^-8 2^floor(log2 |v|) <= 2^-8 |v|, and reaches it (1 + 2^-8 ->
1).  2^-9 |v| is NOT a bound of one bf16 rounding.
    q:  fp32 rotation: fl(b s) and the fma's own rounding, each <= 2^-24 of a value <= |a c| + |b s|: 2^-23 (|a c| + |b s|); then the bf16 store:
        input_statistics.bf16_bound(0, ., stored=|ref|) = SLACK U |ref|.
    k:  the n-term fp32 sum in any order, n 2^-24 sum |o| (Higham 4.4 to first order; |o| <= |a c| + |b s|), the n rotations' own
        2^-23 (|a c| + |b s|) each, times 1 / n: (n + 2) 2^-24 mean(|a c| + |b s|); fl(1 / n) and the product: two fp32 roundings of the result,
        2^-23 |ref|; the bf16 store.
"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_statistics as S  # noqa: E402
import stem_backward_reference as SB  # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
X_MAX, TAB_MAX = 8, 15                      # integer guidance and tables of the exact construction
LDS_TABLE_BUDGET, LDS_MAX = 48 * 1024, 64 * 1024


def tables64(periods, H, W):
    """fp64 ([H, 2, P], [W, 2, P]) cos / sin tables of the oracle's angles."""
    return SB.rope_tables64(periods, H, W)


def integer_tables(Ho, Wo, P, seed):
    """Random integer tables in [-15, 15], fp32 [Ho, 2, P] / [Wo, 2, P]: cos and sin drawn independently."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda L: torch.randint(-TAB_MAX, TAB_MAX + 1, (L, 2, P), generator=g).float()
    return draw(Ho), draw(Wo)


def integer_guidance(shape, seed):
    """Random integers in [-8, 8], fp32 [B, Cq, Ho, Wo]."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-X_MAX, X_MAX + 1, tuple(shape), generator=g).float()


def to5(x, heads):
    """[B, C, H, W] -> dense head-major [B, heads, H, W, D] (same dtype)."""
    B, Cc, H, W = x.shape
    return x.reshape(B, heads, Cc // heads, H, W).permute(0, 1, 3, 4, 2).contiguous()


def nchw(t5):
    """[B, heads, H, W, D] -> [B, heads * D, H, W]."""
    B, n, H, W, D = t5.shape
    return t5.permute(0, 1, 4, 2, 3).reshape(B, n * D, H, W)


def window(i, L, n, floor_end=False):
    """(start, end of the pool window, end of the owned range) of cell i of n over L positions."""
    s, own = (i * L) // n, ((i + 1) * L) // n
    return s, (own if floor_end else -((-(i + 1) * L) // n)), own


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("row_shift_last", "col_shift_last", "col_for_row", "angle_off_by_one", "sin_sign", "halves_swapped", "head_next", "floor_end",
           "neighbour_divisor", "q_whole_window", "cell_decode_swapped", "drop_last_cell", "drop_trip_pixel")


def _cos_sin(ty, tx, Ho, Wo, defect=None):
    """cos, sin [Ho, Wo, Dh/2]: angle index t < Dh/4 from row y of ty, t >= Dh/4 from column x of tx."""
    P = ty.shape[-1]
    row, col = ty[:, None].expand(Ho, Wo, 2, P), tx[None, :].expand(Ho, Wo, 2, P)
    if defect == "col_for_row":                      # the row-angle channels read the column table (at the pixel's column)
        row = col
    c, s = torch.cat([row[:, :, 0], col[:, :, 0]], -1), torch.cat([row[:, :, 1], col[:, :, 1]], -1)
    if defect == "angle_off_by_one":
        c, s = c.roll(-1, -1), s.roll(-1, -1)
    if defect == "sin_sign":
        s = -s
    return c, s


def _rotate(x5, c, s):
    half = x5.shape[-1] // 2
    a, b = x5[..., :half], x5[..., half:]
    o = torch.cat([a * c - b * s, b * c + a * s], -1)
    ab = (a * c).abs() + (b * s).abs()
    return o, torch.cat([ab, (b * c).abs() + (a * s).abs()], -1)


def rope_pool_reference(x, tab_y, tab_x, heads, lr, dtype=F64, defect=None, inv32=False):
    """(q, k, q_abs, k_abs) in ``dtype``, head-major [B, heads, Ho, Wo, Dh] / [B, heads, h, w, Dh], of the logical guidance x [B, Cq, Ho, Wo].
    q_abs = |a c| + |b s| of the element's rotation, k_abs its mean over the window: what the bounds need.  ``inv32``: the divisor is
    fl32(1 / npix) as in the kernel (rope_pool.hip:214), else 1 / npix in ``dtype``.  ``defect``: one of DEFECTS, planted (CPU self-tests); an
    element a defective kernel would not write is 0."""
    assert defect is None or defect in DEFECTS, defect
    B, Cq, Ho, Wo = x.shape
    h, w = lr
    x5 = to5(x.to(dtype), heads)
    if defect == "head_next":
        x5 = x5.roll(-1, 1)
    if defect == "halves_swapped":
        x5 = torch.cat([x5[..., x5.shape[-1] // 2:], x5[..., :x5.shape[-1] // 2]], -1)
    ty, tx = tab_y.to(dtype), tab_x.to(dtype)
    c, s = _cos_sin(ty, tx, Ho, Wo, defect)
    q, q_abs = _rotate(x5, c, s)
    k, k_abs = torch.zeros(B, heads, h, w, Cq // heads, dtype=dtype), torch.zeros(B, heads, h, w, Cq // heads, dtype=dtype)
    wins_y = [window(i, Ho, h, defect == "floor_end") for i in range(h)]
    wins_x = [window(j, Wo, w, defect == "floor_end") for j in range(w)]
    npix = lambda i, j: (wins_y[i][1] - wins_y[i][0]) * (wins_x[j][1] - wins_x[j][0])
    m = min(h, w)
    written = torch.ones(Ho, Wo, dtype=torch.bool)
    for i in range(h):
        for j in range(w):
            (ys, ye, yo), (xs, xe, xo) = wins_y[i], wins_x[j]
            o, oa = q[:, :, ys:ye, xs:xe], q_abs[:, :, ys:ye, xs:xe]
            if defect in ("row_shift_last", "col_shift_last", "drop_trip_pixel") and (i, j) == (0, 0):
                o = o.clone()                       # the LAST pixel of the cell's walk: (ye - 1, xe - 1)
                if defect == "drop_trip_pixel":
                    o[:, :, -1, -1] = 0
                else:
                    ry, rx = (ye, xe - 1) if defect == "row_shift_last" else (ye - 1, xe)      # row y + 1 for y / column x + 1 for x
                    c1, s1 = torch.cat([ty[ry, 0], tx[rx, 0]], -1), torch.cat([ty[ry, 1], tx[rx, 1]], -1)
                    o[:, :, -1, -1] = _rotate(x5[:, :, ye - 1, xe - 1], c1, s1)[0]
                    if ye - 1 < yo and xe - 1 < xo:     # the cell owns the pixel: its query is the shifted one too
                        q = q.clone()
                        q[:, :, ye - 1, xe - 1] = o[:, :, -1, -1]
            n = npix(i, j)
            if defect == "neighbour_divisor":
                n = npix(i, j + 1 if j + 1 < w else j - 1)
            inv = (torch.tensor(1.0, dtype=F32) / n).to(dtype) if inv32 else torch.tensor(1.0, dtype=dtype) / n
            k[:, :, i, j] = o.sum((2, 3)) * inv
            k_abs[:, :, i, j] = oa.sum((2, 3)) / npix(i, j)
            if defect == "cell_decode_swapped" and (i >= m or j >= m):      # the cells a decode with h and w exchanged never reaches
                k[:, :, i, j] = 0
                written[ys:yo, xs:xo] = False
    if not bool(written.all()):
        q = q.clone()
        q[:, :, ~written] = 0
    if defect == "drop_last_cell":                   # the last cell of the launch: the last image's cell (h - 1, w - 1)
        q = q.clone()
        q[-1, :, wins_y[-1][0]:, wins_x[-1][0]:] = 0
        k[-1, :, h - 1, w - 1] = 0
    # "q_whole_window": every cell stores the queries of its whole window.  The pixels two windows share are rotated by the same rows of the same
    # tables in both cells, so both store the same bits: the defect is a benign race and changes no value (guard bands and owned-range
    # arithmetic are what a test can hold it to; tests/test_rope_pool_cpu.py records the count 0).
    return q, k, q_abs, k_abs


def rope_pool_exact(x, tab_y, tab_x, heads, lr, defect=None):
    """The bit-exact bf16 (q, k) of integer guidance and integer tables, head-major.  Asserts the preconditions."""
    for t in (x, tab_y, tab_x):
        assert bool((t.double() == t.double().round()).all()), "integer values only"
    q, k, q_abs, k_abs = rope_pool_reference(x, tab_y, tab_x, heads, lr, F64, defect)
    assert float(q_abs.max()) <= 256, "a query beyond 8 bits is not a bf16 number"
    h, w = lr
    Ho, Wo = x.shape[-2:]
    n = torch.tensor([[(window(i, Ho, h)[1] - window(i, Ho, h)[0]) * (window(j, Wo, w)[1] - window(j, Wo, w)[0]) for j in range(w)] for i in range(h)], dtype=F64)
    assert float((k_abs * n[None, None, :, :, None]).max()) < 2 ** 24, "a window sum beyond 2^24 is not exact in every order"
    q32 = q.float()
    assert torch.equal(q32.double(), q) and torch.equal(q32.to(BF).double(), q)
    # the key as the kernel forms it: fl32(sum) * fl32(1 / npix), rounded to fp32, then to bf16 (the sums are exact integers)
    k32 = rope_pool_reference(x, tab_y, tab_x, heads, lr, F64, defect, inv32=True)[1]          # sum * fl32(1 / npix) in fp64: exact (24 + 24 bits)
    return q32.to(BF), k32.float().to(BF)


def fma32(a, b, c):
    """fl32(a b + c) of fp32 tensors: the product is exact in fp64; the fp64 sum's own rounding is 2^-29 of an fp32 ulp away from the fused result."""
    return (a.double() * b.double() + c.double()).float()


def rope_pool_emulated(x, tab_y, tab_x, heads, lr, nplanes, defect=None):
    """fp32 in the kernel's order: naf_rope_rotate's fused multiply-adds (naf_common.h:157-160), each pixel lane adding its pixels in walk order (pi =
    plane, plane + nplanes, ...), the lanes added in order, times fl32(1 / npix); bf16 stores.  ``defect="row_shift_last"``-style defects are
    planted through the tables by the caller.  Returns (q, k) as fp32 holding bf16 values."""
    B, Cq, Ho, Wo = x.shape
    h, w = lr
    x5 = to5(x.float(), heads)
    half = x5.shape[-1] // 2
    c, s = _cos_sin(tab_y.float(), tab_x.float(), Ho, Wo)
    a, b = x5[..., :half], x5[..., half:]
    o = torch.cat([fma32(a, c, -(b * s)), fma32(b, c, a * s)], -1)
    k = torch.zeros(B, heads, h, w, 2 * half)
    for i in range(h):
        for j in range(w):
            ys, ye, _ = window(i, Ho, h)
            xs, xe, _ = window(j, Wo, w)
            px = o[:, :, ys:ye, xs:xe].reshape(B, heads, -1, 2 * half)
            lanes = []
            for pl in range(min(nplanes, px.shape[2])):
                acc = torch.zeros(B, heads, 2 * half)
                for pi in range(pl, px.shape[2], nplanes):
                    acc = acc + px[:, :, pi]
                lanes.append(acc)
            tot = torch.zeros(B, heads, 2 * half)
            for acc in lanes:
                tot = tot + acc
            k[:, :, i, j] = tot * (torch.tensor(1.0) / px.shape[2])
    return S.bf16r(o), S.bf16r(k)


def float_bounds(q, k, q_abs, k_abs, lr):
    """Per-element bounds of the bf16 q and k of a launch against the fp64 reference fed the same tables (module docstring)."""
    B, n, Ho, Wo, D = q.shape
    h, w = lr
    npix = torch.tensor([[(window(i, Ho, h)[1] - window(i, Ho, h)[0]) * (window(j, Wo, w)[1] - window(j, Wo, w)[0]) for j in range(w)] for i in range(h)], dtype=F64)
    bq = S.bf16_bound(0, q_abs, stored=q.abs()) + 2.0 * S.F32 * q_abs
    bk = S.bf16_bound(0, k_abs, stored=k.abs()) + (npix[None, None, :, :, None] + 2.0) * S.F32 * k_abs + 2.0 * S.F32 * k.abs()
    return bq, bk


def epilogue_key_bound(k, k_abs):
    """naf_stem_conv_keys_fwd's keys against ``rope_pool_reference`` of the layer's own bf16 output: the any-order bound of a 256-term fp32 sum of the
    actual terms, 256 2^-24 mean(|a c| + |b s|) -- the kernel adds the 16 un-rotated values of a row / column first, rotates the 16 sums and adds
    those (stem_conv1x1.hip:74-82): 16 + 2 + 16 + 1 roundings, each relative to a partial sum of the |terms| -- plus the bf16 store."""
    return 256.0 * S.F32 * k_abs + S.bf16_bound(0, k_abs, stored=k.abs())


def first_mismatch(got, want, what):
    """None, or the failure message of an exact comparison of head-major 5-D tensors: first differing (b, head, y, x, d) and the count."""
    bad = got.float() != want.float()
    if not bool(bad.any()):
        return None
    i = tuple(int(v) for v in bad.nonzero()[0])
    return f"{what}: {int(bad.sum())} of {bad.numel()} values differ, first at (b, head, y, x, d) = {i}: got {float(got[i])!r}, expected {float(want[i])!r}"


# ---- the launcher's plan (rope_pool.hip:356-414) --------------------------------------------------------------------------------------------------
def launch_plan(B, Cq, heads, Ho, Wo, h, w, dtype=BF, x_channels_last=True, aligned=True, write_q=True):
    """What naf_launch_rope_pool chooses.  ``aligned``: x, q and the tables 16-byte aligned, q's strides multiples of 8 and, where the channels of x
    are contiguous, its strides multiples of 16 bytes.  A dict; ``status`` is "unsupported" where the launcher refuses."""
    Dh = Cq // heads
    vec = Dh % 32 == 0 and aligned
    VEC = 8 if vec else 1
    nchunk = Cq // (2 * VEC)
    tpp = 1
    while tpp < nchunk:
        tpp <<= 1
    p = dict(VEC=VEC, nchunk=nchunk, tpp=tpp, status="ok", T="__bf16" if dtype == BF else "float")
    if tpp > 256:
        p["status"] = "unsupported"
        return p
    npix_typ = (Ho // h) * (Wo // w)
    ppc = 256 // tpp
    while ppc > 1 and ppc > npix_typ:
        ppc >>= 1
    cpw = (256 // tpp) // ppc
    lds = (256 // tpp) * Cq * 4
    tab_lds = False
    if vec and cpw == 1:
        tl = ((Ho + h - 1) // h + 1 + (Wo + w - 1) // w + 1) * (2 * (Dh // 4) + 4) * 4
        if lds + tl <= LDS_TABLE_BUDGET:
            lds += tl
            tab_lds = True
    if lds > LDS_MAX:
        p["status"] = "unsupported"
        return p
    ncells = B * h * w
    keys_kernel = (not write_q) and dtype == BF and vec and cpw == 1 and tab_lds and x_channels_last and npix_typ >= 256 // tpp
    p.update(ppc=ppc, cpw=cpw, planes=256 // tpp, lds=lds, tab_lds=tab_lds, multi=cpw > 1, ncells=ncells, blocks=-(-ncells // cpw),
             partial_last=cpw > 1 and ncells % cpw != 0, keys_kernel=keys_kernel,
             overlap=Ho % h != 0 or Wo % w != 0, active_lanes=nchunk,
             kernel=("rope_pool_keys_kernel", None) if keys_kernel else ("rope_pool_kernel", f"{p['T']},{VEC},{'true' if cpw > 1 else 'false'}"))
    return p


# ---- the case table: the smallest shapes that reach each instance -------------------------------------------------------------------------------
class Case:
    def __init__(self, name, B, Cq, heads, out, lr, dtype=BF, nhwc=True, offset=0, expect=None, keys_expect=None):
        self.name, self.B, self.Cq, self.heads, self.out, self.lr, self.dtype, self.nhwc, self.offset = name, B, Cq, heads, out, lr, dtype, nhwc, offset
        self.expect, self.keys_expect = expect or {}, keys_expect
        self.Dh = Cq // heads

    def plan(self, write_q=True, aligned=None):
        return launch_plan(self.B, self.Cq, self.heads, *self.out, *self.lr, self.dtype, self.nhwc, self.offset == 0 if aligned is None else aligned, write_q)

    def shape(self):
        return (self.B, self.Cq, *self.out)

    def exact_inputs(self, seed):
        """(x, tab_y, tab_x) of the exact construction, fp32 on the host; the seeds of guidance and tables are unrelated."""
        x = integer_guidance(self.shape(), 7919 * seed + 17 * self.Cq + self.out[1])
        ty, tx = integer_tables(*self.out, self.Dh // 4, 104729 * seed + 31 * self.out[0] + self.Dh)
        return x, ty, tx

    def __repr__(self):
        return self.name


_K = "rope_pool_kernel"
CASES = [
    Case("A", 2, 256, 4, (32, 48), (2, 3), expect=dict(kernel=(_K, "__bf16,8,false"), tab_lds=True, overlap=False), keys_expect=("rope_pool_keys_kernel", None)),
    Case("B", 2, 256, 4, (23, 30), (5, 7), expect=dict(kernel=(_K, "__bf16,8,false"), tab_lds=True, overlap=True), keys_expect=("rope_pool_keys_kernel", None)),
    Case("C", 1, 64, 1, (6, 9), (2, 3), expect=dict(kernel=(_K, "__bf16,8,true"), ppc=8, partial_last=True, blocks=1)),
    Case("D", 1, 128, 2, (16, 24), (2, 3), F32, nhwc=False, expect=dict(kernel=(_K, "float,8,false"))),
    Case("E", 3, 64, 1, (5, 7), (5, 7), expect=dict(kernel=(_K, "__bf16,8,true"), ppc=1, cpw=64, ncells=105, blocks=2, partial_last=True)),
    Case("F", 2, 64, 1, (7, 10), (5, 7), expect=dict(kernel=(_K, "__bf16,8,true"), ppc=1, overlap=True)),
    Case("G", 2, 128, 2, (7, 10), (5, 7), F32, nhwc=False, expect=dict(kernel=(_K, "float,8,true"), ppc=1, overlap=True)),
    Case("H", 1, 24, 2, (20, 24), (2, 3), expect=dict(kernel=(_K, "__bf16,1,false"))),
    Case("I", 2, 24, 2, (9, 8), (3, 4), expect=dict(kernel=(_K, "__bf16,1,true"))),
    Case("J", 1, 24, 2, (20, 24), (2, 3), F32, nhwc=False, expect=dict(kernel=(_K, "float,1,false"))),
    Case("K", 2, 24, 2, (7, 10), (5, 7), F32, nhwc=False, expect=dict(kernel=(_K, "float,1,true"), overlap=True, partial_last=True)),
    Case("L", 1, 128, 2, (16, 24), (2, 3), offset=4, expect=dict(kernel=(_K, "__bf16,1,false"), tpp=64)),
    Case("M", 1, 256, 1, (64, 64), (2, 2), expect=dict(kernel=(_K, "__bf16,8,false"), tab_lds=False), keys_expect=(_K, "__bf16,8,false")),
    Case("N", 1, 96, 1, (16, 16), (4, 4), F32, expect=dict(kernel=(_K, "float,8,true"), active_lanes=6, tpp=8, cpw=2)),
    Case("O", 1, 1024, 16, (16, 16), (1, 1), expect=dict(kernel=(_K, "__bf16,8,false"), tpp=64, planes=4, tab_lds=True), keys_expect=("rope_pool_keys_kernel", None)),
]
CASE = {c.name: c for c in CASES}
REFUSED = Case("refused", 1, 1024, 16, (16, 16), (1, 1), offset=4)           # the scalar path needs 512 pair-chunks per pixel
PRODUCTION = Case("production", 1, 256, 4, (48, 64), (3, 4))                # the model's call: bf16 channels-last guidance, 4 heads of 64
# every rope_pool_kernel instance, tab_lds both ways on the vector path, and the keys kernel: what the GPU module must have seen when it ends
EXPECTED_INSTANCES = {(_K, f"{t},{v},{m}") for t in ("__bf16", "float") for v in (8, 1) for m in ("true", "false")} | {("rope_pool_keys_kernel", None)}


# ---- argument builders: caller-owned views, pointers and strides as they are -----------------------------------------------------------------------
def place_x(c, x, dev):
    """The case's guidance on the device in the case's own layout: a logical [B, Cq, Ho, Wo] view (channels-last or planar, ``offset`` elements
    into its buffer)."""
    B, Cq, Ho, Wo = x.shape
    buf = torch.zeros(x.numel() + 64, dtype=c.dtype, device=dev)
    flat = buf[c.offset:c.offset + x.numel()]
    if c.nhwc:
        v = flat.view(B, Ho, Wo, Cq).permute(0, 3, 1, 2)
    else:
        v = flat.view(B, Cq, Ho, Wo)
    v.copy_(x.to(c.dtype))
    return v


def rope_pool_args(x, q, k, tab_y, tab_x, heads):
    """naf_rope_pool_args from caller-owned views: x logical [B, Cq, Ho, Wo], q [B, heads, Ho, Wo, Dh] or None, k [B, heads, h, w, Dh]."""
    from naf_amd import _lib, ops
    a = _lib.RopePoolArgs()
    a.x, a.q, a.k_lr = x.data_ptr(), (q.data_ptr() if q is not None else None), k.data_ptr()
    a.tab_y, a.tab_x = tab_y.data_ptr(), tab_x.data_ptr()
    a.x_dtype = ops._DT[x.dtype]
    B, Cq, Ho, Wo = x.shape
    a.B, a.Cq, a.heads, a.Ho, a.Wo, a.h, a.w = B, Cq, heads, Ho, Wo, int(k.shape[2]), int(k.shape[3])
    assert k.stride(4) == 1 and (q is None or q.stride(4) == 1) and tab_y.is_contiguous() and tab_x.is_contiguous()
    assert tuple(tab_y.shape) == (Ho, 2, Cq // heads // 4) and tuple(tab_x.shape) == (Wo, 2, Cq // heads // 4)
    a.x_stride = _lib.I64x4(*[int(s) for s in x.stride()])
    a.q_stride = _lib.I64x4(*([int(s) for s in q.stride()[:4]] if q is not None else [0, 0, 0, 0]))
    a.k_stride = _lib.I64x4(*[int(s) for s in k.stride()[:4]])
    return a


def rope_pool_launch(a, x):
    """naf_rope_pool_fwd; returns the status (the caller checks it: the refused case is asked, not launched)."""
    from naf_amd import _lib, ops
    with torch.cuda.device(x.device):
        return int(_lib.load().naf_rope_pool_fwd(C.byref(a), ops._stream(x)))


def args_aligned(a, esz):
    """The launcher's vector-path test on filled args (rope_pool.hip:359-366), without Dh."""
    ok = all(int(p or 0) % 16 == 0 for p in (a.x, a.q, a.tab_y, a.tab_x))
    ok = ok and (not a.q or all(int(s) % 8 == 0 for s in a.q_stride))
    if int(a.x_stride[1]) == 1:
        ok = ok and all(int(a.x_stride[i]) * esz % 16 == 0 for i in (0, 2, 3))
    return ok


def stem_keys_launch(x, stats_in, gw, gb, eps, wp, bias, y, k_slice, tab_y, tab_x):
    """The ``keys=(k, ty, tx)`` form of ops.stem_conv on caller-owned views: k_slice a bf16 [B, h, w, 128] view of any strides with the channels
    contiguous, pointers and strides as they are."""
    from naf_amd import ops
    ops.stem_conv(x, stats_in, gw, gb, eps, wp, bias, y, None, keys=(k_slice, tab_y, tab_x))
