"""The layout contract of the attention entries and the technique that tests it (tests/test_layout_contract_cpu.py without a device,
tests/test_gpu_layout_contract.py on one).  Plain helper module: no test in it.

The contract (include/naf_hip.h, "LAYOUT CONTRACT OF THE ATTENTION ENTRIES"): every operand of naf_xna_fwd, naf_xna_head_fwd,
naf_xna_head_ce_fwd, naf_xna_cos_fwd, naf_xna_cos_ce_fwd, naf_xna_mse_fwd and naf_xna_bwd is a pointer plus four element strides {b, head,
y, x} with the last dim contiguous, and the kernels honour every stride of every operand on its own.  The matrix-core kernels take 16-byte aligned pointers and
strides that are multiples of 8 elements (4 for `out` of the forward); everything else runs, under AUTO, a kernel that reads and writes
that operand element by element, and is refused with NAF_ERR_UNSUPPORTED where a path is insisted on.

The technique.  ``embed`` places a logical [B, heads, H, W, D] tensor into a flat ARENA with the strides of a FAMILY; everything of the
arena that is not the view -- the gaps between pixels, rows, heads and images and a margin of at least 2 rows + 16 pixels + 16 elements
on both sides -- holds a sentinel: the NaN pattern 0x7FC1 for 16-bit floats, 0x7FC0BEEF (a NaN with a payload) for fp32, 0xA5 for bytes.
No kernel produces these patterns.  After a launch
  * the view of an output must be bit-equal to what the same kernel wrote on the canonical dense layout,
  * ``untouched`` must find every element of an output's arena outside the view bit-unchanged (a store of a masked lane, an overshoot
    by a row, a stride of another operand all land in the arena, not in the allocator's slack),
  * every input's arena must be bit-unchanged, and
  * the output must be finite: a read through a wrong stride lands on a NaN.

Families (D contiguous in all; C = heads * D):
  head_major    memory [B, heads, H, W, D] dense: the tests' canonical layout
  channels_last memory [B, H, W, heads, D] dense: what the model hands over
  pixel_gap     channels-last with x stride C + 8
  row_gap       channels-last with y stride W * C + 24
  crop          images 1 .. B of a batch of B + 1, window [2 : 2 + H, 3 : 3 + W] of an (H + 5) x (W + 7) canvas, channels [8 : 8 + C] of
                C + 24; the pointer is 16-byte aligned and NOT 32-byte aligned
  head_gap      channels-last with head stride 2 D
  batch_inner   memory [heads, H, W, B, D]: the batch stride is the smallest
  transposed    memory [B, heads, W, H, D]: y stride < x stride
  expanded      head-major, batch stride 0 (read-only operands whose images are equal)
  expanded_head memory [B, H, W, D], head stride 0: the `dout` that naf_xna_head_ce_fwd's dlogits is (read-only, heads equal)
  odd_offset    head-major, pointer + 4 elements            } not vectorisable (16-bit types): the routing tests only
  odd_stride    channels-last with x stride C + 4           }
``planar`` places a [B, C, H, W] operand whose channel stride is free (the guidance of naf_rope_pool_fwd) in NCHW memory with a row gap and a
plane gap.
"""
import ctypes as C

import torch

NAN16 = 0x7FC1            # the NaN pattern tests/test_gpu_regress.py poisons with
SENT32 = 0x7FC0BEEF       # an fp32 NaN with a payload no arithmetic produces
SENT8 = 0xA5
SENT64 = 0x7FF8DEADBEEF0001

VECTOR_FAMILIES = ("head_major", "channels_last", "pixel_gap", "row_gap", "crop", "head_gap", "batch_inner", "transposed")
READONLY_FAMILIES = ("expanded", "expanded_head")
ROUTING_FAMILIES = ("odd_offset", "odd_stride")
FAMILIES = VECTOR_FAMILIES + READONLY_FAMILIES + ROUTING_FAMILIES

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_SENTINEL = {1: SENT8, 2: NAN16, 4: SENT32, 8: SENT64}


def bits(t):
    """The tensor's memory as integers of the element size (a view): comparisons on it are bit-level, NaN == NaN."""
    return t.view(_BITS[t.element_size()])


def sentinel(dtype):
    return _SENTINEL[torch.empty((), dtype=dtype).element_size()]


def layout(shape, family):
    """(strides {b, head, y, x}, offset of the first element inside the family's own buffer, elements of that buffer), in elements."""
    B, n, H, W, D = shape
    Cc = n * D
    off = 0
    if family in ("head_major", "odd_offset", "expanded"):
        sx = D; sy = W * sx; sh = H * sy; sb = 0 if family == "expanded" else n * sh
        off = 4 if family == "odd_offset" else 0
    elif family in ("channels_last", "pixel_gap", "row_gap", "odd_stride"):
        sh = D
        sx = Cc + {"pixel_gap": 8, "odd_stride": 4}.get(family, 0)
        sy = W * sx + (24 if family == "row_gap" else 0)
        sb = H * sy
    elif family == "crop":
        sh = D; sx = Cc + 24; sy = (W + 7) * sx; sb = (H + 5) * sy
        off = sb + 2 * sy + 3 * sx + 8
    elif family == "head_gap":
        sh = 2 * D; sx = n * sh; sy = W * sx; sb = H * sy
    elif family == "batch_inner":
        sb = D; sx = B * D; sy = W * sx; sh = H * sy
    elif family == "transposed":
        sy = D; sx = H * sy; sh = W * sx; sb = n * sh
    elif family == "expanded_head":
        sh = 0; sx = D; sy = W * sx; sb = H * sy
    else:
        raise ValueError(family)
    extent = off + (B - 1) * sb + (n - 1) * sh + (H - 1) * sy + (W - 1) * sx + D
    if family == "crop":
        extent = (B + 1) * sb
    return (sb, sh, sy, sx), off, extent


def margin(strides):
    """Elements kept on both sides of a view: two rows, sixteen pixels and sixteen elements of ITS strides."""
    return 2 * strides[2] + 16 * strides[3] + 16


def placement(shape, family, itemsize):
    """(strides, start of the view in the arena, elements of the arena).  The start is 32-byte aligned relative to the arena (whose base
    the allocators align to 64 bytes or more) for every family but ``crop`` (16 mod 32) and ``odd_offset`` (32-byte aligned + 4 elements)."""
    strides, off, extent = layout(shape, family)
    m = margin(strides)
    e32 = max(32 // itemsize, 1)
    want = {"crop": e32 // 2, "odd_offset": 4 % e32}.get(family, 0)
    lead = m
    while (lead + off) % e32 != want:
        lead += 1
    return strides, lead + off, lead + extent + m


def view_mask(total, start, shape, strides, device="cpu"):
    """bool [total]: the arena elements a view of ``shape`` with ``strides`` (last dim contiguous) starting at ``start`` owns."""
    idx = torch.full((), start, dtype=torch.int64, device=device)
    for n, s in zip(shape, tuple(strides) + (1,)):
        idx = idx.unsqueeze(-1) + torch.arange(n, dtype=torch.int64, device=device) * s
    mask = torch.zeros(total, dtype=torch.bool, device=device)
    mask[idx.reshape(-1)] = True
    return mask


def arena_for(shape, dtype, family, device="cpu", fill=None, mask=True):
    """(view, arena, inside_mask) of an arena that holds ``fill`` (default: the type's sentinel) everywhere, the view included.
    ``mask=False``: no mask is built (None), for callers that only ask the host checks about pointers and strides."""
    it = torch.empty((), dtype=dtype).element_size()
    strides, start, total = placement(tuple(shape), family, it)
    arena = torch.empty(total, dtype=dtype, device=device)
    assert arena.data_ptr() % 64 == 0, "the allocator's base is not 64-byte aligned"
    bits(arena).fill_(_SENTINEL[it] if fill is None else fill)
    view = arena.as_strided(tuple(shape), strides + (1,), start)
    return view, arena, (view_mask(total, start, shape, strides, device) if mask else None)


def embed(dense5, family, fill=None, device=None):
    """A logical [B, heads, H, W, D] tensor in the strides of ``family``: (view, arena, inside_mask).  The view has the values of
    ``dense5``; the arena is the flat buffer it lives in, ``fill`` (default: the type's sentinel) wherever the view is not; the mask marks
    the arena elements that belong to the view (for the stride-0 families: once each)."""
    device = dense5.device if device is None else device
    src = dense5.to(device)
    view, arena, mask = arena_for(src.shape, src.dtype, family, device, fill)
    if family == "expanded":
        assert torch.equal(bits(src), bits(src[:1].expand_as(src).contiguous())), "expanded: the images must be equal"
        view[:1].copy_(src[:1])
    elif family == "expanded_head":
        assert torch.equal(bits(src), bits(src[:, :1].expand_as(src).contiguous())), "expanded_head: the heads must be equal"
        view[:, :1].copy_(src[:, :1])
    else:
        view.copy_(src)
    return view, arena, mask


def planar(dense4, row_gap=3, plane_gap=40, device=None):
    """A logical [B, C, H, W] tensor in PLANAR (NCHW) memory with x contiguous, rows ``row_gap`` and planes ``plane_gap`` elements apart:
    (view, arena, inside_mask), sentinels in the gaps and in a margin of two rows + 16 elements on both sides.  For the operands whose
    channel stride is free (the guidance of naf_rope_pool_fwd)."""
    device = dense4.device if device is None else device
    B, Cc, H, W = dense4.shape
    sy = W + row_gap
    sc = H * sy + plane_gap
    sb = Cc * sc
    lead = 2 * sy + 16
    it = dense4.element_size()
    while lead % max(32 // it, 1):
        lead += 1
    total = lead + B * sb + 2 * sy + 16
    arena = torch.empty(total, dtype=dense4.dtype, device=device)
    bits(arena).fill_(_SENTINEL[it])
    view = arena.as_strided((B, Cc, H, W), (sb, sc, sy, 1), lead)
    view.copy_(dense4.to(device))
    return view, arena, view_mask(total, lead, (B, Cc, H, W), (sb, sc, sy), device)


def banded(shape, dtype, device="cpu", inside=None, band=512):
    """A DENSE tensor of ``shape`` with a guard band of ``band`` sentinel elements before and after: (tensor, arena, inside_mask).  For
    the outputs that are dense by contract (dk_lr, dv_lr, the scores, the row-streaming backward's workspace, the MSE loss).
    ``inside``: a value to fill the tensor with (dk_lr / dv_lr are zeroed by the caller), None = the sentinel."""
    n = 1
    for s in shape:
        n *= int(s)
    it = torch.empty((), dtype=dtype).element_size()
    band = (band * it + 63) // 64 * 64 // it
    arena = torch.empty(band + n + band, dtype=dtype, device=device)
    bits(arena).fill_(_SENTINEL[it])
    t = arena[band:band + n].view(tuple(shape))
    if inside is not None:
        t.fill_(inside)
    mask = torch.zeros(arena.numel(), dtype=torch.bool, device=device)
    mask[band:band + n] = True
    return t, arena, mask


def outside_writes(arena, before, inside_mask):
    """Number of arena elements outside the mask whose bits differ from ``before`` (a clone taken ahead of the launch)."""
    return int(((bits(arena) != bits(before)) & ~inside_mask).sum())


def untouched(arena, before, inside_mask):
    """True when every element of the arena outside the mask is bit-equal to ``before``."""
    return outside_writes(arena, before, inside_mask) == 0


def unchanged(arena, before):
    return torch.equal(bits(arena), bits(before))


def same_bits(a, b):
    """Two logical tensors bit for bit (any strides)."""
    return a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


# ---- what the host checks admit, restated (naf_common.h xna_qkv_layout_ok and the *_eligible functions) --------------------------
def vec_ok(t, mult=8):
    """16-byte aligned pointer, the four outer strides multiples of ``mult`` elements."""
    return t.data_ptr() % 16 == 0 and all(int(s) % mult == 0 for s in t.stride()[:-1])


def forward_admits(kernel, q, k, v, out):
    """Does the forward kernel's eligibility test admit these LAYOUTS (the geometry is the case's)?  xna_mfma.hip:22-24, xna_union.hip:128-130:
    q / k / v vectorisable, out 16-byte aligned with strides in multiples of 4; xna_rows.hip:226-228: q and k only (values and output go
    element by element); xna_generic.hip: anything."""
    if kernel in ("mfma", "union"):
        return vec_ok(q) and vec_ok(k) and vec_ok(v) and vec_ok(out, 4)
    if kernel == "rows":
        return vec_ok(q) and vec_ok(k)
    return kernel == "generic"


def backward_admits(kernel, q, k, v, dout, dq):
    """xna_bwd.hip:60-62: all five vectorisable; xna_rows_bwd.hip:538-545, :562-564: q and k, and v / dout too unless Dv <= 32 (the gather
    form); dq is stored element by element (:484); xna_generic.hip: anything."""
    if kernel == "mfma":
        return all(vec_ok(t) for t in (q, k, v, dout, dq))
    if kernel == "rows":
        return vec_ok(q) and vec_ok(k) and ((vec_ok(v) and vec_ok(dout)) or v.shape[-1] <= 32)
    return kernel == "generic"


def head_admits(q, k, pv, dlogits=None):
    """xna_head.hip:27: q / k / pv vectorisable (`out`, loss and labels are stored element by element: any strides); :39-49: dlogits too."""
    return vec_ok(q) and vec_ok(k) and vec_ok(pv) and (dlogits is None or vec_ok(dlogits))


def cos_admits(q, k, pv, v, dlogits=None):
    """xna_cos.hip:22-23 (naf_xna_cos_eligible): q / k / pv AND v vectorisable (`out` and norms are stored element by element: any
    strides); :40-50 (naf_xna_cos_ce_eligible): dlogits too -- 16-byte aligned, its strides {b, y, x} multiples of 8 (target, loss, labels
    and dscale are read / stored element by element)."""
    return vec_ok(q) and vec_ok(k) and vec_ok(pv) and vec_ok(v) and (dlogits is None or vec_ok(dlogits))


# ---- the cases of tests/test_gpu_layout_contract.py (here so that the CPU table sweeps the same geometries) -----------------------
B2 = 2
# (FWD_CASES id, out dtype, variant): variant None, "logits" (return_logits), "rope" (rotate-on-load), "half" (float16 values and output)
FWD_RUNS = [
    ("cell-k7", torch.bfloat16, None), ("cell-k7", torch.float32, None), ("cell-k7", torch.bfloat16, "logits"),
    ("cell-k3-ragged", torch.bfloat16, None), ("cell-k9-patch14", torch.bfloat16, None), ("cell-k9-patch14", torch.float32, "rope"),
    ("sliding-k7", torch.float32, None), ("sliding-k15", torch.bfloat16, None),
    ("union-k7", torch.bfloat16, None), ("union-k9-ratio1", torch.bfloat16, None),
    ("rows-k7", torch.bfloat16, None), ("rows-k3-noninteger", torch.bfloat16, None), ("rows-k9", torch.bfloat16, None),
    ("generic-k7", torch.bfloat16, None),
    ("cell-k7", torch.float16, "half"), ("sliding-k7", torch.float16, "half"), ("union-k7", torch.float16, "half"),
    ("rows-k7", torch.float16, "half"), ("generic-k7", torch.float16, "half"),
]
BWD_RUNS = ["cell", "cell-partial-tiles", "cell-chunked-k13", "rows-ratio1", "rows-cells", "generic-noninteger"]
FWD_FAMILY = ("chan_offset", "unit")            # values with per-channel offsets: a head or a channel read from the wrong place shows
BWD_FAMILY = ("chan_offset", "unit", "unit")
HEAD_N = 21
# B, h, w, dy, dx, window, heads: input_statistics.HEAD_GEOM at B = 2 (whole 16-pixel row tiles), and the cells of a patch-14 backbone, where
# 14 of a row tile's 16 lanes hold a pixel and the epilogues mask the other two
HEAD_GEOMS = {"tiles16": (B2, 8, 8, 8, 16, 7, 4), "patch14": (B2, 8, 9, 2, 14, 7, 2)}
MSE_CASE = "b_f4_k3"                            # tests/regress_reference.py: B = 2, ratio 4.6 x 4.3, a 14-pixel partial tile
# The cosine head, (B, heads, Dv, (h, w), (dy, dx), window, N) as tests/cosine_reference.CASES: the smallest geometries that reach the
# paths named, each with Dv != head_npad(N), so that pv_lr's strides and v_lr's differ in every family
COS_GEOMS = {
    "tiles16": (B2, 4, 48, (8, 8), (8, 16), 7, 21),       # whole 16-pixel row tiles, one partly filled 64-channel value chunk, two channel tiles
    "patch14": (B2, 2, 80, (8, 9), (2, 14), 7, 21),       # 14 of 16 lanes hold a pixel, two value chunks of which the second is partial
    "n151": (B2, 2, 128, (5, 6), (2, 16), 5, 151),        # ten channel tiles, two whole value chunks
}
COS_SCALE = {"tiles16": 1.0, "patch14": 1.0, "n151": 14.285714}        # one CLIP-style temperature, as tests/test_gpu_cosine_head.py has
COS_IGNORE = 255


def cos_inputs(gname):
    """cosine_reference.make_inputs on a COS_GEOMS geometry, the value channels with offsets of their own: (q, k, v, E) on the host."""
    import cosine_reference as CR
    return CR.make_inputs(None, geom=COS_GEOMS[gname], chan_offset=1.0)


def cos_shapes(gname):
    """(window, N, {operand: 5-D shape}) of a COS_GEOMS geometry; the maps of the entries are [B, 1, Ho, Wo, channels]."""
    from naf_amd import ops
    B, heads, Dv, (h, w), (dy, dx), ks, N = COS_GEOMS[gname]
    Ho, Wo = h * dy, w * dx
    return ks, N, {"q": (B, heads, Ho, Wo, 64), "k": (B, heads, h, w, 64), "pv": (B, heads, h, w, ops.head_npad(N)), "v": (B, heads, h, w, Dv),
                   "out": (B, 1, Ho, Wo, N), "norms": (B, 1, Ho, Wo, 1), "target": (B, 1, Ho, Wo, 1), "loss": (B, 1, Ho, Wo, 1),
                   "labels": (B, 1, Ho, Wo, 1), "dlogits": (B, 1, Ho, Wo, ops.head_dlogits_channels(N)), "dscale": (B, 1, Ho, Wo, 1)}


COS_DTYPES = {"q": torch.bfloat16, "k": torch.bfloat16, "pv": torch.bfloat16, "v": torch.bfloat16, "out": torch.float32, "norms": torch.float32,
              "target": torch.int64, "loss": torch.float32, "labels": torch.uint8, "dlogits": torch.bfloat16, "dscale": torch.float32}
COS_INPUTS, COS_OUTPUTS = ("q", "k", "pv", "v"), ("out", "norms")
COS_CE_INPUTS, COS_CE_OUTPUTS = ("q", "k", "pv", "v", "target"), ("out", "norms", "loss", "labels", "dlogits", "dscale")


def run_id(run):
    name, dt, variant = run
    return f"{name}-{str(dt).split('.')[-1]}" + (f"-{variant}" if variant else "")


def fwd_case(name):
    import input_statistics as S
    return next(c for c in S.FWD_CASES if c[0] == name)


def bwd_case(name):
    import input_statistics as S
    return next(c for c in S.BWD_CASES if c[0] == name)


def forward_inputs(case, half=False, B=B2):
    """input_statistics.forward_inputs at batch ``B`` (the images differ): fp32 NCHW (q, k, v) holding bf16 (half) values."""
    import half_reference as HR
    import input_statistics as S
    _, path, sub, heads, Dq, lr, out_sz, ksz, Cc, _ = case
    seed = 1000 + 7 * ksz + out_sz[1]
    q, k = S.make_qk((B, heads * Dq, *out_sz), (B, heads * Dq, *lr), FWD_FAMILY[1], seed, heads)
    make = HR.make_half_values if half else S.make_values
    return q, k, make((B, Cc, *lr), FWD_FAMILY[0], seed + 2)


def backward_inputs(case, B=B2):
    import input_statistics as S
    _, path, heads, Dq, lr, out_sz, ksz, Cc, _, _ = case
    seed = 2000 + 7 * ksz + out_sz[1]
    q, k = S.make_qk((B, heads * Dq, *out_sz), (B, heads * Dq, *lr), BWD_FAMILY[2], seed, heads)
    return q, k, S.make_values((B, Cc, *lr), BWD_FAMILY[0], seed + 2), S.make_values((B, Cc, *out_sz), BWD_FAMILY[1], seed + 3)


def to5(x, heads, dtype=torch.bfloat16):
    """[B, C, H, W] fp32 -> dense head-major [B, heads, H, W, D] of ``dtype``."""
    B, Cc, H, W = x.shape
    return x.view(B, heads, Cc // heads, H, W).permute(0, 1, 3, 4, 2).contiguous().to(dtype)


def launch_plans(inputs, outputs, expandable=(), head_expandable=()):
    """The launch set of a case: [(label, {operand: family})].
      (a) every operand in one family, for every vectorisable family;
      (b) each operand in turn in ``crop``, the rest head-major (one operand's strides used for another);
      (c) the production mix: q, k head-major, everything else channels-last;
      (d) ``expanded`` on the operands of ``expandable`` (read-only, their images made equal by the caller), and ``expanded_head`` on
          those of ``head_expandable``."""
    ops_ = tuple(inputs) + tuple(outputs)
    plans = [(f"all-{f}", {o: f for o in ops_}) for f in VECTOR_FAMILIES]
    plans += [(f"{o}-crop", {p: ("crop" if p == o else "head_major") for p in ops_}) for o in ops_]
    plans.append(("production", {o: ("head_major" if o in ("q", "k") else "channels_last") for o in ops_}))
    if expandable:
        plans.append(("expanded", {o: ("expanded" if o in expandable else "head_major") for o in ops_}))
    if head_expandable:
        plans.append(("expanded-head", {o: ("expanded_head" if o in head_expandable else "head_major") for o in ops_}))
    return plans


CANONICAL = "head_major"


# ---- argument builders: operands and outputs in arenas, through the fill functions of naf_amd.ops (as tests/test_cabi.py does) --------
class Placed:
    """Operands of one launch: name -> (view, arena, inside_mask), with the arenas' contents ahead of the launch."""

    def __init__(self):
        self.views, self.arenas, self.masks, self.before, self.outputs = {}, {}, {}, {}, set()

    def add(self, name, placed, output=False):
        self.views[name], self.arenas[name], self.masks[name] = placed
        if output:
            self.outputs.add(name)
        return placed[0]

    def snapshot(self):
        self.before = {n: a.clone() for n, a in self.arenas.items()}

    def problems(self):
        """What the launch did that the contract forbids: a list of strings, empty when all is well."""
        bad = []
        for n, a in self.arenas.items():
            if n in self.outputs:
                w = outside_writes(a, self.before[n], self.masks[n])
                if w:
                    bad.append(f"{n}: {w} elements outside the view were written")
            elif not unchanged(a, self.before[n]):
                bad.append(f"{n}: the input arena changed")
        return bad


def forward_args(q, k, v, out, ksz, path, logits=None, rope_tables=None):
    """(naf_xna_args, kernel the library selects or a negative status): pointers and strides of the views as they are."""
    from naf_amd import _lib, ops
    ky, kx = ops._ksize(ksz)
    a = ops._fill_xna(q, k, v, out, logits, None, None, ky, kx, path, None, rope_tables)
    return a, int(_lib.load().naf_xna_select(C.byref(a)))


def forward_launch(a, sel, q):
    """naf_xna_fwd for args the library accepted (sel >= 0), with the index tables the table-driven kernels read."""
    from naf_amd import _lib, ops
    assert sel >= 0, "only layouts the host checks accept are launched"
    keep = None
    if sel != _lib.XNA_MFMA:
        keep = (ops.device_index_table(a.Ho, a.h, a.ky, q.device), ops.device_index_table(a.Wo, a.w, a.kx, q.device))
        a.idx_y, a.idx_x = keep[0].data_ptr(), keep[1].data_ptr()
    with torch.cuda.device(q.device):
        rc = _lib.load().naf_xna_fwd(C.byref(a), ops._stream(q))
    _lib.check(rc, "naf_xna_fwd")
    return keep


def backward_args(q, k, v, dout, dq, dk, dv, ksz, path):
    from naf_amd import _lib, ops
    ky, kx = ops._ksize(ksz)
    a = ops._fill_xna_bwd(q, k, v, dout, dq, dk, dv, ky, kx, None)
    a.path = ops._BWD_PATHS[path]
    return a, int(_lib.load().naf_xna_bwd_supported(C.byref(a)))


def backward_workspace_bytes(a):
    from naf_amd import _lib
    return int(_lib.load().naf_xna_bwd_workspace_bytes(C.byref(a)))


def backward_launch(a, sel, q, workspace=None):
    from naf_amd import _lib, ops
    assert sel >= 0, "only layouts the host checks accept are launched"
    keep = None
    if sel in (_lib.XNA_GENERIC, _lib.XNA_ROWS):
        keep = (ops.device_index_table(a.Ho, a.h, a.ky, q.device), ops.device_index_table(a.Wo, a.w, a.kx, q.device))
        a.idx_y, a.idx_x = keep[0].data_ptr(), keep[1].data_ptr()
    if sel == _lib.XNA_ROWS:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    with torch.cuda.device(q.device):
        rc = _lib.load().naf_xna_bwd(C.byref(a), ops._stream(q))
    _lib.check(rc, "naf_xna_bwd")
    return keep


def head_args(q, k, pv, bias, out, n_out, ksz, path="fused"):
    """(naf_xna_head_args, naf_xna_head_select's answer).  ``out``: [B, Ho, Wo, N] by strides {b, y, x}."""
    from naf_amd import _lib, ops
    ky, kx = ops._ksize(ksz)
    a = ops._fill_xna_head(q, k, pv, bias, out, n_out, ky, kx, path, None)
    return a, int(_lib.load().naf_xna_head_select(C.byref(a)))


def head_ce_args(q, k, pv, bias, out, n_out, ksz, target, loss, labels, dlogits, ignore_index, path="fused"):
    """(naf_xna_head_ce_args, naf_xna_head_ce_select's answer): ops.xna_head_objective's filling with the caller's buffers."""
    from naf_amd import _lib, ops
    ky, kx = ops._ksize(ksz)
    a = _lib.XnaHeadCEArgs()
    a.head = ops._fill_xna_head(q, k, pv, bias, out if out is not None else q, n_out, ky, kx, path, None)
    if out is None:
        a.head.out, a.head.out_dtype = None, _lib.NAF_F32
    a.ignore_index, a.dlogits_channels = int(ignore_index), (int(dlogits.shape[-1]) if dlogits is not None else ops.head_dlogits_channels(n_out))
    for t, ptr, st in ((target, "target", "t_stride"), (loss, "loss", "loss_stride"), (labels, "labels", "labels_stride"), (dlogits, "dlogits", "dlogits_stride")):
        if t is not None:
            setattr(a, ptr, t.data_ptr())
            setattr(a, st, ops._strides3(t))
    return a, int(_lib.load().naf_xna_head_ce_select(C.byref(a)))


def head_launch(a, sel, q, ce=False):
    from naf_amd import _lib, ops
    assert sel == _lib.XNA_HEAD_FUSED, "only layouts the host checks accept are launched"
    lib = _lib.load()
    with torch.cuda.device(q.device):
        rc = (lib.naf_xna_head_ce_fwd if ce else lib.naf_xna_head_fwd)(C.byref(a), ops._stream(q))
    _lib.check(rc, "naf_xna_head_ce_fwd" if ce else "naf_xna_head_fwd")


def cos_args(q, k, pv, v, out, norms, n_out, ksz, logit_scale=1.0, path="fused", rope_tables=None):
    """(naf_xna_cos_args, naf_xna_cos_select's answer).  ``out``: [B, Ho, Wo, N], ``norms``: [B, Ho, Wo] or None, by strides {b, y, x}."""
    from naf_amd import _lib, ops
    ky, kx = ops._ksize(ksz)
    a = ops._fill_xna_cos(q, k, pv, v, out, norms, n_out, ky, kx, path, None, logit_scale, rope_tables)
    return a, int(_lib.load().naf_xna_cos_select(C.byref(a)))


def cos_ce_args(q, k, pv, v, out, norms, n_out, ksz, target, loss, labels, dlogits, dscale, ignore_index=COS_IGNORE, logit_scale=1.0, path="fused",
                scale_ptr=None, rope_tables=None):
    """(naf_xna_cos_ce_args, naf_xna_cos_ce_select's answer): ops.xna_cos_objective's filling with the caller's buffers, each of which may
    be None.  ``scale_ptr``: a 1-element fp32 device tensor that replaces ``logit_scale``."""
    from naf_amd import _lib, ops
    ky, kx = ops._ksize(ksz)
    a = _lib.XnaCosCEArgs()
    a.cos = ops._fill_xna_cos(q, k, pv, v, out if out is not None else q, norms, n_out, ky, kx, path, None, logit_scale, rope_tables)
    if out is None:
        a.cos.out, a.cos.o_stride = None, ops.I64x3(0, 0, 0)
    a.ignore_index = int(ignore_index)
    a.dlogits_channels = int(dlogits.shape[-1]) if dlogits is not None else ops.head_dlogits_channels(n_out)
    if scale_ptr is not None:
        a.logit_scale_ptr = scale_ptr.data_ptr()
    for t, ptr, st in ((target, "target", "t_stride"), (loss, "loss", "loss_stride"), (labels, "labels", "labels_stride"),
                       (dlogits, "dlogits", "dlogits_stride"), (dscale, "dscale", "dscale_stride")):
        if t is not None:
            setattr(a, ptr, t.data_ptr())
            setattr(a, st, ops._strides3(t))
    return a, int(_lib.load().naf_xna_cos_ce_select(C.byref(a)))


def cos_launch(a, sel, q, ce=False):
    from naf_amd import _lib, ops
    assert sel == _lib.XNA_HEAD_FUSED, "only layouts the host checks accept are launched"
    lib = _lib.load()
    with torch.cuda.device(q.device):
        rc = (lib.naf_xna_cos_ce_fwd if ce else lib.naf_xna_cos_fwd)(C.byref(a), ops._stream(q))
    _lib.check(rc, "naf_xna_cos_ce_fwd" if ce else "naf_xna_cos_fwd")


def mse_args(q, k, v, target, dout, ksz):
    """(naf_xna_mse_args, naf_xna_mse_supported's answer: 1 or a negative status)."""
    from naf_amd import _lib, ops
    ky, kx = ops._ksize(ksz)
    m = ops._fill_xna_mse(q, k, v, target, dout, ky, kx, None)
    return m, int(_lib.load().naf_xna_mse_supported(C.byref(m)))


def mse_workspace_bytes(m):
    from naf_amd import _lib
    return int(_lib.load().naf_xna_mse_workspace_bytes(C.byref(m)))


def mse_launch(m, ok, q, workspace, loss):
    from naf_amd import _lib, ops
    assert ok == 1, "only layouts the host checks accept are launched"
    a = m.a
    keep = (ops.device_index_table(a.Ho, a.h, a.ky, q.device), ops.device_index_table(a.Wo, a.w, a.kx, q.device))
    m.a.idx_y, m.a.idx_x = keep[0].data_ptr(), keep[1].data_ptr()
    m.workspace, m.workspace_bytes, m.loss = workspace.data_ptr(), workspace.numel(), loss.data_ptr()
    with torch.cuda.device(q.device):
        rc = _lib.load().naf_xna_mse_fwd(C.byref(m), ops._stream(q))
    _lib.check(rc, "naf_xna_mse_fwd")
    return keep


def hw3(view5):
    """[B, 1, H, W, D] arena view -> [B, H, W, D] by strides {b, y, x} (the head's `out` and dlogits)."""
    return view5[:, 0]


def hw2(view5):
    """[B, 1, H, W, 1] arena view -> [B, H, W] by strides {b, y, x} (the loss map and the labels)."""
    return view5[:, 0, :, :, 0]
