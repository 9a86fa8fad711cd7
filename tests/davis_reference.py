"""A restatement of the reference's DAVIS measures (evaluation/eval_video_seg.py:145-269) in numpy, shared by tests/test_davis_jf_cpu.py and
tests/test_gpu_davis_jf.py, and the seeded cases both use.  Nothing here is the reference's text; the citations say which lines a
function restates.

Two forms of the boundary term:
  * the DISK form (``counts_disk``): a boundary pixel hits when the other map has a boundary pixel at squared distance <= r2, found by
    brute-force shifts.  No scipy.  This is what ``naf_amd.davis_jf`` is specified to compute and what the GPU tests compare against.
  * the DISTANCE-TRANSFORM form (``counts_edt``): ``scipy.ndimage.distance_transform_edt(1 - boundary) <= bound_pix`` as the reference
    writes it (:189-199).  scipy is imported lazily.
The two differ only in the raw hit counts against an EMPTY boundary (the transform of an array without a zero is arbitrary), never in F.
"""
import math

import numpy as np

DEFAULT_BOUND_TH = 0.008            # davis_f_measure's default (:171)


# ---- items 1-5: counts, J, F --------------------------------------------------------------------------------------------------------
def bound_pix(bound_th, H, W):
    """:183 -- ``bound_th if bound_th >= 1 else ceil(bound_th * ||(H, W)||)``."""
    return float(bound_th) if bound_th >= 1 else float(math.ceil(bound_th * math.sqrt(float(H * H + W * W))))


def boundary(mask):
    """_seg2bmap (:210-226): the 3 x 3 Sobel pair on the 0/1 mask, border reflected WITHOUT repeating the edge (OpenCV's default
    BORDER_REFLECT_101 = numpy's ``reflect``), set where sqrt(ex^2 + ey^2) > 0.1 -- on integers: where ex or ey is non-zero."""
    m = np.pad(np.asarray(mask).astype(bool).astype(np.int64), 1, mode="reflect")
    H, W = m.shape[0] - 2, m.shape[1] - 2

    def at(dy, dx):
        return m[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    ex = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    ey = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return (ex != 0) | (ey != 0)


def dilate_disk(b, r2):
    """Pixels with a set pixel of ``b`` at squared distance <= r2: an OR over every shift inside the disk (zeros shifted in)."""
    H, W = b.shape
    R = int(math.isqrt(int(r2)))
    out = np.zeros_like(b, dtype=bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy * dy + dx * dx > r2 or abs(dy) >= H or abs(dx) >= W:
                continue
            ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
            xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
            out[yd, xd] |= b[ys, xs]
    return out


def _near_disk(b, bp):
    return dilate_disk(b, int(math.floor(bp * bp)))


def _near_edt(b, bp):
    from scipy.ndimage import distance_transform_edt      # lazy: only the distance-transform form needs scipy
    return distance_transform_edt(1 - b.astype(np.uint8)) <= bp


def _counts(annotation, segmentation, num_objects, bound_th, near):
    ann, seg = np.asarray(annotation), np.asarray(segmentation)
    if ann.ndim == 2:
        ann, seg = ann[None], seg[None]
    T, H, W = ann.shape
    bp = bound_pix(bound_th, H, W)
    out = np.zeros((num_objects, T, 6), dtype=np.int64)
    for o in range(1, num_objects + 1):
        for t in range(T):
            g, s = ann[t] == o, seg[t] == o
            bg, bs = boundary(g), boundary(s)
            out[o - 1, t] = ((g & s).sum(), (g | s).sum(), bs.sum(), bg.sum(),          # :160-161, :196, :199
                             (bs & near(bg, bp)).sum(), (bg & near(bs, bp)).sum())
    return out


def counts_disk(annotation, segmentation, num_objects, bound_th=DEFAULT_BOUND_TH):
    """int64 [N, T, 6]: inters, union, n_seg, n_gt, seg_hits, gt_hits -- the disk form."""
    return _counts(annotation, segmentation, num_objects, bound_th, _near_disk)


def counts_edt(annotation, segmentation, num_objects, bound_th=DEFAULT_BOUND_TH):
    """The same through scipy's Euclidean distance transform, as :189-199 write it."""
    return _counts(annotation, segmentation, num_objects, bound_th, _near_edt)


def jf_from_counts(counts):
    """J (:163-167) and F (:195-205) in fp64 from the six counts."""
    c = np.asarray(counts).astype(np.float64)
    inters, union, n_seg, n_gt, seg_hits, gt_hits = (c[..., i] for i in range(6))
    with np.errstate(divide="ignore", invalid="ignore"):
        J = inters / union
    J[union == 0] = 1.0
    P, R = seg_hits / (n_seg + 1e-10), gt_hits / (n_gt + 1e-10)
    with np.errstate(divide="ignore", invalid="ignore"):
        F = 2 * P * R / (P + R)
    F[P + R == 0] = 0.0
    return J, F


def statistics(values):
    """davis_db_statistics (:251-269) of one object's per-frame values [T]: (mean, recall, decay) as fp64 scalars."""
    v = np.asarray(values, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        M, O = np.nanmean(v), np.nanmean(v > 0.5)
    ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.uint8)
    bins = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
    return float(M), float(O), float(np.nanmean(bins[0]) - np.nanmean(bins[3]))


def bin_edges(T):
    return [int(x) for x in (np.round(np.linspace(1, T, 5) + 1e-10) - 1).astype(np.uint8)]


# ---- the seeded cases -----------------------------------------------------------------------------------------------------------------
# (H, W, T, N, bound_th, why).  Object 1 holds the top-left corner and runs along the top border into the top-right corner, object 2 holds
# the bottom-right corner and runs along the bottom border into the bottom-left corner: all four borders and corners are touched.  Further
# objects are ellipses inside.  segmentation is annotation shifted by a few pixels per frame, then 1 % of the pixels of BOTH maps get a
# random label.  The 70 x 150 case drops object 3 from segmentation, object 4 from annotation and object 5 from both.
CASES = [
    (20, 24, 3, 2, DEFAULT_BOUND_TH, "derived radius 1, the smallest"),
    (37, 53, 2, 3, 3, "odd sizes, partial tiles"),
    (37, 53, 2, 3, 2.5, "r2 = 6 with half-width 2: a non-integer threshold"),
    (70, 150, 2, 5, 8, "the 480p radius, halo across tile borders, objects absent from one map or both"),
    (80, 100, 1, 2, 32, "the largest radius: a disk larger than a tile"),
    (480, 854, 1, 2, DEFAULT_BOUND_TH, "the real frame, radius derived as 8"),
]
CASE_IDS = ["20x24-r1", "37x53-r3", "37x53-r2.5", "70x150-r8-absent", "80x100-r32", "480x854-default"]
GOLDEN_CASES = (0, 1, 2)            # the cases tests/golden/davis_jf.npz holds the reference's own results for


def _shift(a, dy, dx):
    out = np.zeros_like(a)
    H, W = a.shape
    ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    out[yd, xd] = a[ys, xs]
    return out


def make_case(ci):
    """(annotation, segmentation) uint8 [T, H, W] of case ``ci``; the same arrays on every call."""
    H, W, T, N, _, _ = CASES[ci]
    rng = np.random.default_rng(1000 + ci)
    yy, xx = np.mgrid[0:H, 0:W]
    ann = np.zeros((T, H, W), dtype=np.uint8)
    seg = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        a = np.zeros((H, W), dtype=np.uint8)
        for o in range(N, 2, -1):                                       # ellipses first, so that objects 1 and 2 keep the borders
            cy, cx = rng.uniform(0.25, 0.75) * H, rng.uniform(0.2, 0.8) * W
            ry, rx = rng.uniform(0.1, 0.22) * H, rng.uniform(0.08, 0.2) * W
            a[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = o
        h1, w1 = max(2, H // 3 + t), max(2, W // 4 + 2 * t)
        a[(yy < h1) & (xx < w1)] = 1
        a[(yy < max(2, H // 8)) & (xx >= w1)] = 1
        a[(yy >= H - h1) & (xx >= W - w1)] = 2
        a[(yy >= H - max(2, H // 8)) & (xx < W - w1)] = 2
        s = np.zeros_like(a)
        for o in range(1, N + 1):
            dy, dx = (int(v) for v in rng.integers(-3, 4, size=2))
            m = _shift(a == o, dy if o > 2 else abs(dy) % 2, dx if o > 2 else abs(dx) % 2)
            s[m & (s == 0)] = o
        s[(a == 1) & (yy < 2)] = 1                                      # the shifted objects keep their borders and corners
        s[(a == 2) & (yy >= H - 2)] = 2
        for m_ in (a, s):
            noise = rng.random((H, W)) < 0.01
            m_[noise] = rng.integers(0, N + 1, size=int(noise.sum()), dtype=np.uint8)
        if ci == 3:
            s[s == 3] = 0
            a[a == 4] = 0
            a[a == 5] = 0
            s[s == 5] = 0
        ann[t], seg[t] = a, s
    return ann, seg


_REFERENCE = {}


def reference(ci):
    """((annotation, segmentation), counts, J, F) of case ``ci`` in the disk form; computed once, shared, never modified."""
    if ci not in _REFERENCE:
        ann, seg = make_case(ci)
        counts = counts_disk(ann, seg, CASES[ci][3], CASES[ci][4])
        J, F = jf_from_counts(counts)
        for arr in (ann, seg, counts, J, F):
            arr.setflags(write=False)
        _REFERENCE[ci] = ((ann, seg), counts, J, F)
    return _REFERENCE[ci]
