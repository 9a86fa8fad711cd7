"""DAVIS J and F: the fused call against the torch composition of the same arithmetic, on one device (device events, warmed).

    python tools/davis_jf_time.py [--frames 70] [--objects 3] [--iters N] [--breakdown] [--out profiles/davis_jf.txt]

Shape: a DAVIS 480p sequence, T = 70 frames of 480 x 854, N = 3 objects, the default boundary threshold (bound_th 0.008: 8 pixels).  The
label maps are blobs (the argmax of upsampled low-resolution noise), the segmentation a perturbed copy of the annotation.

  fused   naf_amd.davis_jf(annotation, segmentation, num_objects=N): uint8 maps in, the [N, T, 6] counts, J and F out; one kernel launch
          plus the dozen elementwise fp64 operations on [N, T] that form J and F
  torch   the same counts composed from torch operations on the same device: one-hot masks [N * T, 1, H, W] in fp32, the Sobel pair as one
          conv2d on a reflect-padded mask, the disk as a conv2d with a (2r + 1)^2 0/1 kernel on the zero-padded boundary map, sums.  (The
          reference itself does this on the host: PNG files, float64 one-hot arrays, cv2.filter2D and scipy's distance transform per
          object and frame on one CPU thread -- not timed here.)

--breakdown adds the kernel alone (naf_davis_jf through the C ABI on a zeroed buffer that is not cleared between calls: the time does not
depend on the counters' values), at the default radius and at R = 1, 3, 16, 32, with an empty segmentation, and with both maps empty
(staging only).

GB/s is over the algorithmic 2 * T * H * W label bytes.  Every arm is warmed for at least half a second of device work before the timed
iterations; per row: median [min .. max] in ms.  The two arms' counts are compared and must be equal."""
import argparse
import ctypes as C
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naf_amd  # noqa: E402

H, W, BOUND_TH = 480, 854, 0.008


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(fn, iters, warm_seconds=0.5):
    t0 = time.perf_counter()
    n_warm = 0
    while n_warm < 2 or time.perf_counter() - t0 < warm_seconds:
        timed(fn)
        n_warm += 1
    t = sorted(timed(fn) for _ in range(iters))
    return f"{t[len(t) // 2]:.3f} [{t[0]:.3f} .. {t[-1]:.3f}]", t[len(t) // 2]


def blobs(T, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(T, N + 1, 9, 16, generator=g)
    low[:, 0] += 0.5
    ann_f = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    seg_f = ann_f + 0.15 * F.interpolate(torch.randn(T, N + 1, 30, 54, generator=g), size=(H, W), mode="bicubic", align_corners=False)
    return ann_f.argmax(1).to(torch.uint8).to(dev), seg_f.argmax(1).to(torch.uint8).to(dev)


def torch_counts(ann, seg, N, r2, half):
    """[N, T, 6] int64 from torch operations (the arithmetic of evaluation/eval_video_seg.py:145-226 in its disk form)."""
    T = ann.shape[0]
    dev = ann.device
    labels = torch.arange(1, N + 1, device=dev, dtype=torch.uint8)[:, None, None, None]
    g = (ann[None] == labels).reshape(N * T, 1, H, W)
    s = (seg[None] == labels).reshape(N * T, 1, H, W)
    sobel = torch.tensor([[[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], [[-1., -2., -1.], [0., 0., 0.], [1., 2., 1.]]], device=dev)[:, None]
    d = torch.arange(-half, half + 1, device=dev)
    disk = ((d[:, None] ** 2 + d[None, :] ** 2) <= r2).float()[None, None]

    def boundary(m):
        e = F.conv2d(F.pad(m.float(), (1, 1, 1, 1), mode="reflect"), sobel)
        return (e != 0).any(1, keepdim=True)

    def near(b):
        return F.conv2d(b.float(), disk, padding=half) > 0

    bg, bs = boundary(g), boundary(s)
    cols = [(g & s), (g | s), bs, bg, bs & near(bg), bg & near(bs)]
    return torch.stack([c.sum((1, 2, 3)) for c in cols], -1).reshape(N, T, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=70)
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--breakdown", action="store_true", help="also time the kernel alone, at several radii and on empty maps")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("davis_jf_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    T, N = args.frames, args.objects
    ann, seg = blobs(T, N, dev, 0)
    r2, half = naf_amd.ops._davis_bound(BOUND_TH, H, W, "davis_jf_time")
    say(f"# {torch.cuda.get_device_name(0)}; T {T}, {H} x {W}, N {N}, bound_th {BOUND_TH} (r2 {r2}, half-width {half}); uint8 label maps; "
        f"iters {args.iters}, each arm warmed >= 0.5 s; ms: median [min .. max]")
    gb = 2.0 * T * H * W / 1e9

    fused = lambda: naf_amd.davis_jf(ann, seg, num_objects=N, bound_th=BOUND_TH)   # noqa: E731
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = fused()
    torch.cuda.synchronize()
    peak_fused = (torch.cuda.max_memory_allocated() - base) / 1e6
    s_fused, m_fused = measure(fused, args.iters)
    say(f"fused  {s_fused} ms, {gb / (m_fused * 1e-3):.1f} GB/s over 2*T*H*W label bytes, peak allocation {peak_fused:.3f} MB beyond its inputs; "
        f"mean J {float(res.J.mean()):.4f}, mean F {float(res.F.mean()):.4f}")

    composed = lambda: torch_counts(ann, seg, N, r2, half)   # noqa: E731
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ref = composed()
    torch.cuda.synchronize()
    peak_torch = (torch.cuda.max_memory_allocated() - base) / 1e6
    s_torch, m_torch = measure(composed, max(3, args.iters // 3))
    equal = bool(torch.equal(ref, res.counts))
    say(f"torch  {s_torch} ms, {gb / (m_torch * 1e-3):.1f} GB/s, peak allocation {peak_torch:.1f} MB beyond its inputs | torch / fused "
        f"{m_torch / m_fused:.1f}x | counts equal: {equal}")
    if args.breakdown:
        from naf_amd import _lib
        lib = _lib.load()
        a = _lib.DavisJFArgs()
        a.T, a.H, a.W, a.N, a.r2, a.half_width = T, H, W, N, r2, half
        counts = torch.zeros(N, T, 6, dtype=torch.int64, device=dev)
        zero = torch.zeros_like(ann)
        a.annotation, a.segmentation, a.counts = ann.data_ptr(), seg.data_ptr(), counts.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def kernel():
            if lib.naf_davis_jf(C.byref(a), stream) != 0:
                raise SystemExit(_lib.last_error())

        say(f"kernel alone (C ABI), R = {half}: {measure(kernel, args.iters)[0]} ms")
        for r in (1, 3, 16, 32):
            a.r2, a.half_width = r * r, r
            say(f"kernel alone, R = {r}: {measure(kernel, args.iters)[0]} ms")
        a.r2, a.half_width, a.segmentation = r2, half, zero.data_ptr()
        say(f"kernel alone, R = {half}, empty segmentation: {measure(kernel, args.iters)[0]} ms")
        a.annotation = zero.data_ptr()
        say(f"kernel alone, R = {half}, both maps empty (staging only): {measure(kernel, args.iters)[0]} ms")
    if sink:
        sink.close()
    if not equal:
        raise SystemExit("the two arms' counts differ")


if __name__ == "__main__":
    main()
