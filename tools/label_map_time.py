"""Soft masks to a label map: the fused call against the torch composition of the same steps and against the reference's own form.

    python tools/label_map_time.py [--channels 4] [--iters N] [--out profiles/label_map.txt]

Shapes: the reference's two DAVIS geometries at 480p with ps 16 -- ``ups_factor`` 1 (30 x 53 -> 480 x 848 -> 480 x 854) and ``ups_factor`` 8
(240 x 424 -> 480 x 848 -> 480 x 854) -- with K = 4 smooth soft masks (the softmax of an upsampled low-resolution noise).

  fused      naf_amd.masks_to_labels(seg, mid, out): two launches, the [K, 480, 848] map never written, no host synchronisation
  torch      the same steps composed on the same device: F.interpolate (bilinear), the normalisation with torch.where instead of the
             reference's branch (no synchronisation), argmax, and the nearest resize as a gather through the same index tables
  reference  evaluation/eval_video_seg.py:444-457 as written: F.interpolate, the norm_mask loop with its ``if mask_cnt.max() > 0`` per
             channel, torch.max, ``.cpu()`` and the nearest resize on the host (Pillow where it is installed, a numpy gather through the
             same table where not); ends on the host, as the reference does before it writes the PNG

``device ms`` is between two device events around the call; ``wall ms`` is a host clock around the call and a synchronise, which is what a
loop over frames pays.  The reference form ends on the host and has no device-event reading.  Every arm is warmed for at least half a
second before the timed iterations; per cell: median [min .. max].  Both kernels are launch-scale work: the table says what was measured,
nothing more.  The fused labels and the composition's are compared; they may differ where two channels are within rounding of each other."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naf_amd  # noqa: E402

GEOMETRIES = [("ups_factor 1", (30, 53), (480, 848), (480, 854)), ("ups_factor 8", (240, 424), (480, 848), (480, 854))]


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(fn, one, iters, warm_seconds=0.5):
    t0 = time.perf_counter()
    n_warm = 0
    while n_warm < 2 or time.perf_counter() - t0 < warm_seconds:
        one(fn)
        n_warm += 1
    t = sorted(one(fn) for _ in range(iters))
    return f"{t[len(t) // 2]:.3f} [{t[0]:.3f} .. {t[-1]:.3f}]", t[len(t) // 2]


def smooth_masks(K, h, w, dev, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(1, K, -(-h // 6), -(-w // 6), generator=g)
    return torch.softmax(3.0 * F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False), dim=1).float().to(dev)


def torch_composition(seg, mid, ty, tx):
    u = F.interpolate(seg, size=list(mid), mode="bilinear", align_corners=False)[0]
    mx, mn = u.amax((1, 2), keepdim=True), u.amin((1, 2), keepdim=True)
    pos = mx > 0
    u = (u - torch.where(pos, mn, torch.zeros_like(mn))) / torch.where(pos, mx - mn, torch.ones_like(mn))
    return u.argmax(0).to(torch.uint8)[ty][:, tx]


def reference_form(seg, mid, out, tables):
    u = F.interpolate(seg, size=list(mid), mode="bilinear", align_corners=False, recompute_scale_factor=False)[0]
    for c in range(u.shape[0]):                        # norm_mask, :488-496
        m = u[c]
        if m.max() > 0:                                # the host synchronisation per channel
            m = m - m.min()
            m = m / m.max()
            u[c] = m
    _, lab = torch.max(u, dim=0)
    lab = np.array(lab.squeeze().cpu(), dtype=np.uint8)
    if tables is None:
        from PIL import Image
        return np.array(Image.fromarray(lab).resize((out[1], out[0]), 0))
    return lab[tables[0]][:, tables[1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_map_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    try:
        import PIL  # noqa: F401
        host_resize = "Pillow"
    except ImportError:
        host_resize = "numpy gather"
    K = args.channels
    say(f"# {torch.cuda.get_device_name(0)}; K {K} fp32 soft masks; iters {args.iters}, each arm warmed >= 0.5 s; ms: median [min .. max]; "
        f"the reference form's host resize: {host_resize}")
    for name, (h, w), mid, out in GEOMETRIES:
        seg = smooth_masks(K, h, w, dev, 0)
        ty, tx = naf_amd.ops.device_nearest_table(mid[0], out[0], dev).long(), naf_amd.ops.device_nearest_table(mid[1], out[1], dev).long()
        tables = None if host_resize == "Pillow" else (ty.cpu().numpy(), tx.cpu().numpy())
        fused = lambda: naf_amd.masks_to_labels(seg, mid, out)                      # noqa: E731
        composed = lambda: torch_composition(seg, mid, ty, tx)                      # noqa: E731
        reference = lambda: reference_form(seg, mid, out, tables)                   # noqa: E731
        a, b, c = fused(), composed(), reference()
        differ = int((a != b).sum())
        differ_ref = int((a.cpu().numpy() != c).sum())
        say(f"{name}: {h} x {w} -> {mid[0]} x {mid[1]} -> {out[0]} x {out[1]}; fused and composition differ on {differ} of {a.numel()} pixels, "
            f"fused and the reference form on {differ_ref}")
        rows = {}
        for arm, fn in (("fused", fused), ("torch", composed)):
            rows[arm] = (measure(fn, device_ms, args.iters), measure(fn, wall_ms, args.iters))
            say(f"  {arm:9s} device {rows[arm][0][0]} ms | wall {rows[arm][1][0]} ms")
        ref = measure(reference, wall_ms, args.iters)
        say(f"  reference device   -   | wall {ref[0]} ms")
        say(f"  wall ratios: torch / fused {rows['torch'][1][1] / rows['fused'][1][1]:.2f}x, reference / fused {ref[1] / rows['fused'][1][1]:.2f}x; "
            f"device ratio torch / fused {rows['torch'][0][1] / rows['fused'][0][1]:.2f}x")
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
