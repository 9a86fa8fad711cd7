"""Frame preparation: ``naf_amd.prepare_views`` (one launch) against the torch composition of the same steps on the same device.

    python tools/image_prep_time.py [--iters N] [--out profiles/image_prep.txt]

Geometries: the DAVIS frame (480 x 854 uint8, ps 16) at ``ups_factor`` 1 and 8 -- the two views of ``davis_frame_views`` -- and the training
step (B 4, 3 x 512 x 512 fp32 -> the three views of ``training_views`` at ps 16: 512 x 512, its 256 x 256 shrink, 128 x 128).

  fused   naf_amd.prepare_views(src, views): one launch, no intermediate image; the DAVIS frame is the uint8 [H, W, 3] it was decoded as
  torch   the reference's lines on the device (evaluation/eval_video_seg.py:579-595, train.py:115-126 with utils/training.py:47):
          F.interpolate, two normalisations, F.interpolate again; its DAVIS input is the fp32 [1, 3, H, W] ``ToTensor`` made on the host,
          already on the device

``device ms`` is between two device events around the call, ``wall ms`` a host clock around the call and a synchronise: both contain the
host's work of issuing the call (for one launch that is most of the time).  ``graph replay ms`` takes the host out: the call is captured
into a graph once and 20 replays are timed between two device events, per replay.  The two arms alternate call by call after half a
second of warm-up each; per cell: median [min .. max].  The last block times the upload a frame loop pays:
the uint8 frame against the fp32 tensor, from pageable host memory, a host clock around the copy and a synchronise.  The work is launch-scale:
the table says what was measured, nothing more."""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naf_amd  # noqa: E402

BACKBONE_MEAN, BACKBONE_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)


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


def interleaved(arms, one, iters, warm_seconds=0.5):
    """{name: (text, median)}: every arm warmed, then the arms alternate call by call.  ``one`` is a function of the arm returning ms, or a
    dict with one such function per arm."""
    ones = one if isinstance(one, dict) else {name: one for name in arms}
    for name, fn in arms.items():
        t0, n = time.perf_counter(), 0
        while n < 2 or time.perf_counter() - t0 < warm_seconds:
            ones[name](fn)
            n += 1
    times = {name: [] for name in arms}
    for _ in range(iters):
        for name, fn in arms.items():
            times[name].append(ones[name](fn))
    out = {}
    for name, t in times.items():
        t.sort()
        out[name] = (f"{t[len(t) // 2]:.3f} [{t[0]:.3f} .. {t[-1]:.3f}]", t[len(t) // 2])
    return out


def replay_ms(fn, replays=20):
    """Device time of one call with the host out of the way: the call is captured into a graph once, and ``replays`` replays are timed
    between two device events.  Returns a function for ``interleaved``."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()

    def one(_):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / replays
    return one


def device_stats(views, dev):
    """The statistics as the reference holds them: [1, 3, 1, 1] tensors on the device, made once."""
    return [None if v.mean is None else (torch.tensor(v.mean, device=dev).view(1, 3, 1, 1), torch.tensor(v.std, device=dev).view(1, 3, 1, 1))
            for v in views]


def torch_views(x, views, stats):
    """The views as the reference composes them: one shared first resize, a normalisation per view, the second resize."""
    res, first = [], {}
    for v, st in zip(views, stats):
        key = (v.size, v.mode)
        if key not in first:
            first[key] = x if v.mode is None else F.interpolate(x, size=list(v.size), mode=v.mode, align_corners=False)
        y = first[key]
        if st is not None:
            m, s = st
            y = (y - m) / s
        if v.then is not None:
            y = F.interpolate(y, size=list(v.then[0]), mode=v.then[1], align_corners=False)
        res.append(y)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_prep_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say(f"# {torch.cuda.get_device_name(0)}; iters {args.iters}, arms alternate call by call, each warmed >= 0.5 s; ms: median [min .. max]")
    g = torch.Generator().manual_seed(0)
    frame = torch.randint(0, 256, (480, 854, 3), dtype=torch.uint8, generator=g)
    frame_f32 = frame.permute(2, 0, 1)[None].float().div(255).contiguous()                     # ToTensor, on the host
    batch = torch.rand(4, 3, 512, 512, generator=g)
    cases = []
    for f in (1, 8):
        views, grid, hr = naf_amd.davis_frame_views((480, 854), 16, f, BACKBONE_MEAN, BACKBONE_STD)
        cases.append((f"DAVIS ups_factor {f}: uint8 480 x 854 -> 480 x 848 (backbone), -> {hr[0]} x {hr[1]} bicubic (upsampler)", frame.to(dev),
                      frame_f32.to(dev), views))
    lr = naf_amd.lr_image_size(512, 512, 0.5, 16)
    cases.append((f"training: fp32 4 x 3 x 512 x 512 -> 512 x 512, {lr[0]} x {lr[1]}, 128 x 128", batch.to(dev), batch.to(dev),
                  naf_amd.training_views(512, (32, 32), lr, BACKBONE_MEAN, BACKBONE_STD)))
    for name, src, src_f32, views in cases:
        fused = lambda: naf_amd.prepare_views(src, views)                           # noqa: E731
        stats = device_stats(views, dev)
        composed = lambda: torch_views(src_f32, views, stats)                       # noqa: E731
        worst = max(float((a - b).abs().max()) for a, b in zip(fused(), composed()))
        say(f"{name}; max |fused - torch| over the views {worst:.3e}")
        arms = {"fused": fused, "torch": composed}
        d, w = interleaved(arms, device_ms, args.iters), interleaved(arms, wall_ms, args.iters)
        r = interleaved(arms, {arm: replay_ms(fn) for arm, fn in arms.items()}, args.iters)
        for arm in arms:
            say(f"  {arm:6s} device {d[arm][0]} ms | wall {w[arm][0]} ms | graph replay {r[arm][0]} ms")
        say(f"  torch / fused: device {d['torch'][1] / d['fused'][1]:.2f}x, wall {w['torch'][1] / w['fused'][1]:.2f}x, "
            f"graph replay {r['torch'][1] / r['fused'][1]:.2f}x")
    up = interleaved({"uint8": lambda: frame.to(dev), "fp32": lambda: frame_f32.to(dev)}, wall_ms, args.iters)
    say(f"upload of one 480 x 854 frame from pageable host memory: uint8 {frame.numel()} bytes, wall {up['uint8'][0]} ms | "
        f"fp32 {frame_f32.numel() * 4} bytes, wall {up['fp32'][0]} ms")
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
