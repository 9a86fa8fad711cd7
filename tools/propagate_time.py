"""Label propagation: the fused call against the dense torch composition it replaces, on one device (device events, warmed).

    python tools/propagate_time.py [--factors 1,2,4,8] [--iters N] [--dense-limit-gb G] [--out profiles/label_propagation.txt]

Grids are 480p-like: (34 f) x (61 f) for an upsampling factor f of a patch-14 backbone's 34 x 61 token grid, with the reference's own
settings (config/eval_video_seg.yaml): C = 384, n = 8 context frames, radius 12 (a 25 x 25 window), topk 5, temperature 0.1; K = 8 objects.

  fused   naf_amd.propagate_labels on FrameFeatures packed once per frame (what a caller's frame queue holds), so the row is the
          propagation kernel alone; `pack` is pack_frame of one bf16 NCHW frame (transpose copy + inverse norms), paid once per frame
  dense   label_propagation as the reference writes it (evaluation/eval_video_seg.py:539-560) on the same device, in fp32: normalise, bmm,
          exp, multiply by the [h*w, h*w] neighbourhood mask (built once, outside the timed region, as the reference caches it), topk along
          the source axis, threshold, normalise, mm.  Its affinity tensor is n * (h*w)^2 fp32 values; it is run where that tensor and
          its temporaries (about 3 x) fit under --dense-limit-gb, and its peak allocation is recorded; beyond, the row gives the size it
          would need

No ratio is fixed in advance: at f = 1 the dense path is tiny.  Every arm is warmed for at least half a second of device work (clocks
settled, code objects loaded) before the timed iterations; per row: median [min .. max] in ms."""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naf_amd  # noqa: E402

C, N_CTX, RADIUS, TOPK, TEMP, K = 384, 8, 12, 5, 0.1, 8


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


def dense_mask(h, w, radius, dev):
    ii, jj = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    return (((ii[:, None] - ii[None, :]).abs() <= radius) & ((jj[:, None] - jj[None, :]).abs() <= radius)).float()


def dense_propagation(target, context, segs, mask, topk, temp):
    """eval_video_seg.py:539-560 on [C, h, w] features."""
    Cc, h, w = target.shape
    n, Kk = segs.shape[:2]
    feat_tar = F.normalize(target.reshape(Cc, h * w).T.float(), dim=1, p=2)
    feat_sources = F.normalize(torch.stack([f.reshape(Cc, h * w) for f in context]).float(), dim=1, p=2)
    aff = torch.exp(torch.bmm(feat_tar.unsqueeze(0).repeat(n, 1, 1), feat_sources) / temp)
    aff *= mask.unsqueeze(0)
    aff = aff.transpose(2, 1).reshape(-1, h * w)
    tk_val, _ = torch.topk(aff, dim=0, k=topk)
    tk_val_min, _ = torch.min(tk_val, dim=0)
    aff[aff < tk_val_min] = 0
    aff = aff / torch.sum(aff, keepdim=True, dim=0)
    sg = segs.reshape(n, Kk, -1).transpose(2, 1).reshape(-1, Kk).T
    return torch.mm(sg, aff).reshape(1, Kk, h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", default="1,2,4,8")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dense-limit-gb", type=float, default=40.0, help="run the dense arm where 3 x its affinity tensor fits under this")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("propagate_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say(f"# {torch.cuda.get_device_name(0)}; C {C}, n {N_CTX}, radius {RADIUS}, topk {TOPK}, T {TEMP}, K {K}; bf16 features; iters {args.iters}, "
        f"each arm warmed >= 0.5 s; ms: median [min .. max]; dense arm run while 3 x affinity tensor <= {args.dense_limit_gb:g} GB")
    for f in (int(x) for x in args.factors.split(",")):
        h, w = 34 * f, 61 * f
        g = torch.Generator().manual_seed(f)
        target = torch.randn(C, h, w, generator=g).to(torch.bfloat16).to(dev)
        context = [torch.randn(C, h, w, generator=g).to(torch.bfloat16).to(dev) for _ in range(N_CTX)]
        segs = torch.rand(N_CTX, K, h, w, generator=g).to(dev)
        tgt, ctx = naf_amd.pack_frame(target), [naf_amd.pack_frame(x) for x in context]
        s_pack, _ = measure(lambda: naf_amd.pack_frame(target), args.iters)
        fused = lambda: naf_amd.propagate_labels(tgt, ctx, segs, radius=RADIUS, topk=TOPK, temperature=TEMP)
        out = fused()
        s_fused, m_fused = measure(fused, args.iters)
        flops = 2.0 * C * (h * w) * N_CTX * (2 * RADIUS + 1) ** 2          # counted inside the window, one pass
        aff_gb = N_CTX * float(h * w) ** 2 * 4 / 1e9
        line = (f"f={f} grid {h}x{w} ({h * w} px): fused {s_fused} ms ({flops / m_fused / 1e9:.1f} TFLOP/s counted inside the window, one pass) | "
                f"pack one frame {s_pack} ms | dense affinity tensor {aff_gb:.2f} GB")
        if 3 * aff_gb <= args.dense_limit_gb:
            mask = dense_mask(h, w, RADIUS, dev)
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            dense = lambda: dense_propagation(target, context, segs, mask, TOPK, TEMP)
            ref = dense()
            peak = (torch.cuda.max_memory_allocated() - base) / 1e9
            s_dense, m_dense = measure(dense, max(3, args.iters // 3))
            diff = float((out - ref).abs().max())
            line += (f" | dense {s_dense} ms, peak allocation {peak:.2f} GB beyond its inputs and mask ({mask.numel() * 4 / 1e9:.2f} GB) | "
                     f"dense / fused {m_dense / m_fused:.2f}x | max |fused - dense(fp32)| {diff:.2e}")
            del mask, ref
            torch.cuda.empty_cache()
        else:
            line += f" | dense NOT RUN: the affinity tensor alone is {aff_gb:.1f} GB (x 3 with its temporaries), the mask {float(h * w) ** 2 * 4 / 1e9:.1f} GB more"
        say(line)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
