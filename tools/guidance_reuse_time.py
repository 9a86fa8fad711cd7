"""Encode the image once: what ``naf.guide`` and ``naf.query`` save on the callers that upsample many things for one image.  Interleaved
A/B in one process (device events around whole arms, warmed), medians with their spread, peak memory.

    python tools/guidance_reuse_time.py [--iters N] [--cases backbones,sizes,click] [--out profiles/guidance_reuse.txt]

  backbones  five feature maps for ONE image at G1 geometry (1024^2, low-res 64^2, C 768, window 7) -- the reference's
             notebooks/inference.ipynb cells 15-16 upsample five backbones for the same image:
             (a) five image calls (the one-call plan, what a user runs today)      (b) guide(image) + five Guidance calls
  sizes      cell 19 of that notebook: one 448^2 image, one feature map (28^2, C 384, window 9) at 64, 128, 256, 512, 1024:
             (a) five image calls      (b) guide(image) + five Guidance calls (four sizes share one stem output, 64 pre-shrinks)
  click      one click of notebooks/attention_maps.ipynb cell 11 at 1024^2, window 9 (low-res 64^2, C 768), the image encoded before:
             (a) naf(g, feats, size, return_weights=True), then one pixel's rows      (b) naf.query(g, point, features=feats, ...)
             and (b') the first click on a fresh Guidance, which also builds the guidance level and the keys

Arm (b) builds its Guidance inside the timed region where the case says ``guide(image) +``: the comparison is one image's whole work."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from naf_amd import NAF  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def peak_of(fn, dev):
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak


def ab(say, name, arms, iters, warmup, dev):
    """Interleave the arms; one line of medians and spreads, one of peak memory."""
    times = [[] for _ in arms]
    for it in range(warmup + iters):
        for i, (_, fn) in enumerate(arms):
            t = timed(fn)
            if it >= warmup:
                times[i].append(t)
    st = [stats(t) for t in times]
    say(f"{name}: " + "   ".join(f"({label}) {m:.3f} [{lo:.3f} .. {hi:.3f}]" for (label, _), (m, lo, hi) in zip(arms, st))
        + f"   a/b {st[0][0] / st[1][0]:.2f}x")
    say(f"{name} peak memory of one pass above the resident state: "
        + "   ".join(f"({label}) {peak_of(fn, dev) / 2**20:.1f} MiB" for label, fn in arms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="backbones,sizes,click")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "guidance_reuse.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guidance_reuse_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cases = args.cases.split(",")
    say(f"# {torch.cuda.get_device_name(dev)}; iters {args.iters}, warm-up {args.warmup}, arms interleaved; ms per arm (all its calls): median [min .. max]")
    with torch.no_grad():
        if "backbones" in cases:
            model = NAF(kernel_size=7).to(dev).eval()
            img = torch.randn(1, 3, 1024, 1024, device=dev)
            feats = [torch.randn(1, 768, 64, 64, device=dev).bfloat16() for _ in range(5)]
            size = (1024, 1024)

            def image_calls():
                return [model(img, f, size) for f in feats]

            def guidance_calls():
                g = model.guide(img)
                return [model(g, f, size) for f in feats]

            a, b = image_calls(), guidance_calls()
            say(f"backbones: max |a - b| over the five maps {max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b)):.3e}")
            del a, b
            ab(say, "backbones (G1, five feature maps)", [("a: 5 image calls", image_calls), ("b: guide + 5 Guidance calls", guidance_calls)],
               args.iters, args.warmup, dev)
        if "sizes" in cases:
            model = NAF(kernel_size=9).to(dev).eval()
            img = torch.randn(1, 3, 448, 448, device=dev)
            ft = torch.randn(1, 384, 28, 28, device=dev).bfloat16()
            sizes = [(s, s) for s in (64, 128, 256, 512, 1024)]

            def image_calls():
                return [model(img, ft, s) for s in sizes]

            def guidance_calls():
                g = model.guide(img)
                return [model(g, ft, s) for s in sizes]

            a, b = image_calls(), guidance_calls()
            say(f"sizes: max |a - b| over the five sizes {max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b)):.3e}")
            del a, b
            ab(say, "sizes (448^2 image, 64 .. 1024)", [("a: 5 image calls", image_calls), ("b: guide + 5 Guidance calls", guidance_calls)],
               args.iters, args.warmup, dev)
        if "click" in cases:
            model = NAF(kernel_size=9).to(dev).eval()
            img = torch.randn(1, 3, 1024, 1024, device=dev)
            ft = torch.randn(1, 768, 64, 64, device=dev).bfloat16()
            size = (1024, 1024)
            pt = torch.tensor([[517, 301]], device=dev)
            g = model.guide(img, size)

            def dense_click():
                _, w = model(g, ft, size, return_weights=True)
                return w[0, :, 517, 301].clone()

            def point_click():
                return model.query(g, pt, features=ft, output_size=size, weights="logits")

            def first_click():
                return model.query(model.guide(img), pt, features=ft, output_size=size, weights="logits")

            a, b = dense_click(), point_click().logits[0]
            say(f"click: max |a - b| over the point's {a.numel()} scores {float((a - b).abs().max()):.3e}")
            del a, b
            ab(say, "click (1024^2, window 9)", [("a: return_weights=True + index", dense_click), ("b: query", point_click),
                                                 ("b': guide + query", first_click)], args.iters, args.warmup, dev)
            say(f"click: the Guidance holds {g.nbytes / 2**20:.1f} MiB")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
