"""Attention backward with and without a score gradient (naf_xna_bwd_scores, C ABI 0.4.3), interleaved A/B on the same inputs.

    python tools/bwd_scores_time.py [--iters N]

Shapes: G1 (1024^2, C 768, window 7, ratio 16) and REF448 (448^2, C 384, window 9, ratio 16), four heads of 64.  Prints the median of
each arm per shape (hip events around one backward call); run it under ``rocprofv3 --kernel-trace --stats`` for kernel times."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from naf_amd import ops  # noqa: E402

SHAPES = {"G1": (1024, 64, 768, 7), "REF448": (448, 28, 384, 9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for name, (H, h, C, k) in SHAPES.items():
        heads, Dq, Dv = 4, 64, C // 4
        q = torch.randn(1, H, H, heads, Dq, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2, 4)
        kl = torch.randn(1, h, h, heads, Dq, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2, 4)
        v = torch.randn(1, h, h, heads, Dv, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2, 4)
        do = torch.randn(1, H, H, heads, Dv, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2, 4)
        G = torch.randn(1, heads, H, H, k * k, device=dev, generator=g)
        sel = (ops.xna_backward_select(q, kl, v, k), ops.xna_backward_select(q, kl, v, k, dlogits=G))
        times = {"plain": [], "scores": []}
        for it in range(args.iters + 3):
            for arm in ("plain", "scores"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.xna_backward(q, kl, v, do, k, dlogits=G if arm == "scores" else None)
                e1.record()
                torch.cuda.synchronize()
                if it >= 3:
                    times[arm].append(e0.elapsed_time(e1))
        med = {a: sorted(t)[len(t) // 2] for a, t in times.items()}
        gbytes = G.numel() * 4 / 1e9
        print(f"{name}: kernels {sel[0]} / {sel[1]}; backward call median plain {med['plain']:.3f} ms, with dlogits {med['scores']:.3f} ms "
              f"(+{med['scores'] - med['plain']:.3f} ms; G = {gbytes:.2f} GB, {gbytes / 4e3 * 1e3:.3f} ms at 4 TB/s)", flush=True)


if __name__ == "__main__":
    main()
