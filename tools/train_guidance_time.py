"""One training step at the reference's own geometry (train.py:113-137 with config/base.yaml: the guidance image is 4x the output per axis,
so naf.py:34 is a real 4x4 pooling on every step): B = 4, image 128^2, output 32^2, features 384 x 16^2, window 9, bf16 autocast, .train(),
loss.backward().  Reports the step time (device events around every step: 20 warm-up steps, then --steps >= 200 timed ones), the device
kernels of one step in launch order with their counts (what runs between the stem's last layer and naf_rope_pool_fwd, and between
naf_rope_pool_bwd and the stem's first backward launch, can be read off it), and torch.cuda.max_memory_allocated.

One process measures one tree: --repo names the checkout whose naf_amd is imported (default: this one), so two commits are compared by
running this file against each in turn, every run under a time limit of its own:

    timeout -k 10 300 python tools/train_guidance_time.py --label this
    timeout -k 10 300 python tools/train_guidance_time.py --label parent --repo /path/to/parent/checkout
"""
import argparse
import collections
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()
if args.steps < 200:
    ap.error("--steps must be at least 200")
sys.path.insert(0, os.path.abspath(args.repo))

import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

from naf_amd import NAF  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
B, C, lr, out, img_sz, ks = 4, 384, 16, 32, 128, 9
model = NAF(kernel_size=ks).to(dev).train()
img = torch.randn(B, 3, img_sz, img_sz, device=dev)
ft = torch.randn(B, C, lr, lr, device=dev)
tgt = torch.randn(B, C, out, out, device=dev)


def step():
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        o = model(img, ft, (out, out))
    loss = (o.float() - tgt).pow(2).mean()
    loss.backward()
    return loss


for _ in range(args.warmup):
    step()
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
for e0, e1 in ev:
    e0.record()
    step()
    e1.record()
torch.cuda.synchronize()
ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
peak = torch.cuda.max_memory_allocated()

with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
    step()
    torch.cuda.synchronize()
kern = sorted((e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA), key=lambda e: e.time_range.start)
short = lambda n: n.split("(")[0][:90]
counts = collections.Counter(short(e.name) for e in kern)
aten_ops = collections.Counter(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU and e.name.startswith("aten::"))

print(f"== {args.label}: {os.path.abspath(args.repo)}")
print(f"device kernels of one step, in launch order ({len(kern)} launches):")
for i, e in enumerate(kern):
    print(f"  {i:3d}  {short(e.name)}")
print("kernel counts per step:")
for n, c in sorted(counts.items(), key=lambda t: (-t[1], t[0])):
    print(f"  {c:3d}  {n}")
print(json.dumps({"label": args.label, "steps": args.steps, "warmup": args.warmup, "step_ms_median": ms[len(ms) // 2],
                  "step_ms_mean": sum(ms) / len(ms), "step_ms_p10": ms[len(ms) // 10], "step_ms_p90": ms[len(ms) * 9 // 10],
                  "launches_per_step": len(kern), "peak_memory_bytes": peak,
                  "aten_pool_or_bilinear_ops": {n: c for n, c in aten_ops.items() if "adaptive_avg_pool" in n or "upsample_bilinear" in n}}))
