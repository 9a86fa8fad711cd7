"""The fused linear head against the composition it replaces, interleaved A/B in one process (device events, warmed).

    python tools/head_forward_time.py [--iters N] [--shapes G1,REF448]

  (a) head(naf(image, feats, size))          the upsampled [B, C, Ho, Wo] features go to memory and the 1x1 convolution reads them back
  (b) naf(image, feats, size, head=head)     the head is applied on the low-res grid, the head-summed attention writes N channels

Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) and the reference's own probing point REF448 (448^2, C 384, low-res 28^2, window 9),
N in {21, 151}, bf16 features, four attention heads of 64, the head in bf16 and in fp32 (arm (a) then casts the features, as a user's
fp32 classifier on bf16 features has to).  Per row: median [min .. max] of each arm over the timed iterations -- the spread to hold a
difference against -- then the head-summed kernel alone (``ops.xna_head_forward``, rotate-on-load) with the bytes it has to move, computed
here from the shapes (queries + one pass over the keys and projected values + the logits; RoPE tables excluded), its share of the
8 TB/s HBM bound, and the shipped cell kernel (``ops.xna_forward`` on the features) on the same queries for scale."""
import argparse
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from naf_amd import NAF, ops  # noqa: E402

SHAPES = {"G1": (1024, 64, 768, 7), "REF448": (448, 28, 384, 9)}
HBM_TBS = 8.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="G1,REF448")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_forward_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    print(f"# iters {args.iters}, warm-up {args.warmup}, arms interleaved; times in ms: median [min .. max]")
    for name in args.shapes.split(","):
        H, h, C, k = SHAPES[name]
        model = NAF(kernel_size=k).to(dev).eval()
        heads = model.upsampler.num_heads
        img = torch.randn(1, 3, H, H, device=dev)
        ft = torch.randn(1, C, h, h, device=dev).to(torch.bfloat16)
        with torch.no_grad():
            for N in (21, 151):
                for hdt in (torch.bfloat16, torch.float32):
                    head = nn.Conv2d(C, N, 1).to(dev).to(hdt)
                    arm_a = lambda: head(model(img, ft, (H, H)).to(hdt))
                    arm_b = lambda: model(img, ft, (H, H), head=head)
                    ta, tb = [], []
                    for it in range(args.warmup + args.iters):
                        a, b = timed(arm_a), timed(arm_b)
                        if it >= args.warmup:
                            ta.append(a)
                            tb.append(b)
                    diff = float((arm_a().float() - arm_b().float()).abs().max())
                    (ma, la, ha), (mb, lb, hb) = stats(ta), stats(tb)
                    print(f"{name} N={N} head {str(hdt)[6:]}: (a) head(naf(...)) {ma:.3f} [{la:.3f} .. {ha:.3f}]   (b) naf(..., head=) {mb:.3f} [{lb:.3f} .. {hb:.3f}]   "
                          f"a/b {ma / mb:.2f}x   max |a - b| {diff:.3e}", flush=True)
                    # the kernels alone, on the queries / keys of this forward
                    lr = ft.shape[-2:]
                    fus = lambda q5, tabs: ops.xna_head_select(q5, lr, N, k, out_dtype=hdt, rope_tables=tabs) == "fused"
                    q5, k5, tabs = model.guidance_qk(img, lr, (H, H), fusable=fus)
                    pv5, b32 = ops.project_head_values(head.weight, head.bias, ft, heads)
                    sel = ops.xna_head_select(q5, lr, N, k, out_dtype=hdt, rope_tables=tabs)
                    run_h = lambda: ops.xna_head_forward(q5, k5, pv5, b32, k, n_out=N, out_dtype=hdt, rope_tables=tabs)
                    vp = ops.pack_values(ft)
                    v5 = vp.view(1, h, h, heads, C // heads).permute(0, 3, 1, 2, 4)
                    run_c = lambda: ops.xna_forward(q5, k5, v5, k, out_dtype=torch.bfloat16, rope_tables=tabs)
                    th, tc = [], []
                    for it in range(args.warmup + args.iters):
                        x, y = timed(run_h), timed(run_c)
                        if it >= args.warmup:
                            th.append(x)
                            tc.append(y)
                    osz = 2 if hdt == torch.bfloat16 else 4
                    by = H * H * heads * 64 * 2 + h * h * heads * 64 * 2 + pv5.numel() * 2 + H * H * N * osz
                    by_c = H * H * heads * 64 * 2 + h * h * heads * 64 * 2 + v5.numel() * 2 + H * H * C * 2
                    (mh, lh, hh), (mc, lc, hc) = stats(th), stats(tc)
                    print(f"    kernel ({sel}, rotate-on-load {tabs is not None}): {mh:.4f} [{lh:.4f} .. {hh:.4f}] ms for {by / 1e9:.3f} GB = "
                          f"{by / 1e9 / mh:.2f} TB/s, {by / (HBM_TBS * 1e9) / mh:.2f} of the HBM bound ({by / (HBM_TBS * 1e9):.4f} ms)   |   "
                          f"cell kernel on the features: {mc:.4f} [{lc:.4f} .. {hc:.4f}] ms for {by_c / 1e9:.3f} GB, {by_c / (HBM_TBS * 1e9) / mc:.2f} of its bound", flush=True)


if __name__ == "__main__":
    main()
