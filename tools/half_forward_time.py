"""float16 features through the forward: the native route against the route it replaces and against bf16, interleaved in one process
(device events, warmed).

    python tools/half_forward_time.py [--iters N] [--shapes G1,REF448] [--out profiles/half_features.txt]

  (a) the route float16 features took before they were served natively, rebuilt here from the same entry points (the bf16 / fp32
      kernels are unchanged): un-fused stem + RoPE / key pooling, the values through fp32 to bf16 (``ops.pack_values(feats.float())``),
      the attention kernel writing an fp32 [B, Ho, Wo, C] map, ``.to(float16)``
  (b) naf(image, feats.half(), size)         half values on the f16 matrix instruction, a float16 map written once, one foreign call
  (c) naf(image, feats.bfloat16(), size)     the bf16 call: same bytes, same matrix rate

Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) and the reference's own point REF448 (448^2, C 384, low-res 28^2, window 9).  Per row:
median [min .. max] of each arm over the timed iterations -- the spread to hold a difference against.  Then the attention kernel alone
(``ops.xna_forward`` with rotate-on-load on this forward's queries and keys) for half and for bf16 values, and the peak memory of one
call of each arm above what is allocated before it."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from naf_amd import NAF, ops  # noqa: E402

SHAPES = {"G1": (1024, 64, 768, 7), "REF448": (448, 28, 384, 9)}


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
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="G1,REF448")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("half_forward_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# iters {args.iters}, warm-up {args.warmup}, arms interleaved; times in ms: median [min .. max]")
    for name in args.shapes.split(","):
        H, h, C, k = SHAPES[name]
        model = NAF(kernel_size=k).to(dev).eval()
        heads = model.upsampler.num_heads
        Dv = C // heads
        img = torch.randn(1, 3, H, H, device=dev)
        ft32 = torch.randn(1, C, h, h, device=dev)
        fh, fb = ft32.half(), ft32.bfloat16()
        lr = (h, h)
        with torch.no_grad():
            def arm_a():
                q5, k5, tabs = model.guidance_qk(img, lr, (H, H), fuse_for=(Dv, torch.float32))
                v5 = ops.pack_values(fh.float()).view(1, h, h, heads, Dv).permute(0, 3, 1, 2, 4)
                o5 = ops.xna_forward(q5, k5, v5, k, out_dtype=torch.float32, scale=model.upsampler.scale, rope_tables=tabs)
                return o5.permute(0, 2, 3, 1, 4).reshape(1, H, H, C).permute(0, 3, 1, 2).to(torch.float16)
            arm_b = lambda: model(img, fh, (H, H))
            # the one-call plan is cached for ONE (shapes, dtype): (b) and (c) alternate, so each gets a model of its own
            model_c = NAF(kernel_size=k).to(dev).eval()
            model_c.load_state_dict(model.state_dict())
            arm_c = lambda: model_c(img, fb, (H, H))
            assert model._forward_plan(img, fh, (H, H)) is not None, "float16 features did not get the one-call plan"
            ta, tb, tc = [], [], []
            for it in range(args.warmup + args.iters):
                a, b, c = timed(arm_a), timed(arm_b), timed(arm_c)
                if it >= args.warmup:
                    ta.append(a)
                    tb.append(b)
                    tc.append(c)
            oa, ob = arm_a().float(), arm_b().float()
            (ma, la, ha), (mb, lb, hb), (mc, lc, hc) = stats(ta), stats(tb), stats(tc)
            say(f"{name} forward: (a) fp16 via bf16 values + fp32 map + cast {ma:.3f} [{la:.3f} .. {ha:.3f}]   (b) fp16 native {mb:.3f} [{lb:.3f} .. {hb:.3f}]   "
                f"(c) bf16 {mc:.3f} [{lc:.3f} .. {hc:.3f}]   a/b {ma / mb:.2f}x   b/c {mb / mc:.3f}   max |a - b| {float((oa - ob).abs().max()):.3e}")
            del oa, ob
            pa, pb, pc = peak_of(arm_a, dev), peak_of(arm_b, dev), peak_of(arm_c, dev)
            say(f"{name} peak memory of one call above the resident state: (a) {pa / 2**20:.1f} MiB   (b) {pb / 2**20:.1f} MiB   (c) {pc / 2**20:.1f} MiB")
            # the attention kernels alone, on the queries / keys of this forward
            q5, k5, tabs = model.guidance_qk(img, lr, (H, H), fuse_for=(Dv, torch.float16))
            vh5 = ops.pack_values(fh).view(1, h, h, heads, Dv).permute(0, 3, 1, 2, 4)
            vb5 = ops.pack_values(fb).view(1, h, h, heads, Dv).permute(0, 3, 1, 2, 4)
            run_h = lambda: ops.xna_forward(q5, k5, vh5, k, out_dtype=torch.float16, rope_tables=tabs)
            run_b = lambda: ops.xna_forward(q5, k5, vb5, k, out_dtype=torch.bfloat16, rope_tables=tabs)
            run_f = lambda: ops.xna_forward(q5, k5, vb5, k, out_dtype=torch.float32, rope_tables=tabs)
            th, tb2, tf = [], [], []
            for it in range(args.warmup + args.iters):
                x, y, z = timed(run_h), timed(run_b), timed(run_f)
                if it >= args.warmup:
                    th.append(x)
                    tb2.append(y)
                    tf.append(z)
            (mh, lh, hh), (m2, l2, h2), (mf, lf, hf) = stats(th), stats(tb2), stats(tf)
            by = H * H * heads * 64 * 2 + h * h * heads * 64 * 2 + vh5.numel() * 2 + H * H * C * 2
            say(f"    attention kernel (rotate-on-load {tabs is not None}), {by / 1e9:.3f} GB for 16-bit output: half {mh:.4f} [{lh:.4f} .. {hh:.4f}]   "
                f"bf16 {m2:.4f} [{l2:.4f} .. {h2:.4f}]   half/bf16 {mh / m2:.3f}   |   bf16 values, fp32 map {mf:.4f} [{lf:.4f} .. {hf:.4f}]")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
