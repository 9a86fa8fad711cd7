"""The fused probe objective against the composition it replaces, interleaved A/B in one process (device events, warmed).

    python tools/head_objective_time.py [--iters N] [--shapes G1,REF448] [--out profiles/head_objective.txt]

  evaluation step   (a) naf(image, feats, size, head=probe).argmax(1)                          the logits go to memory to be reduced to a byte
                    (b) naf(image, feats, size, head=probe, predict=True)                      the kernel's epilogue stores the label
  training step     (a) F.cross_entropy(naf(..., head=probe).float(), t, ignore_index=255).backward()
                    (b) naf(..., head=probe, target=t, ignore_index=255).backward()            loss map + softmax - onehot from one launch
  kernel alone      (a) ops.xna_head_forward (fp32 logits)    (b) ops.xna_head_objective: labels only / loss + gradient of the logits

Arm (a) is always the composition that existed before the objective was fused, never the new code against itself.  Arm (a) is timed TWICE,
interleaved with (b) -- a1, b, a2 per iteration -- so that every row shows the run-to-run spread a difference has to be held against.
Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) and the reference's own probing point REF448 (448^2, C 384, low-res 28^2, window 9),
N in {21, 151}, bf16 features, the probe in fp32 and in bf16.  Per row: median [min .. max] in ms over the timed iterations and the peak
device memory of one call of each arm (torch.cuda.max_memory_allocated, above what is resident before the call)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

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
    return f"{t[len(t) // 2]:.3f} [{t[0]:.3f} .. {t[-1]:.3f}]", t[len(t) // 2]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def ab(arm_a, arm_b, iters, warmup):
    """a1, b, a2 interleaved; returns the three stat strings, median(a) / median(b) and the peak memory of each arm."""
    t1, tb, t2 = [], [], []
    for it in range(warmup + iters):
        x, y, z = timed(arm_a), timed(arm_b), timed(arm_a)
        if it >= warmup:
            t1.append(x)
            tb.append(y)
            t2.append(z)
    (s1, m1), (sb, mb), (s2, m2) = stats(t1), stats(tb), stats(t2)
    return s1, s2, sb, 0.5 * (m1 + m2) / mb, peak_mb(arm_a), peak_mb(arm_b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--shapes", default="G1,REF448")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_objective_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say(f"# {torch.cuda.get_device_name(0)}; iters {args.iters}, warm-up {args.warmup}; per iteration a1, b, a2; ms: median [min .. max]; "
        f"a/b = mean of the two (a) medians over the (b) median; peak = MiB above the resident tensors")
    for name in args.shapes.split(","):
        H, h, C, k = SHAPES[name]
        model = NAF(kernel_size=k).to(dev).eval()
        heads = model.upsampler.num_heads
        img = torch.randn(1, 3, H, H, device=dev)
        ft = torch.randn(1, C, h, h, device=dev).to(torch.bfloat16)
        for N in (21, 151):
            t = torch.randint(0, N, (1, H, H), device=dev)
            t[torch.rand(1, H, H, device=dev) < 0.1] = 255
            for hdt in (torch.float32, torch.bfloat16):
                head = nn.Conv2d(C, N, 1).to(dev).to(hdt)
                tag = f"{name} N={N} probe {str(hdt)[6:]}"
                with torch.no_grad():
                    ev_a = lambda: model(img, ft, (H, H), head=head).argmax(1)
                    ev_b = lambda: model(img, ft, (H, H), head=head, predict=True)
                    same = float((ev_a() == ev_b()).float().mean())
                    s1, s2, sb, r, pa, pb = ab(ev_a, ev_b, args.iters, args.warmup)
                say(f"{tag} eval step : (a) logits.argmax {s1} | again {s2}   (b) predict=True {sb}   a/b {r:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB   "
                    f"labels equal on {same:.6f} of the pixels")

                def tr_a():
                    head.zero_grad(set_to_none=True)
                    F.cross_entropy(model(img, ft, (H, H), head=head).float(), t, ignore_index=255).backward()

                def tr_b():
                    head.zero_grad(set_to_none=True)
                    model(img, ft, (H, H), head=head, target=t, ignore_index=255).backward()

                tr_a()
                ga = head.weight.grad.float().clone()
                tr_b()
                gd = float((head.weight.grad.float() - ga).abs().max()) / max(float(ga.abs().max()), 1e-30)
                s1, s2, sb, r, pa, pb = ab(tr_a, tr_b, args.iters, args.warmup)
                say(f"{tag} train step: (a) cross_entropy(logits) {s1} | again {s2}   (b) target= {sb}   a/b {r:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB   "
                    f"max |dW_a - dW_b| / max |dW_a| {gd:.2e}")
                head.zero_grad(set_to_none=True)
                if hdt != torch.float32:
                    continue
                # the kernels alone on this forward's queries / keys: what the epilogue costs in an issue-bound kernel
                with torch.no_grad():
                    lr = ft.shape[-2:]
                    fus = lambda q5, tabs: ops.xna_head_select(q5, lr, N, k, rope_tables=tabs) == "fused"
                    q5, k5, tabs = model.guidance_qk(img, lr, (H, H), fusable=fus)
                    pv5, b32 = ops.project_head_values(head.weight, head.bias, ft, heads)
                    kw = dict(n_out=N, scale=model.upsampler.scale, rope_tables=tabs)
                    k_a = lambda: ops.xna_head_forward(q5, k5, pv5, b32, k, out_dtype=torch.float32, **kw)
                    k_l = lambda: ops.xna_head_objective(q5, k5, pv5, b32, k, want_labels=True, **kw)
                    k_g = lambda: ops.xna_head_objective(q5, k5, pv5, b32, k, target=t, ignore_index=255, want_loss=True, want_dlogits=True, **kw)
                    for what, k_b in (("labels only", k_l), ("loss + dlogits", k_g)):
                        s1, s2, sb, r, pa, pb = ab(k_a, k_b, args.iters, args.warmup)
                        say(f"    kernel alone (rotate-on-load {tabs is not None}): (a) naf_xna_head_fwd fp32 {s1} | again {s2}   (b) naf_xna_head_ce_fwd {what} {sb}   "
                            f"a/b {r:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB")
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
