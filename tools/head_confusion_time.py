"""The fused probe evaluation against what it replaces, interleaved A/B in one process (device events, warmed).

    python tools/head_confusion_time.py [--iters N] [--shapes G1,REF448] [--only-a] [--out profiles/head_confusion.txt]

  evaluation step   (a) pred = naf(image, feats, size, head=probe, predict=True), then the confusion matrix as a user writes it in torch:
                        mask = target != 255; cm += bincount(target[mask] * N + pred[mask], minlength=N * N).view(N, N)
                    (b) naf(image, feats, size, head=probe, target=target, ignore_index=255, confusion=cm)
  kernel alone      (a) naf_xna_head_ce_fwd, labels only       (b) naf_xna_head_cm_fwd, the matrix only (no label map written),
                    on hashed targets and with every pixel on ONE counter (constant target, a bias that makes one class win everywhere)

Arm (a) of the evaluation step never touches the code this tool's (b) measures: ``predict=True`` runs the classification kernel as it was
before the confusion matrix existed, and the counting is torch's.  ``--only-a`` times arm (a) alone, three times per iteration, so that the
same tool run with ``NAF_HIP_LIB`` pointing at a build of an earlier commit (which has no naf_xna_head_cm_fwd; load it through an earlier
checkout of the package) gives the yardstick on that build.  Arm (a) is timed TWICE, interleaved with (b) -- a1, b, a2 per iteration --
so every row shows the run-to-run spread a difference has to be held against.  Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) and the
reference's probing point REF448 (448^2, C 384, low-res 28^2, window 9), N in {21, 151}, bf16 features, fp32 probe.  Per row: median
[min .. max] in ms over the timed iterations."""
import argparse
import os
import sys

import torch
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


def ab(arm_a, arm_b, iters, warmup):
    """a1, b, a2 interleaved; returns the three stat strings, the three medians."""
    t1, tb, t2 = [], [], []
    for it in range(warmup + iters):
        x, y, z = timed(arm_a), timed(arm_b), timed(arm_a)
        if it >= warmup:
            t1.append(x)
            tb.append(y)
            t2.append(z)
    (s1, m1), (sb, mb), (s2, m2) = stats(t1), stats(tb), stats(t2)
    return s1, s2, sb, m1, m2, mb


def verdict(m1, m2, mb):
    """(b) against the spread of (a)'s own two readings: not slower when its median is at most the larger of the two (a) medians."""
    return f"a/b {0.5 * (m1 + m2) / mb:.2f}x, (b) {'NOT SLOWER' if mb <= max(m1, m2) else 'SLOWER'} than (a) (medians {m1:.3f} / {m2:.3f} vs {mb:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--shapes", default="G1,REF448")
    ap.add_argument("--only-a", action="store_true", help="time arm (a) of the evaluation step alone (a build without the confusion entry)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_confusion_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say(f"# {torch.cuda.get_device_name(0)}; library {os.environ.get('NAF_HIP_LIB') or 'in tree'}; iters {args.iters}, warm-up {args.warmup}; "
        f"per iteration a1, b, a2; ms: median [min .. max]")
    for name in args.shapes.split(","):
        H, h, C, k = SHAPES[name]
        model = NAF(kernel_size=k).to(dev).eval()
        heads = model.upsampler.num_heads
        img = torch.randn(1, 3, H, H, device=dev)
        ft = torch.randn(1, C, h, h, device=dev).to(torch.bfloat16)
        for N in (21, 151):
            t = torch.randint(0, N, (1, H, H), device=dev)
            t[torch.rand(1, H, H, device=dev) < 0.1] = 255
            head = nn.Conv2d(C, N, 1).to(dev)
            tag = f"{name} N={N}"
            cm_a = torch.zeros(N, N, dtype=torch.int64, device=dev)
            cm_b = torch.zeros(N, N, dtype=torch.int64, device=dev)

            def ev_a():
                pred = model(img, ft, (H, H), head=head, predict=True)
                mask = t != 255
                cm_a.add_(torch.bincount(t[mask] * N + pred[mask], minlength=N * N).view(N, N))

            with torch.no_grad():
                if args.only_a:
                    s1, s2, sb, m1, m2, mb = ab(ev_a, ev_a, args.iters, args.warmup)
                    say(f"{tag} eval step, arm (a) only: predict=True + mask / bincount {s1} | again {sb} | again {s2}")
                    continue
                ev_b = lambda: model(img, ft, (H, H), head=head, target=t, ignore_index=255, confusion=cm_b)
                ev_a()
                ev_b()
                same = torch.equal(cm_a, cm_b)
                s1, s2, sb, m1, m2, mb = ab(ev_a, ev_b, args.iters, args.warmup)
                say(f"{tag} eval step : (a) predict=True + mask / bincount {s1} | again {s2}   (b) confusion=cm {sb}   {verdict(m1, m2, mb)}   "
                    f"matrices equal after one call each: {same}")
                # the kernels alone on this forward's queries / keys
                lr = ft.shape[-2:]
                fus = lambda q5, tabs: ops.xna_head_select(q5, lr, N, k, rope_tables=tabs) == "fused"
                q5, k5, tabs = model.guidance_qk(img, lr, (H, H), fusable=fus)
                pv5, b32 = ops.project_head_values(head.weight, head.bias, ft, heads)
                kw = dict(n_out=N, scale=model.upsampler.scale, rope_tables=tabs, path="fused")
                one = torch.full_like(t, 3)
                b_one = b32.clone()
                b_one[5] = 1.0e4
                for what, tt, bb in (("hashed targets", t, b32), ("all pixels on one counter", one, b_one)):
                    cm_k = torch.zeros(N, N, dtype=torch.int64, device=dev)
                    k_a = lambda: ops.xna_head_objective(q5, k5, pv5, bb, k, want_labels=True, **kw)
                    k_b = lambda: ops.xna_head_objective(q5, k5, pv5, bb, k, target=tt, ignore_index=255, confusion=cm_k, **kw)
                    k_b()
                    nz = int((cm_k != 0).sum())
                    s1, s2, sb, m1, m2, mb = ab(k_a, k_b, args.iters, args.warmup)
                    say(f"    kernel alone, {what} ({nz} non-zero entries; rotate-on-load {tabs is not None}): (a) naf_xna_head_ce_fwd labels only {s1} | again {s2}   "
                        f"(b) naf_xna_head_cm_fwd matrix only {sb}   {verdict(m1, m2, mb)}")
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
