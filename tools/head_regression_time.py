"""The fused dense regression probe against the composition it replaces, interleaved A/B in one process (device events, warmed).

    python tools/head_regression_time.py [--iters N] [--shapes G1,REF448] [--out profiles/head_regression.txt]

  training step     (a) F.l1_loss(naf(image, feats, size, head=probe).float()[sel], t[sel]).backward()      logits, boolean gather, autograd
                    (b) naf(image, feats, size, head=probe, dense_target=t, valid=m).backward()              loss map + gradient from one launch
  evaluation step   (a) naf(..., head=probe), then the depth error sums in torch (ops.head_errors_from_prediction)
                    (b) naf(..., head=probe, dense_target=t, valid=m, errors=acc)                            ten sums from the kernel's epilogue
  kernel alone      (a) ops.xna_head_forward (fp32 logits)    (b) ops.xna_head_regression: loss + gradient / error sums only

Arm (a) is always the path that existed before the regression epilogue, never the new code against itself.  Arm (a) is timed TWICE,
interleaved with (b) -- a1, b, a2 per iteration -- so that every row shows the run-to-run spread a difference has to be held against.
Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) and the reference's own probing point REF448 (448^2, C 384, low-res 28^2, window 9),
N in {1, 3}, bf16 features, an fp32 probe.  Per row: median [min .. max] in ms over the timed iterations and the peak device memory of
one call of each arm (torch.cuda.max_memory_allocated, above what is resident before the call)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from naf_amd import NAF, ops  # noqa: E402
from head_objective_time import SHAPES, ab  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--shapes", default="G1,REF448")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_regression_time.py measures on a ROCm device; none found")
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
        valid = torch.rand(1, H, H, device=dev) >= 0.1
        for N in (1, 3):
            t = torch.exp(0.5 * torch.randn(1, N, H, H, device=dev))
            sel = valid.unsqueeze(1).expand_as(t)
            head = nn.Conv2d(C, N, 1).to(dev)
            with torch.no_grad():
                head.bias.fill_(1.0)
            tag = f"{name} N={N}"

            def tr_a():
                head.zero_grad(set_to_none=True)
                F.l1_loss(model(img, ft, (H, H), head=head).float()[sel], t[sel]).backward()

            def tr_b():
                head.zero_grad(set_to_none=True)
                model(img, ft, (H, H), head=head, dense_target=t, valid=valid).backward()

            tr_a()
            ga = head.weight.grad.float().clone()
            tr_b()
            gd = float((head.weight.grad.float() - ga).abs().max()) / max(float(ga.abs().max()), 1e-30)
            s1, s2, sb, r, pa, pb = ab(tr_a, tr_b, args.iters, args.warmup)
            say(f"{tag} train step: (a) l1_loss(logits[sel]) {s1} | again {s2}   (b) dense_target= {sb}   a/b {r:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB   "
                f"max |dW_a - dW_b| / max |dW_a| {gd:.2e}")
            head.zero_grad(set_to_none=True)
            with torch.no_grad():
                lr = ft.shape[-2:]
                fus = lambda q5, tabs: ops.xna_head_select(q5, lr, N, k, rope_tables=tabs) == "fused"
                q5, k5, tabs = model.guidance_qk(img, lr, (H, H), fusable=fus)
                pv5, b32 = ops.project_head_values(head.weight, head.bias, ft, heads)
                kw = dict(n_out=N, scale=model.upsampler.scale, rope_tables=tabs)
                k_a = lambda: ops.xna_head_forward(q5, k5, pv5, b32, k, out_dtype=torch.float32, **kw)
                rows = [("loss + dlogits", lambda: ops.xna_head_regression(q5, k5, pv5, b32, k, target=t, valid=valid, want_loss=True, want_dlogits=True, **kw))]
                if N == 1:
                    acc = torch.zeros(10, dtype=torch.float64, device=dev)
                    ev_a = lambda: ops.head_errors_from_prediction(model(img, ft, (H, H), head=head), t, valid)
                    ev_b = lambda: model(img, ft, (H, H), head=head, dense_target=t, valid=valid, errors=acc)
                    ra, rb = ev_a(), ev_b().clone()
                    dev_rel = float(((ra - rb).abs() / ra.abs().clamp_min(1e-30)).max())
                    s1, s2, sb, r, pa, pb = ab(ev_a, ev_b, args.iters, args.warmup)
                    say(f"{tag} eval step : (a) logits, torch error sums {s1} | again {s2}   (b) errors=acc {sb}   a/b {r:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB   "
                        f"max relative difference of the ten sums {dev_rel:.2e}")
                    rows.append(("error sums only", lambda: ops.xna_head_regression(q5, k5, pv5, b32, k, target=t, valid=valid, errors=acc, **kw)))
                # the kernels alone on this forward's queries / keys: what the epilogue costs in an issue-bound kernel
                for what, k_b in rows:
                    s1, s2, sb, r, pa, pb = ab(k_a, k_b, args.iters, args.warmup)
                    say(f"    kernel alone (rotate-on-load {tabs is not None}): (a) naf_xna_head_fwd fp32 {s1} | again {s2}   (b) naf_xna_head_reg_fwd {what} {sb}   "
                        f"a/b {r:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB")
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
