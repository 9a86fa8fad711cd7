"""The training step's objective: ``naf(image, feats, size, regress=t)`` with the loss in the attention kernel's epilogue against the
composed step, on one device.

    python tools/regress_objective_time.py [--iters N] [--rounds R] [--geometry train|r14|both] [--out profiles/regress_objective.txt]
    python tools/regress_objective_time.py --repo /path/to/parent/checkout --label parent      # the plain step of another tree

Arms (train.py:127-132 in .train() mode under bf16 autocast, zero_grad + forward + loss.backward()):
  fused     naf(image, feats, size, regress=t)                       "auto" at the training geometry; "fused" forced at ratio 14, where
                                                                     "auto" composes (naf_xna_select runs the cell kernel there)
  composed  naf(image, feats, size, regress=t, regress_path="composed")
  plain     F.mse_loss(naf(image, feats, size).float(), t.float())   the expression a user writes today; the ONLY arm a tree without
                                                                     ``regress=`` has (--repo names the tree whose naf_amd is imported)
Geometries: the reference's training geometry (config/base.yaml: B 4, image 128^2, features 768 x 16^2 -> 32^2, window 9) and ratio 14
(B 2, image 448^2, features 384 x 32^2 -> 448^2, window 9).

Protocol: every arm warmed >= 0.5 s; then `rounds` rounds in which the arms alternate, each timed as the mean of `iters` back-to-back
steps between two device events; per arm the median [min .. max] over the rounds.  The spread the tool reports for a comparison is the
larger of the two arms' (max - min); a difference of medians inside it is not a difference.  Peak memory: torch.cuda.max_memory_allocated
over three steps of the arm alone.  Kernel table: one profiled step per arm (a run of its own, after the timing), the attention forward /
backward kernels' device time and the number of device kernels between them.  No ratio is fixed in advance; the file states what was measured."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--geometry", default="both", choices=("train", "r14", "both"))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

import naf_amd  # noqa: E402
from naf_amd import NAF  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("regress_objective_time.py measures on a ROCm device; none found (not measured)")
dev = torch.device("cuda:0")
HAS_REGRESS = "regress" in NAF.forward.__code__.co_varnames
GEOMS = {"train": (4, 128, 768, 16, 32, "auto"), "r14": (2, 448, 384, 32, 448, "fused")}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(arms, iters, rounds, warm_seconds=0.5):
    for fn in arms.values():
        t0, n = time.perf_counter(), 0
        while n < 3 or time.perf_counter() - t0 < warm_seconds:
            timed(fn, 1)
            n += 1
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    return {k: sorted(v) for k, v in t.items()}


def kernel_table(fn):
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = sorted((e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA), key=lambda e: e.time_range.start)
    names = [e.name for e in ev]
    is_fwd = lambda n: any(s in n for s in ("xna_union_kernel", "xna_mfma_kernel", "xna_slide_kernel"))
    is_bwd = lambda n: any(s in n for s in ("xna_rows_bwd_kernel", "xna_bwd2_kernel", "xna_generic_bwd_kernel"))
    fwd = [i for i, n in enumerate(names) if is_fwd(n)]
    bwd = [i for i, n in enumerate(names) if is_bwd(n)]
    us = lambda idx: sum(ev[i].time_range.elapsed_us() for i in idx)
    between = names[fwd[-1] + 1:bwd[0]] if fwd and bwd else []
    return len(names), us(fwd), us(bwd), between


for gname in (("train", "r14") if args.geometry == "both" else (args.geometry,)):
    B, img_sz, C, lr, out, fused_path = GEOMS[gname]
    torch.manual_seed(0)
    model = NAF(kernel_size=9).to(dev).train()
    img = torch.randn(B, 3, img_sz, img_sz, device=dev)
    ft = torch.randn(B, C, lr, lr, device=dev)
    tgt = torch.randn(B, C, out, out, device=dev)

    def make(kind):
        def step():
            model.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                if kind == "plain":
                    loss = F.mse_loss(model(img, ft, (out, out)).float(), tgt.float())
                else:
                    loss = model(img, ft, (out, out), regress=tgt, regress_path=fused_path if kind == "fused" else "composed")
            loss.backward()
            return loss
        return step

    arms = {k: make(k) for k in ((("fused", "composed", "plain") if HAS_REGRESS else ("plain",)))}
    say(f"== {gname}: B {B}, image {img_sz}^2, features {C} x {lr}^2 -> {out}^2, window 9, bf16 autocast, .train(); tree '{args.label}' "
        f"(naf_amd {naf_amd.__version__}, regress= {'yes' if HAS_REGRESS else 'no'}); {args.rounds} rounds x {args.iters} steps, arms alternating")
    t = interleaved(arms, args.iters, args.rounds)
    for k, v in t.items():
        say(f"  {k:9s} step {v[len(v) // 2]:8.4f} ms  [{v[0]:.4f} .. {v[-1]:.4f}]  spread {v[-1] - v[0]:.4f}")
    if "fused" in t:
        f_, c_ = t["fused"], t["composed"]
        spread = max(f_[-1] - f_[0], c_[-1] - c_[0])
        d = f_[len(f_) // 2] - c_[len(c_) // 2]
        say(f"  fused - composed = {d:+.4f} ms; run-to-run spread {spread:.4f} ms -> " +
            ("inside the spread: no difference shown" if abs(d) <= spread else ("fused is faster" if d < 0 else "FUSED IS SLOWER")))
    for k, fn in arms.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        say(f"  {k:9s} peak memory {torch.cuda.max_memory_allocated() / 2 ** 20:8.1f} MiB")
    for k, fn in arms.items():
        n, f_us, b_us, between = kernel_table(fn)
        say(f"  {k:9s} {n} device kernels per step; attention forward {f_us:.1f} us, backward {b_us:.1f} us; {len(between)} kernels between them: "
            + ", ".join(x.split("(")[0][:60] for x in between))
    if "fused" in arms:
        say(f"  loss fused {float(arms['fused']()):.7g}  composed {float(arms['composed']()):.7g}")
    del model, img, ft, tgt, arms
    torch.cuda.empty_cache()

if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
