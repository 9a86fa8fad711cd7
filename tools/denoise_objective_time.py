"""Denoising objective: the fused call against the torch composition of the reference's loss and metrics, on one device, same commit.

    python tools/denoise_objective_time.py [--iters N] [--rounds R] [--skip-steps] [--out profiles/denoise_objective.txt]

  fused   naf_amd.DenoisingLoss / naf_amd.denoising_metrics (naf_denoise_objective: a tile launch and a finishing launch)
  torch   the reference's DenoisingLoss.forward / MetricsCalculator expressions as torch ops in fp32 (tests/denoise_reference.py: loss_terms,
          metrics' composition on the device without the .item() calls), with autograd's backward

Three measurements, each interleaved A/B (fused, torch, fused, torch ... `rounds` times; per arm the median [min .. max] over rounds of the mean of
`iters` back-to-back calls between two device events; every arm warmed >= 0.3 s first):

  1. loss forward + backward alone on a [B, 3, S, S] pair whose pred is the channels-last view the attention writes, weights (1, 5, 0.2):
     2 x 3 x 256^2 and the reference's 4 x 3 x 448^2, with the device-kernel count of one call of each arm from torch.profiler
  2. the whole training step of tools/denoise_train_time.py (model(noisy_norm, noisy, (S, S)) in train mode, loss, backward, SGD step) with the
     real loss, NAF(dim 96 / 256) at 2 x 3 x 256^2 and NAF(dim 96) at 4 x 3 x 448^2
  3. the validation metrics (clamp + PSNR + SSIM) at the same two sizes

No ratio is fixed in advance; the file states what was measured."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import naf_amd  # noqa: E402
import denoise_reference as R  # noqa: E402

WEIGHTS = (1.0, 5.0, 0.2)          # config/base_denoising.yaml


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(arms, iters, rounds, warm_seconds=0.3):
    """{name: (text, median)} of the arms, measured alternately."""
    for fn in arms.values():
        t0 = time.perf_counter()
        n = 0
        while n < 2 or time.perf_counter() - t0 < warm_seconds:
            timed(fn, 1)
            n += 1
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    out = {}
    for k, v in t.items():
        v = sorted(v)
        out[k] = (f"{v[len(v) // 2]:.4f} [{v[0]:.4f} .. {v[-1]:.4f}]", v[len(v) // 2])
    return out


def kernel_count(fn):
    """Device kernels of one call (copies and memsets left out)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.key.lower()
               and "memset" not in e.key.lower())


def torch_metrics(pred, target):
    """denoising.py:302 + MetricsCalculator, on the device, without the host synchronisations of .item()."""
    p = torch.clamp(pred, 0, 1)
    mse = (p - target).pow(2).mean()
    return {"psnr": 20 * torch.log10(1.0 / torch.sqrt(mse)), "ssim": R.ssim_map_metrics(p, target).mean()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-steps", action="store_true", help="leave the whole-training-step measurement out")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_objective_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say(f"# {torch.cuda.get_device_name(0)}; weights {WEIGHTS}; interleaved A/B, {args.rounds} rounds x {args.iters} calls per arm, each arm warmed >= 0.3 s; "
        "ms per call: median [min .. max] over rounds")
    crit = naf_amd.DenoisingLoss(*WEIGHTS)
    for B, S in ((2, 256), (4, 448)):
        pred32, target32 = R.make_inputs((B, 3, S, S), clamped=False)
        target = target32.to(dev)
        pred = pred32.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)        # the attention's channels-last buffer, as an NCHW view

        def fused_loss():
            p = pred.detach().requires_grad_(True)
            crit(p, target)["total"].backward()
            return p.grad

        def torch_loss():
            p = pred.detach().requires_grad_(True)
            R.loss_terms(p, target, WEIGHTS)["total"].backward()
            return p.grad

        gdiff = float((fused_loss() - torch_loss()).abs().max() / torch_loss().abs().max())
        r = interleaved({"fused": fused_loss, "torch": torch_loss}, args.iters, args.rounds)
        say(f"loss fwd+bwd {B}x3x{S}^2: fused {r['fused'][0]} ms, {kernel_count(fused_loss)} device kernels | torch {r['torch'][0]} ms, "
            f"{kernel_count(torch_loss)} device kernels | torch / fused {r['torch'][1] / r['fused'][1]:.2f}x | max |g_fused - g_torch| / max|g| {gdiff:.2e}")
        fm, tm = naf_amd.denoising_metrics(pred, target, clamp=True), torch_metrics(pred, target)
        r = interleaved({"fused": lambda: naf_amd.denoising_metrics(pred, target, clamp=True), "torch": lambda: torch_metrics(pred, target)},
                        args.iters, args.rounds)
        say(f"metrics {B}x3x{S}^2: fused {r['fused'][0]} ms, {kernel_count(lambda: naf_amd.denoising_metrics(pred, target, clamp=True))} device kernels | "
            f"torch {r['torch'][0]} ms, {kernel_count(lambda: torch_metrics(pred, target))} device kernels | torch / fused {r['torch'][1] / r['fused'][1]:.2f}x | "
            f"psnr {float(fm['psnr']):.5f} / {float(tm['psnr']):.5f} dB, ssim {float(fm['ssim']):.7f} / {float(tm['ssim']):.7f}")
    if not args.skip_steps:
        mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
        for dim, B, S in ((96, 2, 256), (256, 2, 256), (96, 4, 448)):
            torch.manual_seed(0)
            m = naf_amd.NAF(dim=dim, heads_attn=1, heads_rope=1, kernel_size=15).to(dev).train()
            opt = torch.optim.SGD(m.parameters(), lr=1e-4)
            clean = torch.rand(B, 3, S, S, device=dev)
            noisy = clean + 0.1 * torch.randn(B, 3, S, S, device=dev)

            def step(loss_fn):
                opt.zero_grad(set_to_none=True)
                out = m((noisy - mean) / std, noisy, (S, S))
                loss_fn(out, clean)["total"].backward()
                opt.step()

            r = interleaved({"fused": lambda: step(crit), "torch": lambda: step(lambda o, c: R.loss_terms(o.float(), c, WEIGHTS))},
                            max(3, args.iters // 2), args.rounds)
            say(f"training step NAF(dim {dim}, 1 head, window 15) {B}x3x{S}^2: fused loss {r['fused'][0]} ms | torch loss {r['torch'][0]} ms | "
                f"torch / fused {r['torch'][1] / r['fused'][1]:.3f}x")
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
