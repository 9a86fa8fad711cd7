"""Feature PCA for display: the fused fit and projection against the torch composition of the reference's pca(), on one device, same commit.

    python tools/feature_pca_time.py [--rounds R] [--sizes 64,128,...] [--channels 384,768] [--out profiles/feature_pca.txt]

  fused   naf_amd.FeaturePCA: fit = naf_feature_moments (two launches) + the C x C eigen-decomposition; projection = transform_rgb
          (naf_pca_project's two launches + two elementwise operations)
  torch   the reference's pca() (utils/visualization.py:135-190) with the tensors left on the device: the map flattened to fp32 [P, C],
          torch.pca_lowrank(X - mean, q=3, center=False, niter=20), then (X - mean) @ V and the min-max

The notebook's call (notebooks/inference.ipynb, upsample_backbone): one image, backbone features at 32 x 32 upsampled by naf(...) to 64^2 ...
1024^2, C = 384 and 768; the map is what naf(...) returns (bf16, channels-last).  Per size and arm: interleaved A/B (fused, torch, fused, torch ...
`rounds` times); per arm the median [min .. max] over rounds of the mean of back-to-back calls between two device events, the number of calls
chosen so that a window lasts about 0.2 s; every arm warmed >= 0.3 s first.  Peak memory: torch.cuda.max_memory_allocated over one call of
the arm, above what was allocated before it (the map itself is not counted).  The moments call is also timed alone; its lines state
  MFMA share  P C (C + 1) FLOP -- the products of the upper triangle, what the algorithm needs -- over the call time, over 2.5 PFLOP/s (bf16 dense peak)
  HBM share   2 P C bytes -- the map read once -- over the call time, over 8 TB/s (peak)
and which of the two bounds the call.  No ratio is fixed in advance; the file states what was measured."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naf_amd  # noqa: E402
from naf_amd import ops  # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(arms, rounds, warm_seconds=0.3, window_seconds=0.2):
    """{name: (text, median ms)} of the arms, measured alternately."""
    iters = {}
    for k, fn in arms.items():
        t0 = time.perf_counter()
        n, last = 0, 0.0
        while n < 2 or time.perf_counter() - t0 < warm_seconds:
            last = timed(fn, 1)
            n += 1
        iters[k] = max(1, min(200, int(window_seconds * 1e3 / max(last, 1e-3))))
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters[k]))
    out = {}
    for k, v in t.items():
        v = sorted(v)
        out[k] = (f"{v[len(v) // 2]:.4f} [{v[0]:.4f} .. {v[-1]:.4f}]", v[len(v) // 2])
    return out


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


class TorchPCA:
    """The reference's TorchPCA with its flatten(), on the device."""

    def fit(self, x):
        X = x[0].permute(1, 2, 0).reshape(-1, x.shape[1]).float()
        self.mean_ = X.mean(dim=0)
        _, S, V = torch.pca_lowrank(X - self.mean_, q=3, center=False, niter=20)
        self.components_, self.singular_values_ = V, S
        return self

    def transform_rgb(self, x):
        _, C, H, W = x.shape
        y = (x[0].permute(1, 2, 0).reshape(-1, C).float() - self.mean_.unsqueeze(0)) @ self.components_
        y = y - y.min(dim=0, keepdim=True).values
        y = y / y.max(dim=0, keepdim=True).values
        return y.reshape(1, H, W, 3).permute(0, 3, 1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="64,128,256,512,1024")
    ap.add_argument("--channels", default="384,768")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_pca_time.py measures on a ROCm device; none found")
    dev = torch.device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say(f"# {torch.cuda.get_device_name(0)}; lr 32 x 32 -> S x S by naf(...), the map bf16 channels-last; interleaved A/B, {args.rounds} rounds per arm, "
        "windows of about 0.2 s, each arm warmed >= 0.3 s; ms per call: median [min .. max] over rounds")
    torch.manual_seed(0)
    model = naf_amd.NAF().to(dev).eval()
    for Cc in (int(v) for v in args.channels.split(",")):
        feats = torch.randn(1, Cc, 32, 32, device=dev)
        for S in (int(v) for v in args.sizes.split(",")):
            image = torch.rand(1, 3, S, S, device=dev)
            with torch.no_grad():
                x = model(image, feats, (S, S))
            P = S * S
            fused, ref = naf_amd.FeaturePCA().fit(x), TorchPCA().fit(x)
            cos = (fused.components_.float() * ref.components_).sum(0).abs()
            pic_f, pic_t = fused.transform_rgb(x), ref.transform_rgb(x)
            diff = max(min(float((pic_f[:, r] - pic_t[:, r]).abs().max()), float((pic_f[:, r] - (1 - pic_t[:, r])).abs().max())) for r in range(3))
            del pic_f, pic_t
            r = interleaved({"fused": lambda: naf_amd.FeaturePCA().fit(x), "torch": lambda: TorchPCA().fit(x)}, args.rounds)
            mf, mt = peak_mib(lambda: naf_amd.FeaturePCA().fit(x)), peak_mib(lambda: TorchPCA().fit(x))
            say(f"fit C={Cc} {S}^2: fused {r['fused'][0]} ms, peak {mf:.1f} MiB | torch {r['torch'][0]} ms, peak {mt:.1f} MiB | "
                f"torch / fused {r['torch'][1] / r['fused'][1]:.2f}x | |cos| of the components {[round(float(c), 6) for c in cos]}")
            r = interleaved({"fused": lambda: fused.transform_rgb(x), "torch": lambda: ref.transform_rgb(x)}, args.rounds)
            mf, mt = peak_mib(lambda: fused.transform_rgb(x)), peak_mib(lambda: ref.transform_rgb(x))
            say(f"projection C={Cc} {S}^2: fused {r['fused'][0]} ms, peak {mf:.1f} MiB | torch {r['torch'][0]} ms, peak {mt:.1f} MiB | "
                f"torch / fused {r['torch'][1] / r['fused'][1]:.2f}x | max |rgb_fused - rgb_torch| up to the flip {diff:.2e}")
            r = interleaved({"moments": lambda: ops.feature_moments(x)}, args.rounds)
            ms = r["moments"][1]
            fl, by = P * Cc * (Cc + 1) / (ms * 1e-3) / PEAK_FLOPS, 2 * P * Cc / (ms * 1e-3) / PEAK_BYTES
            ns, slab = ops.feature_moments_plan(P, Cc)
            bound = "MFMA" if P * Cc * (Cc + 1) / PEAK_FLOPS > 2 * P * Cc / PEAK_BYTES else "HBM"
            say(f"moments C={Cc} {S}^2: {r['moments'][0]} ms per call ({ns} slabs of {slab} pixels) | MFMA share {100 * fl:.1f} % of 2.5 PFLOP/s | "
                f"HBM share {100 * by:.1f} % of 8 TB/s | the least time is set by {bound}")
            del x, fused, ref
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
