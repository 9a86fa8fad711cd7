"""Fused mask pooling against the composition it replaces, interleaved A/B in one process (device events, warmed), and the compiler's
figures of every instantiation.

    python tools/mask_pool_time.py --resources                       (no GPU: compiles the instances with -Rpass-analysis=kernel-resource-usage)
    python tools/mask_pool_time.py [--iters N] [--shapes ...]        (GPU: the A/B table)
  both modes take --out FILE (append; profiles/mask_pool.txt)

  (a) naf(image, feats, size, masks=M, mask_path="composed")   the plain forward, its fp32 copy, the masks' fp32 copy, an einsum:
                                                               what a user could do before the kernel existed
  (b) naf(image, feats, size, masks=M, mask_path="fused")      naf_xna_maskpool_fwd + naf_maskpool_apply: the C-channel map is never written

Arm (a) is timed TWICE, interleaved with (b) -- a1, b, a2 per iteration -- so that every row shows the run-to-run spread a difference has
to be held against: "fused wins" only where (b)'s median is below both (a) medians by more than the largest of the three spreads
(max - min).  Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) with K = 1, 16 and 64 bool masks and 16 bf16 masks, and the reference's
probing point REF448 (448^2, C 384, low-res 28^2, window 9: 16-pixel cells) with K = 16; bf16 features.  Peak memory:
torch.cuda.max_memory_allocated above what is resident before the call.  The kernel's own launches are timed by the library's kernel
timer hooks in a second pass (device events around the two C calls).  The tool fails when it finds no GPU (except --resources)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (H = W, low-res h = w, C, window, K, mask dtype)
SHAPES = {"G1-K1": (1024, 64, 768, 7, 1, "bool"), "G1-K16": (1024, 64, 768, 7, 16, "bool"), "G1-K64": (1024, 64, 768, 7, 64, "bool"),
          "G1-K16-bf16": (1024, 64, 768, 7, 16, "bfloat16"), "REF448-K16": (448, 28, 384, 9, 16, "bool")}


def resources(say):
    """Registers, scratch and occupancy of every instantiation, from the compiler (no GPU)."""
    from naf_amd import build
    csrc = build.CSRC
    say("# compiler figures, hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on naf_amd/csrc/xna_pool_inst.hip, one compile per window;")
    say("# LDS is dynamic (xna_pool_lds_for: the K window + P^T of a 256-pixel round); K (1 .. 64 per launch) is a run-time loop over output tiles,")
    say("# not a template parameter: one instantiation per (window, mask type) serves every K; 'served' = free of scratch")
    say("window  masks  VGPRs  AGPRs  SGPRs  SGPR spill  scratch B/lane  waves/SIMD  LDS bytes  served")
    for ks, _ in build.INSTANCES["xna_pool_inst.hip"]:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", f"-I{build.INCLUDE}", f"-I{csrc}",
                   *build.VGPR_FORM, f"-DNAF_KS={ks}", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "xna_pool_inst.hip"),
                   "-o", os.path.join(tmp, "o.o")]
            txt = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        lds = ks * ks * 72 * 2 + (ks * ks + 15) // 16 * 16 * (256 + 8) * 2
        for m in re.finditer(r"Function Name: _Z15xna_pool_kernelILi(\d+)ELb(\d)EE.*?LDS Size[^\n]*", txt, flags=re.S):
            g = lambda key: int(re.search(key + r"[^:\n]*: (\d+)", m.group(0)).group(1))
            say(f"{ks:<7d} {'bytes' if m.group(2) == '1' else 'bf16':<6s} {g(' VGPRs'):<6d} {g('AGPRs'):<6d} {g('TotalSGPRs'):<6d} {g('SGPRs Spill'):<11d} "
                f"{g('ScratchSize'):<15d} {g('Occupancy'):<11d} {lds:<10d} {'yes' if g('ScratchSize') == 0 else 'NO'}")


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    t = sorted(t)
    return f"{t[len(t) // 2]:.3f} [{t[0]:.3f} .. {t[-1]:.3f}]", t[len(t) // 2], t[-1] - t[0]


def peak_mb(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


class LaunchTimer:
    """ops.KERNEL_TIMER: device events around every timed launch of the library, summed per name."""

    def __init__(self):
        self.open, self.pairs = {}, []

    def start(self, name):
        import torch
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.open[name] = e

    def stop(self, name):
        import torch
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.pairs.append((name, self.open.pop(name), e))

    def totals(self):
        import torch
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.pairs:
            out.setdefault(name, []).append(a.elapsed_time(b))
        return out


def setup(name, dev):
    import torch
    from naf_amd import NAF
    H, h, C, k, K, mdt = SHAPES[name]
    torch.manual_seed(0)
    model = NAF(kernel_size=k).to(dev).eval()
    img = torch.randn(1, 3, H, H, device=dev)
    ft = torch.randn(1, C, h, h, device=dev).to(torch.bfloat16)
    soft = torch.rand(1, K, H, H, device=dev)
    masks = (soft > 0.7) if mdt == "bool" else soft.to(torch.bfloat16)
    return model, img, ft, masks, (H, H)


def ab_table(names, iters, warmup, say):
    import torch
    from naf_amd import ops
    dev = torch.device("cuda:0")
    say(f"# {torch.cuda.get_device_name(0)}; iters {iters}, warm-up {warmup}; per iteration a1, b, a2; ms: median [min .. max]; peak = MiB above the resident tensors;")
    say("# whole calls (stem + RoPE / pooling + attention + pooling), device events; 'fused wins' = (b) median below both (a) medians by more than the largest spread;")
    say("# launches = medians of the fused route's two C calls alone (xna_mask_pool: cell kernel + gather + mass; mask_pool_apply), device events")
    for name in names:
        model, img, ft, masks, size = setup(name, dev)
        with torch.no_grad():
            arm_a = lambda: model(img, ft, size, masks=masks, mask_path="composed")
            arm_b = lambda: model(img, ft, size, masks=masks, mask_path="fused")
            ra, rb_ = arm_a(), arm_b()
            diff = float((ra - rb_).abs().max()) / max(float(ra.abs().max()), 1e-30)
            t1, tb, t2 = [], [], []
            for it in range(warmup + iters):
                x, y, z = timed(arm_a), timed(arm_b), timed(arm_a)
                if it >= warmup:
                    t1.append(x)
                    tb.append(y)
                    t2.append(z)
            (s1, m1, r1), (sb, mb, rb), (s2, m2, r2) = stats(t1), stats(tb), stats(t2)
            pa, pb = peak_mb(arm_a), peak_mb(arm_b)
            timer, old = LaunchTimer(), ops.KERNEL_TIMER
            ops.KERNEL_TIMER = timer
            try:
                for _ in range(iters):
                    arm_b()
            finally:
                ops.KERNEL_TIMER = old
            tot = timer.totals()
            med = lambda n: sorted(tot[n])[len(tot[n]) // 2] if n in tot else float("nan")
        wins = mb + max(r1, r2, rb) < min(m1, m2)
        say(f"{name:<12s} (a) composed {s1} | again {s2}   (b) fused {sb}   a/b {0.5 * (m1 + m2) / mb:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB   "
            f"max |a - b| / max |a| {diff:.2e}   launches: xna_mask_pool {med('xna_mask_pool'):.3f} mask_pool_apply {med('mask_pool_apply'):.3f} ms   "
            f"fused wins: {'yes' if wins else 'NO'}")
        del model, img, ft, masks
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if args.resources:
        resources(say)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("mask_pool_time.py measures on a ROCm device; none found")
        ab_table(args.shapes.split(","), args.iters, args.warmup, say)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
