"""The fused cosine head against the composition it replaces, interleaved A/B in one process (device events, warmed), the compiler's
figures of every instantiation, and the kernel's time from the profiler's table against its HBM bound.

    python tools/cosine_head_time.py --resources                       (no GPU: compiles the instances with -Rpass-analysis=kernel-resource-usage)
    python tools/cosine_head_time.py [--iters N] [--shapes ...]        (GPU: the A/B table)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/NAME -- python tools/cosine_head_time.py --kernel-run NAME     (one shape per run)
    python tools/cosine_head_time.py --kernel-stats DIR                (reads DIR/NAME/*/*kernel_stats.csv: kernel time, HBM bound, share)
  every mode takes --out FILE (append; profiles/cosine_head.txt)

  (a) naf(image, feats, size, head=E, cosine=True, cosine_path="composed")   the plain forward, its fp32 copy, F.normalize, a matrix product:
                                                                             what a user could do before the kernel existed
  (b) naf(image, feats, size, head=E, cosine=True, cosine_path="fused")      naf_xna_cos_fwd: the C-channel map is never written

Arm (a) is timed TWICE, interleaved with (b) -- a1, b, a2 per iteration -- so that every row shows the run-to-run spread a difference has
to be held against; "auto" may take the kernel for a class of shapes only where (b)'s median is below both (a) medians by more than the
larger of the two arms' spreads (max - min).  Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) and the reference's probing point REF448
(448^2, C 384, low-res 28^2, window 9) at N = 21 and 151, and one heat-map call HEAT (1024^2, C 768, window 9, N = 1); bf16 features.
Peak memory: torch.cuda.max_memory_allocated above what is resident before the call.  HBM bound, from the shapes: the queries, the key, PV
and value grids read once, N * Ho * Wo fp32 written, over 8.0 TB/s (the spec peak; a float4 copy reaches 6.29 TB/s on this part).
The tool fails when it finds no GPU (except --resources and --kernel-stats, which launch nothing)."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (H = W, low-res h = w, C, window, N)
SHAPES = {"G1-N21": (1024, 64, 768, 7, 21), "G1-N151": (1024, 64, 768, 7, 151), "REF448-N21": (448, 28, 384, 9, 21),
          "REF448-N151": (448, 28, 384, 9, 151), "HEAT-N1": (1024, 64, 768, 9, 1)}
HBM_PEAK = 8.0e12


def hbm_bytes(H, h, C, N, heads=4, B=1):
    npad = (N + 15) // 16 * 16
    return B * (H * H * heads * 64 * 2 + h * h * heads * 64 * 2 + h * h * heads * npad * 2 + h * h * C * 2 + N * H * H * 4)


def resources(say):
    """Registers, LDS, scratch and occupancy of every instantiation, from the compiler (no GPU)."""
    from naf_amd import build
    csrc = build.CSRC
    say("# compiler figures, hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on naf_amd/csrc/xna_cos_inst.hip, one compile per window;")
    say("# with -DNAF_XNA_COS_ALL so that the instantiations the library leaves out are on record too.  LDS is dynamic (xna_cos_lds_for: K + PV + value-chunk")
    say("# windows); tiles/wave = xna_cos_tpw; 'served' = free of scratch: what naf_xna_cos_select grants and the library instantiates")
    say("window  ch.tiles  N          tiles/wave  VGPRs  AGPRs  SGPRs  scratch B/lane  waves/SIMD  LDS bytes  served")
    nrange = {2: "1..32", 4: "33..64", 10: "65..160", 16: "161..256"}
    for ks, _ in build.INSTANCES["xna_cos_inst.hip"]:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", f"-I{build.INCLUDE}", f"-I{csrc}",
                   *build.VGPR_FORM, f"-DNAF_KS={ks}", "-DNAF_XNA_COS_ALL", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "xna_cos_inst.hip"),
                   "-o", os.path.join(tmp, "o.o")]
            txt = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        seen = set()
        for m in re.finditer(r"Function Name: _Z14xna_cos_kernelILi(\d+)ELi(\d+)E14XnaCosEpilogueE.*?LDS Size[^\n]*", txt, flags=re.S):
            nct = int(m.group(2))
            g = lambda key: int(re.search(key + r"[^:\n]*: (\d+)", m.group(0)).group(1))
            lds = ks * ks * (72 + nct * 16 + 16 + 64 + 16) * 2
            tpw = 1 if ((nct >= 10 and ks >= 11) or ks >= 15 or (nct >= 10 and ks >= 9) or (nct >= 16 and ks >= 7)) else 2
            seen.add(nct)
            say(f"{ks:<7d} {nct:<9d} {nrange[nct]:<10s} {tpw:<11d} {g(' VGPRs'):<6d} {g('AGPRs'):<6d} {g('TotalSGPRs'):<6d} {g('ScratchSize'):<15d} "
                f"{g('Occupancy'):<11d} {lds:<10d} {'yes' if g('ScratchSize') == 0 else 'NO'}")
        for nct in (2, 4, 10, 16):
            if nct not in seen:
                lds = ks * ks * (72 + nct * 16 + 16 + 64 + 16) * 2
                say(f"{ks:<7d} {nct:<9d} {nrange[nct]:<10s} not instantiated: LDS would be {lds} bytes, above 160 KB; the composition serves it")


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


def setup(name, dev):
    import torch
    from naf_amd import NAF
    H, h, C, k, N = SHAPES[name]
    torch.manual_seed(0)
    model = NAF(kernel_size=k).to(dev).eval()
    img = torch.randn(1, 3, H, H, device=dev)
    ft = torch.randn(1, C, h, h, device=dev).to(torch.bfloat16)
    E = torch.randn(N, C, device=dev)
    return model, img, ft, E, (H, H)


def ab_table(names, iters, warmup, say):
    import torch
    dev = torch.device("cuda:0")
    say(f"# {torch.cuda.get_device_name(0)}; iters {iters}, warm-up {warmup}; per iteration a1, b, a2; ms: median [min .. max]; peak = MiB above the resident tensors;")
    say("# whole calls (stem + RoPE / pooling + attention + epilogue work), device events; 'fused wins' = (b) median below both (a) medians by more than the larger spread")
    for name in names:
        model, img, ft, E, size = setup(name, dev)
        with torch.no_grad():
            arm_a = lambda: model(img, ft, size, head=E, cosine=True, cosine_path="composed")
            arm_b = lambda: model(img, ft, size, head=E, cosine=True, cosine_path="fused")
            diff = float((arm_a() - arm_b()).abs().max())
            t1, tb, t2 = [], [], []
            for it in range(warmup + iters):
                x, y, z = timed(arm_a), timed(arm_b), timed(arm_a)
                if it >= warmup:
                    t1.append(x)
                    tb.append(y)
                    t2.append(z)
            (s1, m1, r1), (sb, mb, rb), (s2, m2, r2) = stats(t1), stats(tb), stats(t2)
            pa, pb = peak_mb(arm_a), peak_mb(arm_b)
        wins = mb + max(r1, r2, rb) < min(m1, m2)
        say(f"{name:<12s} (a) composed {s1} | again {s2}   (b) fused {sb}   a/b {0.5 * (m1 + m2) / mb:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB   "
            f"max |a - b| {diff:.2e}   fused wins: {'yes' if wins else 'NO'}")
        del model, img, ft, E
        torch.cuda.empty_cache()


def kernel_run(name):
    """The fused call alone, for the profiler: 3 warm-up + 20 calls of one shape."""
    import torch
    dev = torch.device("cuda:0")
    model, img, ft, E, size = setup(name, dev)
    with torch.no_grad():
        for _ in range(23):
            model(img, ft, size, head=E, cosine=True, cosine_path="fused")
    torch.cuda.synchronize()


def kernel_stats(root, say):
    say("# kernel time: rocprofv3 --kernel-trace --stats, one run per shape (23 calls of the fused route); HBM bound = bytes from the shapes / 8.0 TB/s")
    for name, (H, h, C, k, N) in SHAPES.items():
        files = sorted(glob.glob(os.path.join(root, name, "**", "*kernel_stats.csv"), recursive=True))
        if not files:
            say(f"{name:<12s} no kernel_stats.csv under {os.path.join(root, name)}: not measured")
            continue
        import csv
        rows = [r for r in csv.DictReader(open(files[0])) if "xna_cos_kernel" in r.get("Name", "")]
        if not rows:
            say(f"{name:<12s} xna_cos_kernel not in {files[0]}: not measured")
            continue
        r = rows[0]
        avg_us, calls = float(r["AverageNs"]) / 1e3, int(r["Calls"])
        by = hbm_bytes(H, h, C, N)
        bound_us = by / HBM_PEAK * 1e6
        # matrix work: S (64 dims), PV (npad channels) and P.V (Dv channels per head) per pixel, slot and head, 2 flop per multiply-add
        heads, npad = 4, (N + 15) // 16 * 16
        kpad = (k * k + 31) // 32 * 32
        flop = 2.0 * H * H * heads * kpad * (64 + npad + C // heads)
        say(f"{name:<12s} {r['Name'][:40]:<40s} calls {calls}  avg {avg_us:.1f} us [min {float(r['MinNs']) / 1e3:.1f} .. max {float(r['MaxNs']) / 1e3:.1f}]   "
            f"HBM bytes {by / 1e6:.1f} MB -> bound {bound_us:.1f} us: {100 * bound_us / avg_us:.0f}% of it achieved ({by / avg_us / 1e6:.2f} TB/s)   "
            f"matrix work {flop / 1e9:.1f} GFLOP (padded slots) -> {flop / avg_us / 1e6:.0f} TFLOP/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--kernel-run", default=None)
    ap.add_argument("--kernel-stats", default=None)
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
    elif args.kernel_stats:
        kernel_stats(args.kernel_stats, say)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("cosine_head_time.py measures on a ROCm device; none found")
        if args.kernel_run:
            kernel_run(args.kernel_run)
        else:
            ab_table(args.shapes.split(","), args.iters, args.warmup, say)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
