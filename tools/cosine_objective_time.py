"""The fused cosine objective against the composition it replaces: a TRAINING STEP (forward + backward for the embeddings E), interleaved
A/B in one process (device events, warmed), and the compiler's figures of every instantiation of the classification epilogue.

    python tools/cosine_objective_time.py --resources [--out profiles/cosine_objective.txt]     (no GPU: compiles the instances)
    python tools/cosine_objective_time.py [--iters N] [--shapes ...] [--out profiles/cosine_objective.txt]     (GPU: the A/B table)

  (a) naf(image, feats, size, head=E, cosine=True, logit_scale=s, target=t, loss="ce", cosine_path="composed").backward()
      the plain forward, its fp32 copy, F.normalize, a matrix product and F.cross_entropy, autograd through them: what a user does today
  (b) the same call with cosine_path="fused": naf_xna_cos_ce_fwd (loss map, g' and ds from one launch) and one naf_xna_bwd launch

Arm (a) is timed TWICE, interleaved with (b) -- a1, b, a2 per iteration -- so that every row shows the run-to-run spread a difference has
to be held against.  Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) and the reference's probing point REF448 (448^2, C 384, low-res
28^2, window 9) at N = 21 and 151; bf16 features, E in fp32 with a gradient, s a float.  Per row: median [min .. max] in ms over the timed
iterations, the peak device memory of one step of each arm (torch.cuda.max_memory_allocated above what is resident before the step) and
the largest difference of the two arms' E.grad.  The tool fails when it finds no GPU (except --resources, which launches nothing)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (H = W, low-res h = w, C, window, N)
SHAPES = {"G1-N21": (1024, 64, 768, 7, 21), "G1-N151": (1024, 64, 768, 7, 151), "REF448-N21": (448, 28, 384, 9, 21),
          "REF448-N151": (448, 28, 384, 9, 151)}


def cos_tpw(ks, nct):
    """xna_cos_tpw / xna_cos_ce_tpw of naf_amd/csrc/xna_cos_kernel.h."""
    one = (nct >= 10 and ks >= 11) or ks >= 15 or (nct >= 10 and ks >= 9) or (nct >= 16 and ks >= 7)
    return (1 if one else 2), (1 if one or nct >= 16 else 2)


def resources(say):
    """Registers, LDS, scratch and occupancy of every instantiation of the classification epilogue, from the compiler (no GPU)."""
    from naf_amd import build
    csrc = build.CSRC
    say("# compiler figures, hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on naf_amd/csrc/xna_cos_inst.hip, one compile per window,")
    say("# with -DNAF_XNA_COS_ALL so that the instantiations the library leaves out are on record too.  Rows: xna_cos_kernel<window, ch.tiles, XnaCosCEEpilogue>")
    say("# (naf_xna_cos_ce_fwd); 'cos VGPRs' = the same pair's cosine instantiation (naf_xna_cos_fwd) from the same compile, for comparison.  LDS is dynamic")
    say("# (xna_cos_lds_for: K + PV + value-chunk windows, the same for both); tiles/wave = xna_cos_ce_tpw; 'served' = free of scratch: what")
    say("# naf_xna_cos_ce_select grants and the library instantiates")
    say("window  ch.tiles  N          tiles/wave  VGPRs  AGPRs  SGPRs  scratch B/lane  waves/SIMD  LDS bytes  cos VGPRs  served")
    nrange = {2: "1..32", 4: "33..64", 10: "65..160", 16: "161..256"}
    for ks, _ in build.INSTANCES["xna_cos_inst.hip"]:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", f"-I{build.INCLUDE}", f"-I{csrc}",
                   *build.VGPR_FORM, f"-DNAF_KS={ks}", "-DNAF_XNA_COS_ALL", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "xna_cos_inst.hip"),
                   "-o", os.path.join(tmp, "o.o")]
            txt = subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=tmp).stderr
        fig = {}
        for m in re.finditer(r"Function Name: _Z14xna_cos_kernelILi(\d+)ELi(\d+)E(\d+)(XnaCos\w*?Epilogue)E.*?LDS Size[^\n]*", txt, flags=re.S):
            g = lambda key: int(re.search(key + r"[^:\n]*: (\d+)", m.group(0)).group(1))
            fig[(int(m.group(2)), m.group(4) == "XnaCosCEEpilogue")] = {k_: g(v_) for k_, v_ in (("v", " VGPRs"), ("a", "AGPRs"), ("s", "TotalSGPRs"),
                                                                                               ("scr", "ScratchSize"), ("occ", "Occupancy"))}
        for nct in (2, 4, 10, 16):
            lds = ks * ks * (72 + nct * 16 + 16 + 64 + 16) * 2
            if (nct, True) not in fig:
                say(f"{ks:<7d} {nct:<9d} {nrange[nct]:<10s} not instantiated: LDS would be {lds} bytes, above 160 KB; the composition serves it")
                continue
            f, c = fig[(nct, True)], fig.get((nct, False))
            say(f"{ks:<7d} {nct:<9d} {nrange[nct]:<10s} {cos_tpw(ks, nct)[1]:<11d} {f['v']:<6d} {f['a']:<6d} {f['s']:<6d} {f['scr']:<15d} {f['occ']:<11d} {lds:<10d} "
                f"{(str(c['v']) if c else '-'):<10s} {'yes' if f['scr'] == 0 else 'NO'}")


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
    return f"{t[len(t) // 2]:.3f} [{t[0]:.3f} .. {t[-1]:.3f}]", t[len(t) // 2]


def peak_mb(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def ab_table(names, iters, warmup, say):
    import torch
    from naf_amd import NAF
    dev = torch.device("cuda:0")
    say(f"# {torch.cuda.get_device_name(0)}; training step = forward + backward for E; iters {iters}, warm-up {warmup}; per iteration a1, b, a2; ms: median [min .. max];")
    say("# a/b = mean of the two (a) medians over the (b) median; peak = MiB above the resident tensors; whole calls (stem + RoPE / pooling + attention + backward)")
    for name in names:
        H, h, C, k, N = SHAPES[name]
        torch.manual_seed(0)
        model = NAF(kernel_size=k).to(dev).eval()
        img = torch.randn(1, 3, H, H, device=dev)
        ft = torch.randn(1, C, h, h, device=dev).to(torch.bfloat16)
        E = torch.randn(N, C, device=dev, requires_grad=True)
        t = torch.randint(0, N, (1, H, H), device=dev)
        t[torch.rand(1, H, H, device=dev) < 0.1] = 255

        def step(path):
            E.grad = None
            model(img, ft, (H, H), head=E, cosine=True, logit_scale=10.0, target=t, loss="ce", ignore_index=255, cosine_path=path).backward()

        arm_a, arm_b = (lambda: step("composed")), (lambda: step("fused"))
        arm_a()
        ga = E.grad.clone()
        arm_b()
        gd = float((E.grad - ga).abs().max()) / max(float(ga.abs().max()), 1e-30)
        t1, tb, t2 = [], [], []
        for it in range(warmup + iters):
            x, y, z = timed(arm_a), timed(arm_b), timed(arm_a)
            if it >= warmup:
                t1.append(x)
                tb.append(y)
                t2.append(z)
        (s1, m1), (sb, mb), (s2, m2) = stats(t1), stats(tb), stats(t2)
        pa, pb = peak_mb(arm_a), peak_mb(arm_b)
        say(f"{name:<12s} train step: (a) composed {s1} | again {s2}   (b) fused {sb}   a/b {0.5 * (m1 + m2) / mb:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB   "
            f"max |dE_a - dE_b| / max |dE_a| {gd:.2e}")
        del model, img, ft, E, t, ga
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
            raise SystemExit("cosine_objective_time.py measures on a ROCm device; none found")
        ab_table(args.shapes.split(","), args.iters, args.warmup, say)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
