"""Fused k-means against the composition it replaces, interleaved A/B in one process (device events, warmed), and the compiler's figures
of every instantiation.

    python tools/kmeans_time.py --resources                       (no GPU: compiles the instances with -Rpass-analysis=kernel-resource-usage)
    python tools/kmeans_time.py [--iters N] [--shapes ...]        (GPU: the A/B tables)
  both modes take --out FILE (append; profiles/kmeans.txt)

  (a) naf.kmeans(g, feats, size, k, iters=LLOYD, path="composed")   per Lloyd iteration: the head kernel's labels per image, a one-hot tensor,
                                                                    naf_xna_maskpool_fwd, naf_maskpool_apply -- kernels of the parent commit
  (b) naf.kmeans(g, feats, size, k, iters=LLOYD, path="fused")      per Lloyd iteration: naf_xna_kmeans_fwd, naf_maskpool_apply

Both arms take the same ``Guidance`` (the image is encoded once, outside the timed region) and the same initial centroids, and return equal
bits.  Arm (a) is timed TWICE, interleaved with (b) -- a1, b, a2 per iteration -- so that every row shows the run-to-run spread a
difference has to be held against: "fused wins" only where (b)'s median is below both (a) medians by more than the largest of the
three spreads (max - min).  Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) with K = 8, 16 and 64, and the reference's probing point
REF448 (448^2, C 384, low-res 28^2, window 9: 16-pixel cells) with K = 16; bf16 features.  The second table is the step alone:
``ops.xna_kmeans_step`` against the labels launch (``ops.xna_head_objective``) plus the mask-pooling launches (``ops.xna_mask_pool`` on
the one-hot masks, which are built outside the timed region).  The tool fails when it finds no GPU (except --resources)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLOYD = 5
# name -> (H = W, low-res h = w, C, window, K)
SHAPES = {"G1-K8": (1024, 64, 768, 7, 8), "G1-K16": (1024, 64, 768, 7, 16), "G1-K64": (1024, 64, 768, 7, 64), "REF448-K16": (448, 28, 384, 9, 16)}


def resources(say):
    """Registers, scratch and occupancy of every instantiation, from the compiler (no GPU)."""
    from naf_amd import build
    csrc = build.CSRC
    say("# compiler figures, hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on naf_amd/csrc/xna_kmeans_inst.hip, one compile per window;")
    say("# LDS is dynamic (xna_kmeans_lds_for: the K window + max(PV window, P^T of a 256-pixel round) + 256 label bytes); 'clusters' is the")
    say("# channel-tile instantiation (NCT = 2: K <= 32, NCT = 4: K <= 64); 'served' = free of scratch")
    say("window  clusters  VGPRs  AGPRs  SGPRs  SGPR spill  scratch B/lane  waves/SIMD  LDS bytes  served")
    for ks, _ in build.INSTANCES["xna_kmeans_inst.hip"]:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", f"-I{build.INCLUDE}", f"-I{csrc}",
                   *build.VGPR_FORM, f"-DNAF_KS={ks}", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "xna_kmeans_inst.hip"),
                   "-o", os.path.join(tmp, "o.o")]
            txt = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        for m in re.finditer(r"Function Name: _Z17xna_kmeans_kernelILi(\d+)ELi(\d)EE.*?LDS Size[^\n]*", txt, flags=re.S):
            g = lambda key: int(re.search(key + r"[^:\n]*: (\d+)", m.group(0)).group(1))
            nct = int(m.group(2))
            lds = ks * ks * 72 * 2 + max(ks * ks * (nct * 16 + 16) * 2, (ks * ks + 15) // 16 * 16 * (256 + 8) * 2) + 256
            say(f"{ks:<7d} {'<= ' + str(nct * 16):<9s} {g(' VGPRs'):<6d} {g('AGPRs'):<6d} {g('TotalSGPRs'):<6d} {g('SGPRs Spill'):<11d} "
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


def aba(arm_a, arm_b, iters, warmup):
    t1, tb, t2 = [], [], []
    for it in range(warmup + iters):
        x, y, z = timed(arm_a), timed(arm_b), timed(arm_a)
        if it >= warmup:
            t1.append(x)
            tb.append(y)
            t2.append(z)
    (s1, m1, r1), (sb, mb, rb), (s2, m2, r2) = stats(t1), stats(tb), stats(t2)
    wins = mb + max(r1, r2, rb) < min(m1, m2)
    return f"(a) composed {s1} | again {s2}   (b) fused {sb}   a/b {0.5 * (m1 + m2) / mb:.2f}x   fused wins: {'yes' if wins else 'NO'}"


def ab_tables(names, iters, warmup, say):
    import torch
    from naf_amd import NAF, ops
    dev = torch.device("cuda:0")
    say(f"# {torch.cuda.get_device_name(0)}; iters {iters}, warm-up {warmup}; per iteration a1, b, a2; ms: median [min .. max]; batch 1, bf16 features;")
    say(f"# whole = naf.kmeans(guidance, ..., iters={LLOYD}, init=fixed centroids): {LLOYD} Lloyd iterations + the final assignment, device events; both arms return equal bits (asserted);")
    say("# step = ops.xna_kmeans_step against ops.xna_head_objective(want_labels) + ops.xna_mask_pool on prebuilt one-hot masks (the composition's launches alone)")
    for name in names:
        H, h, C, ks, K = SHAPES[name]
        torch.manual_seed(0)
        model = NAF(kernel_size=ks).to(dev).eval()
        img = torch.randn(1, 3, H, H, device=dev)
        ft = torch.randn(1, C, h, h, device=dev).to(torch.bfloat16)
        heads = model.upsampler.num_heads
        with torch.no_grad():
            g = model.guide(img, (H, H))
            c0 = model.kmeans(g, ft, (H, H), K, iters=0).centroids
            arm_a = lambda: model.kmeans(g, ft, (H, H), K, iters=LLOYD, init=c0, path="composed")
            arm_b = lambda: model.kmeans(g, ft, (H, H), K, iters=LLOYD, init=c0, path="fused")
            ra, rb = arm_a(), arm_b()
            assert all(torch.equal(x, y) for x, y in zip(ra, rb)), "the two arms differ"
            say(f"{name:<11s} whole  {aba(arm_a, arm_b, iters, warmup)}")
            q5, k5, tabs = model.guidance_qk(g, (h, h), (H, H), fusable=lambda q, t: ops.xna_kmeans_select(q, (h, h), K, ks, rope_tables=t) == "fused")
            pv5, bias, _ = ops.project_kmeans_values(c0, ft, heads)
            kw = dict(scale=model.upsampler.scale, rope_tables=tabs)
            labels = ops.xna_head_objective(q5, k5, pv5, bias[0], ks, n_out=K, want_labels=True, **kw)[1]
            onehot = labels[:, None] == torch.arange(K, device=dev, dtype=labels.dtype)[None, :, None, None]

            def step_a():
                ops.xna_head_objective(q5, k5, pv5, bias[0], ks, n_out=K, want_labels=True, **kw)
                ops.xna_mask_pool(q5, k5, onehot, ks, **kw)

            step_b = lambda: ops.xna_kmeans_step(q5, k5, pv5, bias, ks, **kw)
            say(f"{name:<11s} step   {aba(step_a, step_b, iters, warmup)}")
        del model, img, ft, g
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
            raise SystemExit("kmeans_time.py measures on a ROCm device; none found")
        ab_tables(args.shapes.split(","), args.iters, args.warmup, say)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
