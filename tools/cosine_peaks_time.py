"""Peak search from the cosine kernel's epilogue (naf.locate) against the composition it replaces, interleaved A/B in one process (device
events, warmed), and the compiler's figures of every instantiation of the peak epilogue.

    python tools/cosine_peaks_time.py --resources                       (no GPU: compiles the instances with -Rpass-analysis=kernel-resource-usage)
    python tools/cosine_peaks_time.py [--iters N] [--shapes ...]        (GPU: whole calls, naf.locate fused against composed)
    python tools/cosine_peaks_time.py --kernels [--iters N]             (GPU: ops.xna_cos_peaks against ops.xna_cos_forward, both fused)
  every mode takes --out FILE (append; profiles/cosine_peaks.txt)

  (a) naf.locate(image, feats, size, E, path="composed")   the fused cosine call, its [B, N, Ho, Wo] fp32 map, then torch reductions
  (b) naf.locate(image, feats, size, E, path="fused")      naf_xna_cos_peaks_fwd + naf_peaks_topk: the N-channel map is never written

Arm (a) is timed TWICE, interleaved with (b) -- a1, b, a2 per iteration -- so that every row shows the run-to-run spread a difference has
to be held against (the protocol of tools/cosine_head_time.py); medians.  Shapes: G1 (1024^2, C 768, low-res 64^2, window 7) at N = 21
and 151, the reference's probing point REF448 (448^2, C 384, low-res 28^2, window 9) at N = 64, and one point query G1 at N = 1.
Peak memory: torch.cuda.max_memory_allocated above what is resident before the call.
The tool fails when it finds no GPU (except --resources, which launches nothing)."""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (H = W, low-res h = w, C, window, N)
SHAPES = {"G1-N21": (1024, 64, 768, 7, 21), "G1-N151": (1024, 64, 768, 7, 151), "REF448-N64": (448, 28, 384, 9, 64), "G1-N1": (1024, 64, 768, 7, 1)}
NCTS = (2, 4, 10, 16)
NRANGE = {2: "1..32", 4: "33..64", 10: "65..160", 16: "161..256"}
EPILOGUES = {"cosine": "14XnaCosEpilogue", "objective": "16XnaCosCEEpilogue", "peaks": "18XnaCosPeakEpilogue"}


def cos_lds(ks, nct):
    return ks * ks * (72 + nct * 16 + 16 + 64 + 16) * 2


def peak_lds(nct):
    return 8 * nct * 16 * 8


def _compile_window(ks, all_pairs):
    from naf_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
               *build.VGPR_FORM, f"-DNAF_KS={ks}", *(["-DNAF_XNA_COS_ALL"] if all_pairs else []), "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(build.CSRC, "xna_cos_inst.hip"), "-o", os.path.join(tmp, "o.o")]
        return subprocess.run(cmd, capture_output=True, text=True, check=True).stderr


def resource_rows(all_pairs=True, windows=None, jobs=None):
    """One dict per instantiation of xna_cos_kernel the compile produces: epilogue ("cosine", "objective", "peaks"), window, nct, vgprs,
    agprs, sgprs, scratch, occupancy.  ``all_pairs``: compile with -DNAF_XNA_COS_ALL, which also instantiates what the library leaves out."""
    from naf_amd import build
    windows = [k for k, _ in build.INSTANCES["xna_cos_inst.hip"]] if windows is None else list(windows)
    with cf.ThreadPoolExecutor(max_workers=jobs or min(8, os.cpu_count() or 2)) as ex:
        texts = list(ex.map(lambda k: _compile_window(k, all_pairs), windows))
    rows = []
    for ks, txt in zip(windows, texts):
        for epi, tag in EPILOGUES.items():
            for m in re.finditer(r"Function Name: _Z14xna_cos_kernelILi(\d+)ELi(\d+)E" + tag + r"E.*?LDS Size[^\n]*", txt, flags=re.S):
                g = lambda key: int(re.search(key + r"[^:\n]*: (\d+)", m.group(0)).group(1))
                rows.append({"epilogue": epi, "window": ks, "nct": int(m.group(2)), "vgprs": g(" VGPRs"), "agprs": g("AGPRs"), "sgprs": g("TotalSGPRs"),
                             "scratch": g("ScratchSize"), "occupancy": g("Occupancy")})
    return rows


def peak_tpw(ks, nct):
    """xna_cos_peak_tpw of naf_amd/csrc/xna_cos_kernel.h."""
    head1 = (nct >= 10 and ks >= 11)
    cos1 = head1 or ks >= 15 or (nct >= 10 and ks >= 9) or (nct >= 16 and ks >= 7)
    return 1 if (nct >= 16 or cos1) else 2


def resources(say):
    say("# compiler figures, hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on naf_amd/csrc/xna_cos_inst.hip, one compile per window,")
    say("# with -DNAF_XNA_COS_ALL so that the instantiations the library leaves out are on record too.  Epilogue = XnaCosPeakEpilogue.  LDS is dynamic:")
    say("# xna_cos_lds_for (K + PV + value-chunk windows) + 8 waves x channel tiles x 16 x 8 bytes of per-wave pairs; tiles/wave = xna_cos_peak_tpw;")
    say("# 'served' = free of scratch: what naf_xna_cos_peaks_select grants and the library instantiates")
    say("window  ch.tiles  N          tiles/wave  VGPRs  AGPRs  SGPRs  scratch B/lane  waves/SIMD  LDS bytes  served")
    rows = resource_rows(True)
    by = {(r["window"], r["nct"]): r for r in rows if r["epilogue"] == "peaks"}
    for ks in sorted({r["window"] for r in rows}):
        for nct in NCTS:
            r = by.get((ks, nct))
            lds = cos_lds(ks, nct) + peak_lds(nct)
            if r is None:
                say(f"{ks:<7d} {nct:<9d} {NRANGE[nct]:<10s} not instantiated: the windows alone take {cos_lds(ks, nct)} bytes of LDS, above 160 KB; the composition serves it")
                continue
            say(f"{ks:<7d} {nct:<9d} {NRANGE[nct]:<10s} {peak_tpw(ks, nct):<11d} {r['vgprs']:<6d} {r['agprs']:<6d} {r['sgprs']:<6d} {r['scratch']:<15d} "
                f"{r['occupancy']:<11d} {lds:<10d} {'yes' if r['scratch'] == 0 else 'NO'}")
    say("# the cosine and objective instantiations of the same compile (held against profiles/cosine_head.txt and profiles/cosine_objective.txt): VGPRs / scratch")
    for epi in ("cosine", "objective"):
        say(f"{epi:<10s} " + "  ".join(f"k{r['window']}/t{r['nct']}: {r['vgprs']}/{r['scratch']}" for r in sorted(
            (r for r in rows if r["epilogue"] == epi), key=lambda r: (r["window"], r["nct"]))))


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


def a1_b_a2(arm_a, arm_b, iters, warmup):
    t1, tb, t2 = [], [], []
    for it in range(warmup + iters):
        x, y, z = timed(arm_a), timed(arm_b), timed(arm_a)
        if it >= warmup:
            t1.append(x)
            tb.append(y)
            t2.append(z)
    return stats(t1), stats(tb), stats(t2)


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
    say("# whole naf.locate calls (stem + RoPE / pooling + attention + peak search + top-1), device events; 'fused wins' = (b) median below both (a) medians by more than the larger spread")
    for name in names:
        model, img, ft, E, size = setup(name, dev)
        arm_a = lambda: model.locate(img, ft, size, E, path="composed")
        arm_b = lambda: model.locate(img, ft, size, E, path="fused")
        ra, rb_ = arm_a(), arm_b()
        same = float((ra.y == rb_.y).logical_and(ra.x == rb_.x).float().mean())
        (s1, m1, r1), (sb, mb, rb), (s2, m2, r2) = a1_b_a2(arm_a, arm_b, iters, warmup)
        pa, pb = peak_mb(arm_a), peak_mb(arm_b)
        wins = mb + max(r1, r2, rb) < min(m1, m2)
        slower = mb - max(r1, r2, rb) > max(m1, m2)
        say(f"{name:<12s} (a) composed {s1} | again {s2}   (b) fused {sb}   a/b {0.5 * (m1 + m2) / mb:.2f}x   peak (a) {pa:.0f} (b) {pb:.0f} MiB   "
            f"same location {100 * same:.1f}%   fused wins: {'yes' if wins else 'NO'}{'   FUSED SLOWER beyond the spread' if slower else ''}")
        del model, img, ft, E
        torch.cuda.empty_cache()


def kernel_table(names, iters, warmup, say):
    """ops.xna_cos_peaks (fused) against ops.xna_cos_forward (fused, the map written) on the same operands: the kernels and their host glue."""
    import torch
    from naf_amd import ops
    dev = torch.device("cuda:0")
    say(f"# {torch.cuda.get_device_name(0)}; iters {iters}, warm-up {warmup}; (a) ops.xna_cos_forward fused (writes [B, N, Ho, Wo] fp32), (b) ops.xna_cos_peaks fused; ms: median [min .. max]")
    for name in names:
        H, h, C, k, N = SHAPES[name]
        heads = 4
        torch.manual_seed(0)
        q = torch.randn(1, heads, H, H, 64, device=dev).to(torch.bfloat16)
        kl = torch.randn(1, heads, h, h, 64, device=dev).to(torch.bfloat16)
        v = torch.randn(1, heads, h, h, C // heads, device=dev).to(torch.bfloat16)
        E = torch.randn(N, C, device=dev)
        arm_a = lambda: ops.xna_cos_forward(q, kl, v, E, k, path="fused")
        arm_b = lambda: ops.xna_cos_peaks(q, kl, v, E, k, path="fused")
        (s1, m1, r1), (sb, mb, rb), (s2, m2, r2) = a1_b_a2(arm_a, arm_b, iters, warmup)
        say(f"{name:<12s} (a) cosine map {s1} | again {s2}   (b) peaks {sb}   a/b {0.5 * (m1 + m2) / mb:.2f}x")
        del q, kl, v, E
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--kernels", action="store_true")
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
            raise SystemExit("cosine_peaks_time.py measures on a ROCm device; none found")
        (kernel_table if args.kernels else ab_table)(args.shapes.split(","), args.iters, args.warmup, say)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
