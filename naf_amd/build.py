"""Build libnaf_hip.so (gfx950) in-tree with hipcc.  ``python -m naf_amd.build [--force]``.

hipcc cross-compiles for gfx950 without a GPU.  One object per translation unit, compiled in
parallel, then one ``hipcc -shared`` link.  The windowed attention kernels are the exception: each
family has ONE instance source (``xna_*_inst.hip``, explicit template instantiations only) that is
compiled once per entry of ``INSTANCES`` with ``-DNAF_KS=<window>`` (and ``-DNAF_HALF=0|1``), one
object per instance (``xna_mfma_inst_k9_h.o``).  The link refuses undefined symbols, so an instance
a dispatcher declares but the table lacks fails the build.  The library keeps a plain DT_NEEDED on libamdhip64.so.7
and NO rpath: when loaded after ``import torch`` the loader reuses the HIP runtime torch already
mapped (same SONAME), so stream handles and device pointers are shared with torch.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
OBJDIR = os.path.join(CSRC, "build")
LIB = os.path.join(CSRC, "libnaf_hip.so")
ARCH = "gfx950"
# MFMA results in VGPRs (no v_accvgpr_read per result register) wherever the kernel does not need the AGPR half
# of the register file; the weight-stationary 3x3 stem layer fills all 512 registers and keeps the default.
VGPR_FORM = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
NO_VGPR_FORM = {"stem_conv.hip"}
# Per-file flags.  stem_conv.hip: the schedule's GroupNorm / SiLU / sums arithmetic is written as plain f32 operations on purpose
# -- a packed v_pk_*_f32 beside an MFMA stalls the matrix pipe ~16 cycles (profiles/r03_mfma_filler_prices.txt) -- and the SLP
# vectoriser would pack adjacent ones again.  denoise.hip: its fused multiply-adds are written out; with the compiler's own contraction
# off, expressions that are symmetric in pred and target round symmetrically (the SSIM gradient of identical windows is exactly zero).
# mask_labels.hip: its two passes must round the upsampled value identically, so the compiler contracts nothing there either.
# image_prep.hip: its values are defined operation by operation (include/naf_hip.h), and the tests ask for those bits.
EXTRA_FLAGS = {"stem_conv.hip": ["-fno-slp-vectorize"], "denoise.hip": ["-ffp-contract=off"], "mask_labels.hip": ["-ffp-contract=off"],
               "image_prep.hip": ["-ffp-contract=off"]}
# Instance sources -> the (window, half) instances they are compiled for (half None: the family has one value type).  The lists are
# NAF_FOR_WINDOWS / NAF_FOR_SLIDE_WINDOWS of naf_common.h.
_WINDOWS, _SLIDE_WINDOWS = (3, 5, 7, 9, 11, 13, 15), (7, 9, 11, 13, 15)
INSTANCES = {
    "xna_mfma_inst.hip": [(k, h) for h in (0, 1) for k in _WINDOWS],
    "xna_slide_inst.hip": [(k, h) for h in (0, 1) for k in _SLIDE_WINDOWS],
    "xna_union_inst.hip": [(k, h) for h in (0, 1) for k in _WINDOWS],
    "xna_union_mse_inst.hip": [(k, None) for k in _WINDOWS],
    "xna_head_inst.hip": [(k, None) for k in _WINDOWS],
    "xna_cos_inst.hip": [(k, None) for k in _WINDOWS],
    "xna_pool_inst.hip": [(k, None) for k in _WINDOWS],
    "xna_kmeans_inst.hip": [(k, None) for k in _WINDOWS],
    "xna_bwd_inst.hip": [(k, None) for k in _WINDOWS],
}


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def _units():
    """(source, object stem, defines) of every object: plain sources once, instance sources once per INSTANCES entry."""
    units = [(f, os.path.splitext(f)[0], []) for f in os.listdir(CSRC) if f.endswith(".hip") and f not in INSTANCES]
    for src, insts in INSTANCES.items():
        for k, half in insts:
            stem = f"{os.path.splitext(src)[0]}_k{k}" + ("_h" if half else "")
            units.append((src, stem, [f"-DNAF_KS={k}"] + ([] if half is None else [f"-DNAF_HALF={half}"])))
    return sorted(units, key=lambda u: u[1])


def _deps_mtime() -> float:
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    hdrs.append(os.path.join(INCLUDE, "naf_hip.h"))
    hdrs.append(os.path.abspath(__file__))
    return max(os.path.getmtime(h) for h in hdrs)


def _compile(unit, force: bool, hdr_mtime: float, extra) -> str:
    src, stem, defines = unit
    obj = os.path.join(OBJDIR, stem + ".o")
    spath = os.path.join(CSRC, src)
    if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(spath), hdr_mtime):
        return obj
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall",
           "-Wno-unused-function", f"-I{INCLUDE}", f"-I{CSRC}", *([] if src in NO_VGPR_FORM else VGPR_FORM), *EXTRA_FLAGS.get(src, []), *defines, *extra, "-c", spath, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {stem}:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return obj


def build_library(force: bool = False, verbose: bool = False, extra_flags=()) -> str:
    os.makedirs(OBJDIR, exist_ok=True)
    units = _units()
    hdr_mtime = _deps_mtime()
    with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 2)) as ex:
        objs = list(ex.map(lambda s: _compile(s, force, hdr_mtime, list(extra_flags)), units))
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(o) for o in objs):
        cmd = [_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-fno-gpu-rdc", "-Wl,--no-undefined", "-o", LIB, *objs]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    if verbose:
        print(f"built {LIB} ({os.path.getsize(LIB) / 1024:.0f} KiB) from {len(objs)} objects")
    return LIB


if __name__ == "__main__":
    build_library(force="--force" in sys.argv, verbose=True)
