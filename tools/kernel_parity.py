"""Are the gfx950 kernels of two builds the same?  python tools/kernel_parity.py A B

A and B are two object directories (naf_amd/csrc/build of two trees) or two libraries (libnaf_hip.so).  Every host object / library
carries its device code as offload bundles in the .hip_fatbin section; each bundle's gfx950 code object is disassembled and, per kernel
symbol, two things are compared between A and B:
  * the instruction text, with addresses, encodings and branch-target labels stripped (the comment llvm-objdump appends to a line);
  * the kernel's metadata: VGPR / AGPR / SGPR counts, LDS bytes, scratch bytes;
and the number of code objects that define the symbol.  Prints the symbols that differ or exist on one side only; exit status 1 if there
are any, 0 when the two builds hold the same kernels.  A plain equality check for refactors that must not touch device code.
"""
import concurrent.futures as cf
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def _tool(name):
    for d in (os.environ.get("ROCM_LLVM_BIN"), "/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin"):
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    path = shutil.which(name)
    if not path:
        raise RuntimeError(f"{name} not found (set ROCM_LLVM_BIN)")
    return path


def _run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def _code_objects(path, tmp):
    """The gfx950 code objects (ELF files under tmp) of one host object or library: one per offload bundle."""
    stem = os.path.join(tmp, os.path.basename(path))
    fat = stem + ".fatbin"
    r = subprocess.run([_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", path, stem + ".copy"], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(fat):
        return []                      # no device code in this object
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = []
    for n, (lo, hi) in enumerate(zip(starts, starts[1:] + [len(data)])):
        piece, elf = f"{stem}.{n}.bundle", f"{stem}.{n}.elf"
        with open(piece, "wb") as fh:
            fh.write(data[lo:hi])
        r = subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={piece}", f"--output={elf}"],
                           capture_output=True, text=True)
        if r.returncode == 0 and os.path.exists(elf) and os.path.getsize(elf) > 0:
            out.append(elf)
    return out


def _kernels(elf):
    """{kernel symbol: (instruction text, metadata tuple)} of one code object."""
    meta, cur = {}, None
    for line in _run(_tool("llvm-readelf"), "--notes", elf).splitlines():
        if line.startswith("  - ."):
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    \.(\w+): +(\S+)$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = cur
    text, sym = {}, None
    for line in _run(_tool("llvm-objdump"), "-d", "--no-show-raw-insn", elf).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym = m.group(1)
            text[sym] = []
        elif sym is not None and line.startswith("\t"):
            text[sym].append(line.split("//")[0].strip())       # drops address, encoding and <label+offset>
    return {k: ("\n".join(text.get(k, [])), tuple(v.get(f) for f in META)) for k, v in meta.items()}


def collect(path):
    """{symbol: [(text, metadata) per defining code object]} of an object directory or a library."""
    files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".o")) if os.path.isdir(path) else [path]
    tmp = tempfile.mkdtemp(prefix="kernel_parity_")
    try:
        with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 2)) as ex:
            elfs = [e for es in ex.map(lambda f: _code_objects(f, tmp), files) for e in es]
            found = {}
            for ks in ex.map(_kernels, elfs):
                for sym, what in ks.items():
                    found.setdefault(sym, []).append(what)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return found


def main(a, b):
    ka, kb = collect(a), collect(b)
    bad = 0
    for sym in sorted(set(ka) | set(kb)):
        if sym not in ka or sym not in kb:
            print(f"only in {'B' if sym not in ka else 'A'}: {sym}")
        elif len(ka[sym]) != len(kb[sym]):
            print(f"defined by {len(ka[sym])} code objects in A, {len(kb[sym])} in B: {sym}")
        elif sorted(t for t, _ in ka[sym]) != sorted(t for t, _ in kb[sym]):
            print(f"instructions differ: {sym}")
        elif sorted(m for _, m in ka[sym]) != sorted(m for _, m in kb[sym]):
            print(f"metadata differ ({', '.join(META)}): {sorted(m for _, m in ka[sym])} vs {sorted(m for _, m in kb[sym])}: {sym}")
        else:
            continue
        bad += 1
    print(f"{len(ka)} kernel symbols in A, {len(kb)} in B, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
