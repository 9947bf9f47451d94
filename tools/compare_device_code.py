"""Compare the gfx950 device code of two builds, kernel by kernel (run by hand after a change that must not touch kernels).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -Iinclude --cuda-device-only -c uvc_amd/csrc/gemm_tn.hip -o new.o   (and parent.o)
    python tools/compare_device_code.py parent.o new.o > profiles/<name>.txt

Either side may be several objects, the two sides separated by `--` (a file split into several, or the reverse):

    for f in uvc_amd/csrc/gemm*.hip; do hipcc <the same flags> --cuda-device-only -c $f -o new_$(basename $f .hip).o; done
    python tools/compare_device_code.py parent_*.o -- new_gemm*.o > profiles/<name>.txt

(gemm.hip defines no kernel; its device-only object unbundles to an empty code object and adds nothing to its side.)

A side is the union of its objects' kernels by mangled name; a name that two objects of one side define is an error (a kernel must not end up in
two objects).  Unbundles the objects, reads the kernel metadata (llvm-readelf --notes) and the symbol table (llvm-readelf -s), and compares for every kernel:
function size, .vgpr_count, .agpr_count, .sgpr_count, .group_segment_fixed_size, .private_segment_fixed_size, .vgpr_spill_count, and the bytes
of the function in .text.  Exit status 1 when anything differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def load(obj, tmp, tag):
    elf = os.path.join(tmp, tag + ".elf")
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + obj, "--output=" + elf)
    meta = {}
    cur = None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", elf).splitlines():
        m = re.match(r"  ([- ]) (\.\w+):\s*(.*)$", line)      # a kernel's own keys: two levels in ("  - " opens a kernel's map)
        if not m:
            continue
        if m.group(1) == "-":
            cur = {}
        cur[m.group(2)] = m.group(3).strip()
        if m.group(2) == ".name":
            meta[m.group(3).strip().strip("'\"")] = cur
    data = open(elf, "rb").read()
    text_off = text_addr = None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "-S", elf).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text_addr, text_off = int(m.group(1), 16), int(m.group(2), 16)
    syms = {}
    for line in run(os.path.join(LLVM, "llvm-readelf"), "-s", "-W", elf).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND":
            addr, size = int(f[1], 16), int(f[2])
            syms[f[7]] = (size, data[text_off + addr - text_addr: text_off + addr - text_addr + size])
    return meta, syms


def load_side(objs, tmp, tag):
    """union of the objects' kernels; -> (metadata, functions, names defined by more than one object)"""
    meta, syms, twice = {}, {}, []
    for i, obj in enumerate(objs):
        m, s = load(obj, tmp, f"{tag}{i}")
        twice += [f"{k} ({obj})" for k in m if k in meta]
        meta.update(m)
        syms.update(s)
        print(f"  {obj}: {len(m)} kernels")
    return meta, syms, twice


def main(a, b):
    with tempfile.TemporaryDirectory() as tmp:
        ma, sa, ta = load_side(a, tmp, "a")
        mb, sb, tb = load_side(b, tmp, "b")
    ka, kb = set(ma), set(mb)
    print(f"kernels: {len(ka)} in {' '.join(a)}, {len(kb)} in {' '.join(b)}; only in first {sorted(ka - kb)}; only in second {sorted(kb - ka)}")
    print(f"defined by two objects of one side: {ta + tb}")
    bad = len(ka ^ kb) + len(ta) + len(tb)
    nbytes = 0
    for k in sorted(ka & kb):
        diffs = [f"{f} {ma[k].get(f)} -> {mb[k].get(f)}" for f in FIELDS if ma[k].get(f) != mb[k].get(f)]
        if k not in sa or k not in sb:
            diffs.append("no function symbol")
        else:
            if sa[k][0] != sb[k][0]:
                diffs.append(f"size {sa[k][0]} -> {sb[k][0]}")
            if sa[k][1] != sb[k][1]:
                diffs.append("bytes differ")
            nbytes += sa[k][0]
        if diffs:
            bad += 1
            print("DIFFERENT", k, "; ".join(diffs))
    print(f"compared {len(ka & kb)} kernels, {nbytes} bytes of code, {len(FIELDS)} metadata fields each: {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--" in args:
        sys.exit(main(args[:args.index("--")], args[args.index("--") + 1:]))
    sys.exit(main(args[:1], args[1:2]))
