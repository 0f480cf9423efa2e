#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of the library the same bytes?   kernel_identity.py A.so B.so

For each library: dump .hip_fatbin, split it into its offload bundles (one per translation unit), unbundle every gfx950 code object, and key the bytes of
every kernel (FUNC symbol) and kernel descriptor (`*.kd` OBJECT symbol) by its mangled name.  A descriptor is compared without bytes 16-23, the offset
of the code entry from the descriptor, which moves with the kernel's place in its code object.  Prints the names only in A, only in B and those whose
bytes differ, then the three counts; exit status 0 only if all three are zero.  Runs on the CPU: it reads names and bytes, it does not disassemble.
"""
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("FVIT_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"   # first bytes of an (uncompressed) bundle


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def symbols(code_object):
    """{name: bytes} of the FUNC and .kd OBJECT symbols of one code object."""
    blob = open(code_object, "rb").read()
    sections, out = {}, {}
    for line in tool("llvm-readelf", "-S", "-s", "-W", code_object).splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) >= 6 and f[0].isdigit() and f[2].isupper() and not f[0].endswith(":"):   # [Nr] Name Type Address Off Size ...
            sections[f[0]] = (int(f[3], 16), int(f[4], 16))
        elif len(f) == 8 and f[0].endswith(":") and f[6].isdigit():                          # Num: Value Size Type Bind Vis Ndx Name
            value, size, kind, name = int(f[1], 16), int(f[2]), f[3], f[7]
            if kind == "FUNC" or (kind == "OBJECT" and name.endswith(".kd")):
                addr, off = sections[f[6]]
                data = blob[off + value - addr:off + value - addr + size]
                out[name] = data[:16] + data[24:] if kind == "OBJECT" else data
    return out


def kernels(lib, tmp):
    """{name: [bytes, ...]} over all gfx950 code objects of a library (a name may occur in several: one entry each)."""
    tag = os.path.join(tmp, str(len(os.listdir(tmp))))
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + tag + ".fatbin", lib, tag + ".copy")
    fat = open(tag + ".fatbin", "rb").read()
    starts, i = [], fat.find(MAGIC)
    while i >= 0:
        starts.append(i)
        i = fat.find(MAGIC, i + 1)
    out = {}
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(fat)])):
        bundle, co = "%s.%d.bundle" % (tag, n), "%s.%d.co" % (tag, n)
        open(bundle, "wb").write(fat[a:b])
        if TARGET not in tool("clang-offload-bundler", "--list", "--type=o", "--input=" + bundle).split():
            continue
        tool("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + bundle, "--targets=" + TARGET, "--output=" + co)
        for name, data in symbols(co).items():
            out.setdefault(name, []).append(data)
    return {k: sorted(v) for k, v in out.items()}


def main(a_path, b_path):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels(a_path, tmp), kernels(b_path, tmp)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for title, names in (("only in A", only_a), ("only in B", only_b), ("differ", differ)):
        for k in names:
            print("%s: %s" % (title, k))
    print("A = %s: %d symbols\nB = %s: %d symbols" % (a_path, len(a), b_path, len(b)))
    print("only in A: %d, only in B: %d, differ: %d" % (len(only_a), len(only_b), len(differ)))
    return 0 if a and b and not (only_a or only_b or differ) else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
