#!/usr/bin/env python3
"""Manifest of the gfx950 device code the library is built from: for every source the Makefile
compiles, each function symbol with its code size, and each kernel's registers, LDS, scratch,
kernel-argument bytes and - where it has any - the dwords of its argument block the kernel descriptor
asks the command processor to preload into user SGPRs.  A source is compiled with the flags the Makefile
gives it (its `<stem>.o: CXXFLAGS += ...` line included).  A change that touches host code only must leave this manifest as it is:
same kernels, same sizes, same resources (profiles/kernel_manifest.txt holds the committed one).

Needs no GPU.  Reads the symbol table and the metadata notes only.

    python tools/kernel_manifest.py                 # print the manifest
    python tools/kernel_manifest.py --out FILE      # write it
    python tools/kernel_manifest.py --check FILE    # exit 1 and show a diff if FILE differs
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tf-recomm_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
ARCH = "gfx950"
META_KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size")


def makefile_sources(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    m = re.search(r"^SRCS\s*:=\s*(.*\.hip.*)$", text, re.M)
    return [s for s in m.group(1).split() if os.path.exists(os.path.join(csrc, s))]


def makefile_extra_flags(csrc, stem):
    """the flags of a target-specific `<stem>.o: CXXFLAGS += ...` line"""
    m = re.search(r"^%s\.o:\s*CXXFLAGS\s*\+=\s*(.*)$" % re.escape(stem), open(os.path.join(csrc, "Makefile")).read(), re.M)
    return m.group(1).split() if m else []


def preload_lengths(elf, names):
    """{kernel: KERNARG_PRELOAD_SPEC_LENGTH}: bits 0-6 of the 16-bit word at byte 58 of the kernel descriptor <kernel>.kd"""
    sections = run([os.path.join(LLVM, "llvm-readelf"), "-S", "-W", elf])
    where = {}
    for line in sections.splitlines():
        m = re.match(r"^\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            where[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16))
    blob = open(elf, "rb").read()
    out = {}
    for line in run([os.path.join(LLVM, "llvm-objdump"), "-t", elf]).splitlines():
        m = re.match(r"^([0-9a-f]+)\s+\S+\s+O\s+(\S+)\s+[0-9a-f]+\s+(?:\.\w+\s+)?(\S+)\.kd$", line)
        if m and m.group(3) in names and m.group(2) in where:
            addr, off, size = where[m.group(2)]
            at = int(m.group(1), 16) - addr + off + 58
            out[m.group(3)] = int.from_bytes(blob[at:at + 2], "little") & 0x7f
    return out


def run(cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True).stdout


def manifest_of(src, csrc, tmp):
    stem = os.path.splitext(src)[0]
    bundle, elf = os.path.join(tmp, stem + ".bundle.o"), os.path.join(tmp, stem + ".elf")
    run([os.path.join(ROCM, "bin", "hipcc"), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC",
         "-I" + os.path.join(ROOT, "include"), "-I.", "-Wall", "-Wno-unused-result"] + makefile_extra_flags(csrc, stem) +
        ["--cuda-device-only", "-c", src, "-o", bundle], cwd=csrc)
    run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
         "--targets=hip-amdgcn-amd-amdhsa--" + ARCH, "--input=" + bundle, "--output=" + elf])
    funcs = []
    for line in run([os.path.join(LLVM, "llvm-objdump"), "-t", elf]).splitlines():
        # value, flags ("g     F"), section, size, [visibility], name
        m = re.match(r"^[0-9a-f]+\s+\S+\s+F\s+\S+\s+([0-9a-f]+)\s+(?:\.\w+\s+)?(\S+)$", line)
        if m:
            funcs.append((m.group(2), int(m.group(1), 16)))
    kernels, cur = {}, {}
    for line in run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf]).splitlines():
        m = re.match(r"^(  - |    )(\.\w+):\s+(\S+)\s*$", line)   # a kernel's own keys: not those of its .args, nested deeper
        if not m:
            continue
        lead, key, val = m.groups()
        if lead == "  - ":
            cur = {}
        if key == ".name" or key in META_KEYS:
            cur[key] = val
        if len(cur) == len(META_KEYS) + 1:
            kernels[cur[".name"]] = cur
            cur = {}
    preload = preload_lengths(elf, kernels)
    out = ["== %s: %d functions, %d kernels" % (src, len(funcs), len(kernels))]
    for name, size in sorted(funcs):
        out.append("func %s size=%d" % (name, size))
    for name in sorted(kernels):
        k = kernels[name]
        out.append("kernel %s vgpr=%s sgpr=%s lds=%s scratch=%s kernarg=%s%s" % (
            name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"],
            k[".private_segment_fixed_size"], k[".kernarg_segment_size"],
            " preload=%d" % preload[name] if preload.get(name) else ""))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=CSRC, help="source directory with the Makefile (default: the package's)")
    ap.add_argument("--out", help="write the manifest here instead of printing it")
    ap.add_argument("--check", help="compare against this manifest")
    ap.add_argument("-j", type=int, default=4)
    a = ap.parse_args()
    srcs = makefile_sources(a.csrc)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.j) as pool:
        text = "".join(pool.map(lambda s: manifest_of(s, a.csrc, tmp), sorted(srcs)))
    if a.check:
        want = open(a.check).read()
        if want != text:
            sys.stdout.writelines(difflib.unified_diff(want.splitlines(True), text.splitlines(True), a.check, "built now"))
            return 1
        print("manifest unchanged: %d lines" % text.count("\n"))
        return 0
    if a.out:
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
