#!/usr/bin/env python3
"""Instruction mix of a kernel's large basic blocks, from the compiler's assembly. Needs no GPU.

Compiles one .hip file device-only to gfx950 assembly with the flags of zk-proof-of-assets_amd/Makefile (or reads an
assembly file made that way), cuts every kernel whose demangled name contains one of the --kernel substrings into basic
blocks (at labels and after branches), and prints for each block of at least --min-block instructions the
instruction count and a histogram of its vector-ALU (v_...) opcodes, then NumVgprs, ScratchSize and Occupancy from the
kernel's footer. It is a histogram of whatever is there: it looks for no particular instruction.

  python tools/kernel_loop_mix.py zk-proof-of-assets_amd/csrc/msm_g1.hip --kernel msm_accum0_kernel \\
      --kernel 'msm_accumN_kernel<zkpoa::Fp<zkpoa::FqParams>, true>' --kernel 'msm_bucket_sums_kernel<zkpoa::Fp<zkpoa::FqParams>, true>'
  --show OPCODE   also lists, per block, the full text of the instructions with that opcode
"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEFILE = os.path.join(ROOT, "zk-proof-of-assets_amd", "Makefile")
FOOTER_KEYS = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")


def makefile_flags():
    text = open(MAKEFILE).read()
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    flags = var["CXXFLAGS"]
    for _ in range(4):
        flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), flags)
    return var.get("HIPCC", "hipcc"), flags.split()


def compile_to_asm(src, out):
    hipcc, flags = makefile_flags()
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return " ".join(cmd[:-1] + ["<out>"])


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels(lines):
    """{mangled name: (first body line, line after the body, footer dict)} for every .amdhsa kernel"""
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    found = {}
    for name in names:
        begin = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(begin, len(lines)) if lines[i].startswith(".Lfunc_end"))
        footer = {}
        for l in lines[end:end + 80]:
            m = re.match(r";\s*(\w+)\s*:\s*(\d+)", l)
            if m and m.group(1) in FOOTER_KEYS and m.group(1) not in footer:
                footer[m.group(1)] = int(m.group(2))
        found[name] = (begin + 1, end, footer)
    return found


def basic_blocks(body):
    """[(label, [instruction text])]: a block ends before a label and after a branch or the end of the program"""
    blocks, label, cur = [], "entry", []
    for l in body:
        text = l.split(";")[0].rstrip()
        m = re.match(r"(\.?\w+):", text)
        if m:
            if cur:
                blocks.append((label, cur))
            label, cur = m.group(1), []
            continue
        text = text.strip()
        if not text or text.startswith("."):
            continue
        cur.append(text)
        op = text.split()[0]
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            blocks.append((label, cur))
            label, cur = label + "+", []
    if cur:
        blocks.append((label, cur))
    return blocks


def report(name, pretty, lines, begin, end, footer, min_block, show, out):
    blocks = basic_blocks(lines[begin:end])
    total = sum(len(b) for _, b in blocks)
    out.write("kernel %s\n" % pretty)
    out.write("  %d instructions in %d basic blocks; %s\n" % (
        total, len(blocks), ", ".join("%s %s" % (k, footer.get(k, "?")) for k in FOOTER_KEYS)))
    for label, ins in blocks:
        if len(ins) < min_block:
            continue
        ops = collections.Counter(i.split()[0] for i in ins)
        valu = sum(c for o, c in ops.items() if o.startswith("v_"))
        out.write("  block %s: %d instructions, %d vector-ALU, %d other\n" % (label, len(ins), valu, len(ins) - valu))
        for o, c in sorted(ops.items(), key=lambda kv: (-kv[1], kv[0])):
            if o.startswith("v_"):
                out.write("    %6d  %s\n" % (c, o))
        others = ["%s %d" % (o, c) for o, c in sorted(ops.items(), key=lambda kv: (-kv[1], kv[0])) if not o.startswith("v_")]
        if others:
            out.write("    other: %s\n" % ", ".join(others))
        for i in ins:
            if show and i.split()[0] == show:
                out.write("    > %s\n" % i)
    out.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="a .hip file to compile, or a .s file already compiled with the Makefile's flags")
    ap.add_argument("--kernel", action="append", required=True, help="substring of the demangled kernel name (repeatable)")
    ap.add_argument("--min-block", type=int, default=400, help="smallest basic block to print (instructions)")
    ap.add_argument("--show", default=None, help="opcode whose instructions are listed in full")
    ap.add_argument("--keep-asm", default=None, help="write the assembly here as well")
    a = ap.parse_args()

    if a.source.endswith(".s"):
        lines, how = open(a.source).read().splitlines(), "read " + os.path.basename(a.source)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            path = a.keep_asm or os.path.join(tmp, "kernel.s")
            how = compile_to_asm(a.source, path)
            lines = open(path).read().splitlines()
    ks = kernels(lines)
    pretty = demangle(list(ks))
    out = sys.stdout
    out.write("# %s\n\n" % how)
    missing = 0
    for want in a.kernel:
        hits = [n for n in ks if want in pretty[n]]
        if not hits:
            out.write("no kernel matches %r\n\n" % want)
            missing += 1
        for n in hits:
            begin, end, footer = ks[n]
            report(n, pretty[n], lines, begin, end, footer, a.min_block, a.show, out)
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
