#!/usr/bin/env python3
"""Instruction histogram of k_snet6 by SOURCE REGION and instruction class (profiles/s6_adjoint_isa.md).

isa_hist.py / isa_loops.py count per basic block and per loop; a block of the tile program mixes the vector block, the chunk
steps and the deposit of a layer, and the helpers (split2, tag_cos, mfma_x3, first_layer ...) are inlined several times.  Here
every instruction of the code object is attributed to the k_snet6.hip line of its OUTERMOST inlined frame (llvm-symbolizer
--inlines on a -gline-tables-only build: the line tables change no instruction), and the lines to regions by the section comments
of the source.  A basic block that holds fp64 instructions is the large-argument sine fallback: counted apart as "cold".

usage: tools/isa_regions.py [--kernel MANGLED] [--lines] [source.hip]      (default: nif_amd/csrc/k_snet6.hip, k_snet6<4,0,0,0>;
the one-coordinate, one-output form: --kernel _Z7k_snet6ILi4ELi0ELi1ELi1EEv6S6Args)"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter, defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "--cuda-device-only", "--no-gpu-bundle-output", "-gline-tables-only"]

# (region, text that opens it) in source order; a region runs to the next one's opening line
ANCHORS = [
    ("prologue (all waves)", "__global__ __launch_bounds__(1024, 4) void k_snet6"),
    ("consumer", "if (wid >= WAVES) {"),
    ("producer set-up", "producer wave = one 16-point tile per round"),
    ("first layer, forward", "// ---- first layer ---"),
    ("forward layer", "// ---- hidden hyper-matrices, forward"),
    ("last layer + MSE", "// ---- last layer (n -> so"),
    ("adjoint: vector block", "// ---- adjoint through the hidden"),
    ("adjoint: h_j (ring / h_0 again)", "f32x4 U[NBL];"),
    ("adjoint: chunk steps", "if (BIG) S6_CHUNK2(true, q0, q1, U)"),
    ("adjoint: deposit", "{     // deposit j:"),
    ("first-layer adjoint", "lgkmcnt(0): the deposits have landed"),
    ("epilogue", "#undef S6_CHUNK\n"),
]
CLASSES = ["transc", "pk fma", "fp32", "cvt", "mov/sel/bit", "int", "f64", "mfma", "lds", "vmem", "wait/nop", "salu"]


def classify(op):
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if "f64" in op:
        return "f64"
    if op.startswith(("v_sin", "v_cos", "v_sqrt", "v_rsq", "v_rcp", "v_exp", "v_log")):
        return "transc"
    if op.startswith("v_pk_"):
        return "pk fma"
    if op.startswith("v_cvt"):
        return "cvt"
    if op.startswith(("v_mov", "v_cndmask", "v_and", "v_or", "v_xor", "v_not", "v_lshl", "v_lshr", "v_ashr", "v_bfi", "v_bfe", "v_perm",
                      "v_accvgpr", "v_readlane", "v_writelane", "v_readfirstlane", "v_alignbit", "v_swap")):
        return "mov/sel/bit"
    if op.startswith("v_") and ("f32" in op or "f16" in op or "bf16" in op):
        return "fp32"
    if op.startswith("v_"):
        return "int"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier")):
        return "wait/nop"
    return "salu"


def regions_of(src):
    text = open(src).read()
    out, pos = [], 0
    for name, a in ANCHORS:
        pos = text.find(a, pos)
        if pos < 0:
            sys.exit("anchor not found (in order) in %s: %r" % (src, a))
        out.append((text.count("\n", 0, pos) + 1, name))
        pos += 1
    return out


def main():
    kern = sys.argv[sys.argv.index("--kernel") + 1] if "--kernel" in sys.argv else "_Z7k_snet6ILi4ELi0ELi0ELi0EEv6S6Args"
    args = [a for a in sys.argv[1:] if not a.startswith("--") and a != kern]
    src = os.path.abspath(args[0]) if args else os.path.join(ROOT, "nif_amd", "csrc", "k_snet6.hip")
    regs = regions_of(src)
    base = os.path.basename(src)
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "k.co")
        subprocess.check_call([HIPCC] + FLAGS + ["-c", src, "-o", co], stderr=subprocess.DEVNULL)
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--symbolize-operands", co],
                             stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        ins, blk, inside = [], 0, False          # (address, mnemonic, basic block)
        for l in dis.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.*)>:", l)
            if m and re.match(r"^L\d+$", m.group(1)):          # a branch target inside the current function
                blk += 1
                continue
            if m:
                inside = m.group(1) == kern
                continue
            if not inside:
                continue
            m = re.match(r"^\s+([a-z][a-z0-9_]+)\b.*//\s*([0-9A-Fa-f]+):", l)
            if m:
                ins.append((int(m.group(2), 16), m.group(1), blk))
                if m.group(1) in ("s_branch", "s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_execz", "s_cbranch_execnz"):
                    blk += 1
        sym = subprocess.run([os.path.join(LLVM, "llvm-symbolizer"), "--obj=" + co, "--inlines", "--output-style=LLVM", "--functions=none"],
                             input="\n".join("0x%x" % a for a, _, _ in ins), stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    stacks = [s for s in sym.split("\n\n") if s.strip()]
    assert len(stacks) == len(ins), (len(stacks), len(ins))
    cold_blocks = set(b for _, op, b in ins if "f64" in op)
    hist = defaultdict(Counter)
    by_line = defaultdict(Counter)
    for (addr, op, b), st in zip(ins, stacks):
        line = 0
        for fr in st.strip().split("\n"):          # innermost first: the last frame of this file is the kernel's own line
            m = re.match(r"^(.*):(\d+):(\d+)$", fr.strip())
            if m and os.path.basename(m.group(1)) == base:
                line = int(m.group(2))
        name = "?"
        for l0, n in regs:
            if line >= l0:
                name = n
        if b in cold_blocks:
            name += " [cold: fp64 sine fallback]"
        hist[name][classify(op)] += 1
        by_line[(name, line)][op] += 1
    print("| region | " + " | ".join(CLASSES) + " | VALU | all |\n|---|" + "---|" * (len(CLASSES) + 2))
    order = [n for _, n in regs] + ["?"]
    for n in sorted(hist, key=lambda n: (order.index(n.split(" [")[0]), "[" in n)):
        c = hist[n]
        valu = sum(c[k] for k in CLASSES[:7])
        print("| %s | " % n + " | ".join(str(c[k]) for k in CLASSES) + " | %d | %d |" % (valu, sum(c.values())))
    if "--lines" in sys.argv:
        print("\n| region | line | instructions |\n|---|---|---|")
        for (n, line), c in sorted(by_line.items(), key=lambda kv: (kv[0][1], kv[0][0])):
            print("| %s | %d | %s |" % (n, line, ", ".join("%s %d" % kv for kv in c.most_common())))


if __name__ == "__main__":
    main()
