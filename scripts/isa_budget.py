#!/usr/bin/env python3
"""Static instruction budget of one fused conditional-block kernel (cond_split_kernels.hip), from its gfx950 assembly.

    python3 scripts/isa_budget.py [--inst 2,false,false,2] [--asm FILE.s] [--json]

Cross-compiles cond_split_kernels.hip with the Makefile's CXXFLAGS (device only, -S) -- or reads an assembly file made that way -- and
reports for cond_gf_split_kernel<RG, FWD, SAVE, NP>: VGPRs, scratch, waves per SIMD allowed by the registers, and per region the count of
vector instructions, transcendentals, MFMAs and s_nop with their weighted issue cycles, and of the row reductions' lane swaps
(v_permlane16_swap / v_permlane32_swap).  Regions, in text order:
  phase1  everything in front of the layer loop (MLP input staging, tanh, f16 split) -- the layer loop is the one holding the MFMAs
  matrix  the layer loop's blocks up to its last MFMA (chunk DMA, LDS reads, MFMAs)
  flow    the rest of the layer loop (offset, reflections, mixture, inverse CDF, log-det reduction), every branch counted once
  tail    after the layer loop (epilogue)
Issue weights per instruction, one wave's stream on one SIMD (MI355X): transcendental VALU 8 cycles, MFMA 8 (the vector issue it
holds), any other VALU 4, s_nop 4.  Static counts: both sides of every branch are counted, the loop body once.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jammy_flows_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
TRANS = re.compile(r"^v_(exp|log|rcp|rsq|sqrt|sin|cos)_f(16|32)(_e32|_e64)?$")
WEIGHT = {"trans": 8, "mfma": 8, "valu": 4, "nop": 4}
SWAPS = {"swap16": "v_permlane16_swap", "swap32": "v_permlane32_swap"}       # the row reductions' lane exchanges (csrc/jf_cond_split.h)
VGPR_POOL, VGPR_GRANULE, MAX_WAVES = 512, 8, 8


def makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    return [f for f in flags if f not in ("-fPIC",)]


def compile_asm(out_path, hipcc=HIPCC):
    src = os.path.join(CSRC, "cond_split_kernels.hip")
    subprocess.check_call([hipcc] + makefile_flags() + ["--cuda-device-only", "-S", src, "-o", out_path], cwd=CSRC,
                          stderr=subprocess.DEVNULL)


def mangled(rg, fwd, save, np_):
    b = lambda v: "1" if v else "0"
    return "_ZN2jf20cond_gf_split_kernelILi%dELb%sELb%sELi%dEEEvNS_6CsArgsE" % (rg, b(fwd), b(save), np_)


def kernel_text(asm, name):
    # from the function's label to its end label (a kernel may hold more than one s_endpgm)
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def metadata(asm, name):
    m = re.search(r"\.name:\s+%s\n(.*?)(?:\n  - |\n\.\.\.|\Z)" % re.escape(name), asm, re.S)
    blk = m.group(1) if m else ""
    # the metadata map lists its keys alphabetically; .agpr_count precedes .name
    pre = asm[:m.start()] if m else ""
    def g(k, text):
        r = re.findall(r"\.%s:\s+(\d+)" % k, text)
        return int(r[-1]) if r else 0
    return {"vgpr": g("vgpr_count", blk), "agpr": g("agpr_count", pre), "scratch": g("private_segment_fixed_size", blk),
            "vgpr_spill": g("vgpr_spill_count", blk), "sgpr_spill": g("sgpr_spill_count", blk)}


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "mfma"
    if TRANS.match(op):
        return "trans"
    if op.startswith("v_"):
        return "valu"
    if op == "s_nop":
        return "nop"
    return None


def budget(body):
    # the layer loop: the natural loop (LLVM's "Loop: Header=" annotations, depth 1) whose blocks hold the most MFMAs
    block_loop, cur = [], None
    for l in body:
        m = re.match(r"^(\.LBB\w+|; %bb\.\d+):.*?(?:Loop: Header=(\w+) Depth=1|=>This Inner Loop Header: Depth=1)?\s*$", l)
        if m:
            hdr = m.group(2)
            if "=>This Inner Loop Header: Depth=1" in l:
                hdr = m.group(1).lstrip(".L")
            cur = hdr
        block_loop.append(cur)
    ops = [(i, l.split()[0]) for i, l in enumerate(body) if l.startswith("\t") and l.split() and not l.split()[0].startswith((".", ";"))]
    count = {}
    for i, op in ops:
        if classify(op) == "mfma" and block_loop[i]:
            count[block_loop[i]] = count.get(block_loop[i], 0) + 1
    if not count:
        raise SystemExit("no loop holding MFMAs")
    loop = max(count, key=count.get)              # (phase 1's f32 MFMA loops hold a few)
    in_loop = [i for i, _ in ops if block_loop[i] == loop]
    first, last_loop = in_loop[0], in_loop[-1]
    last_mfma = max(i for i, op in ops if block_loop[i] == loop and classify(op) == "mfma")
    regions = {r: {"valu": 0, "trans": 0, "mfma": 0, "nop": 0, "swap16": 0, "swap32": 0} for r in ("phase1", "matrix", "flow", "tail")}
    for i, op in ops:
        c = classify(op)
        if c is None:
            continue
        if block_loop[i] == loop:
            r = "matrix" if i <= last_mfma else "flow"
        else:
            r = "phase1" if i < first else ("tail" if i > last_loop else "phase1")
        regions[r][c] += 1
        for k, name in SWAPS.items():                  # (counted as "valu" above; listed on their own as well)
            if op.startswith(name):
                regions[r][k] += 1
    for r in regions.values():
        r["vector"] = r["valu"] + r["trans"]          # non-MFMA vector instructions
        r["cycles"] = sum(WEIGHT[k] * r[k] for k in WEIGHT)
    return regions


def report(asm, inst):
    rg, fwd, save, np_ = inst
    name = mangled(rg, fwd, save, np_)
    if name + ":" not in asm:
        raise SystemExit("no kernel %s in the assembly" % name)
    md = metadata(asm, name)
    regs = md["vgpr"] + md["agpr"]
    alloc = -(-regs // VGPR_GRANULE) * VGPR_GRANULE
    md["waves_per_simd"] = min(MAX_WAVES, VGPR_POOL // max(alloc, 1))
    return {"kernel": "cond_gf_split_kernel<%d,%s,%s,%d>" % (rg, str(fwd).lower(), str(save).lower(), np_), **md,
            "regions": budget(kernel_text(asm, name))}


def parse_inst(s):
    p = s.split(",")
    tf = lambda v: v.strip().lower() in ("1", "true")
    return int(p[0]), tf(p[1]), tf(p[2]), int(p[3])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--inst", default="2,false,false,2", help="RG,FWD,SAVE,NP of cond_gf_split_kernel (default: the benchmarked one)")
    ap.add_argument("--asm", help="read this assembly instead of compiling")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "cs.s")
            compile_asm(out)
            asm = open(out).read()
    r = report(asm, parse_inst(a.inst))
    if a.json:
        print(json.dumps(r, indent=1))
        return
    print("%s: %d VGPRs (+%d AGPRs), scratch %d B, spills v%d s%d, %d waves per SIMD by registers" %
          (r["kernel"], r["vgpr"], r["agpr"], r["scratch"], r["vgpr_spill"], r["sgpr_spill"], r["waves_per_simd"]))
    print("%-7s %7s %7s %7s %7s %9s %7s %7s" % ("region", "vector", "trans", "mfma", "s_nop", "cycles", "swap16", "swap32"))
    for k, v in r["regions"].items():
        print("%-7s %7d %7d %7d %7d %9d %7d %7d" % (k, v["vector"], v["trans"], v["mfma"], v["nop"], v["cycles"], v["swap16"], v["swap32"]))


if __name__ == "__main__":
    sys.exit(main())
