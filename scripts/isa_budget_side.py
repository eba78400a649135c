#!/usr/bin/env python3
"""Static instruction budget of the conditional manifold block (cond_manifold_kernels.hip), from its gfx950 assembly.

    python3 scripts/isa_budget_side.py [--asm FILE.s] [--no-ocml] [--json]

Cross-compiles cond_manifold_kernels.hip with the Makefile's CXXFLAGS (device only, -S) -- or reads an assembly file made that way -- and
reports for cond_mchain_kernel<float, FFam, 256, false> (`jf_cond_f_chain_inv_f32`, the s2 block of the benchmarked step): VGPRs, scratch,
waves per SIMD allowed by the registers, and per region the count of vector instructions, transcendentals, MFMAs and s_nop with their
weighted issue cycles (the weights of scripts/isa_budget.py).  Regions, in text order:
  stage    everything in front of the first v_mfma_f32_16x16x4_f32: W1 / b1 / W2 staging once per workgroup, the row tile's input staging
  product  the K1 -> 128 product (first to last f32 MFMA)
  act      between the last f32 MFMA and the first v_mfma_f32_16x16x32_f16: tanh and the f16 split of a lane's 32 hidden values
  second   the 128 -> N product (first to last f16 MFMA)
  hidden   = stage + product + act + second: the hidden layer, up to the last v_mfma_f32_16x16x32_f16
  layers   everything behind it: parameter tile write, the `f` layers lane-per-row, epilogue
Static counts: both sides of every branch are counted, a loop body once -- `layers` holds every option of the `f` layer (nested splines,
the correlated variant, four rotation modes), of which the default layer runs a small part.

The OCML listing: each float32 library routine of jf_math.h is compiled alone (one probe kernel per routine, same flags); its size is the
probe's count above an empty probe's.  The 32-bit literals that occur in one probe only are the routine's signature, and the number of
copies inlined in `layers` is the median count of the signature's literals there (0 if it has no literal of its own).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_budget as ib  # noqa: E402

SRC = os.path.join(ib.CSRC, "cond_manifold_kernels.hip")
KERNEL_RE = re.compile(r"^(_ZN2jf18cond_mchain_kernelIfNS_4FFamELi256ELb0E\w*):", re.M)
REGIONS = ("stage", "product", "act", "second", "hidden", "layers")
HIDDEN_VALUES = 32                                 # hidden values per lane and row tile: 128 units x 16 rows / 64 lanes
# float32 routines of jf::M<float> that expand to OCML code: name -> expression of the probe (a, b: the probe's inputs)
ROUTINES = {
    "sin": "jf::M<float>::sin(a)", "cos": "jf::M<float>::cos(a)", "acos": "jf::M<float>::acos(a)", "atan2": "jf::M<float>::atan2(a, b)",
    "log": "jf::M<float>::log(a)", "log1p": "jf::M<float>::log1p(a)", "exp": "jf::M<float>::exp(a)", "expm1": "jf::M<float>::expm1(a)",
    "tanh": "jf::M<float>::tanh(a)", "sqrt": "jf::M<float>::sqrt(a)", "erf": "jf::M<float>::erf(a)", "erfinv": "jf::M<float>::erfinv(a)",
    "div": "a / b",
}


def compile_asm(out_path, src=SRC, hipcc=ib.HIPCC):
    subprocess.check_call([hipcc] + ib.makefile_flags() + ["--cuda-device-only", "-S", "-I", ib.CSRC, src, "-o", out_path], cwd=ib.CSRC,
                          stderr=subprocess.DEVNULL)


def kernel_name(asm):
    m = KERNEL_RE.search(asm)
    if not m:
        raise SystemExit("no cond_mchain_kernel<float, FFam, 256, false> in the assembly")
    return m.group(1)


def ops_of(body):
    return [(i, l.split()[0]) for i, l in enumerate(body) if l.startswith("\t") and l.split() and not l.split()[0].startswith((".", ";"))]


def count(ops):
    c = {"valu": 0, "trans": 0, "mfma": 0, "nop": 0}
    for _, op in ops:
        k = ib.classify(op)
        if k:
            c[k] += 1
    c["vector"] = c["valu"] + c["trans"]
    c["cycles"] = sum(ib.WEIGHT[k] * c[k] for k in ib.WEIGHT)
    return c


def budget(body):
    ops = ops_of(body)
    f32 = [i for i, op in ops if op.startswith("v_mfma_f32_16x16x4")]
    f16 = [i for i, op in ops if op.startswith("v_mfma_f32_16x16x32_f16")]
    if not f32 or not f16 or f32[-1] > f16[0]:
        raise SystemExit("hidden layer not found: f32 MFMAs %s, f16 MFMAs %s" % (f32[:1] + f32[-1:], f16[:1] + f16[-1:]))
    cut = {"stage": (0, f32[0]), "product": (f32[0], f32[-1] + 1), "act": (f32[-1] + 1, f16[0]), "second": (f16[0], f16[-1] + 1),
           "hidden": (0, f16[-1] + 1), "layers": (f16[-1] + 1, len(body))}
    return {r: count([(i, op) for i, op in ops if lo <= i < hi]) for r, (lo, hi) in cut.items()}, cut["layers"]


def literals(lines):
    return re.findall(r"\b0x[0-9a-f]{8}\b", "\n".join(l for l in lines if l.startswith("\t")))


def ocml_listing(layer_lines, hipcc=ib.HIPCC):
    src = ['#include "jf_math.h"', 'extern "C" __global__ void probe_none(const float* x, float* o) { o[threadIdx.x] = x[threadIdx.x]; }']
    for name, expr in ROUTINES.items():
        src.append('extern "C" __global__ void probe_%s(const float* x, float* o) { const float a = x[threadIdx.x], b = x[threadIdx.x + 64]; '
                   'o[threadIdx.x] = %s; }' % (name, expr))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe.hip")
        open(path, "w").write("\n".join(src) + "\n")
        out = os.path.join(d, "probe.s")
        compile_asm(out, src=path, hipcc=hipcc)
        asm = open(out).read()
    text = {n: ib.kernel_text(asm, "probe_" + n) for n in list(ROUTINES) + ["none"]}
    base = count(ops_of(text["none"]))
    lits = {n: set(literals(text[n])) for n in ROUTINES}
    in_layers = {}
    for l in literals(layer_lines):
        in_layers[l] = in_layers.get(l, 0) + 1
    rows = []
    for n in ROUTINES:
        c = count(ops_of(text[n]))
        own = lits[n] - set().union(*(lits[o] for o in ROUTINES if o != n))
        copies = int(statistics.median([in_layers.get(l, 0) for l in own])) if own else 0
        rows.append({"routine": n, "vector": c["vector"] - base["vector"], "trans": c["trans"] - base["trans"],
                     "cycles": c["cycles"] - base["cycles"], "signature_literals": len(own), "copies_in_layers": copies})
    rows.sort(key=lambda r: -r["cycles"])
    return rows


def report(asm, ocml=True):
    name = kernel_name(asm)
    md = ib.metadata(asm, name)
    regs = md["vgpr"] + md["agpr"]
    alloc = -(-regs // ib.VGPR_GRANULE) * ib.VGPR_GRANULE
    md["waves_per_simd"] = min(ib.MAX_WAVES, ib.VGPR_POOL // max(alloc, 1))
    body = ib.kernel_text(asm, name)
    regions, (lo, hi) = budget(body)
    r = {"kernel": "cond_mchain_kernel<float, FFam, 256, false>", **md, "regions": regions}
    if ocml:
        r["ocml"] = ocml_listing(body[lo:hi])
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="read this assembly instead of compiling")
    ap.add_argument("--no-ocml", action="store_true", help="skip the listing of the OCML routines")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "cm.s")
            compile_asm(out)
            asm = open(out).read()
    r = report(asm, ocml=not a.no_ocml)
    if a.json:
        print(json.dumps(r, indent=1))
        return
    print("%s: %d VGPRs (+%d AGPRs), scratch %d B, spills v%d s%d, %d waves per SIMD by registers" %
          (r["kernel"], r["vgpr"], r["agpr"], r["scratch"], r["vgpr_spill"], r["sgpr_spill"], r["waves_per_simd"]))
    print("%-8s %7s %7s %7s %7s %9s" % ("region", "vector", "trans", "mfma", "s_nop", "cycles"))
    for k in REGIONS:
        v = r["regions"][k]
        print("%-8s %7d %7d %7d %7d %9d" % (k, v["vector"], v["trans"], v["mfma"], v["nop"], v["cycles"]))
    if "ocml" in r:
        print("\nlibrary routines (float32), stand-alone size and copies inlined in `layers`")
        print("%-8s %7s %7s %9s %7s" % ("routine", "vector", "trans", "cycles", "copies"))
        for o in r["ocml"]:
            print("%-8s %7d %7d %9d %7s" % (o["routine"], o["vector"], o["trans"], o["cycles"],
                                           o["copies_in_layers"] if o["signature_literals"] else "?"))


if __name__ == "__main__":
    sys.exit(main())
