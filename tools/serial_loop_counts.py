#!/usr/bin/env python3
"""Instruction counts of the solve's two serial loops, from the disassembly of the built object (a report, not a gate).

Phases R (riccati_mfma) and F (forward_smem) are one-lane chains on a wavefront that has its SIMD to itself: every issued
instruction of a step costs it a slot (tools/ubench_slot.hip), so the count per step is the figure to watch.  For one kernel
(default: cilqr_solve_share_kernel<2, false, false, false>, the one bench.py's config 2 runs) this finds the innermost loop
that holds the matrix instructions and the innermost loop that holds the forward records' s_load_dwordx16 — both run two steps
per trip — and counts their instructions by kind.

    python tools/serial_loop_counts.py [path/to/cilqr_solve.o] [kernel-name substring]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_smem_hazard import ROOT, disassemble, parse

KINDS = ["matrix", "fp64 vector", "other vector", "scalar", "LDS", "scalar memory", "vector memory", "s_nop", "wait"]
FP64 = ("v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_add_f64", "v_min_f64", "v_max_f64", "v_rcp_f64", "v_rsq_f64", "v_div_", "v_trunc_f64",
        "v_rndne_f64", "v_ldexp_f64", "v_frexp_", "v_cmp_", "v_cvt_f64", "v_cvt_i32_f64")


def kind(op):
    if op.startswith("v_mfma"):
        return "matrix"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "wait"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_dcache")):
        return "scalar memory"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vector memory"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith(FP64) and "f64" in op:
        return "fp64 vector"
    return "other vector"


def innermost_loop(code, holds):
    """The shortest backward-branch span [target, branch] that contains an instruction for which holds(op) is true."""
    index = {off: i for i, (off, _, _) in enumerate(code)}
    best = None
    for i, (off, ins, target) in enumerate(code):
        if not ins.startswith("s_cbranch") and not ins.startswith("s_branch"):
            continue
        if target is None or target not in index or target > off:
            continue
        body = code[index[target]:i + 1]
        if any(holds(b[1].split()[0]) for b in body) and (best is None or len(body) < len(best)):
            best = body
    return best


def report(name, body, steps_per_trip=2):
    counts = dict.fromkeys(KINDS, 0)
    for _, ins, _ in body:
        counts[kind(ins.split()[0])] += 1
    total = sum(counts.values())
    print("%s: %d instructions per trip of %d steps = %.1f per step" % (name, total, steps_per_trip, total / steps_per_trip))
    print("    " + " | ".join("%s %g" % (k, counts[k] / steps_per_trip) for k in KINDS if counts[k]))
    nop_states = sum(int(ins.split()[1], 0) + 1 for _, ins, _ in body if ins.split()[0] == "s_nop")
    if nop_states:
        print("    (wait states asked of the s_nop: %g per step)" % (nop_states / steps_per_trip))


def main():
    obj = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd", "build", "cilqr_solve.o")
    want = sys.argv[2] if len(sys.argv) > 2 else "cilqr_solve_share_kernelILi2ELb0ELb0ELb0E"
    kernels = {n: c for n, c in parse(disassemble(obj)).items() if want in n}
    if not kernels:
        raise SystemExit("no kernel matching %r in %s" % (want, obj))
    for name, code in kernels.items():
        print(name)
        r = innermost_loop(code, lambda op: op.startswith("v_mfma_f64"))
        f = innermost_loop(code, lambda op: op.startswith("s_load_dwordx16"))
        if r:
            report("  phase R loop (riccati_mfma)", r)
        if f:
            report("  phase F loop (forward_smem)", f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
