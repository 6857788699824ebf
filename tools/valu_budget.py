"""Dev tool: static vector-instruction budget of the device functions on the filter kernels' issue-bound paths (no GPU needed).

Cross-compiles one small translation unit for gfx950 with the flags of bayesssm_amd/csrc/Makefile, in which every function
of interest sits in a `noinline` device function of its own (all called from one kernel), and counts the vector-ALU
instructions (mnemonics starting `v_`) of each in the compiler's assembly.  Every body must be straight-line code (selects, no
branches: count() refuses a body with a branch in it), so the count IS the count on the path the workload takes.  For each
library function the table has the library form (`lib_*`: the call the kernels made before bayesssm_amd/csrc/fastmath.hip.h)
and, where fastmath.hip.h has one, the range-specialised form (`fast_*`).

    python tools/valu_budget.py [--csrc DIR] [--json]

--csrc: the kernel source directory to read rng.h / kernels.hip.h (and fastmath.hip.h, if it is there) from -- e.g. an
export of another commit's bayesssm_amd/csrc.  profiles/r10_a_valu_budget*.txt are this tool's output."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function"]

# (library form, specialised form or None)
PAIRS = [("lib_exp", "fast_exp_nonpos"), ("lib_sqrt", "fast_sqrt_pos_normal"), ("lib_sincospi", "fast_sincospi_0_2"),
         ("lib_u01_from_bits", "fast_u01_from_bits"), ("r_dnorm_log", None), ("philox4x32_10", None),
         ("log_unit_interval", None), ("normal_pair", None)]

TU = r"""
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kernels.hip.h"
using namespace bssm;
#define NI extern "C" __device__ __attribute__((noinline))
NI double vb_lib_exp(double x) { return exp(x); }
NI double vb_lib_sqrt(double x) { return sqrt(x); }
NI double2 vb_lib_sincospi(double x) { double2 r; sincospi(x, &r.x, &r.y); return r; }
NI double vb_lib_u01_from_bits(uint32_t lo, uint32_t hi) { const uint64_t b = ((uint64_t)hi << 32) | lo; return ((double)(b >> 11) + 0.5) * 0x1.0p-53; }
NI double vb_r_dnorm_log(double x, double mu, double sd, double lsd) { return r_dnorm_log(x, mu, sd, lsd); }
NI u32x4 vb_philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) { return philox4x32_10(c, k0, k1); }
NI double vb_log_unit_interval(double x) { return log_unit_interval(x); }
NI double2 vb_normal_pair(PhiloxKey key, uint32_t pair) { double2 r; normal_pair(key, DRAW_TRANS, 7, 0, pair, r.x, r.y); return r; }
#if __has_include("fastmath.hip.h")
NI double vb_fast_exp_nonpos(double x) { return exp_nonpos(x); }
NI double vb_fast_sqrt_pos_normal(double x) { return sqrt_pos_normal(x); }
NI double2 vb_fast_sincospi_0_2(double x) { double2 r; sincospi_0_2(x, &r.x, &r.y); return r; }
NI double vb_fast_u01_from_bits(uint32_t lo, uint32_t hi) { return u01_from_bits_dev(lo, hi); }
#define FAST 1
#else
#define FAST 0
#endif
extern "C" __global__ void vb_kernel(double* o, const double* in, const uint32_t* u)
{
    const int i = threadIdx.x;
    PhiloxKey key; key.k0 = u[0]; key.k1 = u[1]; key.stream = u[2];
    u32x4 c; c.x = u[i]; c.y = u[i + 1]; c.z = u[i + 2]; c.w = u[i + 3];
    const u32x4 r = vb_philox4x32_10(c, key.k0, key.k1);
    const double2 a = vb_lib_sincospi(in[i + 1]), n = vb_normal_pair(key, u[i + 4]);
    double acc = vb_lib_exp(in[i]) + vb_lib_sqrt(in[i + 2]) + a.x + a.y + n.x + n.y + vb_lib_u01_from_bits(r.x, r.y) + (double)(r.z ^ r.w)
                 + vb_r_dnorm_log(in[i], in[i + 1], in[i + 2], in[i + 3]) + vb_log_unit_interval(in[i + 4]);
#if FAST
    const double2 b = vb_fast_sincospi_0_2(in[i + 1]);
    acc += vb_fast_exp_nonpos(in[i]) + vb_fast_sqrt_pos_normal(in[i + 2]) + b.x + b.y + vb_fast_u01_from_bits(r.x, r.y);
#endif
    o[i] = acc;
}
"""

INT_MUL = re.compile(r"^v_(mul_lo_u32|mul_hi_u32|mul_hi_i32|mul_lo_i32|mad_u64_u32|mad_i64_i32|mul_u32_u24|mul_i32_i24|mul_hi_u32_u24|mad_u32_u24)")
F64_TRANS = re.compile(r"^v_(rcp|rsq|sqrt|exp|log|sin|cos)_f64")


def disassemble(csrc):
    """The compiler's gfx950 assembly of the translation unit, built against the sources in `csrc`."""
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "valu_budget.hip"), os.path.join(tmp, "valu_budget.s")
        with open(src, "w") as f:
            f.write(TU)
        cmd = [HIPCC] + FLAGS + ["-I", csrc, "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S", "-o", out, src]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        if done.returncode != 0:
            raise RuntimeError("%s\nexit status %d:\n%s" % (" ".join(cmd), done.returncode, done.stdout))
        with open(out) as f:
            return f.read()


def count(asm):
    """{function: {"valu", "valu_no_mov", "int_mul", "f64_trans"}} of every vb_* function in the assembly text."""
    res, cur, name = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^vb_(\w+):", line)
        if m:
            name = m.group(1)
            cur = res.setdefault(name, {"valu": 0, "valu_no_mov": 0, "int_mul": 0, "f64_trans": 0})
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        op = line.strip().split(" ")[0] if line.startswith("\t") else ""
        if cur is not None and (op.startswith("s_cbranch") or op == "s_branch"):
            raise RuntimeError("vb_%s is not straight-line code (%s): its instruction count is not the count on the path taken" % (name, op))
        if cur is None or not op.startswith("v_"):
            continue
        cur["valu"] += 1
        cur["valu_no_mov"] += 0 if op.startswith("v_mov") else 1
        cur["int_mul"] += 1 if INT_MUL.match(op) else 0
        cur["f64_trans"] += 1 if F64_TRANS.match(op) else 0
    res.pop("kernel", None)
    return res


def budget(csrc=None):
    return count(disassemble(csrc or os.path.join(ROOT, "bayesssm_amd", "csrc")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "bayesssm_amd", "csrc"))
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    res = budget(args.csrc)
    if args.json:
        print(json.dumps(res, indent=1, sort_keys=True))
        return
    print("vector-ALU instructions per call (gfx950, %s)" % " ".join(FLAGS[1:4]))
    print("%-24s %6s %10s %8s %10s" % ("function", "v_*", "no v_mov", "int mul", "f64 trans"))
    for lib, fast in PAIRS:
        for name in (lib, fast):
            if name and name in res:
                r = res[name]
                print("%-24s %6d %10d %8d %10d" % (name, r["valu"], r["valu_no_mov"], r["int_mul"], r["f64_trans"]))
    print("(int mul: 32-bit integer multiplies, v_mad_u64_u32 included; f64 trans: v_rcp_f64 / v_rsq_f64 / v_sqrt_f64.\n"
          " normal_pair = philox4x32_10 + 2 u01_from_bits + log_unit_interval + sqrt + sincospi, as the kernels inline it.)")


if __name__ == "__main__":
    sys.exit(main())
