"""The range-specialised device functions of bayesssm_amd/csrc/fastmath.hip.h against the library functions they replace,
BIT FOR BIT: tests/harness/fastmath_bits.hip evaluates both forms on the same arguments in one kernel (built here with the
library's own flags) and returns the results as 64-bit patterns.  Per function: 2^22 random arguments over the stated
domain, plus the domain's edges."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesssm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "fastmath_bits.hip")
NRAND = 1 << 22
EXP, SQRT, SINCOSPI, U01 = range(4)


@pytest.fixture(scope="module")
def harness():
    out_dir = os.path.join(ROOT, "tests", "harness", "_build")
    os.makedirs(out_dir, exist_ok=True)
    lib = os.path.join(out_dir, "libfastmath_bits.so")
    deps = [SRC, os.path.join(CSRC, "rng.h"), os.path.join(CSRC, "fastmath.hip.h")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                               "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, "-o", lib, SRC])
    h = C.CDLL(lib)
    h.fastmath_bits.restype = C.c_int
    h.fastmath_bits.argtypes = [C.c_int, C.c_void_p, C.c_longlong] + [C.c_void_p] * 4

    def run(fn, patterns):
        a = np.ascontiguousarray(patterns, dtype=np.uint64)
        outs = [np.empty_like(a) for _ in range(4)]
        rc = h.fastmath_bits(fn, a.ctypes.data, a.size, *[o.ctypes.data for o in outs])
        assert rc == 0, "HIP error %d" % rc
        return outs
    return run


def _neighbours(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return np.concatenate([np.nextafter(xs, -np.inf), xs, np.nextafter(xs, np.inf)])


def _check(name, args, lib, fast):
    bad = np.flatnonzero(lib != fast)
    assert bad.size == 0, "%s: %d of %d differ; first at %r (bits %#018x): library %#018x, specialised %#018x" % (
        name, bad.size, args.size, args.view(np.float64)[bad[0]], int(args[bad[0]]), int(lib[bad[0]]), int(fast[bad[0]]))


def test_exp_nonpos(harness):
    rng = np.random.default_rng(101)
    # the weights' range (0 down to a few hundred), the whole range down to underflow and beyond, and log-uniform magnitudes
    rand = np.concatenate([-rng.uniform(0.0, 50.0, NRAND // 2), -rng.uniform(0.0, 800.0, NRAND // 4),
                           -np.exp(rng.uniform(np.log(1e-300), np.log(1e10), NRAND // 4))])
    edges = np.concatenate([
        [0.0, -0.0, -np.finfo(np.float64).tiny, -750.0, -1e8, -np.inf],
        _neighbours(-708.0 - 0.1 * np.arange(19)),                   # -708.0 ... -709.8: the last normal results and the first subnormal ones
        _neighbours(np.linspace(-745.1, -745.2, 101)),               # the last non-zero result (exp(-745.13...) = 2^-1075)
        _neighbours([-1075.0, -1074.0, -1022.0 * np.log(2.0), -1075.0 * np.log(2.0), -2147483648.0 * np.log(2.0), -1e300])])
    args = np.concatenate([rand, edges]).view(np.uint64)
    lib, fast, _, _ = harness(EXP, args)
    _check("exp", args, lib, fast)
    v = fast.view(np.float64)
    assert v[rand.size] == 1.0 and v[rand.size + 5] == 0.0                        # exp(0) and exp(-inf)
    assert ((v > 0) & (v < np.finfo(np.float64).tiny)).any()                      # the subnormal end was exercised


def test_sqrt_pos_normal(harness):
    rng = np.random.default_rng(102)
    rand = np.concatenate([np.exp2(rng.uniform(-53.0, np.log2(75.0), NRAND // 2)), rng.uniform(0.0, 75.0, NRAND // 2) + 2.0 ** -53])
    pow2 = np.exp2(np.arange(-53, 8, dtype=np.float64))
    below, above = np.nextafter(pow2, 0.0), np.nextafter(pow2, np.inf)
    edges = np.concatenate([[2.0 ** -53, 1.0, 4.0, 75.0, 0.0, -0.0], below[1:], pow2, above])   # (below 2^-53 is outside the generator's range but inside the domain)
    args = np.concatenate([rand, edges, below[:1]]).view(np.uint64)
    lib, fast, _, _ = harness(SQRT, args)
    _check("sqrt", args, lib, fast)


def test_sincospi_0_2(harness):
    rng = np.random.default_rng(103)
    k = rng.integers(0, 1 << 53, NRAND // 2, dtype=np.uint64)
    rand = np.concatenate([2.0 * ((k.astype(np.float64) + 0.5) * 2.0 ** -53),     # the generator's own arguments 2 u
                           rng.uniform(0.0, 2.0, NRAND // 4), np.exp2(rng.uniform(-60.0, 1.0, NRAND // 4))])
    # both neighbours of every quadrant boundary; those of 0 and 2 that lie outside [0, 2] reduce to the same remainder and
    # quadrant bits in both forms (fastmath.hip.h), so they are held to the library as well
    edges = _neighbours([0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0])
    args = np.concatenate([rand, edges]).view(np.uint64)
    lib_s, fast_s, lib_c, fast_c = harness(SINCOSPI, args)
    _check("sinpi", args, lib_s, fast_s)
    _check("cospi", args, lib_c, fast_c)


def test_u01_from_bits(harness):
    rng = np.random.default_rng(104)
    rand = rng.integers(0, 1 << 64, NRAND, dtype=np.uint64)
    # quotient b >> 11 odd and >= 2^52: the ones where + 0.5 is a tie that rounds
    ties = rng.integers(0, 1 << 64, 1 << 16, dtype=np.uint64) | np.uint64(1 << 63) | np.uint64(1 << 11)
    edges = np.array([0, (1 << 11) - 1, 1 << 63, (1 << 64) - 1, (1 << 64) - (1 << 11), (1 << 63) | (1 << 11), ((1 << 64) - 1) ^ (1 << 11)],
                     dtype=np.uint64)
    args = np.concatenate([rand, ties, edges])
    lib, fast, _, _ = harness(U01, args)
    _check("u01_from_bits", args, lib, fast)
    v = fast.view(np.float64)
    assert v.min() >= 2.0 ** -54 and v.max() <= 1.0
