"""CPU-side checks: the C-ABI library loads and exports every symbol include/bayesssm_amd.h declares
(no compute without a GPU), the host mirror validates like the reference, and the product never
touches oracle/."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "bayesssm_amd", "csrc"), "-s"])
    from bayesssm_amd import _lib
    return _lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "bayesssm_amd.h")).read()
    declared = set(re.findall(r"\b(bssm_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = built.load()
    for sym in sorted(declared):
        assert hasattr(lib, sym), sym
    assert declared == set(built.EXPORTED_SYMBOLS)


def test_header_options_match_python(built):
    """every per-context option the header defines is reachable by name from Context.set_option, with the header's number"""
    hdr = open(os.path.join(ROOT, "include", "bayesssm_amd.h")).read()
    declared = {name.lower(): int(v) for name, v in re.findall(r"#define BSSM_OPT_([A-Z_]+)\s+(\d+)", hdr)}
    assert {"force_fallback", "fused_tag"} <= set(declared)
    assert declared == {k: v for k, v in built.Context.OPTIONS.items() if k in declared}
    assert len(set(declared.values())) == len(declared)


def test_no_cpu_path(built):
    lib = built.load()
    if lib.bssm_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(built.BssmError, match="no HIP device"):
        built.Context()
    import bayesssm_amd as b
    with pytest.raises(built.BssmError):
        b.resample_systematic_cpp(3, [1, 1, 1], U=0.5)


def test_product_does_not_import_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "bayesssm_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("CPU oracle", "").replace("the oracle's", "").replace("(values match the oracle", ""), \
                    os.path.join(dirpath, f)


def test_status_strings(built):
    lib = built.load()
    assert lib.bssm_status_string(1).decode() == "Weights must be non-negative"
    assert lib.bssm_status_string(2).decode() == "Sum of weights must be greater than 0"
    assert lib.bssm_status_string(3).decode() == "Number of particles must match the length of weights"


def test_host_validation():
    import bayesssm_amd as b
    m = b.models.linear_gaussian()
    with pytest.raises(ValueError, match="should be one of"):
        b.bootstrap_filter([0.0], 10, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_fn="bogus",
                           phi=1, sigma_x=1, sigma_y=1)
    with pytest.raises(ValueError, match="num_particles"):
        b.bootstrap_filter([0.0], 0, m.init_fn, m.transition_fn, m.log_likelihood_fn, phi=1, sigma_x=1, sigma_y=1)
    with pytest.raises(TypeError, match='argument "phi" is missing'):
        b.bootstrap_filter([0.0], 10, m.init_fn, m.transition_fn, m.log_likelihood_fn, sigma_x=1, sigma_y=1)
    with pytest.raises(TypeError, match="built-in model descriptor"):
        b.bootstrap_filter([0.0], 10, lambda n: 0, m.transition_fn, m.log_likelihood_fn, phi=1, sigma_x=1, sigma_y=1)
    with pytest.raises(ValueError, match="missing values"):
        b.bootstrap_filter([np.nan], 10, m.init_fn, m.transition_fn, m.log_likelihood_fn, phi=1, sigma_x=1, sigma_y=1)
    tc = b.default_tune_control()
    # tests/testthat/test-pmmh.R:5-25
    assert tc == {"pilot_proposal_sd": 0.5, "pilot_n": 100, "pilot_m": 2000, "pilot_target_var": 1,
                  "pilot_burn_in": 500, "pilot_reps": 100, "pilot_resample_algorithm": "SISAR",
                  "pilot_resample_fn": "stratified"}
    with pytest.raises(ValueError):
        b.default_tune_control(pilot_n=0)


def test_diagnostics_match_oracle(oracle):
    import bayesssm_amd as b
    rng = np.random.default_rng(0)
    x = np.zeros((400, 3))
    for c in range(3):
        for i in range(1, 400):
            x[i, c] = 0.7 * x[i - 1, c] + rng.standard_normal()
    assert b.ess(x) == pytest.approx(oracle.mcmc_ess(x), rel=1e-9)
    iid = rng.standard_normal((1000, 4))
    assert b.rhat(iid) == 1.0 or abs(b.rhat(iid) - 1) < 0.02
    assert 2500 < b.ess(iid) < 6000
    with pytest.raises(ValueError, match="at least 2"):
        b.ess(np.zeros((5, 1)))


def test_rng_header_on_host(oracle):
    """csrc/rng.h compiled for the host: Philox4x32-10 known answers (Random123 kat_vectors) and the
    AS241 quantile against scipy."""
    import ctypes as C
    from scipy import stats
    src = os.path.join(ROOT, "tests", "harness", "rng_harness.cpp")
    so = os.path.join(ROOT, "tests", "harness", "_build", "librng_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    out = (C.c_uint32 * 4)()
    kats = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kats:
        lib.h_philox(*[C.c_uint32(v) for v in ctr], *[C.c_uint32(v) for v in key], out)
        assert tuple(out) == want
    lib.h_qnorm.restype = C.c_double
    lib.h_qnorm.argtypes = [C.c_double]
    ps = np.concatenate([np.linspace(1e-15, 1 - 1e-15, 2001), 10.0 ** -np.arange(2, 16), [0.5, 0.075, 0.925]])
    got = np.array([lib.h_qnorm(float(p)) for p in ps])
    np.testing.assert_allclose(got, stats.norm.ppf(ps), rtol=2e-14, atol=1e-15)


def test_pilot_chain_logic():
    """.run_pilot_chain / .pilot_run (R/pmmh_tuning.R:29-64,111-317) with a synthetic filter: target_n bounds
    (tests/testthat/test-pmmh_tuning.R:48,102) and posterior mean near the optimum (:573-575)."""
    from bayesssm_amd.pmmh import run_pilot_chain, pilot_run, prior_normal, prior_exponential
    rng = np.random.default_rng(0)

    def pf(theta, n, tag):
        return float(-25 * np.sum((np.asarray(theta) - np.array([0.5, 1.0])) ** 2) + rng.standard_normal() * 0.3)

    r = run_pilot_chain(pf, 400, 100, 50, [prior_normal(0, 1), prior_exponential(1)], 0.5, ["identity", "log"],
                        [0.2, 0.7], np.random.default_rng(1), message=lambda *_: None)
    assert 50 <= r["target_n"] <= 1000
    assert abs(r["pilot_theta_mean"][0] - 0.5) < 0.2 and abs(r["pilot_theta_mean"][1] - 1.0) < 0.3
    assert r["pilot_theta_cov"].shape == (2, 2) and r["pilot_theta_chain"].shape == (400, 2)
    lo = pilot_run(lambda n, rep: 0.0 + 1e-3 * rep, 100, 10)
    hi = pilot_run(lambda n, rep: 10.0 * rep, 100, 10)
    assert lo["target_n"] == 50 and hi["target_n"] == 1000                     # clamp :55-57
    with pytest.raises(ValueError, match="Initial parameter values are invalid"):
        run_pilot_chain(pf, 10, 100, 5, [prior_normal(0, 1), prior_exponential(1)], 0.5, ["identity", "log"],
                        [0.2, -1.0], np.random.default_rng(1), message=lambda *_: None)


def test_r_compatible_rng():
    """The host generator behind set_seed() is R's Mersenne-Twister with R's seeding and inversion rnorm (bayesssm_amd/rrng.py).
    Pinned by R's own, widely published known answers (set.seed(s); runif(3) / rnorm(3)); with them the resampling shims
    consume, after set_seed(s), the uniforms the reference's C++ draws after set.seed(s) (src/resampling.cpp:28,55)."""
    from bayesssm_amd.rrng import RRandom
    kat_unif = {1: (0.2655087, 0.3721239, 0.5728534), 42: (0.9148060, 0.9370754, 0.2861395), 123: (0.2875775, 0.7883051, 0.4089769)}
    kat_norm = {1: (-0.6264538, 0.1836433, -0.8356286), 42: (1.37095845, -0.56469817, 0.36312841),
                123: (-0.56047565, -0.23017749, 1.55870831)}
    for seed, want in kat_unif.items():
        np.testing.assert_allclose(RRandom(seed).runif(3), want, rtol=0, atol=5e-8)
    for seed, want in kat_norm.items():
        np.testing.assert_allclose(RRandom(seed).rnorm(3), want, rtol=0, atol=5e-8)
    # block boundaries of the vectorised generator: one draw at a time == in bulk, across several 624-word refills
    a, g = RRandom(1405).runif(2000), RRandom(1405)
    assert (a == np.array([g.unif_rand() for _ in range(2000)])).all() and a.min() > 0 and a.max() < 1
    # what set.seed(1); resample_systematic_cpp(5, c(.1,.5,.1,.15,.15)) returns in R: U = 0.2655087,
    # u_i = (i + U)/5 = .053 .253 .453 .653 .853 against cum = .1 .6 .7 .85 1   (src/resampling.cpp:55-63)
    from oracle import oracle as orc
    assert orc.resample_systematic(5, [0.1, 0.5, 0.1, 0.15, 0.15], RRandom(1).unif_rand()).tolist() == [1, 2, 2, 3, 5]


def test_readme_series_regression():
    """The README's data set regenerated with the R-compatible generator (README.md:97-114: set.seed(1405) and its rnorm calls, in
    order).  Regression lock on this build's values; they follow from the generator pinned above, not from a run of R."""
    from bayesssm_amd.rrng import RRandom, readme_series, r_seeded_draws
    x, y = readme_series()
    assert x.shape == (21,) and y.shape == (20,)
    np.testing.assert_allclose(x[:3], [0.2725, 0.8444, 2.2314], atol=5e-4)
    np.testing.assert_allclose(y[:3], [0.4135, 2.5377, 2.2431], atol=5e-4)
    # 41 normals consumed = 82 uniforms: the stream position after the data simulation
    g = RRandom(1405); g.runif(82)
    h = RRandom(1405); [h.norm_rand() for _ in range(41)]
    assert g.unif_rand() == h.unif_rand()
    # draw bookkeeping of the seeded filter mode: sizes follow the resample decisions
    d = r_seeded_draws(7, 5, 10, "stratified", [True, False, True, True, False])
    assert d["z_init"].shape == (10,) and d["z_trans"].shape == (5, 10) and d["u_res"].shape == (5, 10)
    assert (d["u_res"][3:] == 0).all() and (d["u_res"][:3] > 0).all()
    d1 = r_seeded_draws(7, 5, 10, "systematic", [True] * 5, obs_times=[1, 3, 3, 4, 6])
    assert d1["z_trans"].shape == (6, 10) and d1["u_res"].shape == (5,)


def test_r_glue_file_binds_declared_symbols():
    """r/bayesssm_amd_glue.c (the `.Call` glue of INTEGRATION.md; not compilable here -- no R headers): every bssm_*
    function it calls is declared in include/bayesssm_amd.h, the three original entry points keep their names and arity 2
    (src/RcppExports.cpp:50-55), and <string.h> is there for its memset."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    glue = open(os.path.join(root, "r", "bayesssm_amd_glue.c")).read()
    header = open(os.path.join(root, "include", "bayesssm_amd.h")).read()
    assert "#include <string.h>" in glue
    for fn in set(re.findall(r"\b(bssm_[a-z_]+)\s*\(", glue)):
        assert re.search(r"\b%s\s*\(" % fn, header), fn
    for name in ("multinomial", "stratified", "systematic"):
        assert re.search(r'\{"_bayesSSM_resample_%s_cpp",\s+\(DL_FUNC\)&_bayesSSM_resample_%s_cpp, 2\}' % (name, name), glue)
    assert "R_registerRoutines(dll, NULL, CallEntries, NULL, NULL)" in glue and "R_useDynamicSymbols(dll, FALSE)" in glue


def test_r_glue_compiles_against_api_stub():
    """Compile hygiene only (NOT parity evidence): `gcc -fsyntax-only` type-checks r/bayesssm_amd_glue.c against a
    declarations-only stand-in for the R API names it uses (tests/harness/r_api_stub/) and the real include/bayesssm_amd.h.
    Also pins the order the reference has in all three entry points: validation before any draw
    (src/resampling.cpp:6-8,17-23,44-50 precede :11,:28,:55)."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types",
                        "-Werror=int-conversion", "-fsyntax-only", "-I" + os.path.join(root, "tests", "harness", "r_api_stub"),
                        "-I" + os.path.join(root, "include"), os.path.join(root, "r", "bayesssm_amd_glue.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    glue = open(os.path.join(root, "r", "bayesssm_amd_glue.c")).read()
    for name in ("systematic", "stratified", "multinomial"):
        body = re.search(r"SEXP _bayesSSM_resample_%s_cpp\(.*?\n}\n" % name, glue, re.S).group(0)
        assert 0 < body.index("validate_weights(w)") < body.index("draw_uniforms("), name
