"""Tau-leaping for the reaction networks (models.reaction_network(..., method="tau_leap", leaps=K)) without a GPU: the numpy
restatement of the definition (tests/rnet_leap_restated.py) -- its Poisson sampler against the closed-form moments and dpois, its
transition inside the restated filter core (conservation, the cap, the mean of a pure birth) --, the keyword refusals, the option
refusal behind the ABI, the new prototype and option against the header, and the packed block, which the keyword does not touch."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_leap_restated as LR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAMS = (0.3, 9.99, 10.0, 57.5, 1e4, 1e7)            # both branches, the threshold from both sides, large means
N_DRAWS = 1 << 16


def moment_bars(x, lam):
    """|mean - lam| and |variance - lam| in units of their closed-form standard errors sqrt(lam / n) and sqrt((lam + 2 lam^2) / n)"""
    n = x.size
    return abs(x.mean() - lam) / math.sqrt(lam / n), abs(x.var() - lam) / math.sqrt((lam + 2.0 * lam * lam) / n)


@pytest.mark.parametrize("k,lam", list(enumerate(LAMS)))
def test_restated_sampler_has_the_poisson_moments(oracle, k, lam):
    """2^16 draws per mean under fixed seeds: the sample mean within 5 sqrt(lam / n) of lam and the sample variance within
    5 sqrt((lam + 2 lam^2) / n) of lam (the standard errors in closed form; the bars are not tuned)"""
    counts = LR.new_counts()
    x = LR.sample(oracle, 1000 + k, 3, call=k, leap=5 * k, r=k % 8, lam=np.full(N_DRAWS, lam), counts=counts)
    assert np.all(x == np.floor(x)) and x.min() >= 0
    em, ev = moment_bars(x, lam)
    print("lam", lam, "mean", x.mean(), "var", x.var(), "errors in s.e.", em, ev, counts)
    assert em <= 5.0 and ev <= 5.0
    if lam < 10.0:
        assert counts["inv"] == N_DRAWS and counts["ptrs"] == 0
    else:
        assert counts["ptrs"] == N_DRAWS and counts["inv"] == 0 and counts["fallback"] == 0
        assert counts["squeeze"] > 0 and counts["full"] > 0 and counts["rejected"] > 0
        assert counts["squeeze"] + counts["full"] == N_DRAWS


def test_restated_inversion_matches_dpois(oracle):
    """lam = 3: the frequencies of k = 0 .. 12 within 5 sqrt(p (1 - p) / n) of dpois(k, 3)"""
    lam, n = 3.0, N_DRAWS
    x = LR.sample(oracle, 77, 1, call=2, leap=0, r=1, lam=np.full(n, lam))
    for k in range(13):
        p = math.exp(-lam + k * math.log(lam) - math.lgamma(k + 1.0))
        f = float(np.mean(x == k))
        assert abs(f - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n), (k, f, p)


def test_restated_sampler_edges(oracle):
    """not lam > 0 gives 0 without a draw; distinct (call, leap, r) and particles draw differently; the key stride is 8, not R"""
    c = LR.new_counts()
    x = LR.sample(oracle, 5, 0, 0, 0, 0, [0.0, -1.0, float("nan")], c)
    assert np.all(x == 0.0) and c["zero"] == 3
    lam = np.full(64, 40.0)
    a = LR.sample(oracle, 5, 0, 1, 2, 3, lam)
    assert len(set(a)) > 8
    for other in ((2, 2, 3), (1, 3, 3), (1, 2, 4)):
        assert not np.array_equal(a, LR.sample(oracle, 5, 0, *other, lam))
    # leap l, reaction r sits at l * 8 + r: (leap 1, r 0) is not (leap 0, r R) for any R < 8, but it is "(leap 0, r 8)"
    key, sw = [5, 0], LR.stream_word(0)
    assert LR.rpois(oracle, key, sw, 3, 1, 1, 0, 40.0) == LR.rpois(oracle, key, sw, 3, 1, 0, 8, 40.0)


def closed_sir(B, **kw):
    return B.models.reaction_network(("S", "I", "R"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma")],
                                     x0=(60, 12, 0), observe={"I": 0.5}, **kw)


CLOSED_SIR_PAR = dict(beta=0.02, gamma=2.5)          # K = 1: the removal's lam = 2.5 I exceeds I, so the cap acts at every leap with I > 0


def test_closed_sir_conserves_and_stays_nonnegative(oracle):
    """S + I + R is kept exactly and no component goes below 0 for every particle, at a rate where `counts` shows cap hits"""
    import bayesssm_amd as B
    N, T = 48, 4
    m = closed_sir(B, method="tau_leap", leaps=1)
    y = np.array([4.0, 6.0, 2.0, 0.0])
    counts = {}
    u = np.random.default_rng(2).random((T, N))
    ref = LR.pf_run_rn(oracle, m.pack(CLOSED_SIR_PAR), y, N, u, 1, seed=9, stream=2, counts=counts, resample_algorithm="SISAR",
                       resample_fn="stratified", return_particles=True)
    ph = ref["particles_history"].reshape(-1, 3, N)
    print({k: counts[k] for k in LR.KEYS})
    assert counts["cap"] > 0 and counts["ptrs"] > 0 and counts["inv"] > 0
    assert ph.shape[0] == T + 1 and np.all(ph == np.floor(ph))
    assert np.all(ph.sum(axis=1) == 72.0) and ph.min() >= 0.0
    assert (ph[-1, 2] > 0).any()


@pytest.mark.parametrize("K", [1, 16])
def test_pure_birth_has_the_exact_mean(oracle, K):
    """0 -> A at rate b (order 0): the propensity does not depend on x, so x(t) - x0 is Poisson(b t) for any K and the mean of N
    unweighted particles lies within 5 sqrt(b t / N) of x0 + b t.  K = 1 draws by PTRS (lam = 12.5), K = 16 by inversion."""
    import bayesssm_amd as B
    N, T, b, x0 = 192, 3, 12.5, 7.0
    m = B.models.reaction_network(("A",), [({}, {"A": 1}, b)], x0=(x0,), observe=np.zeros((1, 1)), method="tau_leap", leaps=K)
    counts = {}
    u = np.random.default_rng(4).random((T, N))
    ref = LR.pf_run_rn(oracle, m.pack(), np.zeros(T), N, u, K, seed=21, stream=K, counts=counts, resample_algorithm="SIS",
                       resample_fn="stratified", return_particles=True)
    assert ref["loglike"] == 0.0 and counts["cap"] == 0
    assert (counts["ptrs"], counts["inv"]) == ((T * N, 0) if K == 1 else (0, T * N * K))
    ph = ref["particles_history"].reshape(T + 1, N)
    for t in range(1, T + 1):
        err, bar = abs(ph[t].mean() - (x0 + b * t)), 5.0 * math.sqrt(b * t / N)
        print("t", t, "mean", ph[t].mean(), "error", err, "bar", bar)
        assert err <= bar


def test_keyword_refusals():
    import bayesssm_amd as B
    with pytest.raises(ValueError, match="method must be one of 'gillespie', 'tau_leap'"):
        closed_sir(B, method="euler")
    with pytest.raises(ValueError, match="leaps is the number of tau-leaps .* needs method='tau_leap'"):
        closed_sir(B, leaps=4)
    with pytest.raises(ValueError, match="leaps is the number of tau-leaps"):
        closed_sir(B, method="gillespie", leaps=4)
    with pytest.raises(ValueError, match="method='tau_leap' needs leaps"):
        closed_sir(B, method="tau_leap")
    with pytest.raises(ValueError, match="leaps must be an integer, got 4.0"):
        closed_sir(B, method="tau_leap", leaps=4.0)
    with pytest.raises(ValueError, match="leaps must be an integer, got '4'"):
        closed_sir(B, method="tau_leap", leaps="4")
    with pytest.raises(ValueError, match="not a bool"):
        closed_sir(B, method="tau_leap", leaps=True)
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match=r"leaps must lie in 1 \.\. 1024, got %d" % bad):
            closed_sir(B, method="tau_leap", leaps=bad)
    for ok in (1, 1024, np.int64(16)):
        m = closed_sir(B, method="tau_leap", leaps=ok)
        assert (m.method, m.leaps, m.rn_leaps) == ("tau_leap", int(ok), int(ok)) and type(m.leaps) is int
    m = closed_sir(B)
    assert (m.method, m.leaps, m.rn_leaps) == ("gillespie", None, 0)
    # what the family refuses stays refused, before any context exists
    m = closed_sir(B, method="tau_leap", leaps=4)
    y = np.array([3.0, 4.0])
    with pytest.raises(ValueError, match="RMPF"):
        m.rw_move_fn()
    with pytest.raises(ValueError, match="bootstrap filter"):
        B.auxiliary_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, [CLOSED_SIR_PAR] * 2)
    with pytest.raises(ValueError):
        B.bootstrap_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_fn="multinomial", **CLOSED_SIR_PAR)


def test_build_cannot_change_the_method():
    import bayesssm_amd as B
    for key in ("method", "leaps"):
        m = closed_sir(B, method="tau_leap", leaps=4, build=lambda beta, gamma, key=key: {key: 8}, param_names=("beta", "gamma"))
        with pytest.raises(TypeError, match="build may return"):
            m.pack(CLOSED_SIR_PAR)
        assert (m.method, m.leaps) == ("tau_leap", 4)


def test_pack_is_the_gillespie_block():
    """the descriptor's packed block does not know the method: byte for byte the block without the keyword, with every tail"""
    import bayesssm_amd as B
    M = np.linspace(0.5, 1.5, 12).reshape(6, 2)
    for kw in (dict(), dict(missing="skip"), dict(rate_schedule=M), dict(obs="negbin", size=3.5), dict(obs="negbin", size="s", rate_schedule=M)):
        par = dict(CLOSED_SIR_PAR, s=2.0)
        plain, leap, named = closed_sir(B, **kw), closed_sir(B, method="tau_leap", leaps=7, **kw), closed_sir(B, method="gillespie", **kw)
        assert plain.pack(par).tobytes() == leap.pack(par).tobytes() == named.pack(par).tobytes()
        assert plain.n_theta() == leap.n_theta() and plain.param_order == leap.param_order
    c = B.models.reaction_network(("S", "I", "C"), [({"S": 1, "I": 1}, {"I": 2, "C": 1}, "beta"), ({"I": 1}, {}, "gamma")], x0=(60, 12, 0),
                                  observe={"C": 0.5}, counters=("C",), method="tau_leap", leaps=2)
    assert np.array_equal(c.pack(CLOSED_SIR_PAR)[-3:], [0.0, 0.0, 1.0])


def test_option_and_prototype_match_the_header():
    from bayesssm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bayesssm_amd.h")).read()
    assert re.search(r"#define\s+BSSM_OPT_RN_LEAPS\s+14\b", header)
    assert _lib.Context.OPTIONS["rn_leaps"] == 14 == max(_lib.Context.OPTIONS.values())
    assert re.search(r"\bint\s+bssm_dump_rpois\s*\(\s*bssm_ctx\s*\*\s*ctx\s*,\s*unsigned long long seed\s*,\s*unsigned long long stream\s*,\s*int call\s*,"
                     r"\s*int leap\s*,\s*int r\s*,\s*long long n\s*,\s*const double\s*\*\s*lam[^,]*,\s*double\s*\*\s*out[^)]*\)\s*;", header)
    assert "bssm_dump_rpois" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.bssm_dump_rpois.argtypes == [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    # the sampler is stated where the option is
    for piece in ("0.931 + 2.53 * slam", "-0.059 + 0.02483 * b", "1.1239 + 1.1328 / (b - 3.4)", "0.9277 - 3.6224 / (b - 2.0)", "k < 128.0",
                  "(l * 8 + r) << 6 | a) << 8"):
        assert piece in header, piece


def test_option_refusals_behind_the_abi():
    """bssm_ctx_set_option refuses a number of leaps outside 0 .. 1024 by the value alone (no context, no device: the check of the
    value comes first); a value inside reaches the check of the context; bssm_dump_rpois refuses a NULL context"""
    from bayesssm_amd import _lib
    lib = _lib.load()
    for bad in (-1, 1025, 1 << 20):
        assert lib.bssm_ctx_set_option(None, 14, bad) == _lib.ERR_ARG
        assert "rn_leaps takes 0" in lib.bssm_last_error().decode()
    for ok in (0, 1, 1024):
        assert lib.bssm_ctx_set_option(None, 14, ok) == _lib.ERR_ARG
        assert lib.bssm_last_error().decode() == "ctx is NULL"
    lam, out = np.ones(4), np.zeros(4)
    assert lib.bssm_dump_rpois(None, 1, 0, 0, 0, 0, 4, lam.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == _lib.ERR_ARG
    assert "bssm_dump_rpois" in lib.bssm_last_error().decode()


def test_option_scope_restores_the_previous_value():
    """Context.rn_leaps without a device: a stand-in records what set_option is given -- K inside, the previous value afterwards,
    also on an exception, and no call at all when the value is already there"""
    from bayesssm_amd import _lib

    class Stub(_lib.Context):
        def __init__(self):
            self._h, self._set_options, self.calls = None, {}, []

        def set_option(self, name, value):
            self.calls.append((name, int(value)))
            self._set_options[name] = int(value)

    s = Stub()
    with s.rn_leaps(0):
        pass
    assert s.calls == []
    with s.rn_leaps(16):
        assert s._set_options["rn_leaps"] == 16
    assert s.calls == [("rn_leaps", 16), ("rn_leaps", 0)]
    s.calls.clear()
    s.set_option("rn_leaps", 4)                        # left on the context by hand
    with pytest.raises(RuntimeError):
        with s.rn_leaps(64):
            raise RuntimeError("inside")
    assert s._set_options["rn_leaps"] == 4 and s.calls[-2:] == [("rn_leaps", 64), ("rn_leaps", 4)]
    with s.rn_leaps(0):                                # a Gillespie descriptor's call puts a hand-set value at 0 for its length
        assert s._set_options["rn_leaps"] == 0
    assert s._set_options["rn_leaps"] == 4
