"""Euler-multinomial leaps for the reaction networks (models.reaction_network(..., method="euler_multinomial", leaps=K)) without a GPU:
the numpy restatement of the definition (tests/rnet_em_restated.py) -- its binomial sampler against the exact pmf, its transition's
properties (conservation, no negative count, the symmetric split of competing exits, the exact mean of a linear death process) --, the
classification and the keyword refusals, the option refusal behind the ABI, the new prototype and option against the header, and the
scope of the context option rn_method on a stand-in context."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_em_restated as ER  # noqa: E402
import rnet_leap_restated as LR  # noqa: E402
import rnet_restated as RN  # noqa: E402
from test_rnet_leap_cpu import closed_sir  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, q): both sides of n qq = 10 (at qq = q and at qq = 1 - q), both sides of q = 0.5, q near 0 and near 1, n = 1, n up to 10^6
BINOMS = ((1.0, 0.3), (1.0, 0.7), (7.0, 1e-9), (20.0, 0.4), (19.0, 0.5), (21.0, 0.5), (25.0, 0.39), (25.0, 0.41), (40.0, 0.75), (50.0, 0.98),
          (1000.0, 0.0099), (1000.0, 0.0101), (1000.0, 0.9899), (1000.0, 0.9901), (1e4, 0.5), (1e4, 0.5000001), (1e6, 1e-6), (1e6, 0.3),
          (1e6, 0.999995))
N_DRAWS = 1 << 16


def binom_moment_bars(x, n, q):
    """|mean - n q| and |variance - n q (1 - q)| in units of their closed-form standard errors: sqrt(s2 / N) and
    sqrt((mu4 - s2^2 (N - 3) / (N - 1)) / N) with s2 = n q (1 - q) and the fourth central moment mu4 = s2 (1 + 3 (n - 2) q (1 - q))"""
    N = x.size
    s2 = n * q * (1.0 - q)
    mu4 = s2 * (1.0 + 3.0 * (n - 2.0) * q * (1.0 - q))
    return abs(x.mean() - n * q) / math.sqrt(s2 / N), abs(x.var() - s2) / math.sqrt((mu4 - s2 * s2 * (N - 3.0) / (N - 1.0)) / N)


def binom_logpmf(k, n, q):
    return math.lgamma(n + 1.0) - math.lgamma(k + 1.0) - math.lgamma(n - k + 1.0) + k * math.log(q) + (n - k) * math.log1p(-q)


def chi_square(x, n, q):
    """(statistic, degrees of freedom) of the counts of x against the exact pmf over k = 0 .. n, neighbouring cells merged from the left
    until each expects at least 5 draws (the last cell takes the rest)"""
    N = x.size
    cells, obs, e, o = [], np.bincount(x.astype(int), minlength=int(n) + 1), 0.0, 0
    for k in range(int(n) + 1):
        e, o = e + N * math.exp(binom_logpmf(float(k), n, q)), o + int(obs[k])
        if e >= 5.0:
            cells.append((e, o)); e, o = 0.0, 0
    if cells:
        cells[-1] = (cells[-1][0] + e, cells[-1][1] + o)
    return sum((o - e) ** 2 / e for e, o in cells), len(cells) - 1


def test_restated_philox_is_the_oracles(oracle):
    """the vectorised Philox4x32-10 of the restatement against the oracle's C restatement, word for word"""
    j = np.array([0, 1, 2, 77, 2560, 0xFFFFFFFF])
    for call, word, sw, key in ((0, 2, 0, [0, 0]), (3, 2 | (((5 * 8 + 7) << 6 | 63) << 8), 0x9E3779B9, [123, 0xDEADBEEF]), (1 << 20, 0xFFFFFF02, 5, [0xFFFFFFFF, 1])):
        w = ER.philox4x32_10(j, call, word, sw, key)
        for i, jj in enumerate(j):
            assert [int(w[k][i]) for k in range(4)] == [int(v) for v in oracle.philox4x32_10([int(jj), call, word, sw], key)]


@pytest.mark.parametrize("i,n,q", [(i, n, q) for i, (n, q) in enumerate(BINOMS)])
def test_restated_sampler_against_the_exact_pmf(oracle, i, n, q):
    """2^16 draws per (n, q) under fixed seeds: every draw integral and in [0, n]; the sample mean within 5 standard errors of n q and the
    sample variance within 5 of n q (1 - q) (closed forms, binom_moment_bars; the bar of test_rnet_leap_cpu.py's rpois test); for n <= 1000
    a chi-square of the counts against the pmf from math.lgamma, at most df + 5 sqrt(2 df) (mean + 5 standard deviations of a chi-square
    with df degrees of freedom; the bars are not tuned).  The branch counts say which path the pair exercises."""
    counts = ER.new_counts()
    x = ER.sample(oracle, 2000 + i, 3, call=i, leap=7 * i, r=i % 8, n=np.full(N_DRAWS, n), q=q, counts=counts)
    assert np.all(x == np.floor(x)) and x.min() >= 0.0 and x.max() <= n
    em, ev = binom_moment_bars(x, n, q)
    print("n", n, "q", q, "mean", x.mean(), "var", x.var(), "errors in s.e.", em, ev, counts)
    assert em <= 5.0 and ev <= 5.0
    if n <= 1000.0:
        stat, df = chi_square(x, n, q)
        print("chi-square", stat, "df", df, "bar", df + 5.0 * math.sqrt(2.0 * df))
        assert stat <= df + 5.0 * math.sqrt(2.0 * df)
    qq = 1.0 - q if q > 0.5 else q
    assert counts["flip"] == (N_DRAWS if q > 0.5 else 0) and counts["zero"] == counts["all"] == counts["fallback"] == 0
    if n * qq < 10.0:
        assert counts["inv"] == N_DRAWS and counts["btrs"] == 0
    else:
        assert counts["btrs"] == N_DRAWS and counts["inv"] == 0
        assert counts["squeeze"] > 0 and counts["full"] > 0 and counts["rejected"] > 0 and counts["squeeze"] + counts["full"] == N_DRAWS


def test_restated_sampler_edges(oracle):
    """not n > 0 and not q > 0 give 0 and q >= 1 gives n without a draw; distinct (call, leap, r) and particles draw differently; the key
    stride is 8, not R; the keys are rpois's: an inversion draw walks on the same u1"""
    c = ER.new_counts()
    x = ER.sample(oracle, 5, 0, 0, 0, 0, [0.0, -1.0, float("nan"), 9.0, 9.0, 9.0, 9.0, 9.0], [0.5, 0.5, 0.5, 0.0, -0.1, float("nan"), 1.0, 1.5], c)
    assert np.array_equal(x, [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 9.0, 9.0]) and c["zero"] == 6 and c["all"] == 2 and c["inv"] == c["btrs"] == 0
    n = np.full(64, 90.0)
    a = ER.sample(oracle, 5, 0, 1, 2, 3, n, 0.4)
    assert len(set(a)) > 8
    for other in ((2, 2, 3), (1, 3, 3), (1, 2, 4)):
        assert not np.array_equal(a, ER.sample(oracle, 5, 0, *other, n, 0.4))
    assert np.array_equal(ER.sample(oracle, 5, 0, 1, 1, 0, n, 0.4), ER.sample(oracle, 5, 0, 1, 0, 8, n, 0.4))
    # Binomial(n, lam / n) at n = 10^9 is Poisson(lam) to 1e-9: the two inversions, on the same u1, give the same count almost always
    lam = 3.0
    b = ER.sample(oracle, 9, 1, 2, 3, 4, np.full(4096, 1e9), lam / 1e9)
    p = LR.sample(oracle, 9, 1, 2, 3, 4, np.full(4096, lam))
    assert int(np.sum(b != p)) <= 2


# --- the transition -----------------------------------------------------------------------------------------------------------------------
def transitions(oracle, m, par, K, N, steps, seed=11, stream=2, counts=None, x0=None):
    """`steps` restated transitions (calls 0 .. steps-1) of N particles from x0: [steps + 1][d][N]"""
    q = RN.unpack(m.pack(par)[:3 + m.dim + 3 * m.R + m.R * m.dim + m.p * m.dim])
    trans, _, _ = ER.make(K, oracle, seed, stream, counts)
    x = np.repeat(np.asarray(q["x0"] if x0 is None else x0, dtype=np.float64)[:, None], N, axis=1)
    out = [x]
    for call in range(steps):
        x = trans(q, x, np.full((m.dim, N), float(call)))
        out.append(x)
    return np.array(out)


def test_closed_sir_conserves_and_stays_nonnegative(oracle):
    """S + I + R is kept exactly and no component is negative for every particle inside the restated filter (test_rnet_leap_cpu's closed
    SIR and rates, K = 1 and 4), and at K = 1 with hazards so large that pe rounds to 1.0 (beta I = 600, gamma = 800: everybody leaves)"""
    import bayesssm_amd as B
    N, T = 48, 4
    y = np.array([4.0, 6.0, 2.0, 0.0])
    u = np.random.default_rng(2).random((T, N))
    for K in (1, 4):
        m = closed_sir(B, method="euler_multinomial", leaps=K)
        counts = {}
        ref = ER.pf_run_rn(oracle, m.pack(dict(beta=0.02, gamma=2.5)), y, N, u, K, seed=9, stream=2, counts=counts, resample_algorithm="SISAR",
                           resample_fn="stratified", return_particles=True)
        ph = ref["particles_history"].reshape(-1, 3, N)
        print(K, {k: counts[k] for k in ER.KEYS})
        assert ph.shape[0] == T + 1 and np.all(ph == np.floor(ph))
        assert np.all(ph.sum(axis=1) == 72.0) and ph.min() >= 0.0 and (ph[-1, 2] > 0).any()
        assert counts["inv"] > 0 and counts["poisson"] == 0
    assert -math.expm1(-600.0) == 1.0
    m = closed_sir(B, method="euler_multinomial", leaps=1)
    counts = {}
    ph = transitions(oracle, m, dict(beta=50.0, gamma=800.0), 1, 64, 3, counts=counts)
    assert np.all(ph == np.floor(ph)) and np.all(ph.sum(axis=1) == 72.0) and ph.min() >= 0.0
    assert np.all(ph[1, 0] == 0.0) and np.all(ph[1, 1] == 60.0) and np.all(ph[1, 2] == 12.0)      # (what arrives cannot leave in the same leap)
    assert np.all(ph[2, 2] == 72.0) and counts["all"] > 0


def two_exits(B, order, **kw):
    exits = [({"I": 1}, {"R": 1}, "gamma"), ({"I": 1}, {}, "mu")]
    return B.models.reaction_network(("I", "R"), exits if order == 0 else exits[::-1], x0=(100, 0), observe={"I": 1.0}, **kw)


@pytest.mark.parametrize("order", [0, 1])
def test_competing_exits_are_split_by_their_hazards(oracle, order):
    """I -> R at gamma = 3 next to I -> 0 at mu = 6, K = 1, I = 100, in both orders of writing.  Under method="tau_leap" each exit wants
    Poisson(300 | 600) > 100 firings, so the exit written first takes everybody (asserted: that is the network on which it visibly favours
    the first).  Under "euler_multinomial" the L leavers of all particles split as Binomial(L, gamma / (gamma + mu)) whatever the order
    (the multinomial's margin given its total): the count to R lies within 5 sqrt(L p (1 - p)) of L p."""
    import bayesssm_amd as B
    par, N, p = dict(gamma=3.0, mu=6.0), 512, 3.0 / 9.0
    m = two_exits(B, order, method="tau_leap", leaps=1)
    q = RN.unpack(m.pack(par))
    x0 = np.repeat(q["x0"][:, None], N, axis=1)
    cut = LR.make(1, oracle, 3, 1)[0](q, x0, np.zeros((2, N)))
    assert np.all(cut[0] == 0.0) and np.all(cut[1] == (100.0 if order == 0 else 0.0))
    counts = {}
    ph = transitions(oracle, two_exits(B, order, method="euler_multinomial", leaps=1), par, 1, N, 1, seed=3, stream=1, counts=counts)
    to_r, left = ph[1, 1].sum(), (100.0 - ph[1, 0]).sum()
    err, bar = abs(to_r - left * p), 5.0 * math.sqrt(left * p * (1.0 - p))
    print("order", order, "leavers", left, "to R", to_r, "error", err, "bar", bar, {k: counts[k] for k in ER.KEYS})
    assert left > 0.99 * 100 * N and err <= bar
    assert ph.min() >= 0.0 and np.all(ph[1, 1] <= 100.0 - ph[1, 0])


@pytest.mark.parametrize("K", [1, 3, 16])
def test_linear_death_has_the_exact_mean(oracle, K):
    """A -> 0 at rate k: a survivor of one leap stays with probability exp(-k / K), so after a unit of time x is Binomial(x0, exp(-k))
    for any K and the mean of N particles lies within 5 sqrt(x0 e^-k (1 - e^-k) / N) of x0 e^-k.  The cut Poisson leap at K = 1 has the
    mean x0 (1 - k) there (asserted to miss the same bar)."""
    import bayesssm_amd as B
    N, x0, k = 1024, 200.0, 0.7
    net = lambda **kw: B.models.reaction_network(("A",), [({"A": 1}, {}, k)], x0=(x0,), observe={"A": 1.0}, **kw)  # noqa: E731
    ph = transitions(oracle, net(method="euler_multinomial", leaps=K), {}, K, N, 2, seed=31, stream=K)
    for t in (1, 2):
        s = math.exp(-k * t)
        err, bar = abs(ph[t, 0].mean() - x0 * s), 5.0 * math.sqrt(x0 * s * (1.0 - s) / N)
        print("K", K, "t", t, "mean", ph[t, 0].mean(), "exact", x0 * s, "error", err, "bar", bar)
        assert err <= bar
    if K == 1:
        q = RN.unpack(net(method="tau_leap", leaps=1).pack())
        cut = LR.make(1, oracle, 31, 1)[0](q, np.full((1, N), x0), np.zeros((1, N)))
        assert abs(cut[0].mean() - x0 * math.exp(-k)) > 5.0 * math.sqrt(x0 * math.exp(-k) * (1.0 - math.exp(-k)) / N)


def test_sourceless_reactions_draw_poisson_counts(oracle):
    """0 -> A (order 0) and X -> 2 X (catalytic birth) are sourceless: Poisson counts at the propensity of the leap's start, next to a
    death A -> 0 with a source.  Nothing negative; the immigration's mean is exact"""
    import bayesssm_amd as B
    m = B.models.reaction_network(("A", "X"), [({}, {"A": 1}, 12.5), ({"X": 1}, {"X": 2}, 0.2), ({"A": 1}, {}, 0.5)], x0=(0, 30), observe={"A": 1.0},
                                  method="euler_multinomial", leaps=2)
    assert ER.classify(RN.unpack(m.pack())) == [(-1, -1), (-1, -1), (0, -1)]
    counts = {}
    N = 256
    ph = transitions(oracle, m, {}, 2, N, 1, counts=counts)
    assert counts["poisson"] == 2 * 2 * N and ph.min() >= 0.0 and np.all(ph == np.floor(ph)) and np.all(ph[1, 1] >= 30.0)
    # A after one unit from 0: immigrants of leap 1 thinned once by the death of leap 2, plus those of leap 2: mean 6.25 e^-0.25 + 6.25, and
    # the count is Poisson (a thinned Poisson plus a Poisson)
    mean = 6.25 * math.exp(-0.25) + 6.25
    assert abs(ph[1, 0].mean() - mean) <= 5.0 * math.sqrt(mean / N)


# --- classification, keywords, options ---------------------------------------------------------------------------------------------------
def test_classification_and_keyword_refusals():
    import bayesssm_amd as B
    both = [({"A": 1, "B": 1}, {"C": 1}, 0.1)]
    with pytest.raises(ValueError, match=r"reaction 0 consumes both of its reactants \(A \+ B -> \.\.\.\).*method='tau_leap'"):
        B.models.reaction_network(("A", "B", "C"), both, x0=(5, 5, 0), observe={"C": 1.0}, method="euler_multinomial", leaps=4)
    for method, kw in (("gillespie", {}), ("tau_leap", dict(leaps=4))):            # (the other methods keep taking it)
        assert B.models.reaction_network(("A", "B", "C"), both, x0=(5, 5, 0), observe={"C": 1.0}, method=method, **kw).method == method
    with pytest.raises(ValueError, match="method='euler_multinomial' needs leaps"):
        closed_sir(B, method="euler_multinomial")
    with pytest.raises(ValueError, match="leaps is the number of tau-leaps"):
        closed_sir(B, method="gillespie", leaps=4)
    with pytest.raises(ValueError, match="method must be one of 'gillespie', 'tau_leap', 'euler_multinomial'"):
        closed_sir(B, method="binomial")
    for bad in (0, 1025):
        with pytest.raises(ValueError, match=r"leaps must lie in 1 \.\. 1024"):
            closed_sir(B, method="euler_multinomial", leaps=bad)
    with pytest.raises(ValueError, match="leaps must be an integer"):
        closed_sir(B, method="euler_multinomial", leaps=4.0)
    m = closed_sir(B, method="euler_multinomial", leaps=np.int64(16))
    assert (m.method, m.leaps, m.rn_leaps, m.rn_method) == ("euler_multinomial", 16, 16, 1) and type(m.leaps) is int
    assert [closed_sir(B, **kw).rn_method for kw in (dict(), dict(method="tau_leap", leaps=4))] == [0, 0]
    # a catalyst (I in S + I -> 2 I has nu = +1; in S + I -> E + I nu = 0), a catalytic birth and an order 0 reaction are accepted
    m = B.models.reaction_network(("S", "E", "I"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, 0.1), ({"E": 1}, {"I": 1}, 0.2), ({}, {"S": 1}, 1.0), ({"I": 1}, {"I": 2}, 0.1),
                                                    ({"I": 1, "S": 1}, {"I": 2}, 0.1)],
                                  x0=(9, 1, 1), observe={"I": 1.0}, method="euler_multinomial", leaps=2)
    assert ER.classify(RN.unpack(m.pack())) == [(0, 2), (1, -1), (-1, -1), (-1, -1), (0, 2)]
    # the block does not know the method; build cannot change it; what the family refuses stays refused before any context exists
    assert m.pack().tobytes() == B.models.reaction_network(m.species, [({"S": 1, "I": 1}, {"E": 1, "I": 1}, 0.1), ({"E": 1}, {"I": 1}, 0.2), ({}, {"S": 1}, 1.0),
                                                                       ({"I": 1}, {"I": 2}, 0.1), ({"I": 1, "S": 1}, {"I": 2}, 0.1)], x0=(9, 1, 1), observe={"I": 1.0}).pack().tobytes()
    par = dict(beta=0.02, gamma=2.5)
    for key in ("method", "leaps"):
        b = closed_sir(B, method="euler_multinomial", leaps=4, build=lambda beta, gamma, key=key: {key: 8}, param_names=("beta", "gamma"))
        with pytest.raises(TypeError, match="build may return"):
            b.pack(par)
    m = closed_sir(B, method="euler_multinomial", leaps=4)
    y = np.array([3.0, 4.0])
    with pytest.raises(ValueError, match="RMPF"):
        m.rw_move_fn()
    with pytest.raises(ValueError, match="bootstrap filter"):
        B.auxiliary_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, [par] * 2)
    with pytest.raises(ValueError):
        B.bootstrap_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_fn="multinomial", **par)
    with pytest.raises(ValueError, match="consumes both"):
        ER.classify(RN.unpack(B.models.reaction_network(("A", "B", "C"), both, x0=(5, 5, 0), observe={"C": 1.0}).pack()))


def test_option_and_prototype_match_the_header():
    from bayesssm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bayesssm_amd.h")).read()
    # (the option qualifies rn_leaps and is declared next to it in both places: BSSM_OPT_RN_LEAPS + 1 = 15)
    assert re.search(r"#define\s+BSSM_OPT_RN_METHOD\s+\(BSSM_OPT_RN_LEAPS \+ 1\)\s+/\* = 15\b", header) and re.search(r"#define\s+BSSM_OPT_RN_LEAPS\s+14\b", header)
    assert _lib.Context.QUALIFIERS["rn_method"] == 15 == _lib.Context.OPTIONS["rn_leaps"] + 1 and "rn_method" not in _lib.Context.OPTIONS
    assert re.search(r"\bint\s+bssm_dump_rbinom\s*\(\s*bssm_ctx\s*\*\s*ctx\s*,\s*unsigned long long seed\s*,\s*unsigned long long stream\s*,\s*int call\s*,"
                     r"\s*int leap\s*,\s*int r\s*,\s*long long n_draws\s*,\s*const double\s*\*\s*n[^,]*,\s*const double\s*\*\s*q[^,]*,\s*double\s*\*\s*out[^)]*\)\s*;", header)
    assert "bssm_dump_rbinom" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.bssm_dump_rbinom.argtypes == [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    # the definition is stated where the option is, in the kernels' file and in DESIGN.md
    texts = [header, open(os.path.join(ROOT, "bayesssm_amd", "csrc", "rnet.hip.h")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()]
    for piece in ("1.15 + 2.53 * spq", "(-0.0873 + 0.0248 * b) + 0.01 * qq", "0.92 - 4.2 / b", "(2.83 + 5.1 / b) * spq", "k < 128.0", "-expm1(-H / (double)K)",
                  "pr = exp(n * log1p(-qq))"):
        for text in texts:
            assert piece in text, piece


def test_option_refusals_behind_the_abi():
    """bssm_ctx_set_option refuses an rn_method outside {0, 1} by the value alone (no context, no device: the check of the value comes
    first); a value inside reaches the check of the context; bssm_dump_rbinom refuses a NULL context"""
    from bayesssm_amd import _lib
    lib = _lib.load()
    for bad in (-1, 2, 15):
        assert lib.bssm_ctx_set_option(None, 15, bad) == _lib.ERR_ARG
        assert "rn_method takes 0" in lib.bssm_last_error().decode()
    for ok in (0, 1):
        assert lib.bssm_ctx_set_option(None, 15, ok) == _lib.ERR_ARG
        assert lib.bssm_last_error().decode() == "ctx is NULL"
    n, q, out = np.ones(4), np.full(4, 0.5), np.zeros(4)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.bssm_dump_rbinom(None, 1, 0, 0, 0, 0, 4, ptr(n), ptr(q), ptr(out)) == _lib.ERR_ARG
    assert "bssm_dump_rbinom" in lib.bssm_last_error().decode()


def test_option_scope_restores_the_previous_values():
    """Context.rn_method without a device: a stand-in records what set_option is given -- (K, method) inside, the previous values
    afterwards in the reverse order, also on an exception, and no call at all for a value that is already there"""
    from bayesssm_amd import _lib

    class Stub(_lib.Context):
        def __init__(self):
            self._h, self._set_options, self.calls = None, {}, []

        def set_option(self, name, value):
            self.calls.append((name, int(value)))
            self._set_options[name] = int(value)

    s = Stub()
    with s.rn_method(0, 0):
        pass
    assert s.calls == []
    with s.rn_method(1, 16):
        assert (s._set_options["rn_leaps"], s._set_options["rn_method"]) == (16, 1)
    assert s.calls == [("rn_leaps", 16), ("rn_method", 1), ("rn_method", 0), ("rn_leaps", 0)]
    s.calls.clear()
    with s.rn_method(0, 8):                              # (a tau-leap descriptor touches rn_leaps alone)
        assert s._set_options == {"rn_leaps": 8, "rn_method": 0}
    assert s.calls == [("rn_leaps", 8), ("rn_leaps", 0)]
    s.set_option("rn_method", 1)                         # left on the context by hand, with its leaps
    s.set_option("rn_leaps", 4)
    with pytest.raises(RuntimeError):
        with s.rn_method(1, 64):
            assert s._set_options == {"rn_leaps": 64, "rn_method": 1}
            raise RuntimeError("inside")
    assert s._set_options == {"rn_leaps": 4, "rn_method": 1}
    with s.rn_method(0, 0):                              # a Gillespie descriptor's call puts both at 0 for its length
        assert s._set_options == {"rn_leaps": 0, "rn_method": 0}
    assert s._set_options == {"rn_leaps": 4, "rn_method": 1}
