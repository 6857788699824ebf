"""Gamma white noise on the rates of the reaction networks (models.reaction_network(..., method="euler_multinomial", leaps=K, noise={...}))
without a GPU: the numpy restatement of the definition (tests/rnet_gwn_restated.py) -- its gamma sampler against numpy's own (an independent
implementation), its normal quantile against the standard library's, the key layout, the closed form of the linear death process --, the
descriptor's groups, leaders, block layout and refusals, the option and the prototype against the header, and the option's scope on a
stand-in context."""
import ctypes as C
import math
import os
import re
import statistics
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_gwn_restated as GR  # noqa: E402
import rnet_restated as RN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sh = 1 / (K sigma^2): deep in the boost (0.01), the boost (0.25), the boundary (1.0: no boost), sigma = 0.1 at K = 16 (6.25), sigma = 0.05 at K = 1
SHAPES = (0.01, 0.25, 1.0, 6.25, 400.0)
N_DRAWS = 100000
KS_BAR = 2.225 * math.sqrt(2.0 / N_DRAWS)                 # the two-sample critical value at 1e-4: sqrt(-log(1e-4 / 2) / 2) = 2.225, times sqrt((n + m) / (n m))


def gamma_moment_bars(x, sh):
    """|mean - sh| and |variance - sh| of draws from Gamma(shape sh, scale 1) in units of their closed-form standard errors, as
    test_rnet_em_cpu.binom_moment_bars takes them: sqrt(s2 / N) and sqrt((mu4 - s2^2 (N - 3) / (N - 1)) / N), s2 = sh, mu4 = 3 sh^2 + 6 sh"""
    N = x.size
    s2, mu4 = sh, 3.0 * sh * sh + 6.0 * sh
    return abs(x.mean() - sh) / math.sqrt(s2 / N), abs(x.var() - s2) / math.sqrt((mu4 - s2 * s2 * (N - 3.0) / (N - 1.0)) / N)


def ks_two_sample(a, b):
    a, b = np.sort(a), np.sort(b)
    pts = np.concatenate([a, b])
    return float(np.max(np.abs(np.searchsorted(a, pts, side="right") / a.size - np.searchsorted(b, pts, side="right") / b.size)))


@pytest.mark.parametrize("i,sh", list(enumerate(SHAPES)))
def test_restated_sampler_against_numpys(i, sh):
    """10^5 draws per shape under fixed seeds against numpy.random.Generator.gamma: the two-sample Kolmogorov-Smirnov statistic at most the
    critical value at 1e-4, mean and variance within 5 standard errors of the closed forms.  The counts say which branches the shape takes."""
    counts = GR.new_counts()
    x = GR.sample(3000 + i, 4, call=i, leap=9 * i, g=i % 8, sh=np.full(N_DRAWS, sh), counts=counts)
    ref = np.random.default_rng(77 + i).gamma(sh, size=N_DRAWS)
    ks = ks_two_sample(x, ref)
    em, ev = gamma_moment_bars(x, sh)
    print("shape", sh, "KS", ks, "bar", KS_BAR, "mean", x.mean(), "var", x.var(), "errors in s.e.", em, ev, counts)
    assert np.all(np.isfinite(x)) and x.min() >= 0.0
    assert ks <= KS_BAR
    assert em <= 5.0 and ev <= 5.0
    assert counts["gamma"] == N_DRAWS and counts["fallback"] == 0 and counts["squeeze"] + counts["full"] == N_DRAWS
    assert (counts["boost"], counts["plain"]) == ((N_DRAWS, 0) if sh < 1.0 else (0, N_DRAWS))
    assert counts["squeeze"] > 0 and counts["full"] > 0 and counts["rejected"] > 0
    if sh <= 1.0:                                           # (cc = 1 / sqrt(9 dd) is large enough for 1 + cc x <= 0 only at small shapes)
        assert counts["v<=0"] > 0


def test_restated_sampler_is_keyed():
    sh = np.full(64, 2.5)
    a = GR.sample(5, 0, 1, 2, 3, sh)
    assert len(set(a)) == 64
    for other in ((2, 2, 3), (1, 3, 3), (1, 2, 4)):
        assert not np.array_equal(a, GR.sample(5, 0, *other, sh))
    assert np.array_equal(GR.sample(5, 0, 1, 1, 0, sh), GR.sample(5, 0, 1, 0, 8, sh))       # (the stride over the leaders is 8)
    assert not np.array_equal(a, GR.sample(6, 0, 1, 2, 3, sh)) and not np.array_equal(a, GR.sample(5, 1, 1, 2, 3, sh))


def test_restated_qnorm_against_the_standard_library():
    """AS 241 restated against statistics.NormalDist().inv_cdf to 4 ulp, on a sweep that covers the central branch and both tail branches"""
    p = np.concatenate([np.linspace(0.001, 0.999, 1999), 10.0 ** -np.linspace(0.1, 300.0, 1500), 1.0 - 10.0 ** -np.linspace(1.0, 15.5, 300),
                        [0.075, 0.925, 0.0749999, 0.9250001, 0.5, 2.0 ** -53 * 0.5, 1.0 - 2.0 ** -53]])
    branches = {}
    got = GR.qnorm_as241(p, branches)
    inv = statistics.NormalDist().inv_cdf
    want = np.array([inv(float(v)) for v in p])
    ulp = np.abs(got - want) / np.spacing(np.abs(want))
    ulp[want == 0.0] = np.abs(got[want == 0.0]) / np.spacing(0.0)
    print("branches", branches, "largest difference in ulp", ulp.max(), "at p =", p[np.argmax(ulp)])
    assert all(branches[k] > 100 for k in ("central", "near", "far"))
    assert ulp.max() <= 4.0


def test_key_layout_collides_with_no_binomial_or_poisson_key():
    """bit 27 of the third counter word: the binomial and Poisson draws' largest word (l = 1023, r = 7, a = 63) ends at bit 26, every gamma
    word has bit 27 set, is below 2^32 and is distinct from every other gamma word"""
    largest = RN.DRAW_TRANS | ((((1023 * 8 + 7) << 6) | 63) << 8)
    assert largest < (1 << 27) and largest.bit_length() == 27
    lg, a = np.meshgrid(np.arange(1024 * 8), np.arange(64), indexing="ij")
    others = RN.DRAW_TRANS | (((lg << 6) | a) << 8)
    words = np.array([[GR.gamma_key(int(l_), int(a_)) for a_ in (0, 1, 62, 63)] for l_ in (0, 1, 7, 8, 8 * 1023, 8 * 1023 + 7)]).reshape(-1)
    assert np.all(words & (1 << 27)) and words.max() < (1 << 32) and len(set(words)) == words.size
    assert GR.gamma_key(8 * 1023 + 7, 63) == largest | (1 << 27)
    assert not np.isin(words, others).any() and int(others.max()) == largest
    assert np.array_equal((lg.reshape(-1) * 64 + a.reshape(-1)), np.arange(1024 * 8 * 64))      # (the words are a bijection of (lg, a))


# --- the transition -----------------------------------------------------------------------------------------------------------------------
def death(B, sigma=0.5, K=4, x0=1000.0, **kw):
    return B.models.reaction_network(("X",), [({"X": 1}, {}, "h")], x0=(x0,), observe={"X": 0.1}, method="euler_multinomial", leaps=K,
                                     noise={"h": sigma}, **kw)


def restated_step(oracle, m, par, N, seed, stream, counts=None):
    """one restated transition (call 0) of N particles from x0: [d][N]"""
    plain, lead, sigma = GR.strip(m.pack(par), nb=m.obs == "negbin")
    q = RN.unpack(plain[:3 + m.dim + 3 * m.R + m.R * m.dim + m.p * m.dim])
    trans, _, _ = GR.make(m.leaps, lead, sigma, oracle, seed, stream, counts)
    x = np.repeat(np.asarray(q["x0"], dtype=np.float64)[:, None], N, axis=1)
    return trans(q, x, np.zeros((m.dim, N)))


def death_bars(x1, h, sigma, x0):
    """|mean - E| and |variance - Var| of the survivors in units of their standard errors: sqrt(Var / N) and
    sqrt((m4 - Var^2 (N - 3) / (N - 1)) / N) with the closed forms E, Var (rnet_gwn_restated.death_moments) and m4 the sample's fourth central
    moment about E (the mixture's own has no short closed form)"""
    N = x1.size
    mean, var = GR.death_moments(h, sigma, x0)
    m4 = float(np.mean((x1 - mean) ** 4))
    return abs(x1.mean() - mean) / math.sqrt(var / N), abs(x1.var() - var) / math.sqrt((m4 - var * var * (N - 3.0) / (N - 1.0)) / N)


@pytest.mark.parametrize("K", [1, 4])
def test_linear_death_process_closed_form(oracle, K):
    """X -> 0 at h = 0.7 with sigma = 0.5 from x0 = 1000, N = 4096: the sum of the K noise weights is Gamma(1 / sigma^2, sigma^2) whatever K
    is, and every individual survives the K leaps with probability exp(-h W): mean and variance of x_1 are exact at any K"""
    import bayesssm_amd as B
    counts = {}
    x1 = restated_step(oracle, death(B, 0.5, K), dict(h=0.7), 4096, seed=31, stream=K, counts=counts)[0]
    em, ev = death_bars(x1, 0.7, 0.5, 1000.0)
    print("K", K, "mean", x1.mean(), "var", x1.var(), "closed form", GR.death_moments(0.7, 0.5, 1000.0), "errors in s.e.", em, ev, counts["rgamma"])
    assert np.all(x1 == np.floor(x1)) and x1.min() >= 0 and x1.max() <= 1000
    assert counts["rgamma"]["gamma"] == 4096 * K and counts["rgamma"]["fallback"] == 0
    assert em <= 5.0 and ev <= 5.0
    # without the noise the variance would be the binomial's x0 s (1 - s), far below
    assert x1.var() > 20.0 * 1000.0 * math.exp(-0.7) * (1.0 - math.exp(-0.7))


def test_restated_transition_shares_a_groups_draw_and_conserves(oracle):
    """two strata infected under one beta (one group, leader 0) and a sourceless immigration with noise of its own: totals are conserved
    apart from the immigrants, nothing is negative, and the group's draw is one per leap (counts)"""
    import bayesssm_amd as B
    m = B.models.reaction_network(("S1", "S2", "I", "R"), [({"S1": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"S2": 1, "I": 1}, {"I": 2}, "beta"),
                                                           ({}, {"R": 1}, "imm")],
                                  x0=(400, 300, 20, 0), observe={"I": 0.1}, method="euler_multinomial", leaps=3, noise={"beta": 0.4, 3: "s_imm"})       # sh = 1 / (3 * 0.16) > 1 and 1 / (3 * 2.25) < 1
    assert m.noise_lead == [0, -1, 0, 3] and m.param_order == ("beta", "gamma", "imm", "s_imm")
    counts = {}
    x1 = restated_step(oracle, m, dict(beta=0.004, gamma=0.3, imm=5.0, s_imm=1.5), 512, seed=3, stream=1, counts=counts)
    assert np.all(x1 == np.floor(x1)) and x1.min() >= 0
    assert counts["rgamma"]["gamma"] == 2 * 3 * 512 and counts["rgamma"]["boost"] == counts["rgamma"]["plain"] == 3 * 512
    assert np.all(x1.sum(axis=0) >= 720) and x1.sum(axis=0).max() > 720 and counts["poisson"] == 3 * 512


# --- the descriptor ---------------------------------------------------------------------------------------------------------------------------
SIRS = (("S", "I", "R"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"R": 1, "I": 1}, {"S": 1, "I": 1}, "beta"), ({"R": 1}, {"S": 1}, 0.1)])


def sirs(B, **kw):
    kw = dict(dict(method="euler_multinomial", leaps=4), **kw)
    return B.models.reaction_network(*SIRS, x0=(90, 10, 0), observe={"I": 0.5}, **kw)


def test_groups_leaders_and_block_layout():
    import bayesssm_amd as B
    plain = sirs(B)
    par = dict(beta=0.01, gamma=0.3)
    base = plain.pack(par)
    assert plain.noise is None and plain.rn_method == 1 and plain.n_theta() == base.size
    m = sirs(B, noise={"beta": "sigma_se", 3: 0.25})
    assert m.noise_lead == [0, -1, 0, 3] and m.noise_key == ["beta", None, "beta", 3] and m.rn_method == 2 and m.rn_leaps == 4
    assert m.param_order == ("beta", "gamma", "sigma_se") and m.transition_fn.params == m.param_order and m.log_likelihood_fn.params == ()
    blk = m.pack(dict(par, sigma_se=0.4))
    o = 3 + 3 + 3 * 4 + 4 * 3 + 1 * 3
    assert blk.size == base.size + 8 == m.n_theta() and m.n_theta_ok(blk.size) and not m.n_theta_ok(base.size)
    assert np.array_equal(blk[:o], base[:o]) and np.array_equal(blk[o + 8:], base[o:])
    assert np.array_equal(blk[o:o + 8], [0, -1, 0, 3, 0.4, 0.0, 0.4, 0.25])
    stripped, lead, sigma = GR.strip(blk)
    assert stripped.tobytes() == base.tobytes() and list(lead) == [0, -1, 0, 3] and list(sigma) == [0.4, 0.0, 0.4, 0.25]
    with pytest.raises(TypeError, match='argument "sigma_se" is missing'):
        m.pack(par)
    # explicit indices: two groups of one, leaders 0 and 2
    e = sirs(B, noise={0: 0.4, 2: 0.4})
    assert e.noise_lead == [0, -1, 2, -1] and np.array_equal(e.pack(par)[o:o + 8], [0, -1, 2, -1, 0.4, 0.0, 0.4, 0.0])
    # with everything else: size[p] in front, the tails behind
    sched = np.ones((6, 4))
    full = B.models.reaction_network(("S", "I", "R", "C"), [({"S": 1, "I": 1}, {"I": 2, "C": 1}, "beta"), ({"I": 1}, {"R": 1}, "gamma")], x0=(90, 10, 0, 0),
                                     observe={"C": 0.5}, counters=("C",), rate_schedule=np.ones((6, 2)), obs="negbin", size="r", missing="skip",
                                     method="euler_multinomial", leaps=2, noise={"beta": "s"})
    assert full.param_order == ("beta", "gamma", "r", "s") and full.log_likelihood_fn.params == ("r",)
    fb = full.pack(dict(beta=0.01, gamma=0.2, r=7.0, s=0.3))
    of = 3 + 4 + 3 * 2 + 2 * 4 + 4
    assert np.array_equal(fb[of:of + 5], [7.0, 0, -1, 0.3, 0.0]) and np.array_equal(fb[of + 5:of + 9], [0, 0, 0, 1]) and fb[of + 9] == 6.0
    assert fb.size == full.n_theta() == of + 1 + 4 + 4 + 1 + 12 and sched.size == 24
    full.check_times(fb.size, 6)
    with pytest.raises(ValueError, match="short of the last observation time"):
        full.check_times(fb.size, 7)
    # build may return noise_sigma: a number for every group, or a dict by noise key
    b = sirs(B, noise={"beta": 0.4, 3: 0.25}, build=lambda beta, gamma, v: {"noise_sigma": {"beta": v}}, param_names=("beta", "gamma", "v"))
    assert np.array_equal(b.pack(dict(par, v=0.9))[o + 4:o + 8], [0.9, 0.0, 0.9, 0.25]) and b.n_theta() is None and b.n_theta_ok(blk.size)
    b = sirs(B, noise={"beta": 0.4, 3: 0.25}, build=lambda beta, gamma, v: {"noise_sigma": v}, param_names=("beta", "gamma", "v"))
    assert np.array_equal(b.pack(dict(par, v=0.9))[o + 4:o + 8], [0.9, 0.0, 0.9, 0.9])
    assert np.array_equal(m.pack_many([dict(par, sigma_se=s) for s in (0.1, 0.2)])[:, o + 4], [0.1, 0.2])


def test_refusals_on_the_host():
    import bayesssm_amd as B
    for kw in (dict(method="gillespie", leaps=None), dict(method="tau_leap", leaps=4)):
        with pytest.raises(ValueError, match="noise .* needs method='euler_multinomial'"):
            sirs(B, noise={"beta": 0.3}, **kw)
    with pytest.raises(ValueError, match="noise names the unknown rate 'bta'"):
        sirs(B, noise={"bta": 0.3})
    with pytest.raises(ValueError, match=r"noise names the unknown reaction index 4 \(0 .. 3\)"):
        sirs(B, noise={4: 0.3})
    with pytest.raises(ValueError, match="noise names the unknown rate 1.5"):
        sirs(B, noise={1.5: 0.3})
    with pytest.raises(ValueError, match="noise names reaction 2 twice"):
        sirs(B, noise={"beta": 0.3, 2: 0.3})
    with pytest.raises(ValueError, match="noise names reaction 0 twice"):
        sirs(B, noise={0: 0.3, "beta": 0.3})
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="a noise sigma must be finite and > 0"):
            sirs(B, noise={"beta": bad})
        with pytest.raises(ValueError, match="a noise sigma must be finite and > 0"):
            sirs(B, noise={"beta": "s"}).pack(dict(beta=0.01, gamma=0.3, s=bad))
    with pytest.raises(ValueError, match="a noise sigma is a number or a parameter name"):
        sirs(B, noise={"beta": [0.3]})
    with pytest.raises(ValueError, match="noise is empty"):
        sirs(B, noise={})
    with pytest.raises(ValueError, match="noise is a dict"):
        sirs(B, noise=0.3)
    with pytest.raises(ValueError, match="build returned noise_sigma; it needs noise="):
        sirs(B, build=lambda beta, gamma: {"noise_sigma": 0.3}, param_names=("beta", "gamma")).pack(dict(beta=0.01, gamma=0.3))
    with pytest.raises(ValueError, match="which noise= does not name"):
        sirs(B, noise={"beta": 0.3}, build=lambda beta, gamma: {"noise_sigma": {1: 0.3}}, param_names=("beta", "gamma")).pack(dict(beta=0.01, gamma=0.3))


# --- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_option_and_prototype_match_the_header():
    from bayesssm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bayesssm_amd.h")).read()
    assert re.search(r"#define\s+BSSM_OPT_RN_NOISE\s+\(BSSM_OPT_RN_LEAPS \+ 2\)\s+/\* = 16\b", header)
    assert _lib.Context.QUALIFIERS["rn_noise"] == 16 == _lib.Context.OPTIONS["rn_leaps"] + 2 and "rn_noise" not in _lib.Context.OPTIONS
    assert 16 not in _lib.Context.OPTIONS.values()
    assert re.search(r"\bint\s+bssm_dump_rgamma\s*\(\s*bssm_ctx\s*\*\s*ctx\s*,\s*unsigned long long seed\s*,\s*unsigned long long stream\s*,\s*int call\s*,"
                     r"\s*int leap\s*,\s*int g\s*,\s*long long n\s*,\s*const double\s*\*\s*shape[^,]*,\s*double\s*\*\s*out[^)]*\)\s*;", header)
    assert "bssm_dump_rgamma" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.bssm_dump_rgamma.argtypes == [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    # the definition is stated where the option is, in the kernels' file and in DESIGN.md
    texts = [header, open(os.path.join(ROOT, "bayesssm_amd", "csrc", "rnet.hip.h")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()]
    for piece in ("sh = 1.0 / ((double)K * s2)", "dd = al - 1.0 / 3.0", "cc = 1.0 / sqrt(9.0 * dd)", "u2 < 1.0 - 0.0331 * (x2 * x2)",
                  "log(u2) < 0.5 * x2 + dd * ((1.0 - v) + log(v))", "exp(log(ub) / sh)", "pe = -expm1(-H)", "(1u << 27)"):
        for text in texts:
            assert piece in text, piece


def test_option_refusals_behind_the_abi():
    """bssm_ctx_set_option refuses an rn_noise outside {0, 1} by the value alone (no context, no device); a value inside reaches the check
    of the context; bssm_dump_rgamma refuses a NULL context"""
    from bayesssm_amd import _lib
    lib = _lib.load()
    for bad in (-1, 2):
        assert lib.bssm_ctx_set_option(None, 16, bad) == _lib.ERR_ARG
        assert "rn_noise takes 0 or 1" in lib.bssm_last_error().decode()
    for ok in (0, 1):
        assert lib.bssm_ctx_set_option(None, 16, ok) == _lib.ERR_ARG
        assert lib.bssm_last_error().decode() == "ctx is NULL"
    sh, out = np.ones(4), np.zeros(4)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.bssm_dump_rgamma(None, 1, 0, 0, 0, 0, 4, ptr(sh), ptr(out)) == _lib.ERR_ARG
    assert "bssm_dump_rgamma" in lib.bssm_last_error().decode()


def test_option_scope_restores_the_previous_values():
    """Context.rn_method(2, K) without a device: a stand-in records what set_option is given -- rn_leaps = K, rn_method = 1, rn_noise = 1
    inside, the previous values afterwards in the reverse order, also on an exception; the other methods put a hand-left rn_noise at 0 for
    the length of the call and touch nothing that is 0 already"""
    from bayesssm_amd import _lib

    class Stub(_lib.Context):
        def __init__(self):
            self._h, self._set_options, self.calls = None, {}, []

        def set_option(self, name, value):
            self.calls.append((name, int(value)))
            self._set_options[name] = int(value)

    s = Stub()
    with s.rn_method(2, 16):
        assert s._set_options == {"rn_leaps": 16, "rn_method": 1, "rn_noise": 1}
    assert s.calls == [("rn_leaps", 16), ("rn_method", 1), ("rn_noise", 1), ("rn_noise", 0), ("rn_method", 0), ("rn_leaps", 0)]
    s.calls.clear()
    with s.rn_method(1, 4):                               # (plain Euler-multinomial leaps do not touch rn_noise)
        pass
    assert ("rn_noise", 0) not in s.calls and ("rn_noise", 1) not in s.calls
    with pytest.raises(RuntimeError):
        with s.rn_method(2, 64):
            raise RuntimeError("inside")
    assert s._set_options == {"rn_leaps": 0, "rn_method": 0, "rn_noise": 0}
    s.set_option("rn_method", 1); s.set_option("rn_leaps", 4); s.set_option("rn_noise", 1)      # left on the context by hand
    for method, leaps in ((0, 0), (0, 8), (1, 8)):
        with s.rn_method(method, leaps):
            assert s._set_options == {"rn_leaps": leaps, "rn_method": method, "rn_noise": 0}
        assert s._set_options == {"rn_leaps": 4, "rn_method": 1, "rn_noise": 1}
