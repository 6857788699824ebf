"""GPU tests of gamma white noise on the rates of the reaction networks (models.reaction_network(..., method="euler_multinomial", leaps=K,
noise={...}); rn_rgamma, rn_noise_w, the RN_EULER_MULTINOM_GWN instantiations of k_step_rn and k_pf_batch_rn, the context option rn_noise,
bssm_dump_rgamma).  The reference is the numpy restatement of the definition (tests/rnet_gwn_restated.py) on the same Philox blocks, at
the bars of tests/test_gpu_rnet_limits.py; the closed form of the linear death process, bit-for-bit identities (batched = single, an
appended zero-rate reaction, a group against explicit indices, the other methods after a noisy call), pmmh and the refusals behind the ABI
cover the rest."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_gwn_restated as GR  # noqa: E402
from test_gpu_rnet import run, same  # noqa: E402
from test_gpu_rnet_em import EM8_OBSERVE, EM8_PAR, EM8_REACTIONS, EM8_SPECIES, EM8_X0, NETS, em8, loop3, sir2  # noqa: E402, F401
from test_gpu_rnet_limits import OT, compare_with_restatement, u_res_for  # noqa: E402
from test_rnet_gwn_cpu import SHAPES, death, death_bars, gamma_moment_bars  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 15, 8)
    yield c
    c.close()


def noisy(make, B, K, noise, **kw):
    return make(B, method="euler_multinomial", leaps=K, noise=noise, **kw)


# --- 0. fails without the feature -------------------------------------------------------------------------------------------------------
def test_noise_runs_and_differs_from_plain_leaps(B, ctx):
    make, par, y = NETS["loop3"]
    par = dict(par, beta=0.002)
    kw = dict(resample_algorithm="SISAR", obs_times=OT, seed=3, stream=1)
    a = run(B, noisy(make, B, 4, {"beta": 0.3}), "BPF", y, 385, ctx, par, **kw)
    b = run(B, noisy(make, B, 4, {"beta": 0.6}), "BPF", y, 385, ctx, par, **kw)
    plain = run(B, make(B, method="euler_multinomial", leaps=4), "BPF", y, 385, ctx, par, **kw)
    for r in (a, b):
        ph = r["particles_history"].reshape(len(y) + 1, 3, 385)
        assert np.isfinite(r["loglike"]) and np.all(np.isfinite(r["state_est"]))
        assert np.all(ph == np.floor(ph)) and ph.min() >= 0 and np.all(ph.sum(axis=1) == 500.0)
    for x, z in ((a, plain), (a, b), (b, plain)):
        assert x["loglike"] != z["loglike"] and not np.array_equal(x["particles_history"], z["particles_history"])
        assert not np.array_equal(x["state_est"], z["state_est"])


# --- 1. the sampler against its restatement ---------------------------------------------------------------------------------------------
MIXED_SH = np.tile(np.array([0.01, 400.0, 0.25, 1.0, 6.25, 0.999999, 1.000001, 0.0625, 1e-3, 2.0, 1e4, 0.5, 3.0, 0.1, 25.0, 1.0 / 3.0]), 8)      # two waves


def agree(got, ref):
    """equal, or within 1e-10 relative: the boost's exp(log(u) / sh) amplifies a last-bit difference between the device's and the host's log
    by at most 37.4 / 0.01 (|log u| <= 53 log 2 = 37.4 at the smallest shape of the list), a few ulp times that is about 2e-12, and 1e-10
    leaves a margin of 50"""
    return (got == ref) | (np.abs(got - ref) <= 1e-10 * np.abs(ref))


def test_sampler_equals_its_restatement(B, ctx):
    """bssm_dump_rgamma against rnet_gwn_restated.sample: 4096 draws per shape of the CPU test's list and a two-wave vector that mixes
    shapes.  At most 1 draw in 10^4 disagrees (an accept decision that flipped on a last bit is the only admitted cause); the device's
    draws meet the CPU test's moment bars; every branch is reached and no draw runs out of attempts."""
    n_draws, total, differ = 4096, 0, 0
    counts = GR.new_counts()
    for i, sh in enumerate(SHAPES):
        key = dict(seed=900 + i, stream=2, call=i, leap=200 * i, g=i % 8)
        got = B.dump_rgamma(np.full(n_draws, sh), ctx=ctx, **key)
        ref = GR.sample(key["seed"], key["stream"], key["call"], key["leap"], key["g"], np.full(n_draws, sh), counts)
        bad = int(np.sum(~agree(got, ref)))
        total, differ = total + n_draws, differ + bad
        em, ev = gamma_moment_bars(got, sh)
        print("shape", sh, "disagreeing", bad, "bitwise different", int(np.sum(got != ref)), "mean", got.mean(), "var", got.var(), "errors in s.e.", em, ev)
        assert np.all(np.isfinite(got)) and got.min() >= 0.0
        assert em <= 5.0 and ev <= 5.0
    got = B.dump_rgamma(MIXED_SH, seed=11, stream=5, call=3, leap=1023, g=7, ctx=ctx)
    ref = GR.sample(11, 5, 3, 1023, 7, MIXED_SH, counts)
    total, differ = total + MIXED_SH.size, differ + int(np.sum(~agree(got, ref)))
    print("disagreeing draws: %d of %d" % (differ, total), counts)
    assert differ * 10000 <= total
    assert all(counts[k] > 0 for k in ("boost", "plain", "squeeze", "full", "rejected", "v<=0")) and counts["fallback"] == 0


# --- 2. filters against the restatement ---------------------------------------------------------------------------------------------------
def restated(oracle, m, par, y, N, algorithm, K, seed, stream, nb=False):
    u = u_res_for(algorithm, len(y), N, "stratified")
    counts = {}
    t0 = time.perf_counter()
    ref = GR.pf_run_rn(oracle, m.pack(par), y, N, u, K, nb=nb, seed=seed, stream=stream, algorithm=algorithm, counts=counts, resample_algorithm="SISAR",
                       resample_fn="stratified", obs_times=OT, return_particles=True)
    print("restatement: %.2f s" % (time.perf_counter() - t0), counts["rgamma"])
    return ref, counts, u


# sir2: one noisy reaction; loop3: noise on the infection and, by index, on R -> S; em8: noise on the sourceless k0 and on a name that two
# reactions share (k3 for C -> D and C -> E: leader 3, member 4).  The sigmas put sh = 1 / (K sigma^2) on both sides of 1 within every case.
GWN_NETS = {"sir2": (sir2, {"beta": 0.3, 1: 1.2}), "loop3": (loop3, {"beta": 0.4, 3: 1.5}), "em8": (None, {"k0": 1.1, "k3": 0.2})}
CASES = [(net, alg, 385, K) for net in ("sir2", "loop3") for alg in ("BPF", "APF") for K in (1, 4)] + [("em8", "BPF", 385, 4), ("em8", "APF", 385, 1)]


def em8_shared(B, **kw):
    reactions = [rx if i != 4 else (rx[0], rx[1], "k3") for i, rx in enumerate(EM8_REACTIONS)]
    return B.models.reaction_network(EM8_SPECIES, reactions, x0=EM8_X0, observe=EM8_OBSERVE, **kw)


@pytest.mark.parametrize("net,algorithm,N,K", CASES)
def test_filters_against_the_restatement(B, ctx, oracle, net, algorithm, N, K):
    make, par, y = NETS[net]
    make, noise = GWN_NETS[net]
    if net == "em8":
        make, par = em8_shared, {k: v for k, v in par.items() if k != "k4"}
    m = noisy(make, B, K, noise)
    if net == "em8":
        assert m.noise_lead == [0, -1, -1, 3, 3, -1, -1, -1]
    ref, counts, u = restated(oracle, m, par, y, N, algorithm, K, seed=23, stream=4)
    assert np.isfinite(ref["loglike"]) and ref["early_return_step"] == 0
    g = counts["rgamma"]
    assert g["boost"] > 0 and g["plain"] > 0 and g["fallback"] == 0, g
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=23, stream=4, draws={"u_res": u})
    compare_with_restatement(got, ref)


def everything(B, K, noise):
    sched = 0.6 + 0.05 * np.arange(5 * 4, dtype=np.float64).reshape(5, 4)
    return B.models.reaction_network(("S", "I", "R", "C"), [({"S": 1, "I": 1}, {"I": 2, "C": 1}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"I": 1}, {"S": 1}, "delta"),
                                                            ({"R": 1}, {"S": 1}, "rho")],
                                     x0=(300, 160, 40, 0), observe=[{"C": 0.05}, {"I": 0.05, "R": 0.1}], counters=("C",), rate_schedule=sched, missing="skip",
                                     obs="negbin", size=(2.0, 15.0), method="euler_multinomial", leaps=K, noise=noise)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_everything_together_against_the_restatement(B, ctx, oracle, algorithm):
    """a counter, a rate schedule whose entries all differ, missing="skip" with a NaN, obs="negbin" and a named sigma, with K = 4"""
    N, K = 385, 4
    m = everything(B, K, {"beta": "sigma_se", "rho": 0.3})
    par = dict(NETS["loop3"][1], beta=0.002, sigma_se=0.7)
    y = np.array([[5, 12], [6, np.nan], [7, 12], [np.nan, 11], [5, 10]], dtype=np.float64)
    ref, counts, u = restated(oracle, m, par, y, N, algorithm, K, seed=41, stream=6, nb=True)
    assert np.isfinite(ref["loglike"]) and counts["rgamma"]["boost"] > 0 and counts["rgamma"]["plain"] > 0 and len(counts["rows"]) > 0
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=41, stream=6, draws={"u_res": u})
    compare_with_restatement(got, ref)
    ph = got["particles_history"].reshape(len(y) + 1, 4, N)
    assert np.all(ph[:, :3].sum(axis=1) == 500.0) and ph.min() >= 0


# --- 3. the closed form on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4])
def test_linear_death_process_closed_form_on_the_device(B, ctx, K):
    """X -> 0 at h = 0.7, sigma = 0.5, x0 = 1000: mean and variance of x_1 over N = 4096 particles (SIS: no resampling before the record)
    within 5 standard errors of the closed forms, from the single filter's particles_history, and from the batched filters' state estimates"""
    N = 4096
    m = death(B, 0.5, K)
    y = np.array([50.0])
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    one = B.bootstrap_filter(y, N, *fns, ctx=ctx, resample_algorithm="SIS", seed=17, stream=K, h=0.7)
    x1 = one["particles_history"].reshape(2, 1, N)[1, 0]
    em, ev = death_bars(x1, 0.7, 0.5, 1000.0)
    print("K", K, "mean", x1.mean(), "var", x1.var(), "closed form", GR.death_moments(0.7, 0.5, 1000.0), "errors in s.e.", em, ev)
    assert np.all(x1 == np.floor(x1)) and x1.min() >= 0 and x1.max() <= 1000
    assert em <= 5.0 and ev <= 5.0
    # the batched path has no particle histories: with the one observation missing every weight is equal and under SIS the state estimate
    # of a filter is the mean of its x_1.  F = 64 filters of 1024 particles under streams of their own: the mean of the 64 means within
    # 5 standard errors sqrt(Var / (F N)); their variance times N estimates Var, and as means of 1024 draws are close to normal its
    # standard error is Var sqrt(2 / (F - 1))
    F, Nb = 64, 1024
    ms = death(B, 0.5, K, missing="skip")
    bat = B.bootstrap_filter_batch(np.array([np.nan]), Nb, ms.init_fn, ms.transition_fn, ms.log_likelihood_fn, [dict(h=0.7)] * F, [17] * F, list(range(100, 100 + F)),
                                   resample_algorithm="SIS", ctx=ctx)
    means = bat["state_est"].reshape(F, 2)[:, 1]
    mean, var = GR.death_moments(0.7, 0.5, 1000.0)
    em, ev = abs(means.mean() - mean) / np.sqrt(var / (F * Nb)), abs(means.var(ddof=1) * Nb - var) / (var * np.sqrt(2.0 / (F - 1)))
    print("batched: mean of means", means.mean(), "N var of means", means.var(ddof=1) * Nb, "errors in s.e.", em, ev)
    assert np.all(bat["status"] == 0) and len(set(means)) == F
    assert em <= 5.0 and ev <= 5.0


# --- 4. bit-for-bit identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["sir2", "loop3", "em8"])
def test_batched_equals_single(B, ctx, net):
    make, par, y = NETS[net]
    make, noise = GWN_NETS[net]
    if net == "em8":
        make, par = em8_shared, {k: v for k, v in par.items() if k != "k4"}
    noise = dict(noise, **{list(noise)[0]: "sg"})
    first = list(par)[0]
    pars = [dict(par, sg=0.3), dict(par, sg=0.9, **{first: 1.2 * par[first]}), dict(par, sg=1.4)]
    for N, ra, rf, K in [(1, "SISAR", "stratified", 4), (7, "SISR", "systematic", 1), (385, "SISAR", "stratified", 4), (1000, "SIS", "stratified", 1)]:
        m = noisy(make, B, K, noise)
        fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
        bat = B.bootstrap_filter_batch(y, N, *fns, pars, [11, 12, 13], [3, 4, 5], obs_times=OT, resample_algorithm=ra, resample_fn=rf, ctx=ctx)
        assert np.all(bat["status"] == 0)
        if N >= 385:
            assert len(set(bat["loglike"])) == 3 and np.all(np.isfinite(bat["loglike"]))
        for f in range(3):
            one = B.bootstrap_filter(y, N, *fns, obs_times=OT, resample_algorithm=ra, resample_fn=rf, ctx=ctx, return_particles=False, seed=11 + f, stream=3 + f, **pars[f])
            assert bat["loglike"][f] == one["loglike"], (net, N, ra, rf, K)
            np.testing.assert_array_equal(bat["loglike_history"][f], one["loglike_history"])
            np.testing.assert_array_equal(bat["ess"][f], one["ess"])
            np.testing.assert_array_equal(bat["state_est"][f].reshape(one["state_est"].shape), one["state_est"])


BASE3 = [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"R": 1, "I": 1}, {"S": 1, "I": 1}, "beta"), ({"R": 1}, {"S": 1}, "rho")]


def net3(B, reactions, noise):
    return B.models.reaction_network(("S", "I", "R"), reactions, x0=(300, 160, 40), observe=[{"I": 0.05}, {"R": 0.2, "I": 0.01}], method="euler_multinomial", leaps=4,
                                     noise=noise)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_zero_rate_reaction_and_group_identities(B, ctx, algorithm):
    """an appended zero-rate reaction (with noise of its own or without) moves no key; the group {"beta": s} over reactions 0 and 2 differs
    from {0: s, 2: s} (two leaders, separate draws) and equals {0: s} where reaction 2 has rate 0 either way (its weight multiplies 0)"""
    y = NETS["loop3"][2]
    par = dict(beta=0.004, gamma=0.5, rho=3.2)
    kw = dict(resample_algorithm="SISAR", obs_times=OT, seed=8, stream=3)
    for N in (385, 2561):                                  # (one odd block, two blocks)
        ref = run(B, net3(B, BASE3, {"beta": 0.5}), algorithm, y, N, ctx, par, **kw)
        assert np.isfinite(ref["loglike"])
        same(ref, run(B, net3(B, BASE3 + [({"S": 1}, {"R": 1}, 0.0)], {"beta": 0.5}), algorithm, y, N, ctx, par, **kw))
        same(ref, run(B, net3(B, BASE3 + [({"S": 1}, {"R": 1}, 0.0), ({}, {"I": 1}, 0.0)], {"beta": 0.5, 5: 2.0}), algorithm, y, N, ctx, par, **kw))
        split = run(B, net3(B, BASE3, {0: 0.5, 2: 0.5}), algorithm, y, N, ctx, par, **kw)
        assert split["loglike"] != ref["loglike"] and not np.array_equal(split["particles_history"], ref["particles_history"])
        # leaders coincide: reaction 2 switched off, so only leader 0's draw matters under either spelling
        off = [BASE3[0], BASE3[1], (BASE3[2][0], BASE3[2][1], 0.0), BASE3[3]]
        same(run(B, net3(B, off, {0: 0.5}), algorithm, y, N, ctx, par, **kw), run(B, net3(B, off, {0: 0.5, 2: 0.5}), algorithm, y, N, ctx, par, **kw))


def test_nothing_else_moved(B, ctx):
    """plain Euler-multinomial, tau-leap and Gillespie outputs after a noisy call on the same context equal those before it; the three
    options are back at 0 after each call, also after a refused one"""
    make, par, y = NETS["loop3"]
    par = dict(par, beta=0.002)
    kw = dict(resample_algorithm="SISAR", obs_times=OT, seed=5, stream=2)
    opts = lambda: tuple(ctx._set_options.get(k, 0) for k in ("rn_method", "rn_leaps", "rn_noise"))  # noqa: E731
    nets = [make(B), make(B, method="tau_leap", leaps=4), make(B, method="euler_multinomial", leaps=4)]
    before = [run(B, m, a, y, N, ctx, par, **kw) for m in nets for a in ("BPF", "APF") for N in (7, 2561)]
    g = noisy(make, B, 4, {"beta": 0.5})
    fns = (g.init_fn, g.transition_fn, g.log_likelihood_fn)
    first = B.bootstrap_filter(y, 100, *fns, ctx=ctx, seed=1, **par)
    assert opts() == (0, 0, 0)
    with pytest.raises(B.BssmError):                                              # (more particles than the context holds)
        B.bootstrap_filter(y, 1 << 16, *fns, ctx=ctx, seed=1, **par)
    assert opts() == (0, 0, 0)
    B.bootstrap_filter_batch(y, 100, *fns, [par] * 2, ctx=ctx)
    assert opts() == (0, 0, 0)
    after = [run(B, m, a, y, N, ctx, par, **kw) for m in nets for a in ("BPF", "APF") for N in (7, 2561)]
    for a, b in zip(before, after):
        same(a, b)
    again = B.bootstrap_filter(y, 100, *fns, ctx=ctx, seed=1, **par)
    for k in ("loglike", "loglike_history", "ess", "state_est", "particles_history"):
        np.testing.assert_array_equal(first[k], again[k], err_msg=k)


# --- 5. pmmh --------------------------------------------------------------------------------------------------------------------------------
def test_pmmh_learns_sigma_on_the_lockstep_path(B):
    m = B.models.reaction_network(("S", "E", "I", "R", "C"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1, "C": 1}, 0.5), ({"I": 1}, {"R": 1}, 0.3)],
                                  x0=(180, 8, 12, 0, 0), observe={"C": 0.8}, counters=("C",), missing="skip", obs="negbin", size=10.0,
                                  method="euler_multinomial", leaps=4, noise={"beta": "sigma_se"})
    assert m.param_order == ("beta", "sigma_se")
    priors = {"beta": B.prior_exponential(100.0), "sigma_se": B.prior_exponential(2.0)}
    init = [dict(beta=0.004, sigma_se=0.3), dict(beta=0.0045, sigma_se=0.4)]
    tc = B.default_tune_control(pilot_m=20, pilot_burn_in=5, pilot_n=100, pilot_reps=3, pilot_proposal_sd=0.05)
    y = np.array([3, 4, np.nan, 5, 6, 6, 8, 7], dtype=np.float64)

    def chains():
        return B.pmmh(B.bootstrap_filter, y, 25, m.init_fn, m.transition_fn, m.log_likelihood_fn, priors, init, 5, num_chains=2,
                      param_transform={k: "log" for k in priors}, tune_control=tc, seed=7, print_result=False, batch_chains=True)

    a, b = chains(), chains()
    assert a["_extras"]["batched"] is True and a["_extras"]["batched_launches"] > 0
    for k in priors:
        ca = np.asarray(a["theta_chain"][k])
        assert np.all(np.isfinite(ca)) and np.all(ca > 0)
        np.testing.assert_array_equal(ca, np.asarray(b["theta_chain"][k]))
    assert len(set(np.asarray(a["theta_chain"]["sigma_se"]).reshape(-1))) > 2


# --- 6. refusals behind the ABI -------------------------------------------------------------------------------------------------------------
def test_refusals_behind_the_abi(B, ctx):
    """What models.reaction_network refuses in Python, refused again by bssm_pf_run and bssm_pf_run_batch with BSSM_ERR_ARG: `call` hands the
    library a block of its own making under the options as a C caller might set them"""
    from bayesssm_amd import _lib
    m = noisy(loop3, B, 4, {"beta": 0.5, 2: 0.7})
    par = NETS["loop3"][1]
    y = NETS["loop3"][2]
    o = 3 + 3 + 3 * 4 + 4 * 3 + 2 * 3                       # lead[4], sigma[4]
    good = m.pack(par)
    assert list(good[o:o + 8]) == [0, -1, 2, -1, 0.5, 0.0, 0.7, 0.0]

    def call(block, method, leaps, batch):
        m.pack = lambda params=None: np.array(block, dtype=np.float64)
        m.method, m.leaps = ("euler_multinomial" if method else "tau_leap" if leaps else "gillespie"), (leaps or None)
        saved = m.noise
        if method != 2:
            m.noise = None
        fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
        try:
            if batch:
                return B.bootstrap_filter_batch(y, 64, *fns, [par] * 2, [1, 2], [3, 4], ctx=ctx)
            return B.bootstrap_filter(y, 64, *fns, ctx=ctx, seed=1, **par)
        finally:
            m.noise = saved

    def edit(i, v):
        b = good.copy(); b[o + i] = v
        return b

    for batch in (False, True):
        assert np.all(np.isfinite(np.atleast_1d(call(good, 2, 4, batch)["loglike"])))
        for block, leaps, msg in ((good, 0, "needs rn_leaps = K"), (edit(0, 4.0), 4, "leader"), (edit(2, 1.0), 4, "lowest reaction index"),
                                  (edit(1, 2.0), 4, "lowest reaction index"), (edit(4, 0.0), 4, "sigma must be finite and > 0"),
                                  (edit(6, -0.7), 4, "sigma must be finite and > 0"), (edit(4, float("nan")), 4, "sigma must be finite and > 0"),
                                  (np.concatenate([good[:o], [-1, -1, -1, -1, 0, 0, 0, 0], good[o + 8:]]), 4, "no noise group")):
            with pytest.raises(B.BssmError, match=msg) as e:
                call(block, 2, leaps, batch)
            assert e.value.status == _lib.ERR_ARG
        assert tuple(ctx._set_options.get(k, 0) for k in ("rn_method", "rn_leaps", "rn_noise")) == (0, 0, 0)
    # the qualifier without its method: rn_noise = 1 under tau-leaping and under Gillespie's method
    plain = np.concatenate([good[:o], good[o + 8:]])
    for leaps in (4, 0):
        ctx.set_option("rn_noise", 1)
        try:
            for batch in (False, True):
                m.pack = lambda params=None: plain
                m.method, m.leaps, saved = ("tau_leap" if leaps else "gillespie"), (leaps or None), m.noise
                m.noise = None
                fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
                # (the binding's scope would put rn_noise at 0 for the call: go below it, as a C caller would)
                ctx.set_option("rn_leaps", leaps)
                try:
                    with pytest.raises(B.BssmError, match="needs rn_method = 1"):
                        with _bare_scope(ctx):
                            if batch:
                                B.bootstrap_filter_batch(y, 64, *fns, [par] * 2, [1, 2], [3, 4], ctx=ctx)
                            else:
                                B.bootstrap_filter(y, 64, *fns, ctx=ctx, seed=1, **par)
                finally:
                    ctx.set_option("rn_leaps", 0)
                    m.noise = saved
        finally:
            ctx.set_option("rn_noise", 0)
    lib = _lib.load()
    assert lib.bssm_ctx_set_option(ctx.handle, 16, 2) == _lib.ERR_ARG and "rn_noise takes 0 or 1" in lib.bssm_last_error().decode()


class _bare_scope:
    """for the length of the block Context.rn_method leaves the options as they are on the context (what a C caller sees)"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        import contextlib
        self.saved = type(self.ctx).rn_method
        type(self.ctx).rn_method = lambda self_, method, leaps: contextlib.nullcontext()

    def __exit__(self, *exc):
        type(self.ctx).rn_method = self.saved
        return False
