"""GPU tests of Euler-multinomial leaps for the reaction networks (models.reaction_network(..., method="euler_multinomial", leaps=K);
rn_rbinom, rn_transition_em, the RN_EULER_MULTINOM instantiations of k_step_rn and k_pf_batch_rn, the context option rn_method,
bssm_dump_rbinom).  The reference is the numpy restatement of the definition (tests/rnet_em_restated.py) on the same Philox blocks, at the
bars of tests/test_gpu_rnet_limits.py; bit-for-bit identities (batched = single, the other methods with the option machinery in place, an
appended zero-rate reaction), the option's scope, conservation on the device, pmmh and the refusals behind the ABI cover the rest."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_em_restated as ER  # noqa: E402
from test_gpu_rnet import run, same  # noqa: E402
from test_gpu_rnet_limits import OT, compare_with_restatement, u_res_for  # noqa: E402
from test_rnet_em_cpu import BINOMS, binom_moment_bars  # noqa: E402
from test_rnet_leap_cpu import closed_sir  # noqa: E402

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


# --- the nets.  Rates and populations are chosen so that, for K = 1 and K = 4 alike, the restatement's counts from N = 385 on show every
# branch of the sampler: a hazard H / K >= 37 somewhere (pe rounds to 1.0: q >= 1), a q in (0.5, 1) (the flip), n qq on both sides of 10
# (inversion; BTRS with squeeze accepts, full-test accepts and rejections), and -- where the net has a sourceless reaction -- Poisson draws.
# Every removal hazard of an observed species stays below 1, so the look-ahead's Euler mean keeps the auxiliary filter alive. -------------
def sir2(B, **kw):
    """the two-reaction SIR (d = 2, DM = 2).  Three infectious among 3000: the first leap's infection hazard is 3 beta / K (a flip on
    n = 3000), from the second on it is about 1500 beta / K or more (everybody left is infected: q >= 1); the three infectious draw their
    removal by inversion, the thousands after them by BTRS"""
    return B.models.reaction_network(("S", "I"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {}, "gamma")], x0=(3000, 3), observe={"I": 0.01}, **kw)


def loop3(B, **kw):
    """d = 3 under DM = 4, p = 2: two exits compete for I (I -> R, I -> S), and R -> S closes a reinfection loop.  Infection empties S in
    every leap (q >= 1) and the loop refills it; R -> S at rho = 3.2 flips for K = 1 and 4; I -> S at delta = 0.05 draws by inversion"""
    return B.models.reaction_network(("S", "I", "R"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"I": 1}, {"S": 1}, "delta"),
                                                       ({"R": 1}, {"S": 1}, "rho")],
                                     x0=(300, 160, 40), observe=[{"I": 0.05}, {"R": 0.2, "I": 0.01}], **kw)


EM8_SPECIES = tuple("ABCDEFGH")
EM8_REACTIONS = [({}, {"A": 1}, "k0"),                          # 0 -> A           order 0 immigration (sourceless)
                 ({"A": 1, "C": 1}, {"B": 1, "C": 1}, "k1"),    # A + C -> B + C   second-order infection, C a catalyst
                 ({"B": 1}, {"C": 1}, "k2"),                    # B -> C
                 ({"C": 1}, {"D": 1}, "k3"),                    # C -> D           two exits compete for C
                 ({"C": 1}, {"E": 1}, "k4"),                    # C -> E
                 ({"D": 1}, {"A": 1}, "k5"),                    # D -> A           the loop
                 ({"F": 1}, {"F": 2}, "k6"),                    # F -> 2 F         catalytic birth (sourceless)
                 ({"F": 1}, {"G": 1, "H": 1}, "k7")]            # F -> G + H
EM8_X0 = (900.0, 20.0, 200.0, 30.0, 5.0, 40.0, 4.0, 2.0)
EM8_PAR = dict(k0=45.0, k1=1.0, k2=0.4, k3=0.5, k4=0.04, k5=3.2, k6=0.3, k7=0.2)
EM8_OBSERVE = [{"A": 0.001, "B": 0.02}, {"B": 0.02}, {"C": 0.02}, {"D": 0.01, "C": 0.02}, {"E": 0.1}, {"F": 0.1}, {"G": 0.2, "F": 0.02}, {"H": 0.2, "F": 0.02}]
Y_EM8 = np.array([[15, 15, 7, 9, 2, 4, 2, 2], [10, 10, 10, 6, 3, 5, 3, 3], [11, 10, 10, 5, 3, 4, 3, 3], [5, 4, 12, 5, 7, 5, 6, 5], [3, 3, 11, 4, 9, 6, 7, 7]], dtype=np.float64)


def em8(B, **kw):
    """d = R = p = 8 (DM = 8): order 0, catalytic birth, second-order infection at a hazard that empties A in every leap"""
    return B.models.reaction_network(EM8_SPECIES, EM8_REACTIONS, x0=EM8_X0, observe=EM8_OBSERVE, **kw)


NETS = {"sir2": (sir2, dict(beta=1.0, gamma=0.5), np.array([24, 15, 16, 6, 3], dtype=np.float64)),
        "loop3": (loop3, dict(beta=1.0, gamma=0.5, delta=0.05, rho=3.2), np.array([[20, 14], [21, 13], [20, 15], [19, 14], [21, 14]], dtype=np.float64)),
        "em8": (em8, EM8_PAR, Y_EM8)}
SOURCELESS = {"sir2": False, "loop3": False, "em8": True}


def restated(oracle, m, par, y, N, algorithm, K, seed, stream, nb=False, ra="SISAR", rf="stratified", ot=OT):
    u = u_res_for(algorithm, len(y), N, rf)
    counts = {}
    t0 = time.perf_counter()
    ref = ER.pf_run_rn(oracle, m.pack(par), y, N, u, K, nb=nb, seed=seed, stream=stream, algorithm=algorithm, counts=counts, resample_algorithm=ra,
                       resample_fn=rf, obs_times=ot, return_particles=True)
    print("restatement: %.2f s" % (time.perf_counter() - t0), {k: counts[k] for k in ER.KEYS}, "n_inf", counts["n_inf"])
    return ref, counts, u


def every_branch(counts, sourceless):
    return all(counts[k] > 0 for k in ("all", "flip", "inv", "btrs", "squeeze", "full", "rejected")) and counts["fallback"] == 0 and (counts["poisson"] > 0) == sourceless


# --- 0. fails without the feature -------------------------------------------------------------------------------------------------------
def test_euler_multinomial_runs_and_differs_from_the_other_methods(B, ctx):
    make, par, y = NETS["loop3"]
    kw = dict(resample_algorithm="SISAR", obs_times=OT, seed=3, stream=1)
    em = run(B, make(B, method="euler_multinomial", leaps=4), "BPF", y, 385, ctx, dict(par, beta=0.002), **kw)
    leap = run(B, make(B, method="tau_leap", leaps=4), "BPF", y, 385, ctx, dict(par, beta=0.002), **kw)
    gill = run(B, make(B), "BPF", y, 385, ctx, dict(par, beta=0.002), **kw)
    ph = em["particles_history"]
    assert np.isfinite(em["loglike"]) and np.all(np.isfinite(em["state_est"]))
    assert np.all(ph == np.floor(ph)) and ph.min() >= 0
    for other in (leap, gill):
        assert np.isfinite(other["loglike"]) and em["loglike"] != other["loglike"]
        assert not np.array_equal(ph, other["particles_history"]) and not np.array_equal(em["state_est"], other["state_est"])


# --- 1. the sampler against its restatement ---------------------------------------------------------------------------------------------
# two waves of 64: zeros, q >= 1, both sides of n qq = 10 and of q = 0.5, n = 10^6
MIXED_N = np.tile(np.array([0.0, 7.0, 19.0, 21.0, 1e6, 1e6, -1.0, 40.0, 1000.0, 1000.0, 1e6, 50.0, 9.0, 25.0, 25.0, 1e6]), 8)
MIXED_Q = np.tile(np.array([0.5, 0.0, 0.5, 0.5, 1e-6, 0.3, 0.5, 0.75, 0.0099, 0.0101, 1.0, 0.98, 1.5, 0.39, 0.41, 0.999995]), 8)


def test_sampler_equals_its_restatement(B, ctx, oracle):
    """bssm_dump_rbinom against rnet_em_restated.sample: 4096 draws per (n, q) of the CPU test's list and a vector of mixed (n, q) within a
    wave.  Equal except for at most 1 draw in 10^4 (a last-bit difference between the device's and the host's exp / log / log1p / lgamma at
    an accept boundary is the only admitted cause); the device's draws meet the CPU test's moment bars and lie in [0, n]; the inputs reach
    every branch, a rejection included, and no draw runs out of attempts."""
    n_draws, total, differ = 4096, 0, 0
    counts = ER.new_counts()
    for i, (n, q) in enumerate(BINOMS):
        key = dict(seed=700 + i, stream=2, call=i, leap=50 * i, r=i % 8)
        got = B.dump_rbinom(np.full(n_draws, n), q, ctx=ctx, **key)
        ref = ER.sample(oracle, key["seed"], key["stream"], key["call"], key["leap"], key["r"], np.full(n_draws, n), q, counts)
        total, differ = total + n_draws, differ + int(np.sum(got != ref))
        em, ev = binom_moment_bars(got, n, q)
        print("n", n, "q", q, "differing", int(np.sum(got != ref)), "mean", got.mean(), "var", got.var(), "errors in s.e.", em, ev)
        assert np.all(got == np.floor(got)) and got.min() >= 0 and got.max() <= n
        assert em <= 5.0 and ev <= 5.0
    got = B.dump_rbinom(MIXED_N, MIXED_Q, seed=11, stream=5, call=3, leap=1023, r=7, ctx=ctx)
    ref = ER.sample(oracle, 11, 5, 3, 1023, 7, MIXED_N, MIXED_Q, counts)
    total, differ = total + MIXED_N.size, differ + int(np.sum(got != ref))
    assert np.all(got[~(MIXED_N > 0) | ~(MIXED_Q > 0)] == 0.0) and np.all(got[(MIXED_N > 0) & (MIXED_Q >= 1)] == MIXED_N[(MIXED_N > 0) & (MIXED_Q >= 1)])
    print("differing draws: %d of %d" % (differ, total), counts)
    assert differ * 10000 <= total
    assert all(counts[k] > 0 for k in ("zero", "all", "flip", "inv", "btrs", "squeeze", "full", "rejected")) and counts["fallback"] == 0


# --- 2. filters against the restatement ---------------------------------------------------------------------------------------------------
# every N with both filters, every net with both K; (385, 2561: one odd block and two blocks); the APF at 2561 under DM = 4 and DM = 8
CASES = [("sir2", "BPF", 1, 1), ("sir2", "APF", 7, 4), ("sir2", "BPF", 385, 4), ("sir2", "APF", 385, 1), ("sir2", "APF", 2561, 1),
         ("loop3", "APF", 1, 4), ("loop3", "BPF", 7, 1), ("loop3", "APF", 385, 1), ("loop3", "BPF", 385, 4), ("loop3", "BPF", 2561, 4),
         ("em8", "BPF", 1, 4), ("em8", "APF", 7, 1), ("em8", "BPF", 385, 1), ("em8", "APF", 385, 4), ("em8", "BPF", 2561, 1),
         ("loop3", "APF", 2561, 4), ("em8", "APF", 2561, 1)]


@pytest.mark.parametrize("net,algorithm,N,K", CASES)
def test_filters_against_the_restatement(B, ctx, oracle, net, algorithm, N, K):
    """BPF and APF with K leaps against the numpy restatement on OT = 1, 2, 2, 4, 5 (a repeated time, a gap) at test_gpu_rnet_limits'
    bars: where every ancestor agrees the integer states are equal exactly.  From N = 385 on the restatement's counts show every branch
    of the sampler (every_branch)."""
    make, par, y = NETS[net]
    m = make(B, method="euler_multinomial", leaps=K)
    ref, counts, u = restated(oracle, m, par, y, N, algorithm, K, seed=23, stream=4)
    assert np.isfinite(ref["loglike"]) and ref["early_return_step"] == 0
    if N >= 385:
        assert every_branch(counts, SOURCELESS[net]), counts
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=23, stream=4, draws={"u_res": u})
    compare_with_restatement(got, ref)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_everything_together_against_the_restatement(B, ctx, oracle, algorithm):
    """a counter, a rate schedule whose entries all differ, missing="skip" with a NaN, and obs="negbin", with K = 4"""
    N, K = 385, 4
    sched = 0.6 + 0.05 * np.arange(5 * 4, dtype=np.float64).reshape(5, 4)
    assert len(set(sched.reshape(-1))) == sched.size
    m = B.models.reaction_network(("S", "I", "R", "C"), [({"S": 1, "I": 1}, {"I": 2, "C": 1}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"I": 1}, {"S": 1}, "delta"),
                                                         ({"R": 1}, {"S": 1}, "rho")],
                                  x0=(300, 160, 40, 0), observe=[{"C": 0.05}, {"I": 0.05, "R": 0.1}], counters=("C",), rate_schedule=sched, missing="skip",
                                  obs="negbin", size=(2.0, 15.0), method="euler_multinomial", leaps=K)
    par = dict(NETS["loop3"][1], beta=0.002)
    y = np.array([[5, 12], [6, np.nan], [7, 12], [np.nan, 11], [5, 10]], dtype=np.float64)
    ref, counts, u = restated(oracle, m, par, y, N, algorithm, K, seed=41, stream=6, nb=True)
    assert np.isfinite(ref["loglike"]) and counts["inv"] > 0 and counts["btrs"] > 0 and counts["flip"] > 0 and len(counts["rows"]) > 0
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=41, stream=6, draws={"u_res": u})
    compare_with_restatement(got, ref)
    ph = got["particles_history"].reshape(len(y) + 1, 4, N)
    assert np.all(ph[:, :3].sum(axis=1) == 500.0) and ph.min() >= 0           # (the counter aside, the net is closed)


# --- 3. bit-for-bit identities ------------------------------------------------------------------------------------------------------------
def bd1(B, **kw):
    return B.models.reaction_network(("A",), [({}, {"A": 1}, "b"), ({"A": 1}, {}, "m")], x0=(12.0,), observe={"A": 0.5}, **kw)


BATCH_NETS = {1: (bd1, dict(b=30.0, m=1.5), np.array([5, 13, 3, 7, 1], dtype=np.float64)), 3: NETS["loop3"], 8: NETS["em8"]}


@pytest.mark.parametrize("d", [1, 3, 8])
def test_batched_equals_single(B, ctx, d):
    """k_pf_batch_rn<.., RN_EULER_MULTINOM> = pf_run_rn under rn_method bit for bit: N in {1, 7, 385, 1000}, three filters of different
    rates, seeds and streams per launch, SIS / SISR / SISAR, with the repeated observation time and the gap"""
    make, par, y = BATCH_NETS[d]
    assert B.batch_max_particles(d, "rnet") > 1000
    first = list(par)[0]
    pars = [par, dict(par, **{first: 1.2 * par[first]}), dict(par, **{first: 0.7 * par[first]})]
    cases = [(1, "SISAR", "stratified", 4), (7, "SISR", "systematic", 1), (385, "SISAR", "stratified", 4), (385, "SIS", "stratified", 1),
             (1000, "SISR", "stratified", 4)]
    for N, ra, rf, K in cases:
        m = make(B, method="euler_multinomial", leaps=K)
        assert m.dim == d
        fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
        bat = B.bootstrap_filter_batch(y, N, *fns, pars, [11, 12, 13], [3, 4, 5], obs_times=OT, resample_algorithm=ra, resample_fn=rf, ctx=ctx)
        assert np.all(bat["status"] == 0)
        if N >= 385:                                       # (the three draws gave three different, finite filters)
            assert len(set(bat["loglike"])) == 3 and np.all(np.isfinite(bat["loglike"]))
        for f in range(3):
            one = B.bootstrap_filter(y, N, *fns, obs_times=OT, resample_algorithm=ra, resample_fn=rf, ctx=ctx, return_particles=False,
                                     seed=11 + f, stream=3 + f, **pars[f])
            assert bat["loglike"][f] == one["loglike"], (d, N, ra, rf, K)
            np.testing.assert_array_equal(bat["loglike_history"][f], one["loglike_history"])
            np.testing.assert_array_equal(bat["ess"][f], one["ess"])
            np.testing.assert_array_equal(bat["state_est"][f].reshape(one["state_est"].shape), one["state_est"])
            assert bat["n_res_calls"][f] == one["_extras"]["n_res_calls"]
            assert bat["early_return_step"][f] == one["_extras"]["early_return_step"]


def test_nothing_else_moved(B, ctx):
    """method="gillespie" and method="tau_leap", leaps=4 give the same outputs bit for bit whether or not an Euler-multinomial call ran
    in between and whatever rn_method was left on the context by hand; rn_method and rn_leaps are back at 0 after each call, also after
    a refused one; another family ignores the option"""
    make, par, y = NETS["loop3"]
    par = dict(par, beta=0.002)                                                   # (Gillespie's cost grows with the rates)
    kw = dict(resample_algorithm="SISAR", obs_times=OT, seed=5, stream=2)
    opts = lambda: (ctx._set_options.get("rn_method", 0), ctx._set_options.get("rn_leaps", 0))  # noqa: E731
    nets = [make(B), make(B, method="gillespie"), make(B, method="tau_leap", leaps=4)]
    lg = B.models.linear_gaussian()
    lgp = dict(phi=0.8, sigma_x=1.0, sigma_y=0.5)
    yl = np.array([0.1, -0.4, 0.3, 1.2, 0.7])
    before = [run(B, m, a, y, N, ctx, par, **kw) for m in nets for a in ("BPF", "APF") for N in (7, 2561)]
    lg_before = B.bootstrap_filter(yl, 1000, lg.init_fn, lg.transition_fn, lg.log_likelihood_fn, ctx=ctx, seed=2, **lgp)
    assert opts() == (0, 0)
    for k in range(4):                                                            # no keyword = "gillespie"
        same(before[k], before[4 + k])
    em = make(B, method="euler_multinomial", leaps=4)
    fns = (em.init_fn, em.transition_fn, em.log_likelihood_fn)
    first = B.bootstrap_filter(y, 100, *fns, ctx=ctx, seed=1, **par)
    assert opts() == (0, 0)
    with pytest.raises(B.BssmError):                                              # (more particles than the context holds)
        B.bootstrap_filter(y, 1 << 16, *fns, ctx=ctx, seed=1, **par)
    assert opts() == (0, 0)
    B.bootstrap_filter_batch(y, 100, *fns, [par] * 2, ctx=ctx)
    assert opts() == (0, 0)
    ctx.set_option("rn_method", 1)                                                # left on the context by hand, with its leaps
    ctx.set_option("rn_leaps", 4)
    try:
        after = [run(B, m, a, y, N, ctx, par, **kw) for m in nets for a in ("BPF", "APF") for N in (7, 2561)]
        lg_after = B.bootstrap_filter(yl, 1000, lg.init_fn, lg.transition_fn, lg.log_likelihood_fn, ctx=ctx, seed=2, **lgp)
        again = B.bootstrap_filter(y, 100, *fns, ctx=ctx, seed=1, **par)
        assert opts() == (1, 4)
    finally:
        ctx.set_option("rn_method", 0)
        ctx.set_option("rn_leaps", 0)
    for a, b in zip(before, after):
        same(a, b)
    for k in ("loglike", "loglike_history", "ess", "state_est", "particles_history"):
        np.testing.assert_array_equal(lg_before[k], lg_after[k], err_msg=k)
        np.testing.assert_array_equal(first[k], again[k], err_msg=k)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_appended_zero_rate_reaction_changes_no_bit(B, ctx, algorithm):
    """the draw keys stride over RNR = 8, not R: reactions of rate 0 behind the others (one with a source, one sourceless) draw nothing and
    move no key"""
    _, par, y = NETS["loop3"]
    base = [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"I": 1}, {"S": 1}, "delta"), ({"R": 1}, {"S": 1}, "rho")]
    nets = [B.models.reaction_network(("S", "I", "R"), base + extra, x0=(300, 160, 40), observe=[{"I": 0.05}, {"R": 0.2, "I": 0.01}], method="euler_multinomial", leaps=4)
            for extra in ([], [({"S": 1}, {"R": 1}, 0.0)], [({"S": 1}, {"R": 1}, 0.0), ({}, {"I": 1}, 0.0)])]
    for N in (7, 2561):
        kw = dict(resample_algorithm="SISAR", obs_times=OT, seed=8, stream=N)
        ref = run(B, nets[0], algorithm, y, N, ctx, par, **kw)
        assert np.isfinite(ref["loglike"])
        for other in nets[1:]:
            same(ref, run(B, other, algorithm, y, N, ctx, par, **kw))


# --- 4. conservation on the device --------------------------------------------------------------------------------------------------------
def test_closed_sir_conserves_on_the_device(B, ctx):
    """the closed SIR of the CPU test: every particle keeps S + I + R exactly and no component is negative at N = 2561 (two blocks), at the
    CPU test's rates over 8 observations and at K = 1 with hazards so large that pe rounds to 1.0 (everybody leaves: the state is known)"""
    N = 2561
    y = np.array([4, 6, 2, 0, 5, 3, 1, 0], dtype=np.float64)
    for K in (1, 4):
        got = run(B, closed_sir(B, method="euler_multinomial", leaps=K), "BPF", y, N, ctx, dict(beta=0.02, gamma=2.5), resample_algorithm="SISAR",
                  obs_times=[1, 2, 2, 4, 5, 6, 7, 8], seed=9, stream=2)
        ph = got["particles_history"].reshape(len(y) + 1, 3, N)
        assert got["_extras"]["early_return_step"] == 0
        assert np.all(ph == np.floor(ph)) and np.all(ph.sum(axis=1) == 72.0) and ph.min() >= 0.0
        assert (ph[-1, 2] > 0).all()
    got = run(B, closed_sir(B, method="euler_multinomial", leaps=1), "BPF", np.array([30.0, 0.0]), N, ctx, dict(beta=50.0, gamma=800.0), resample_algorithm="SIS", seed=9, stream=2)
    ph = got["particles_history"].reshape(3, 3, N)
    assert np.all(ph[1] == np.array([0.0, 60.0, 12.0])[:, None]) and np.all(ph[2] == np.array([0.0, 0.0, 72.0])[:, None])


# --- 5. pmmh --------------------------------------------------------------------------------------------------------------------------------
def _pmmh(B, m, batch_chains):
    priors = {"beta": B.prior_exponential(100.0), "sigma": B.prior_exponential(1.0), "gamma": B.prior_exponential(1.0)}
    init = [dict(beta=0.004, sigma=0.5, gamma=0.3), dict(beta=0.0045, sigma=0.45, gamma=0.33)]
    tc = B.default_tune_control(pilot_m=20, pilot_burn_in=5, pilot_n=100, pilot_reps=3, pilot_proposal_sd=0.05)
    y = np.array([8, 9, 12, 13, 17, 19, 20, 24], dtype=np.float64)
    return y, B.pmmh(B.bootstrap_filter, y, 25, m.init_fn, m.transition_fn, m.log_likelihood_fn, priors, init, 5, num_chains=2,
                     param_transform={k: "log" for k in priors}, tune_control=tc, seed=7, print_result=False, batch_chains=batch_chains)


SEIR = (("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"), ({"I": 1}, {"R": 1}, "gamma")])


def test_pmmh_lockstep_equals_one_at_a_time(B, monkeypatch):
    """an SEIR with euler_multinomial: the lock-step batched path = batch_chains=False draw for draw, and the log-likelihoods the batched
    path handed to the accept / reject step equal bootstrap_filter's for the same draw, seed and stream"""
    import bayesssm_amd.filters as filters
    m = B.models.reaction_network(*SEIR, x0=(180, 8, 12, 0), observe={"I": 0.6, "S": 0.01}, method="euler_multinomial", leaps=4)
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    seen = []
    real = filters.bootstrap_filter_batch

    def recording(y_, n, i_, t_, l_, thetas, seeds, streams, **kw):
        out = real(y_, n, i_, t_, l_, thetas, seeds, streams, **kw)
        seen.append((int(n), np.array(thetas), list(seeds), list(streams), dict(kw), np.array(out["loglike"])))
        return out

    monkeypatch.setattr(filters, "bootstrap_filter_batch", recording)
    y, a = _pmmh(B, m, True)
    n_seen = len(seen)
    _, b = _pmmh(B, m, False)
    assert a["_extras"]["batched"] is True and a["_extras"]["batched_launches"] == n_seen > 0 and b["_extras"]["batched"] is False
    assert len(seen) == n_seen
    for k in ("beta", "sigma", "gamma"):
        np.testing.assert_array_equal(np.asarray(a["theta_chain"][k]), np.asarray(b["theta_chain"][k]))
    assert len(set(np.asarray(a["theta_chain"]["beta"]).reshape(-1))) > 2
    o_k, checked = 3 + m.dim, 0
    for n, thetas, seeds, streams, kw, ll in seen[:2] + seen[-3:]:
        for f in range(thetas.shape[0]):
            extra = {k: v for k, v in kw.items() if k in ("resample_algorithm", "resample_fn") and v is not None}
            one = B.bootstrap_filter(y, n, *fns, obs_times=kw.get("obs_times"), return_particles=False, seed=seeds[f], stream=streams[f],
                                     beta=float(thetas[f, o_k]), sigma=float(thetas[f, o_k + 1]), gamma=float(thetas[f, o_k + 2]), **extra)
            np.testing.assert_array_equal(ll[f], one["loglike"])
            checked += 1
    assert checked >= 5
    # the same chains under tau-leaping differ: the method reached the filters
    g = B.models.reaction_network(*SEIR, x0=(180, 8, 12, 0), observe={"I": 0.6, "S": 0.01}, method="tau_leap", leaps=4)
    _, c = _pmmh(B, g, True)
    assert not np.array_equal(np.asarray(a["theta_chain"]["beta"]), np.asarray(c["theta_chain"]["beta"]))


# --- 6. refusals behind the ABI -------------------------------------------------------------------------------------------------------------
def test_refusals_behind_the_abi(B, ctx):
    """What models.reaction_network refuses in Python, refused again by bssm_pf_run and bssm_pf_run_batch: descriptors built under another
    method carry the block, and `call` rewrites their method and leaps so that the binding sets the two options as a C caller might.  A block
    with two consumed reactants under rn_method = 1, rn_method = 1 with rn_leaps = 0, and an rn_method outside {0, 1} are error returns with
    a message (the checks stand in front of the first device call of the entry points); the same blocks run under the options that fit them,
    and the options are back at 0 afterwards"""
    from bayesssm_amd import _lib
    lib = _lib.load()
    with pytest.raises(B.BssmError, match="rn_method takes 0"):
        ctx.set_option("rn_method", 2)
    assert ctx._set_options.get("rn_method", 0) == 0
    both = B.models.reaction_network(("A", "B", "C"), [({"A": 1, "B": 1}, {"C": 1}, 0.01), ({"C": 1}, {"A": 1}, 0.1)], x0=(50, 40, 0), observe={"C": 1.0})
    fine = B.models.reaction_network(("A", "B", "C"), [({"A": 1, "B": 1}, {"C": 1, "B": 1}, 0.01), ({"C": 1}, {"A": 1}, 0.1)], x0=(50, 40, 0), observe={"C": 1.0})
    y = np.array([3.0, 5.0, 4.0])

    def call(m, method, leaps, batch):
        """bssm_pf_run (batch: bssm_pf_run_batch) on m's block with the two options as given, whatever m's own method says"""
        m.method, m.leaps = ("euler_multinomial" if method else "tau_leap" if leaps else "gillespie"), (leaps or None)
        fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
        if batch:
            return B.bootstrap_filter_batch(y, 64, *fns, [{}] * 2, [1, 2], [3, 4], ctx=ctx)
        return B.bootstrap_filter(y, 64, *fns, ctx=ctx, seed=1)

    for batch in (False, True):
        assert np.all(np.isfinite(np.atleast_1d(call(fine, 1, 4, batch)["loglike"])))
        with pytest.raises(B.BssmError, match="consumes both of its reactants"):
            call(both, 1, 4, batch)
        with pytest.raises(B.BssmError, match="needs rn_leaps = K"):
            call(fine, 1, 0, batch)
        assert np.all(np.isfinite(np.atleast_1d(call(both, 0, 4, batch)["loglike"])))         # (tau-leaping takes the block)
        assert (ctx._set_options.get("rn_method", 0), ctx._set_options.get("rn_leaps", 0)) == (0, 0)
    assert lib.bssm_ctx_set_option(ctx.handle, 15, -1) == _lib.ERR_ARG and "rn_method takes 0" in lib.bssm_last_error().decode()
