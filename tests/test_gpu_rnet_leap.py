"""GPU tests of tau-leaping for the reaction networks (models.reaction_network(..., method="tau_leap", leaps=K); rn_rpois,
rn_transition_leap, the RN_TAU_LEAP instantiations of k_step_rn and k_pf_batch_rn, the context option rn_leaps, bssm_dump_rpois).
The reference is the numpy restatement of the definition (tests/rnet_leap_restated.py) on the same Philox blocks, at the bars of
tests/test_gpu_rnet_limits.py; bit-for-bit identities (batched = single, "gillespie" = no keyword, an appended zero-rate reaction),
the option's scope, conservation on the device and pmmh cover the rest."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_leap_restated as LR  # noqa: E402
from test_gpu_rnet import run, same  # noqa: E402
from test_gpu_rnet_limits import (FULL8_OBSERVE, FULL8_PAR, FULL8_REACTIONS, FULL8_SPECIES, FULL8_X0, OT, Y_FULL8,  # noqa: E402
                                  compare_with_restatement, u_res_for)
from test_rnet_leap_cpu import CLOSED_SIR_PAR, LAMS, closed_sir, moment_bars  # noqa: E402

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


# --- the nets: rates under which lam = a_r / K falls on both sides of 10 and the cap is hit, for K = 1 and K = 4 ----------------------
def sir2(B, **kw):
    """the SIR instance (d = 2, DM = 2): infection at beta S I, removal at gamma I > I"""
    return B.models.reaction_network(("S", "I"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {}, "gamma")], x0=(430, 70), observe={"I": 1.0}, **kw)


def sirs3(B, **kw):
    """three live species under DM = 4, p = 2"""
    return B.models.reaction_network(("S", "I", "R"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"R": 1}, {"S": 1}, "rho")],
                                     x0=(40, 6, 4), observe=[{"I": 0.3}, {"S": 0.05, "R": 0.2}], **kw)


def full8(B, **kw):
    """d = R = p = 8 with orders 0, 1 and 2 (test_gpu_rnet_limits' net)"""
    return B.models.reaction_network(FULL8_SPECIES, FULL8_REACTIONS, x0=[FULL8_X0[s] for s in FULL8_SPECIES], observe=FULL8_OBSERVE, **kw)


NETS = {"sir2": (sir2, dict(beta=0.0012, gamma=1.2), np.array([35, 18, 20, 6, 3], dtype=np.float64)),
        "sirs3": (sirs3, dict(beta=0.15, gamma=1.5, rho=0.6), np.array([[5, 2], [6, 3], [5, 3], [4, 4], [3, 3]], dtype=np.float64)),
        "full8": (full8, dict(FULL8_PAR, k0=45.0, k1=0.6, k3=3.0), Y_FULL8)}


def restated(oracle, m, par, y, N, algorithm, K, seed, stream, nb=False, ra="SISAR", rf="stratified", ot=OT):
    u = u_res_for(algorithm, len(y), N, rf)
    counts = {}
    t0 = time.perf_counter()
    ref = LR.pf_run_rn(oracle, m.pack(par), y, N, u, K, nb=nb, seed=seed, stream=stream, algorithm=algorithm, counts=counts, resample_algorithm=ra,
                       resample_fn=rf, obs_times=ot, return_particles=True)
    print("restatement: %.2f s" % (time.perf_counter() - t0), {k: counts[k] for k in LR.KEYS}, "n_inf", counts["n_inf"])
    return ref, counts, u


def every_branch(counts):
    return all(counts[k] > 0 for k in ("inv", "ptrs", "squeeze", "full", "rejected", "cap"))


# --- 0. fails without the feature -------------------------------------------------------------------------------------------------------
def test_tau_leap_runs_and_differs_from_gillespie(B, ctx):
    make, par, y = NETS["sir2"]
    kw = dict(resample_algorithm="SISAR", obs_times=OT, seed=3, stream=1)
    leap = run(B, make(B, method="tau_leap", leaps=4), "BPF", y, 385, ctx, par, **kw)
    gill = run(B, make(B), "BPF", y, 385, ctx, par, **kw)
    assert np.isfinite(leap["loglike"]) and np.isfinite(gill["loglike"])
    assert leap["loglike"] != gill["loglike"]
    assert not np.array_equal(leap["particles_history"], gill["particles_history"])
    assert not np.array_equal(leap["state_est"], gill["state_est"])
    ph = leap["particles_history"]
    assert np.all(ph == np.floor(ph)) and ph.min() >= 0


# --- 1. the sampler against its restatement ---------------------------------------------------------------------------------------------
MIXED = np.tile(np.array([0.0, 0.5, 9.5, 10.0, 10.5, 1e6, 0.0, 3.0, 57.5, 9.999999, 1e6, 12.0, -1.0, 2.0, 40.0, 1e6]), 8)      # two waves of 64


def test_sampler_equals_its_restatement(B, ctx, oracle):
    """bssm_dump_rpois against rnet_leap_restated.sample: n = 4096 draws per lam of the CPU test's list and a vector of mixed lam within
    a wave (zeros, both sides of 10, 1e6).  Equal except for at most 1 draw in 10^4 (a last-bit difference between the device's and
    the host's exp / log / lgamma at an accept boundary is the only admitted cause); the device's draws meet the CPU test's moment
    bars; the inputs reach every branch, a rejection included."""
    n, total, differ = 4096, 0, 0
    counts = LR.new_counts()
    for k, lam in enumerate(LAMS):
        key = dict(seed=500 + k, stream=2, call=k, leap=100 * k, r=k % 8)
        got = B.dump_rpois(np.full(n, lam), ctx=ctx, **key)
        ref = LR.sample(oracle, key["seed"], key["stream"], key["call"], key["leap"], key["r"], np.full(n, lam), counts)
        total, differ = total + n, differ + int(np.sum(got != ref))
        em, ev = moment_bars(got, lam)
        print("lam", lam, "differing", int(np.sum(got != ref)), "mean", got.mean(), "var", got.var(), "errors in s.e.", em, ev)
        assert np.all(got == np.floor(got)) and got.min() >= 0
        assert em <= 5.0 and ev <= 5.0
    got = B.dump_rpois(MIXED, seed=11, stream=5, call=3, leap=1023, r=7, ctx=ctx)
    ref = LR.sample(oracle, 11, 5, 3, 1023, 7, MIXED, counts)
    total, differ = total + MIXED.size, differ + int(np.sum(got != ref))
    assert np.all(got[~(MIXED > 0)] == 0.0)
    print("differing draws: %d of %d" % (differ, total), counts)
    assert differ * 10000 <= total
    assert all(counts[k] > 0 for k in ("zero", "inv", "ptrs", "squeeze", "full", "rejected")) and counts["fallback"] == 0


# --- 2. filters against the restatement ---------------------------------------------------------------------------------------------------
# every N with both filters, every net with both K; (385, 2561: one odd block and two blocks)
CASES = [("sir2", "BPF", 1, 1), ("sir2", "APF", 7, 4), ("sir2", "BPF", 385, 4), ("sir2", "APF", 385, 1), ("sir2", "APF", 2561, 1),
         ("sirs3", "APF", 1, 4), ("sirs3", "BPF", 7, 1), ("sirs3", "APF", 385, 1), ("sirs3", "BPF", 385, 4), ("sirs3", "BPF", 2561, 4),
         ("full8", "BPF", 1, 4), ("full8", "APF", 7, 1), ("full8", "BPF", 385, 1), ("full8", "APF", 385, 4), ("full8", "BPF", 2561, 1),
         # the auxiliary filter across a block boundary under DM = 4 and DM = 8 (the instantiations that keep spilled VGPRs)
         # (full8 at K = 4 here would spend 5 s in the restatement; APF / 385 / 4 above runs that kernel)
         ("sirs3", "APF", 2561, 4), ("full8", "APF", 2561, 1)]


@pytest.mark.parametrize("net,algorithm,N,K", CASES)
def test_filters_against_the_restatement(B, ctx, oracle, net, algorithm, N, K):
    """BPF and APF with K leaps against the numpy restatement on OT = 1, 2, 2, 4, 5 (a repeated time, a gap) at
    test_gpu_rnet_limits' bars: where every ancestor agrees the integer states are equal exactly.  From N = 385 on the restatement's
    counts show lam on both sides of 10, squeeze and full-test accepts, a rejection and cap hits."""
    make, par, y = NETS[net]
    m = make(B, method="tau_leap", leaps=K)
    # (with 1 or 7 particles a filter ends early once every particle has lost the species that y counts: under seed 39 the restatement
    #  runs through all five observations in each of the six small cases -- compare_with_restatement asks for that)
    seed = 23 if N >= 385 else 39
    ref, counts, u = restated(oracle, m, par, y, N, algorithm, K, seed=seed, stream=4)
    assert np.isfinite(ref["loglike"]) and ref["early_return_step"] == 0
    if N >= 385:
        assert every_branch(counts), counts
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=seed, stream=4, draws={"u_res": u})
    compare_with_restatement(got, ref)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_everything_together_against_the_restatement(B, ctx, oracle, algorithm):
    """a counter, a rate schedule whose entries all differ, missing="skip" with a NaN, and obs="negbin", with K = 4"""
    N, K = 385, 4
    sched = 0.6 + 0.05 * np.arange(5 * 3, dtype=np.float64).reshape(5, 3)
    assert len(set(sched.reshape(-1))) == sched.size
    m = B.models.reaction_network(("S", "I", "R", "C"), [({"S": 1, "I": 1}, {"I": 2, "C": 1}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"R": 1}, {"S": 1}, "rho")],
                                  x0=(40, 6, 4, 0), observe=[{"C": 0.5}, {"I": 0.3, "R": 0.1}], counters=("C",), rate_schedule=sched, missing="skip",
                                  obs="negbin", size=(2.0, 15.0), method="tau_leap", leaps=K)
    par = NETS["sirs3"][1]
    y = np.array([[6, 4], [9, np.nan], [16, 3], [np.nan, 5], [7, 4]], dtype=np.float64)
    ref, counts, u = restated(oracle, m, par, y, N, algorithm, K, seed=41, stream=6, nb=True)
    assert np.isfinite(ref["loglike"]) and counts["inv"] > 0 and counts["ptrs"] > 0 and counts["cap"] > 0 and len(counts["rows"]) > 0
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=41, stream=6, draws={"u_res": u})
    compare_with_restatement(got, ref)
    ph = got["particles_history"].reshape(len(y) + 1, 4, N)
    assert np.all(ph[:, :3].sum(axis=1) == 50.0) and ph.min() >= 0           # (the counter aside, the net is closed)


# --- 3. bit-for-bit identities ------------------------------------------------------------------------------------------------------------
def bd1(B, **kw):
    return B.models.reaction_network(("A",), [({}, {"A": 1}, "b"), ({"A": 1}, {}, "m")], x0=(12.0,), observe={"A": 0.5}, **kw)


BATCH_NETS = {1: (bd1, dict(b=30.0, m=1.5), np.array([5, 13, 3, 7, 1], dtype=np.float64)), 3: NETS["sirs3"], 8: NETS["full8"]}


@pytest.mark.parametrize("d", [1, 3, 8])
def test_batched_equals_single(B, ctx, d):
    """k_pf_batch_rn<.., RN_TAU_LEAP> = pf_run_rn under rn_leaps bit for bit: N in {1, 7, 385, 1000, capacity}, three different parameter
    draws, seeds and streams per launch, SIS / SISR / SISAR, with the repeated observation time and the gap"""
    make, par, y = BATCH_NETS[d]
    cap = B.batch_max_particles(d, "rnet")
    assert 1000 < cap <= 2048
    first = list(par)[0]
    pars = [par, dict(par, **{first: 1.2 * par[first]}), dict(par, **{first: 0.7 * par[first]})]
    cases = [(1, "SISAR", "stratified", 4), (7, "SISR", "systematic", 1), (385, "SISAR", "stratified", 4), (385, "SIS", "stratified", 1),
             (1000, "SISR", "stratified", 4), (cap, "SISAR", "systematic", 1)]
    for N, ra, rf, K in cases:
        m = make(B, method="tau_leap", leaps=K)
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


@pytest.mark.parametrize("net", ["sir2", "full8"])
def test_gillespie_keyword_changes_no_bit(B, ctx, net):
    """method="gillespie" = no keyword on every output of BPF, APF and the batched filter"""
    make, _, y = NETS[net]
    par = dict(beta=0.001, gamma=0.2) if net == "sir2" else FULL8_PAR            # (Gillespie's cost grows with the rates)
    a, b = make(B), make(B, method="gillespie")
    for algorithm in ("BPF", "APF"):
        for N in (7, 2561):
            kw = dict(resample_algorithm="SISAR", obs_times=OT, seed=5, stream=N)
            same(run(B, a, algorithm, y, N, ctx, par, **kw), run(B, b, algorithm, y, N, ctx, par, **kw))
    out = [B.bootstrap_filter_batch(y, 385, m.init_fn, m.transition_fn, m.log_likelihood_fn, [par] * 2, [1, 2], [3, 4], obs_times=OT, ctx=ctx) for m in (a, b)]
    for k in ("loglike", "loglike_history", "ess", "state_est", "n_res_calls"):
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_appended_zero_rate_reaction_changes_no_bit(B, ctx, algorithm):
    """the draw keys stride over RNR = 8, not R: a reaction of rate 0 behind the others draws nothing and moves no key"""
    _, par, y = NETS["sirs3"]
    base = [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"R": 1}, {"S": 1}, "rho")]
    nets = [B.models.reaction_network(("S", "I", "R"), base + extra, x0=(40, 6, 4), observe=[{"I": 0.3}, {"S": 0.05, "R": 0.2}], method="tau_leap", leaps=4)
            for extra in ([], [({"S": 1}, {"R": 1}, 0.0)], [({"S": 1}, {"R": 1}, 0.0), ({}, {"I": 1}, 0.0)])]
    for N in (7, 2561):
        kw = dict(resample_algorithm="SISAR", obs_times=OT, seed=8, stream=N)
        ref = run(B, nets[0], algorithm, y, N, ctx, par, **kw)
        assert np.isfinite(ref["loglike"])
        for other in nets[1:]:
            same(ref, run(B, other, algorithm, y, N, ctx, par, **kw))


def test_option_scope_and_other_families(B, ctx):
    """the option rn_leaps is back at its previous value after a call and after a call that raised; a value left on the context by
    hand changes nothing for another family, and a Gillespie descriptor still runs Gillespie's method"""
    make, par, y = NETS["sir2"]
    m = make(B, method="tau_leap", leaps=4)
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    assert ctx._set_options.get("rn_leaps", 0) == 0
    leap = B.bootstrap_filter(y, 100, *fns, ctx=ctx, seed=1, **par)
    assert ctx._set_options.get("rn_leaps", 0) == 0
    with pytest.raises(B.BssmError):                                          # (more particles than the context holds)
        B.bootstrap_filter(y, 1 << 16, *fns, ctx=ctx, seed=1, **par)
    assert ctx._set_options.get("rn_leaps", 0) == 0
    B.bootstrap_filter_batch(y, 100, *fns, [par] * 2, ctx=ctx)
    assert ctx._set_options.get("rn_leaps", 0) == 0
    with pytest.raises(B.BssmError, match="rn_leaps takes 0"):
        ctx.set_option("rn_leaps", 1025)
    lg = B.models.linear_gaussian()
    lgp = dict(phi=0.8, sigma_x=1.0, sigma_y=0.5)
    yl = np.array([0.1, -0.4, 0.3, 1.2, 0.7])
    gil = make(B)
    gfn = (gil.init_fn, gil.transition_fn, gil.log_likelihood_fn)
    gpar = dict(beta=0.001, gamma=0.2)
    before = B.bootstrap_filter(yl, 1000, lg.init_fn, lg.transition_fn, lg.log_likelihood_fn, ctx=ctx, seed=2, **lgp)
    gbefore = B.bootstrap_filter(y, 100, *gfn, ctx=ctx, seed=1, **gpar)
    ctx.set_option("rn_leaps", 4)
    try:
        after = B.bootstrap_filter(yl, 1000, lg.init_fn, lg.transition_fn, lg.log_likelihood_fn, ctx=ctx, seed=2, **lgp)
        gafter = B.bootstrap_filter(y, 100, *gfn, ctx=ctx, seed=1, **gpar)
        assert ctx._set_options["rn_leaps"] == 4
        again = B.bootstrap_filter(y, 100, *fns, ctx=ctx, seed=1, **par)
        assert ctx._set_options["rn_leaps"] == 4
    finally:
        ctx.set_option("rn_leaps", 0)
    for k in ("loglike", "loglike_history", "ess", "state_est", "particles_history"):
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
        np.testing.assert_array_equal(gbefore[k], gafter[k], err_msg=k)
        np.testing.assert_array_equal(leap[k], again[k], err_msg=k)


# --- 4. conservation on the device --------------------------------------------------------------------------------------------------------
def test_closed_sir_conserves_on_the_device(B, ctx):
    """the closed SIR of the CPU test at the rate where the restatement showed cap hits: every particle keeps S + I + R exactly and no
    component is negative, at N = 2561 (two blocks) over 8 observations.  (Under the auxiliary filter the look-ahead's Euler mean of I
    is negative for every particle at this removal rate: its first stage has no weights to resample from.)"""
    N, m = 2561, closed_sir(B, method="tau_leap", leaps=1)
    y = np.array([4, 6, 2, 0, 5, 3, 1, 0], dtype=np.float64)
    got = run(B, m, "BPF", y, N, ctx, CLOSED_SIR_PAR, resample_algorithm="SISAR", obs_times=[1, 2, 2, 4, 5, 6, 7, 8], seed=9, stream=2)
    ph = got["particles_history"].reshape(len(y) + 1, 3, N)
    assert got["_extras"]["early_return_step"] == 0
    assert np.all(ph == np.floor(ph)) and np.all(ph.sum(axis=1) == 72.0) and ph.min() >= 0.0
    assert (ph[-1, 2] > 0).all()


# --- 5. pmmh --------------------------------------------------------------------------------------------------------------------------------
def _pmmh(B, m, batch_chains):
    priors = {"beta": B.prior_exponential(100.0), "sigma": B.prior_exponential(1.0), "gamma": B.prior_exponential(1.0)}
    init = [dict(beta=0.004, sigma=0.5, gamma=0.3), dict(beta=0.0045, sigma=0.45, gamma=0.33)]
    tc = B.default_tune_control(pilot_m=20, pilot_burn_in=5, pilot_n=100, pilot_reps=3, pilot_proposal_sd=0.05)
    y = np.array([8, 9, 12, 13, 17, 19, 20, 24], dtype=np.float64)
    return y, B.pmmh(B.bootstrap_filter, y, 25, m.init_fn, m.transition_fn, m.log_likelihood_fn, priors, init, 5, num_chains=2,
                     param_transform={k: "log" for k in priors}, tune_control=tc, seed=7, print_result=False, batch_chains=batch_chains)


def test_pmmh_lockstep_equals_one_at_a_time(B, monkeypatch):
    """an SEIR with tau_leap: the lock-step batched path = batch_chains=False draw for draw, and the log-likelihoods the batched path
    handed to the accept / reject step equal bootstrap_filter's for the same draw, seed and stream"""
    import bayesssm_amd.filters as filters
    m = B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"), ({"I": 1}, {"R": 1}, "gamma")],
                                  x0=(180, 8, 12, 0), observe={"I": 0.6, "S": 0.01}, method="tau_leap", leaps=4)
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
    # the same chains under Gillespie's method differ: the keyword reached the filters
    g = B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"), ({"I": 1}, {"R": 1}, "gamma")],
                                  x0=(180, 8, 12, 0), observe={"I": 0.6, "S": 0.01})
    _, c = _pmmh(B, g, True)
    assert not np.array_equal(np.asarray(a["theta_chain"]["beta"]), np.asarray(c["theta_chain"]["beta"]))
