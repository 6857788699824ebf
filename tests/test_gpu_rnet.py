"""GPU tests of the reaction-network family (models.reaction_network, BSSM_MODEL_RNET: rnet.hip.h, pf_run_rn, k_pf_batch_rn).
The pin is bit identity with the built-in SIR model at the SIR instance; padding and permutation carry it to d > 2 and to all
three register-array sizes; the numpy restatement (tests/rnet_restated.py), an exact mean and the batched = single identity
cover what the built-in model cannot."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_restated as RN  # noqa: E402

pytestmark = pytest.mark.gpu

Y_SIR = np.array([76, 89, 93, 101, 117, 120, 135, 128, 140, 139, 131, 150], dtype=np.float64)      # T = 12, counts of I
OBS_TIMES = [1, 2, 2, 4, 5, 6, 7, 9, 10, 11, 12, 13]                                               # a repeated time and two gaps
PAR = dict(lam=0.5, gamma=0.2)


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 15, 8)
    yield c
    c.close()


def sir_net(B, extra_species=0, zero_reaction=False, n_total=500, i0=70):
    """the built-in SIR as a network, optionally padded with species nothing touches and a reaction of rate 0"""
    species = ("S", "I") + tuple("P%d" % k for k in range(extra_species))
    reactions = [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {}, "gamma")]
    if zero_reaction:
        reactions.append(({"S": 1}, {"I": 1}, 0.0))
    return B.models.reaction_network(species, reactions, x0=(n_total - i0, i0) + (3,) * extra_species, observe={"I": 1.0},
                                     build=lambda lam, gamma: {"rates": {"beta": lam / n_total, "gamma": gamma}}, param_names=("lam", "gamma"))


def run(B, m, algorithm, y, N, ctx, par, **kw):
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    if algorithm == "APF":
        return B.auxiliary_filter(y, N, *fns, m.aux_log_likelihood_fn, ctx=ctx, return_ancestors=True, **kw, **par)
    return B.bootstrap_filter(y, N, *fns, ctx=ctx, return_ancestors=True, **kw, **par)


def same(a, b, cols=None):
    """every output of two runs bit for bit; cols: the components of run b (a wider or permuted state) that are run a's"""
    assert a["loglike"] == b["loglike"] or (np.isnan(a["loglike"]) and np.isnan(b["loglike"]))
    for k in ("loglike_history", "ess", "weights_history"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(a["_extras"]["ancestors"], b["_extras"]["ancestors"])
    np.testing.assert_array_equal(a["_extras"]["resampled"], b["_extras"]["resampled"])
    assert a["_extras"]["early_return_step"] == b["_extras"]["early_return_step"]
    sa, sb, pa, pb = a["state_est"], b["state_est"], a["particles_history"], b["particles_history"]
    if cols is not None:
        N = a["weights_history"].shape[1]
        sb = sb[:, cols]
        pb = pb.reshape(pb.shape[0], -1, N)[:, cols].reshape(pb.shape[0], -1)
    np.testing.assert_array_equal(sa, sb, err_msg="state_est")
    np.testing.assert_array_equal(pa, pb, err_msg="particles_history")


SCHEDULES = [("SIS", "stratified", None), ("SISR", "stratified", None), ("SISAR", "stratified", None), ("SISR", "systematic", None),
             ("SISAR", "systematic", OBS_TIMES), ("SISAR", "stratified", OBS_TIMES)]


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("N", [1, 7, 2561])
def test_sir_instance_equals_builtin_sir(B, ctx, N, algorithm):
    """(a) the SIR instance of the family = models.sir(), every output bit for bit"""
    net, sir = sir_net(B), B.models.sir()
    for ra, rf, ot in SCHEDULES:
        kw = dict(resample_algorithm=ra, resample_fn=rf, obs_times=ot, seed=41, stream=2)
        got = run(B, net, algorithm, Y_SIR, N, ctx, PAR, **kw)
        ref = run(B, sir, algorithm, Y_SIR, N, ctx, {"lambda_": 0.5, "gamma": 0.2}, **kw)
        assert np.isfinite(ref["loglike"]) and (N == 1 or ra == "SIS" or ref["_extras"]["n_res_calls"] >= 1)
        same(ref, got)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("N", [1, 7, 2561])
def test_padding_changes_no_bit(B, ctx, N, algorithm):
    """(b) a reaction of rate 0 and species that nothing touches (d = 2 -> 3 -> 5: the three DM instantiations) leave every bit,
    under every schedule of (a)"""
    for ra, rf, ot in SCHEDULES:
        kw = dict(resample_algorithm=ra, resample_fn=rf, obs_times=ot, seed=9, stream=1)
        ref = run(B, sir_net(B), algorithm, Y_SIR, N, ctx, PAR, **kw)
        same(ref, run(B, sir_net(B, zero_reaction=True), algorithm, Y_SIR, N, ctx, PAR, **kw))
        for extra in (1, 3):
            wide = run(B, sir_net(B, extra_species=extra, zero_reaction=True), algorithm, Y_SIR, N, ctx, PAR, **kw)
            same(ref, wide, cols=[0, 1])
            assert np.all(wide["particles_history"][:, 2 * N:] == 3.0)          # (the padded species never move)


SEIR_SPECIES = ("S", "E", "I", "R")


def seir(B, order=SEIR_SPECIES, observe=({"I": 0.6},)):
    x0 = {"S": 180.0, "E": 8.0, "I": 12.0, "R": 0.0}
    return B.models.reaction_network(order, [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"), ({"I": 1}, {"R": 1}, "gamma")],
                                     x0=[x0[s] for s in order], observe=list(observe))


SEIR_PAR = dict(beta=0.004, sigma=0.5, gamma=0.3)
Y_SEIR = np.array([[8, 9], [9, 12], [12, 12], [13, 17], [17, 20], [19, 22], [20, 24], [24, 25]], dtype=np.float64)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("N", [1, 7, 2561])
def test_permuted_species_give_permuted_outputs(B, ctx, N, algorithm):
    """(c) SEIR against the same network with its species permuted (reactions in the same order), under every schedule of (a)"""
    perm = ("I", "R", "S", "E")
    cols = [perm.index(s) for s in SEIR_SPECIES]
    T = Y_SEIR.shape[0]
    for ra, rf, ot in SCHEDULES:
        kw = dict(resample_algorithm=ra, resample_fn=rf, obs_times=None if ot is None else ot[:T], seed=5, stream=N)
        a = run(B, seir(B), algorithm, Y_SEIR[:, 0], N, ctx, SEIR_PAR, **kw)
        b = run(B, seir(B, perm), algorithm, Y_SEIR[:, 0], N, ctx, SEIR_PAR, **kw)
        assert np.isfinite(a["loglike"])
        if N > 1 and (ra == "SISR" or algorithm == "APF"):        # (SISR resamples at every observation, the APF's first stage always)
            assert a["_extras"]["n_res_calls"] >= 1
        same(a, b, cols=cols)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_seir_against_the_restatement(B, ctx, oracle, algorithm):
    """(d) SEIR with a two-component observation against the numpy restatement at the project's T2 bar: log-likelihood 1e-6
    relative; ESS and state estimates 1e-9 where no ancestor flipped"""
    N, T = 385, 8
    m = seir(B, observe=({"I": 0.6}, {"E": 0.5, "I": 0.9}))
    rng = np.random.default_rng(17)
    u = rng.random((2 * T if algorithm == "APF" else T, N))
    got = run(B, m, algorithm, Y_SEIR, N, ctx, SEIR_PAR, resample_algorithm="SISAR", resample_fn="stratified", seed=23, stream=4,
              draws={"u_res": u})
    ref = RN.pf_run_rn(oracle, m.pack(SEIR_PAR), Y_SEIR, N, u, seed=23, stream=4, algorithm=algorithm, resample_algorithm="SISAR",
                       resample_fn="stratified")
    print("loglike", got["loglike"], ref["loglike"])
    assert abs(got["loglike"] - ref["loglike"]) <= 1e-6 * abs(ref["loglike"])
    np.testing.assert_allclose(got["loglike_history"], ref["loglike_history"], rtol=1e-6)
    assert (got["_extras"]["resampled"] == ref["resampled"]).all()
    anc_g, anc_r = got["_extras"]["ancestors"], ref["ancestors"]
    assert anc_g.shape == anc_r.shape
    if np.array_equal(anc_g, anc_r):
        np.testing.assert_allclose(got["ess"], ref["ess"], rtol=1e-9)
        np.testing.assert_allclose(got["state_est"], ref["state_est"], rtol=1e-9, atol=1e-9)
    else:                                           # a flipped ancestor moves one particle: the coarse bar of the other parity tests
        np.testing.assert_allclose(got["ess"], ref["ess"], rtol=1e-6)
        np.testing.assert_allclose(got["state_est"], ref["state_est"], rtol=1e-6, atol=1e-8)


def test_linear_chain_has_the_exact_mean(B, ctx):
    """(e) A -> B -> 0 from (40, 0) with G = 0, y = 0: every log-weight is 0.0, so the SIS state estimate is the sample mean of
    N = 2^14 independent chains.  Each molecule is in A, in B or gone independently, so a component's variance is at most x0 / 4 and
    the mean lies within 6 sqrt(x0 / 4 / N) of expm(M t) x0."""
    N, T, a, b, n0 = 1 << 14, 5, 0.3, 0.2, 40.0
    m = B.models.reaction_network(("A", "B"), [({"A": 1}, {"B": 1}, a), ({"B": 1}, {}, b)], x0=(n0, 0), observe=np.zeros((1, 2)))
    res = B.bootstrap_filter(np.zeros(T), N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SIS", ctx=ctx, seed=3, stream=0)
    assert res["loglike"] == 0.0 and np.all(res["weights_history"] == 1.0 / N)
    t = np.arange(T + 1, dtype=np.float64)
    exact = np.stack([n0 * np.exp(-a * t), n0 * a / (b - a) * (np.exp(-a * t) - np.exp(-b * t))], axis=1)      # expm(M t) x0, M = [[-a, 0], [a, -b]]
    bound = 6.0 * np.sqrt(n0 / 4.0 / N)
    err = np.abs(res["state_est"] - exact)
    print("max error", err.max(axis=0), "bound", bound)
    assert np.all(err <= bound)
    assert np.all(res["particles_history"] == np.floor(res["particles_history"])) and res["particles_history"].min() >= 0


def test_degenerate_weights_return_early(B, ctx, algorithm="BPF"):
    """(f) lambda = 0 with y > 0: every log-weight is -inf, the reference returns at once"""
    m = B.models.reaction_network(("A", "B"), [({"A": 1}, {"B": 1}, 0.5)], x0=(10, 0), observe={"B": 0.0})
    res = run(B, m, algorithm, np.array([0.0, 0.0, 2.0, 0.0]), 100, ctx, {})
    assert res["loglike"] == -np.inf and res["_extras"]["early_return_step"] == 3
    assert np.all(np.isnan(res["state_est"][3:])) and np.all(np.isfinite(res["state_est"][:3]))
    assert res["particles_history"].shape[0] == 3 and np.all(res["ess"][3:] == 0.0)
    bat = B.bootstrap_filter_batch(np.array([0.0, 0.0, 2.0, 0.0]), 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, [{}] * 2, 1, [0, 1])
    assert np.all(bat["loglike"] == -np.inf) and np.all(bat["early_return_step"] == 3) and np.all(np.isnan(bat["state_est"][:, 3:]))


def _net_of_dim(B, d):
    return sir_net(B) if d == 2 else seir(B) if d == 4 else sir_net(B, extra_species=3, zero_reaction=True)


@pytest.mark.parametrize("d", [2, 4, 5])
def test_batched_equals_single(B, ctx, d):
    """(g) k_pf_batch_rn = pf_run_rn bit for bit: N in {1, 7, 385, 1000, capacity}, every schedule, both sides of batch_literal_max"""
    m = _net_of_dim(B, d)
    par = SEIR_PAR if d == 4 else PAR
    y = Y_SEIR[:, 0] if d == 4 else Y_SIR[:8]
    cap = B.batch_max_particles(d, "rnet")
    assert 1000 <= cap <= 2048
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    ot = [1, 2, 2, 4, 5, 6, 7, 9]
    cases = [(1, "SISAR", "stratified", None), (7, "SISR", "systematic", ot), (385, "SISAR", "stratified", ot), (385, "SIS", "stratified", None),
             (1000, "SISR", "stratified", None), (cap, "SISAR", "systematic", None)]
    for lit in (0, 512):                                   # N above / at most batch_literal_max: block scan / in-order sums
        ctx.set_option("batch_literal_max", lit)
        try:
            for N, ra, rf, o in cases:
                pars = [par, dict(par, gamma=0.25)]
                bat = B.bootstrap_filter_batch(y, N, *fns, pars, [11, 12], [3, 4], obs_times=o, resample_algorithm=ra, resample_fn=rf, ctx=ctx)
                assert np.all(bat["status"] == 0)
                for f in range(2):
                    one = B.bootstrap_filter(y, N, *fns, obs_times=o, resample_algorithm=ra, resample_fn=rf, ctx=ctx, return_particles=False,
                                             seed=11 + f, stream=3 + f, **pars[f])
                    assert bat["loglike"][f] == one["loglike"], (d, N, ra, rf, lit)
                    np.testing.assert_array_equal(bat["loglike_history"][f], one["loglike_history"])
                    np.testing.assert_array_equal(bat["ess"][f], one["ess"])
                    np.testing.assert_array_equal(bat["state_est"][f], one["state_est"])
                    assert bat["n_res_calls"][f] == one["_extras"]["n_res_calls"]
        finally:
            ctx.set_option("batch_literal_max", 512)
    with pytest.raises(ValueError, match="bootstrap filter"):
        B.auxiliary_filter_batch(y, 100, *fns, m.aux_log_likelihood_fn, [par] * 2, ctx=ctx)
    with pytest.raises(ValueError, match="at most"):
        B.bootstrap_filter_batch(y, cap + 1, *fns, [par] * 2, ctx=ctx)


def _pmmh(B, wrapper, batch_chains):
    # (a small share of S is counted too: the Poisson mean stays positive when a proposal lets the epidemic die out, so the
    #  auxiliary filter's first-stage weights never are all -inf)
    m = seir(B, observe=({"I": 0.6, "S": 0.01},))
    priors = {"beta": B.prior_exponential(100.0), "sigma": B.prior_exponential(1.0), "gamma": B.prior_exponential(1.0)}
    init = [dict(SEIR_PAR), dict(beta=0.0045, sigma=0.45, gamma=0.33)]
    # (small proposal steps: a wild draw can make the Euler look-ahead's Poisson mean <= 0 for every particle, and the auxiliary
    #  filter's first stage has no early return for all -inf weights -- in the reference neither)
    tc = B.default_tune_control(pilot_m=30, pilot_burn_in=10, pilot_n=100, pilot_reps=5, pilot_proposal_sd=0.05)
    extra = {"aux_log_likelihood_fn": m.aux_log_likelihood_fn} if wrapper is B.auxiliary_filter else {}
    y = np.array([8, 9, 12, 13, 17, 19, 20, 24, 22, 25], dtype=np.float64)
    return B.pmmh(wrapper, y, 40, m.init_fn, m.transition_fn, m.log_likelihood_fn, priors, init, 5, num_chains=2,
                  param_transform={k: "log" for k in priors}, tune_control=tc, seed=7, print_result=False, batch_chains=batch_chains, **extra)


def test_pmmh_lockstep_equals_one_at_a_time(B):
    """(h) pmmh on SEIR (T = 10, m = 40, 2 chains): the lock-step batched path = batch_chains=False; once over auxiliary_filter"""
    a, b = _pmmh(B, B.bootstrap_filter, True), _pmmh(B, B.bootstrap_filter, False)
    for k in ("beta", "sigma", "gamma"):
        np.testing.assert_array_equal(np.asarray(a["theta_chain"][k]), np.asarray(b["theta_chain"][k]))
    assert a["_extras"]["batched"] is True and a["_extras"]["batched_launches"] > 0 and b["_extras"]["batched"] is False
    c = _pmmh(B, B.auxiliary_filter, True)
    assert c["_extras"]["batched"] is False and np.all(np.isfinite(np.asarray(c["theta_chain"]["beta"])))


def test_abi_refusals(B):
    """(i) the C ABI through ctypes: model id 6 with a short block, an n_theta mismatch, the refusals, and a valid call"""
    from bayesssm_amd import _lib
    lib = _lib.load()
    cx = B.Context(0, 4096, 8)
    p_ = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    T, N = 4, 64
    y = np.array([70, 75, 80, 90], dtype=np.float64)
    good = sir_net(B).pack(PAR)

    def call(theta, n_theta=None, algorithm="BPF", rf="stratified", yv=y, z=None, batch=False):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        se, ess, llh, ll = np.zeros((T + 1, 2)), np.zeros(T + 1), np.zeros(T), np.zeros(1)
        nth = int(theta.size if n_theta is None else n_theta)
        cfg = _lib.PfConfig(_lib.MODEL["rnet"], _lib.ALGORITHM[algorithm], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN[rf], N, T, float("nan"),
                            None if batch else p_(theta), nth, p_(yv), None, 1, 0, p_(z), None, None, 0, 0, 0.5, None, None)
        if batch:
            th2 = np.ascontiguousarray(np.stack([theta, theta]))
            st = np.zeros(2, np.int32)
            res = _lib.PfBatchResult(p_(np.zeros(2)), None, None, None, None, None, p_(st), None)
            rc = lib.bssm_pf_run_batch(cx.handle, C.byref(cfg), 2, p_(th2), p_(np.ones(2, np.uint64)), p_(np.arange(2, dtype=np.uint64)), C.byref(res))
        else:
            res = _lib.PfResult(p_(se), p_(ess), p_(llh), p_(ll), None, None, None, None, None, None, None, None)
            rc = lib.bssm_pf_run(cx.handle, C.byref(cfg), C.byref(res))
        return rc, lib.bssm_last_error().decode(), float(ll[0])

    try:
        for batch in (False, True):
            rc, msg, _ = call(good[:2], batch=batch)
            assert rc == _lib.ERR_ARG and "packed parameter block" in msg
            rc, msg, _ = call(good, n_theta=good.size - 1, batch=batch)
            assert rc == _lib.ERR_ARG and "wrong length" in msg
            dimer = good.copy(); dimer[9] = 0.0                                       # s2 of the infection := its s1
            rc, msg, _ = call(dimer, batch=batch)
            assert rc == _lib.ERR_ARG and "s1 == s2" in msg
            for k, v in ((0, 9.0), (0, np.nan), (1, 1e300), (2, -np.inf), (1, 2.5)):      # the header is checked before it is converted
                big = good.copy(); big[k] = v
                rc, msg, _ = call(big, batch=batch)
                assert rc == _lib.ERR_ARG and "1 <= d <= 8" in msg
            for bad in (-1.0, 0.5):
                yb = y.copy(); yb[2] = bad
                rc, msg, _ = call(good, yv=yb, batch=batch)
                assert rc == _lib.ERR_ARG and "Poisson observations must be finite non-negative integers" in msg
            rc, msg, _ = call(good, algorithm="RMPF", batch=batch)
            assert rc == _lib.ERR_ARG and ("no move step" in msg or "bootstrap filter" in msg)
            rc, msg, _ = call(good, rf="multinomial", batch=batch)
            assert rc == _lib.ERR_ARG and "stratified / systematic" in msg
        rc, msg, _ = call(good, algorithm="APF", batch=True)
        assert rc == _lib.ERR_ARG and "bootstrap filter" in msg
        rc, msg, _ = call(good, z=np.zeros(2 * N))
        assert rc == _lib.ERR_ARG and "injected z_" in msg
        rc, msg, ll = call(good)
        assert rc == _lib.OK and np.isfinite(ll) and ll < 0
        assert call(good, batch=True)[0] == _lib.OK
    finally:
        cx.close()
