"""GPU tests of rate schedules in the reaction-network family (models.reaction_network(rate_schedule=); rnet.hip.h: the rates pointer
of rn_propensities, k_step_rn's krow, k_pf_batch_rn's rows from prev_t + step; pf_run_rn, rn_sched_products, rn_block_check).
A schedule of ones changes no bit; a schedule whose entries all differ is compared with the numpy restatement of the definition
(tests/rnet_tv_restated.py) at the bars of tests/test_gpu_rnet_limits.py; the indicator identity, a closed form, the batched = single
identity, pmmh and the refusals behind the ABI need no restatement."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_tv_restated as RT  # noqa: E402
from test_gpu_rnet import OBS_TIMES, PAR, Y_SIR, run, same  # noqa: E402
from test_gpu_rnet_limits import (FULL8_OBSERVE, FULL8_PAR, FULL8_REACTIONS, FULL8_SPECIES, FULL8_X0, OT, Y_FULL8, compare_with_restatement,  # noqa: E402
                                  u_res_for)
from test_gpu_rnet_incidence import NETS as INC_NETS, OT as OT_INC, seir5  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 16, 8)
    yield c
    c.close()


def pattern(nt, R, f=0):
    """M[tau][r] = 0.5 + ((7 tau + 3 r) mod 11) / 10, every entry of a row and neighbouring rows different; f > 0: offset by a value
    that depends on the filter and on tau"""
    tau, r = np.arange(nt)[:, None], np.arange(R)[None, :]
    return 0.5 + ((7 * tau + 3 * r) % 11) / 10.0 + (((5 * f + 3 * tau) % 7) / 20.0 if f else 0.0)


# --- the networks, each a function of the schedule -----------------------------------------------------------------------------------
def sir2(B, sched=None, n_total=500, i0=70):
    """test_gpu_rnet.sir_net: the built-in SIR as a network"""
    return B.models.reaction_network(("S", "I"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {}, "gamma")], x0=(n_total - i0, i0), observe={"I": 1.0},
                                     build=lambda lam, gamma: {"rates": {"beta": lam / n_total, "gamma": gamma}}, param_names=("lam", "gamma"),
                                     rate_schedule=sched)


def seir_c(B, sched=None):
    """test_gpu_rnet_incidence.seir5: d = 5, R = 3, the onsets counted"""
    return seir5(B, rate_schedule=sched)


def full8(B, sched=None):
    """test_gpu_rnet_limits.full8: d = R = p = 8"""
    return B.models.reaction_network(FULL8_SPECIES, FULL8_REACTIONS, x0=[FULL8_X0[s] for s in FULL8_SPECIES], observe=FULL8_OBSERVE, rate_schedule=sched)


def sirs3(B, sched=None):
    return B.models.reaction_network(("S", "I", "R"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"R": 1}, {"S": 1}, "rho")],
                                     x0=(40, 6, 4), observe=[{"I": 0.3}, {"S": 0.05, "R": 0.2}], rate_schedule=sched)


def bd1(B, sched=None):
    return B.models.reaction_network(("A",), [({}, {"A": 1}, "b"), ({"A": 1}, {}, "m")], x0=(12.0,), observe={"A": 0.5}, rate_schedule=sched)


SEIR_C_PAR = INC_NETS["seir5"][1]
Y_SEIR_C = np.array([[1, 4], [2, 5], [9, 5], [4, 5], [3, 6], [12, 6]], dtype=np.float64)         # T = 6 on OT_INC (last time 9)
Y_SEIR_5 = Y_SEIR_C[:5]                                                                           # T = 5 on OT (last time 5)
# name: (constructor, parameters, y, obs_times)
ONES = {"sir2": (sir2, PAR, Y_SIR, OBS_TIMES), "seir_c": (seir_c, SEIR_C_PAR, Y_SEIR_C, OT_INC), "full8": (full8, FULL8_PAR, Y_FULL8, OT)}


# --- 1. a schedule of ones changes no bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("N", [7, 2561])
@pytest.mark.parametrize("name", ["sir2", "seir_c", "full8"])
def test_ones_change_no_bit(B, ctx, name, N, algorithm):
    """rate_schedule = ones against no schedule, every output of bootstrap_filter / auxiliary_filter bit for bit (k * 1.0 is exact),
    under SISAR with a gap and a repeated time and under SISR without obs_times.  (Catches: the multiplier applied after x[s1]; a
    schedule changing a draw key, the reset or the walk.)"""
    make, par, y, ot = ONES[name]
    for ra, rf, times in (("SISAR", "stratified", ot), ("SISR", "systematic", None)):
        nt = int(times[-1]) if times is not None else len(y)
        kw = dict(resample_algorithm=ra, resample_fn=rf, obs_times=times, seed=19, stream=7)
        a = run(B, make(B), algorithm, y, N, ctx, par, **kw)
        b = run(B, make(B, np.ones((nt, make(B).R))), algorithm, y, N, ctx, par, **kw)
        assert a["_extras"]["early_return_step"] == 0 and np.isfinite(a["loglike"])
        same(a, b)


@pytest.mark.parametrize("N", [7, 1000])
@pytest.mark.parametrize("name", ["sir2", "seir_c", "full8"])
def test_ones_change_no_bit_batched(B, ctx, name, N):
    """the same through k_pf_batch_rn: two filters, SISAR with the gap and the repeated time"""
    make, par, y, ot = ONES[name]
    plain, ones = make(B), make(B, np.ones((int(ot[-1]), make(B).R)))
    outs = [B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, [par] * 2, 5, [1, 2], obs_times=ot, ctx=ctx) for m in (plain, ones)]
    assert np.all(outs[0]["status"] == 0) and np.all(np.isfinite(outs[0]["loglike"]))
    for key in ("loglike", "loglike_history", "ess", "state_est", "n_res_calls", "early_return_step"):
        np.testing.assert_array_equal(outs[0][key], outs[1][key], err_msg=key)


def test_ones_change_no_bit_sisar_gap_and_repeat(B, ctx):
    """SISAR on an obs_times with a gap and a repeated time, where the filter does and does not resample (both nets above ran it too;
    here the decisions are asserted)"""
    m0, m1 = seir_c(B), seir_c(B, np.ones((9, 3)))
    kw = dict(resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT_INC, seed=3, stream=1)
    y = Y_SEIR_C.copy(); y[2, 0] = 20.0                          # (a count that surprises the filter: SISAR resamples there)
    a, b = run(B, m0, "BPF", y, 2561, ctx, SEIR_C_PAR, **kw), run(B, m1, "BPF", y, 2561, ctx, SEIR_C_PAR, **kw)
    same(a, b)
    print("resampled", a["_extras"]["resampled"], "ess", a["ess"])
    assert np.isfinite(a["loglike"]) and a["_extras"]["resampled"].any()


# --- 2. against the restatement ---------------------------------------------------------------------------------------------------
REST = {"seir_c": (seir_c, SEIR_C_PAR, Y_SEIR_5), "full8": (full8, FULL8_PAR, Y_FULL8)}


@pytest.mark.parametrize("N", [385, 2561])
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("name", ["seir_c", "full8"])
def test_against_the_restatement(B, ctx, oracle, name, algorithm, N):
    """a schedule whose entries all differ against the numpy restatement, on OT = 1, 2, 2, 4, 5 (a repeated time, a gap), at
    test_gpu_rnet_limits' bars: log-likelihood and history 1e-6 relative, `resampled` equal, at most 1 ancestor in 1000 different, and
    where none differs ESS and state estimates at 1e-9 and the integer states exactly.  (Catches, for one: row tau instead of
    tau - 1; the APF's second stage or look-ahead at prev_t + 1; the column index r taken modulo something; the row of the gap's
    first step used for the whole gap.)"""
    make, par, y = REST[name]
    T, nt = len(y), OT[-1]
    M = pattern(nt, make(B).R)
    # within a row every entry differs, neighbouring rows differ in every column, and no two rows are equal
    assert all(len(set(row)) == min(M.shape[1], 11) for row in M) and np.all(M[1:] != M[:-1]) and len({tuple(row) for row in M}) == nt
    m = make(B, M)
    u = u_res_for(algorithm, T, N, "stratified")
    counts = {}
    t0 = time.perf_counter()
    ref = RT.pf_run_rn(oracle, m.pack(par), y, N, u, seed=23, stream=4, algorithm=algorithm, counts=counts, resample_algorithm="SISAR",
                       resample_fn="stratified", obs_times=OT, return_particles=True)
    print("restatement: %.2f s" % (time.perf_counter() - t0), "fired", sorted(counts["fired"].items()), "n_inf", counts["n_inf"])
    # the restatement's own inputs, checked here on the CPU: every reaction fires; some but not all particles at -inf (what the
    # ancestor cap assumes); the rows are the definition's
    assert all(counts["fired"].get(r, 0) > 0 for r in range(m.R)), counts["fired"]
    assert np.isfinite(ref["loglike"]) and any(1 <= n <= N - 1 for n in counts["n_inf"])
    rows = counts["rows"]
    assert [r[2] for r in rows if r[0] == "gap"] == [0, 1, 2, 3, 4]                   # the gap 2 -> 4 reads rows 2 and 3, two different ones
    if algorithm == "APF":
        second = [r[2] for r in rows if r[0] == "second"]
        assert second == [t - 1 for t in OT] == [r[2] for r in rows if r[0] == "aux"]
        # at the repeated time (observation 3, time 2) the second stage reads row 1 again -- not row 2, where prev_t + 1 would land --
        # and after the gap it reads row 3, the row of the gap's LAST step
        assert second[2] == second[1] == 1 and second[3] == 3
    else:
        assert all(r[0] == "gap" for r in rows)
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=23, stream=4, draws={"u_res": u})
    compare_with_restatement(got, ref)


# --- 3. the indicator identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, 2561])
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_indicator_columns_equal_a_rate_column(B, ctx, algorithm, N):
    """network A: infection at beta1, infection at beta2, recovery, with the columns 1[tau <= t0], 1[tau > t0] = network B: infection
    at rate 1.0, recovery, with the column beta(tau): every output bit for bit (a zero multiplier gives propensity 0.0, which adds
    nothing to the total, the running sum or the Euler mean).  (Catches: a propensity of a switched-off reaction other than 0.0.)"""
    nt, t0, beta1, beta2, gamma = 13, 5, 0.0011, 0.0004, 0.2
    tau = np.arange(1, nt + 1)
    inf = ({"S": 1, "I": 1}, {"I": 2})
    A = B.models.reaction_network(("S", "I"), [inf + ("beta1",), inf + ("beta2",), ({"I": 1}, {}, "gamma")], x0=(430, 70), observe={"I": 1.0},
                                  rate_schedule={"beta1": (tau <= t0).astype(float), "beta2": (tau > t0).astype(float)})
    Bn = B.models.reaction_network(("S", "I"), [inf + (1.0,), ({"I": 1}, {}, "gamma")], x0=(430, 70), observe={"I": 1.0},
                                   rate_schedule={0: np.where(tau <= t0, beta1, beta2)})
    for ra, rf, ot in (("SISAR", "stratified", OBS_TIMES), ("SISR", "systematic", None)):
        kw = dict(resample_algorithm=ra, resample_fn=rf, obs_times=ot, seed=41, stream=2)
        a = run(B, A, algorithm, Y_SIR, N, ctx, dict(beta1=beta1, beta2=beta2, gamma=gamma), **kw)
        b = run(B, Bn, algorithm, Y_SIR, N, ctx, dict(gamma=gamma), **kw)
        assert a["_extras"]["early_return_step"] == 0 and np.isfinite(a["loglike"])
        same(a, b)
        ph = a["particles_history"].reshape(len(Y_SIR) + 1, 2, N)
        assert (ph[4, 0] < 430).any()                                                 # (infections before t0 ...)
        off = run(B, A, algorithm, Y_SIR, N, ctx, dict(beta1=beta1, beta2=0.0, gamma=gamma), **kw)
        assert not np.array_equal(off["particles_history"], a["particles_history"])   # (... and after it: the second copy matters)


# --- 4. closed form -------------------------------------------------------------------------------------------------------------------
def test_pure_birth_counter_has_the_poisson_mean(B, ctx):
    """0 -> C of order 0 at rate k, C a counter, M[tau][0] = m_tau, G = 0 and y = 0 under SIS: every log-weight is 0.0, so the state
    estimate of C at observation i is the mean of N = 2^16 independent draws of Poisson(lambda_i), lambda_i = sum of k m_tau over
    the gap: within 5 sqrt(lambda_i / N).  Gaps whose rows are all 0.0 give exactly 0.0; the repeated time keeps the estimate."""
    N, k = 1 << 16, 3.0
    mt = np.array([1.0, 0.0, 0.5, 2.0, 1.5, 0.7, 0.0, 0.0, 0.0])
    m = B.models.reaction_network(("C",), [({}, {"C": 1}, "k")], x0=(0,), observe=np.zeros((1, 1)), counters=("C",), rate_schedule=mt[:, None])
    res = B.bootstrap_filter(np.zeros(len(OT_INC)), N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SIS", obs_times=OT_INC,
                             ctx=ctx, seed=3, stream=0, return_particles=False, k=k)
    assert res["loglike"] == 0.0
    se = res["state_est"]
    lam, prev = [], 0
    for t in OT_INC:
        lam.append(k * mt[prev:t].sum() if t > prev else lam[-1])      # (the repeated time: nothing moves, nothing is reset)
        prev = t
    lam = np.array(lam)
    assert np.allclose(lam, [3.0, 0.0, 12.0, 12.0, 2.1, 0.0])
    err, bound = np.abs(se[1:] - lam), 5.0 * np.sqrt(lam / N)
    print("state_est", se, "lambda", lam, "errors", err, "bound", bound)
    assert se[0] == 0.0 and np.all(err <= bound)
    assert se[2] == 0.0 and se[6] == 0.0 and se[4] == se[3] and se[3] > 0


# --- 5. batched = single --------------------------------------------------------------------------------------------------------------
BATCH = {"bd1": (bd1, dict(b=2.0, m=0.25), np.array([5, 13, 3, 7, 1], dtype=np.float64)),
         "sirs3": (sirs3, dict(beta=0.02, gamma=0.4, rho=0.3), np.array([[2, 3], [7, 2], [2, 4], [8, 1], [3, 3]], dtype=np.float64)),
         "full8": (full8, FULL8_PAR, Y_FULL8)}


@pytest.mark.parametrize("name", ["bd1", "sirs3", "full8"])
def test_batched_equals_single(B, ctx, name):
    """k_pf_batch_rn = pf_run_rn bit for bit at d = 1, 3, 8 with six filters whose schedules differ (filter f's entries offset by a
    value depending on f and tau; filter 2 carries a schedule of ones), N in {1, 7, 385, 1000, capacity}, SIS, SISR and SISAR, on
    the obs_times with the repeated time and the gap.  (Catches: a block stride that leaves the schedule out, so that every filter
    reads filter 0's; a row computed from the observation index instead of prev_t + step.)"""
    make, par, y = BATCH[name]
    R, nt, F = make(B).R, OT[-1], 6
    scheds = [np.ones((nt, R)) if f == 2 else pattern(nt, R, f) for f in range(F)]
    assert all(not np.array_equal(scheds[f], scheds[g]) for f in range(F) for g in range(f))
    nets = [make(B, s) for s in scheds]
    blocks = np.stack([m.pack(par) for m in nets])
    assert blocks.shape[1] == make(B).pack(par).size + (0 if make(B).counters else nets[0].dim) + 1 + nt * R
    cap = B.batch_max_particles(nets[0].dim, "rnet")
    assert 1000 <= cap <= 2048
    seeds, streams = [11 + f for f in range(F)], [3 + f for f in range(F)]
    m0 = nets[0]
    ll = set()
    for N in (1, 7, 385, 1000, cap):
        for ra, rf in (("SIS", "stratified"), ("SISR", "systematic"), ("SISAR", "stratified")):
            bat = B.bootstrap_filter_batch(y, N, m0.init_fn, m0.transition_fn, m0.log_likelihood_fn, blocks, seeds, streams, obs_times=OT,
                                           resample_algorithm=ra, resample_fn=rf, ctx=ctx)
            assert np.all(bat["status"] == 0)
            for f, m in enumerate(nets):
                one = B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, obs_times=OT, resample_algorithm=ra, resample_fn=rf,
                                         ctx=ctx, return_particles=False, seed=seeds[f], stream=streams[f], **par)
                assert bat["loglike"][f] == one["loglike"] or (np.isnan(bat["loglike"][f]) and np.isnan(one["loglike"])), (name, N, ra, f)
                np.testing.assert_array_equal(bat["loglike_history"][f], one["loglike_history"])
                np.testing.assert_array_equal(bat["ess"][f], one["ess"])
                np.testing.assert_array_equal(bat["state_est"][f].reshape(one["state_est"].shape), one["state_est"])
                assert bat["n_res_calls"][f] == one["_extras"]["n_res_calls"]
                assert bat["early_return_step"][f] == one["_extras"]["early_return_step"]
                if N >= 385:
                    assert np.isfinite(one["loglike"]), (name, N, ra, f)
            if N == 1000 and ra == "SISAR":
                ll = {float(v) for v in bat["loglike"]}
    assert len(ll) == F                                               # (six different filters)


# --- 6. pmmh ------------------------------------------------------------------------------------------------------------------------
def _pmmh(B, wrapper, batch_chains):
    t0, T = 4, 10

    def build(beta, sigma, gamma, rho):
        col = np.ones(T); col[t0:] = rho                                      # an intervention effect from day t0 + 1
        return {"rates": {"beta": beta, "sigma": sigma, "gamma": gamma}, "rate_schedule": {"beta": col}}

    m = B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                        ({"I": 1}, {"R": 1}, "gamma")], x0=(180, 8, 12, 0), observe={"I": 0.6, "S": 0.01},
                                  build=build, param_names=("beta", "sigma", "gamma", "rho"))
    priors = {"beta": B.prior_exponential(100.0), "sigma": B.prior_exponential(1.0), "gamma": B.prior_exponential(1.0), "rho": B.prior_exponential(1.0)}
    init = [dict(beta=0.004, sigma=0.5, gamma=0.3, rho=0.6), dict(beta=0.0045, sigma=0.45, gamma=0.33, rho=0.7)]
    tc = B.default_tune_control(pilot_m=20, pilot_burn_in=5, pilot_n=100, pilot_reps=3, pilot_proposal_sd=0.05)
    extra = {"aux_log_likelihood_fn": m.aux_log_likelihood_fn} if wrapper is B.auxiliary_filter else {}
    y = np.array([8, 9, 12, 13, 17, 16, 15, 16, 14, 15], dtype=np.float64)
    return B.pmmh(wrapper, y, 25, m.init_fn, m.transition_fn, m.log_likelihood_fn, priors, init, 5, num_chains=2,
                  param_transform={k: "log" for k in priors}, tune_control=tc, seed=7, print_result=False, batch_chains=batch_chains, **extra)


def test_pmmh_lockstep_equals_one_at_a_time(B):
    """pmmh on the SEIR whose `build` returns rate_schedule = rho from day t0 + 1 (rho sampled): the lock-step batched path, every
    draw carrying its own schedule in its block, = batch_chains=False draw for draw; once over auxiliary_filter"""
    a, b = _pmmh(B, B.bootstrap_filter, True), _pmmh(B, B.bootstrap_filter, False)
    for k in ("beta", "sigma", "gamma", "rho"):
        np.testing.assert_array_equal(np.asarray(a["theta_chain"][k]), np.asarray(b["theta_chain"][k]))
    assert a["_extras"]["batched"] is True and a["_extras"]["batched_launches"] > 0 and b["_extras"]["batched"] is False
    assert len(set(np.asarray(a["theta_chain"]["rho"]).reshape(-1))) > 2      # (rho moved: the schedules of the draws differed)
    c = _pmmh(B, B.auxiliary_filter, True)
    assert c["_extras"]["batched"] is False and np.all(np.isfinite(np.asarray(c["theta_chain"]["rho"])))


# --- 7. behind the ABI ----------------------------------------------------------------------------------------------------------------
def test_block_check_behind_the_abi(B, ctx):
    """rn_block_check and the length check of pf_run_rn / pf_run_batch_rn through ctypes: the third length passes; an n_times entry
    that disagrees with n_theta, an n_times short of the last observation time, a negative and a NaN multiplier return BSSM_ERR_ARG,
    single and batched"""
    from bayesssm_amd import _lib
    lib = _lib.load()
    p_ = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    N, T, R, d = 64, len(OT_INC), 3, 5
    nt = OT_INC[-1]
    y = np.ascontiguousarray(Y_SEIR_C)
    good = seir_c(B, pattern(nt, R)).pack(SEIR_C_PAR)
    o_nt = good.size - nt * R - 1
    assert good[o_nt] == nt and np.array_equal(good[o_nt - d:o_nt], [0, 0, 0, 0, 1])

    def single(theta, obs_times=OT_INC):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        ot = np.ascontiguousarray(obs_times, dtype=np.int32)
        se, ess, llh, ll = np.zeros((T + 1, d)), np.zeros(T + 1), np.zeros(T), np.zeros(1)
        cfg = _lib.PfConfig(_lib.MODEL["rnet"], _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN["stratified"], N, T,
                            float("nan"), p_(theta), int(theta.size), p_(y), p_(ot), 1, 0, None, None, None, 0, 0, 0.0, None, None)
        res = _lib.PfResult(p_(se), p_(ess), p_(llh), p_(ll), None, None, None, None, None, None, None, None)
        rc = lib.bssm_pf_run(ctx.handle, C.byref(cfg), C.byref(res))
        return rc, lib.bssm_last_error().decode(), float(ll[0])

    def batched(thetas, obs_times=OT_INC):
        thetas = np.ascontiguousarray(thetas, dtype=np.float64)
        F = thetas.shape[0]
        ot = np.ascontiguousarray(obs_times, dtype=np.int32)
        ll, status = np.zeros(F), np.zeros(F, dtype=np.int32)
        seeds, streams = np.arange(F, dtype=np.uint64) + 1, np.arange(F, dtype=np.uint64)
        cfg = _lib.PfConfig(_lib.MODEL["rnet"], _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN["stratified"], N, T,
                            float("nan"), None, int(thetas.shape[1]), p_(y), p_(ot), 0, 0, None, None, None, 0, 0, 0.0, None, None)
        res = _lib.PfBatchResult(p_(ll), None, None, None, None, None, p_(status), None)
        rc = lib.bssm_pf_run_batch(ctx.handle, C.byref(cfg), F, p_(thetas), p_(seeds), p_(streams), C.byref(res))
        return rc, lib.bssm_last_error().decode(), ll

    rc, _, ll = single(good)
    assert rc == _lib.OK and np.isfinite(ll)
    rc, _, lls = batched(np.stack([good, good]))
    assert rc == _lib.OK and np.all(np.isfinite(lls))
    longer = seir_c(B, pattern(nt + 3, R)).pack(SEIR_C_PAR)              # more rows than the data needs: fine
    assert single(longer)[0] == _lib.OK
    bad_nt = good.copy(); bad_nt[o_nt] = nt - 1                          # the entry disagrees with the length
    frac_nt = good.copy(); frac_nt[o_nt] = nt + 0.5
    nan_nt = good.copy(); nan_nt[o_nt] = np.nan
    for blk in (bad_nt, frac_nt, nan_nt, good[:-1], np.append(good, 1.0), good[:o_nt + 1]):
        rc, msg, _ = single(blk)
        assert rc == _lib.ERR_ARG and "wrong length" in msg, msg
    rc, msg, _ = batched(np.stack([good, bad_nt]))                       # (one cfg->n_theta: a block whose entry disagrees with it)
    assert rc == _lib.ERR_ARG and "wrong length" in msg
    short = seir_c(B, pattern(nt - 1, R)).pack(SEIR_C_PAR)
    rc, msg, _ = single(short)
    assert rc == _lib.ERR_ARG and "short of the last observation time" in msg
    rc, msg, _ = batched(np.stack([short, short]))
    assert rc == _lib.ERR_ARG and "short of the last observation time" in msg
    assert single(short, obs_times=(1, 2, 5, 5, 6, 8))[0] == _lib.OK     # (the same block reaches time 8)
    neg = good.copy(); neg[-4] = -0.25
    rc, msg, _ = single(neg)
    assert rc == _lib.ERR_ARG and "multipliers must be >= 0" in msg
    rc, msg, _ = batched(np.stack([good, neg]))
    assert rc == _lib.ERR_ARG and "multipliers must be >= 0" in msg
    nan = good.copy(); nan[-4] = np.nan
    rc, msg, _ = single(nan)
    assert rc == _lib.ERR_ARG and "non-finite" in msg
    rc, msg, _ = batched(np.stack([nan, good]))
    assert rc == _lib.ERR_ARG and "non-finite" in msg
    half = good.copy(); half[o_nt - 1] = 0.5                             # the counters' flags are still checked in front of a schedule
    rc, msg, _ = single(half)
    assert rc == _lib.ERR_ARG and "counter flags" in msg
