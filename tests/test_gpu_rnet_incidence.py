"""GPU tests of counter species and missing observations in the reaction-network family (models.reaction_network(counters=,
missing=); rnet.hip.h: k_step_rn's first-step argument, rn_loglik's skip; pf_run_rn, k_pf_batch_rn).  The reference is the numpy
restatement of the definition (tests/rnet_inc_restated.py) at the bars of tests/test_gpu_rnet_limits.py; an invariant of the pure
birth network, the batched = single identity, "a column of NaN = the component dropped", "a row of NaN adds 0.0" and "flagging
nothing changes no bit" need no restatement.  Shapes: N in {7, 2561} (one block; two blocks with a ragged tail), T = 6 with a gap of 1,
a gap of 3, a repeated time and a gap of 3 at the end, one network per register-array size DM (d = 2, 3, 5)."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_inc_restated as RI  # noqa: E402
import rnet_restated as RN  # noqa: E402
from test_gpu_rnet import run, same  # noqa: E402
from test_gpu_rnet_limits import compare_with_restatement, u_res_for  # noqa: E402

pytestmark = pytest.mark.gpu

OT = (1, 2, 5, 5, 6, 9)              # gap 1, gap 1, gap 3, a repeated time, gap 1, gap 3
T = len(OT)
NAN = np.nan


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 15, 8)
    yield c
    c.close()


# --- the three networks, each with two observation components (the counter first) so that a row can be observed in part ----------
def birth2(B, observe=({"C": 0.5}, {"X": 0.1}), **kw):
    """0 -> X + C of order 0: d = 2 (DM = 2)"""
    kw.setdefault("counters", ("C",))
    return B.models.reaction_network(("X", "C"), [({}, {"X": 1, "C": 1}, "b")], x0=(3, 0), observe=list(observe), **kw)


def sir3(B, observe=({"C": 0.7}, {"I": 0.3}), **kw):
    """SIR with the infections counted: d = 3 (DM = 4)"""
    kw.setdefault("counters", ("C",))
    return B.models.reaction_network(("S", "I", "C"), [({"S": 1, "I": 1}, {"I": 2, "C": 1}, "beta"), ({"I": 1}, {}, "gamma")], x0=(60, 6, 0),
                                     observe=list(observe), **kw)


def seir5(B, observe=({"C": 0.6}, {"I": 0.3}), **kw):
    """the README's SEIR with the onsets counted: d = 5 (DM = 8)"""
    kw.setdefault("counters", ("C",))
    return B.models.reaction_network(("S", "E", "I", "R", "C"),
                                     [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1, "C": 1}, "sigma"), ({"I": 1}, {"R": 1}, "gamma")],
                                     x0=(180, 8, 12, 0, 0), observe=list(observe), **kw)


# name: (constructor, parameters, y [T][2] with NaNs, index of the counted reaction, the counter's column,
#        the columns whose sum grows by one with every counted firing and by nothing else, its sign)
NETS = {
    "birth2": (birth2, dict(b=2.0), [[1, 0], [1, 1], [3, NAN], [NAN, 1], [NAN, NAN], [3, 2]], 0, 1, ([0], 1.0)),
    "sir3": (sir3, dict(beta=0.01, gamma=0.3), [[2, 2], [3, NAN], [12, 4], [NAN, 5], [NAN, NAN], [7, 3]], 0, 2, ([0], -1.0)),       # -S
    # (rates below the README's: a third of the events, for the restatement's sake)
    "seir5": (seir5, dict(beta=0.0015, sigma=0.25, gamma=0.1), [[1, 4], [2, NAN], [9, 5], [NAN, 5], [NAN, NAN], [12, 6]], 1, 4, ([2, 3], 1.0)),   # I + R
}
README_PAR = dict(beta=0.004, sigma=0.5, gamma=0.3)


def net(B, name, **kw):
    make, par, y, fired, col, grows = NETS[name]
    return make(B, **kw), par, np.array(y, dtype=np.float64), fired, col, grows


def traced_growth(ph, src, cols, sign, i):
    """per particle, what the columns `cols` gained between observation i - 1 (through the ancestors src) and observation i"""
    return sign * (ph[i][cols].sum(axis=0) - ph[i - 1][cols][:, src].sum(axis=0))


def one_unit_mean(oracle, block, x, col):
    """what the counter holds on average after ONE unit of time from the particles x [d][N] (the restatement's transition, a call
    number no filter run uses)"""
    base, _ = RI.split(block)
    q = RN.unpack(base)
    x = np.array(x, dtype=np.float64)
    x[col] = 0.0
    trans = RN.make(oracle, 1234567, 89)[0]
    return float(trans(q, x, np.full((q["d"], x.shape[1]), 999.0))[col].mean())


# --- 1. against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ra", [(7, "SISAR"), (7, "SISR"), (2561, "SISR")])
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("name", ["birth2", "sir3", "seir5"])
def test_against_the_restatement(B, ctx, oracle, name, algorithm, N, ra):
    """counters and NaNs against the numpy restatement at test_gpu_rnet_limits' bars (log-likelihood and history 1e-6, `resampled`
    equal, and where every ancestor agrees ESS and state estimates at 1e-9 and the integer states -- the counters among them --
    exactly).  The counted reaction fired, and after a gap of 3 the filtered mean counter is above what one unit of time from the
    previous observation's particles holds on average (the restatement's transition): the reset did not happen in mid-gap.
    (Catches, for one: the reset at every step or at none; the second-stage transition of the APF resetting; the flags read at
    o_G; the look-ahead summing a NaN component.)"""
    m, par, y, fired, col, _ = net(B, name, missing="skip")
    block = m.pack(par)
    u = u_res_for(algorithm, T, N, "stratified")
    counts = {}
    t0 = time.perf_counter()
    ref = RI.pf_run_rn(oracle, block, y, N, u, seed=23, stream=4, algorithm=algorithm, counts=counts, resample_algorithm=ra,
                       resample_fn="stratified", obs_times=OT, return_particles=True)
    print("restatement: %.2f s" % (time.perf_counter() - t0), "fired", sorted(counts["fired"].items()))
    assert counts["fired"].get(fired, 0) > 0 and np.isfinite(ref["loglike"])
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm=ra, resample_fn="stratified", obs_times=OT, seed=23, stream=4,
              draws={"u_res": u})
    assert ra != "SISR" or ref["resampled"].all()
    compare_with_restatement(got, ref)
    d = m.dim
    ph = ref["particles_history"].reshape(T + 1, d, N)
    caps = {i: one_unit_mean(oracle, block, ph[i - 1], col) for i in (3, 6)}       # the observations after a gap of 3
    print("mean counter", got["state_est"][:, col], "one unit holds", caps)
    assert all(c > 0 for c in caps.values())
    assert any(got["state_est"][i, col] > caps[i] for i in caps)
    assert np.all(got["particles_history"].reshape(T + 1, d, N)[0] == np.asarray(m.x0)[:, None])      # row 0 is x0


# --- 2. an invariant that needs no restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, 2561])
@pytest.mark.parametrize("name", ["birth2", "sir3", "seir5"])
@pytest.mark.parametrize("ra", ["SIS", "SISR"])
def test_counter_equals_the_growth_since_the_previous_observation(B, ctx, name, ra, N):
    """bootstrap filter with return_particles: the counter of every particle equals, exactly, what the counted reaction added to the
    rest of the state since the previous observation -- X_i - X_{i-1} for the pure birth, S_{i-1} - S_i for the SIR, (I + R)_i -
    (I + R)_{i-1} for the SEIR -- at every observation with gap >= 1, the previous state traced through the returned ancestors
    (SISR; SIS never resamples); at the repeated time the whole state is the previous one's, resampled.  (Catches: a reset in
    mid-gap, none at all, or one at the repeated time.)"""
    m, par, y, _, col, (cols, sign) = net(B, name, missing="skip")
    got = run(B, m, "BPF", y, N, ctx, par, resample_algorithm=ra, resample_fn="systematic", obs_times=OT, seed=3, stream=N)
    assert got["_extras"]["early_return_step"] == 0 and np.isfinite(got["loglike"])
    ph = got["particles_history"].reshape(T + 1, m.dim, N)
    anc, res = got["_extras"]["ancestors"], got["_extras"]["resampled"]
    assert res.all() if ra == "SISR" else not res.any()
    prev_t, kres, grew = 0, 0, 0.0
    for i in range(1, T + 1):
        gap, prev_t = OT[i - 1] - prev_t, OT[i - 1]
        src = np.arange(N)
        if res[i - 1]:
            src = anc[kres] - 1; kres += 1
        if gap >= 1:
            np.testing.assert_array_equal(ph[i, col], traced_growth(ph, src, cols, sign, i), err_msg="observation %d" % i)
            grew += ph[i, col].sum()
        else:
            np.testing.assert_array_equal(ph[i], ph[i - 1][:, src], err_msg="the repeated time")
    assert grew > 0


# --- 3. batched = single ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["birth2", "sir3", "seir5"])
def test_batched_equals_single(B, ctx, name):
    """k_pf_batch_rn = pf_run_rn bit for bit with counters and NaNs at d = 2, 3 and 5: four filters of different rates, seeds and
    streams, N on both sides of batch_literal_max.  (Catches: step_emul_rn resetting at another step than k_step_rn, or not at all.)"""
    m, par, y, _, col, _ = net(B, name, missing="skip")
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    first = list(par)[0]
    pars = [dict(par, **{first: s * par[first]}) for s in (1.0, 1.25, 0.8, 1.1)]
    seeds, streams = [11, 12, 13, 14], [3, 4, 5, 6]
    for N, ra, rf in ((7, "SISR", "systematic"), (385, "SISAR", "stratified"), (1000, "SIS", "stratified")):
        bat = B.bootstrap_filter_batch(y, N, *fns, pars, seeds, streams, obs_times=OT, resample_algorithm=ra, resample_fn=rf, ctx=ctx)
        assert np.all(bat["status"] == 0)
        for f in range(4):
            one = B.bootstrap_filter(y, N, *fns, obs_times=OT, resample_algorithm=ra, resample_fn=rf, ctx=ctx, return_particles=False,
                                     seed=seeds[f], stream=streams[f], **pars[f])
            assert bat["loglike"][f] == one["loglike"] and np.isfinite(one["loglike"]), (name, N, ra, rf, f)
            np.testing.assert_array_equal(bat["loglike_history"][f], one["loglike_history"])
            np.testing.assert_array_equal(bat["ess"][f], one["ess"])
            np.testing.assert_array_equal(bat["state_est"][f], one["state_est"])
            assert bat["n_res_calls"][f] == one["_extras"]["n_res_calls"]
            assert bat["early_return_step"][f] == one["_extras"]["early_return_step"] == 0
        assert np.all(bat["state_est"][:, 3, col] > 0)                  # (the counters count)
    assert len({float(v) for v in bat["loglike"]}) == 4


# --- 4. a column of NaN = the component dropped -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, 2561])
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("name", ["birth2", "sir3", "seir5"])
def test_a_column_of_nan_is_a_dropped_component(B, ctx, name, algorithm, N):
    """y[:, k] all NaN = the same network without component k in `observe` and y, every output bit for bit (the remaining additions
    happen in the same order), for k = 0 and k = 1, single and batched.  (Catches: 0.0 + dpois(NaN, ...) added, lambda of a skipped
    component reaching the sum, a shifted lgamma table.)"""
    make, par, y, _, _, _ = NETS[name]
    y = np.array(y, dtype=np.float64)
    full = make(B, missing="skip")
    observe = [dict(zip([full.species[c] for c in np.flatnonzero(g)], g[np.flatnonzero(g)])) for g in full.G]
    fill = np.array([2.0, 3.0, 4.0, 3.0, 2.0, 5.0])
    for k in (0, 1):
        keep = 1 - k
        col = np.where(np.isnan(y[:, keep]), fill, y[:, keep])          # (the kept column fully observed)
        col[4] = NAN                                                    # ... but for one row, which then has nothing observed
        yk = np.full((T, 2), NAN); yk[:, keep] = col
        kw = dict(resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=31, stream=2)
        a = run(B, full, algorithm, yk, N, ctx, par, **kw)
        less = make(B, observe=[observe[keep]], missing="skip")
        b = run(B, less, algorithm, col, N, ctx, par, **kw)
        assert np.isfinite(a["loglike"]) and a["_extras"]["early_return_step"] == 0
        same(a, b)
        if algorithm == "BPF" and N == 7:
            fa, fb = (full.init_fn, full.transition_fn, full.log_likelihood_fn), (less.init_fn, less.transition_fn, less.log_likelihood_fn)
            ba = B.bootstrap_filter_batch(yk, N, *fa, [par] * 2, 5, [1, 2], obs_times=OT, ctx=ctx)
            bb = B.bootstrap_filter_batch(col, N, *fb, [par] * 2, 5, [1, 2], obs_times=OT, ctx=ctx)
            for key in ("loglike", "loglike_history", "ess", "state_est"):
                np.testing.assert_array_equal(ba[key], bb[key], err_msg=key)


# --- 5. a row of NaN --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, 2561])
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_a_row_of_nan_adds_nothing(B, ctx, algorithm, N):
    """a row with nothing observed (row 5 of every network's y; here the SEIR under SISR): its loglike_history increment is exactly
    0.0 and, the particles having been resampled just before, its ESS is N.  Batched too."""
    m, par, y, _, _, _ = net(B, "seir5", missing="skip")
    assert np.all(np.isnan(y[4]))
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISR", resample_fn="stratified", obs_times=OT, seed=8, stream=1)
    llh = got["loglike_history"]
    print("loglike_history", llh, "ess", got["ess"])
    assert np.isfinite(got["loglike"]) and llh[4] - llh[3] == 0.0 and llh[4] == llh[3]
    assert got["ess"][5] == float(N)
    assert llh[3] != llh[2] and llh[5] != llh[4]
    if algorithm == "BPF":
        bat = B.bootstrap_filter_batch(y, 385, m.init_fn, m.transition_fn, m.log_likelihood_fn, [par] * 2, 8, [1, 2], obs_times=OT,
                                       resample_algorithm="SISR", ctx=ctx)
        assert np.all(bat["loglike_history"][:, 4] == bat["loglike_history"][:, 3]) and np.all(bat["ess"][:, 5] == 385.0)


# --- 6. flagging nothing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, 2561])
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_flagging_nothing_changes_no_bit(B, ctx, algorithm, N):
    """the README's SEIR: counters=() with missing="skip" on a finite y = the call without either argument, every output bit for
    bit (C then is an ordinary species that keeps growing)"""
    ys = {OT: np.array([3, 7, 24, 24, 30, 50], dtype=np.float64), None: np.array([3, 7, 12, 18, 24, 30], dtype=np.float64)}
    old = seir5(B, observe=({"C": 0.6},), counters=())
    new = seir5(B, observe=({"C": 0.6},), counters=(), missing="skip")
    plain = B.models.reaction_network(old.species, [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1, "C": 1}, "sigma"),
                                                    ({"I": 1}, {"R": 1}, "gamma")], x0=(180, 8, 12, 0, 0), observe={"C": 0.6})
    par = README_PAR
    assert np.array_equal(new.pack(par), plain.pack(par))
    for ra, rf, ot in (("SISAR", "stratified", OT), ("SISR", "systematic", None)):
        kw = dict(resample_algorithm=ra, resample_fn=rf, obs_times=ot, seed=19, stream=7)
        y = ys[ot]
        a = run(B, plain, algorithm, y, N, ctx, par, **kw)
        same(a, run(B, old, algorithm, y, N, ctx, par, **kw))
        same(a, run(B, new, algorithm, y, N, ctx, par, **kw))
        assert np.isfinite(a["loglike"]) and a["_extras"]["early_return_step"] == 0
        assert a["state_est"][T, 4] > a["state_est"][1, 4]              # (nothing resets C)


# --- 7. pmmh ----------------------------------------------------------------------------------------------------------------------
def test_pmmh_runs_batched_with_a_counter_and_a_nan(B):
    """pmmh(bootstrap_filter, ...) on the SEIR with the onset counter: 2 chains, 3 iterations, 64 particles in the pilot, one NaN --
    on the lock-step batched path, finite log-likelihoods"""
    m = seir5(B, observe=({"C": 0.6, "S": 0.01},), missing="skip")        # (a small share of S keeps the Poisson mean positive)
    priors = {"beta": B.prior_exponential(100.0), "sigma": B.prior_exponential(1.0), "gamma": B.prior_exponential(1.0)}
    init = [dict(README_PAR), dict(beta=0.0045, sigma=0.45, gamma=0.33)]
    tc = B.default_tune_control(pilot_m=4, pilot_burn_in=1, pilot_n=64, pilot_reps=3, pilot_proposal_sd=0.05)
    y = np.array([5, 6, NAN, 7, 8, 9, 9, 11], dtype=np.float64)
    out = B.pmmh(B.bootstrap_filter, y, 3, m.init_fn, m.transition_fn, m.log_likelihood_fn, priors, init, 1, num_chains=2,
                 param_transform={k: "log" for k in priors}, tune_control=tc, seed=7, print_result=False)
    assert out["_extras"]["batched"] is True and out["_extras"]["batched_launches"] > 0
    for k in priors:
        assert np.all(np.isfinite(np.asarray(out["theta_chain"][k])))
    ll = B.bootstrap_filter_batch(y, 64, m.init_fn, m.transition_fn, m.log_likelihood_fn, init, 7, [1, 2])["loglike"]
    assert np.all(np.isfinite(ll))


# --- 8. the same refusals behind the ABI --------------------------------------------------------------------------------------------
def test_block_check_behind_the_abi(B, ctx):
    """rn_block_check through packed blocks handed to bootstrap_filter_batch: both lengths pass, a tail entry other than 0 / 1 and a
    flagged reactant are refused, as is NaN without the option and +-inf with it"""
    m, par, y, _, _, _ = net(B, "sir3", missing="skip")
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    good = m.pack(par)
    assert np.array_equal(good[-3:], [0, 0, 1])
    ok = B.bootstrap_filter_batch(y, 64, *fns, np.stack([good, good]), 1, [0, 1], obs_times=OT, ctx=ctx)
    assert np.all(ok["status"] == 0) and np.all(np.isfinite(ok["loglike"]))
    half = good.copy(); half[-1] = 0.5
    with pytest.raises(Exception, match="counter flags"):
        B.bootstrap_filter_batch(y, 64, *fns, np.stack([good, half]), 1, [0, 1], obs_times=OT, ctx=ctx)
    react = good.copy(); react[-2] = 1.0                                  # I is a reactant of both reactions
    with pytest.raises(Exception, match="may not be a reactant"):
        B.bootstrap_filter_batch(y, 64, *fns, np.stack([react, react]), 1, [0, 1], obs_times=OT, ctx=ctx)
    from bayesssm_amd import _lib
    import ctypes as C
    lib = _lib.load()
    p_ = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    N = 64

    def call(theta, yv):
        yv = np.ascontiguousarray(yv, dtype=np.float64)
        ot = np.ascontiguousarray(OT, dtype=np.int32)
        se, ess, llh, ll = np.zeros((T + 1, 3)), np.zeros(T + 1), np.zeros(T), np.zeros(1)
        cfg = _lib.PfConfig(_lib.MODEL["rnet"], _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN["stratified"], N, T,
                            float("nan"), p_(theta), int(theta.size), p_(yv), p_(ot), 1, 0, None, None, None, 0, 0, 0.0, None, None)
        res = _lib.PfResult(p_(se), p_(ess), p_(llh), p_(ll), None, None, None, None, None, None, None, None)
        rc = lib.bssm_pf_run(ctx.handle, C.byref(cfg), C.byref(res))
        return rc, lib.bssm_last_error().decode(), float(ll[0])

    rc, msg, _ = call(good, y)                                            # the option is off: NaN refused
    assert rc == _lib.ERR_ARG and "Contains missing values" in msg
    yf = np.where(np.isnan(y), 1.0, y)
    rc, _, ll = call(good, yf)
    assert rc == _lib.OK and np.isfinite(ll)
    assert call(good[:-3], yf)[0] == _lib.OK                              # (today's length)
    rc, msg, _ = call(good[:-1], yf)
    assert rc == _lib.ERR_ARG and "wrong length" in msg
    rc, msg, _ = call(half, yf)
    assert rc == _lib.ERR_ARG and "counter flags" in msg
    rc, msg, _ = call(react, yf)
    assert rc == _lib.ERR_ARG and "may not be a reactant" in msg
    with ctx.mv_y_missing(True):
        rc, _, ll = call(good, y)
        assert rc == _lib.OK and np.isfinite(ll)
        yi = y.copy(); yi[0, 0] = np.inf
        rc, msg, _ = call(good, yi)
        assert rc == _lib.ERR_ARG and "Contains missing values" in msg
