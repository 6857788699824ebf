"""Missing and partially observed y for the multivariate family on the device (models.linear_gaussian_mv(..., missing="skip"); the
context option mv_y_missing through pf_run_mv and k_pf_batch_mv): a NaN in y[i, k] means that component k of observation i was not
observed, and every log-likelihood is the sum over the observed components only.

  1. parity with tests/mv_missing_restated.py on injected draws at tests/test_gpu_mv_obs.py's bar (its _compare, plus the weights
     history at 1e-9): three families x BPF / APF / RMPF x the three register-array sizes; fully missing first / interior / last
     rows, rows with only k = 0 and only k = p - 1 missing; once with time-varying h0 / H; once with every row missing;
  2. a NaN-free y with missing="skip" = the default descriptor, bit for bit;   3. generator run = run on its dump;
  4. batched filters = single runs, bit for bit;   5. the exact Kalman filter with missing data (statistical);
  6. SIS: rows with nothing observed = rows that are not there;   7. closure mode with the mask captured;   8. pmmh;   9. the C ABI.
The shapes are small: a wrong mask, a wrong row or a wrong k shows at any size."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402
import mv_missing_restated as MS  # noqa: E402
import test_gpu_mv_obs as TO  # noqa: E402      (its helpers ARE the bar: _compare, _pieces, _draws, _run, _pmmh, _Closures)

pytestmark = pytest.mark.gpu

T, OT, INCR, N_PAR = TO.T, TO.OT, TO.INCR, TO.N_PAR
FAMILIES = ["gaussian", "poisson", "logvar"]
SHAPES = [(1, 1), (3, 2), (8, 8)]
FULL_ROWS = [0, 4, 7, T - 1]          # nothing observed: the first row, the repeated time (the weight-only launch), an interior row, the last


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    cx = B.Context(0, 1 << 13, 8)
    yield cx
    cx.close()


def _simulate(rng, obs, q, d, p, ot, tv=None):
    if obs != "gaussian":
        return TO._simulate(rng, obs, q, d, p, ot, tv)
    x = q["m0"] + q["L0"] @ rng.standard_normal(d)
    ys, prev = np.zeros((len(ot), p)), 0
    for i, t in enumerate(ot):
        for tau in range(prev + 1, t + 1):
            x = q["A"] @ x + (tv["b"][tau - 1] if tv else q["b"]) + q["L"] @ rng.standard_normal(d)
        prev = t
        ys[i] = ((tv["h0"][i] + tv["H"][i] @ x) if tv else (q["h0"] + q["H"] @ x)) + q["sd"] * rng.standard_normal(p)
    return ys


def _punch(ys, p):
    """the missing pattern of the parity tests: FULL_ROWS with nothing observed; row 3 with only k = 0 missing, row 8 with only
    k = p - 1 missing, and (p > 2) row 6 with two interior components missing.  At p = 1 the two partial kinds are one and the
    same fully missing row, so rows 3 and 8 join the rows with nothing observed there (_full_rows); the partial kinds proper are
    exercised at (3, 2) and (8, 8)."""
    ys = np.array(ys, dtype=np.float64)
    ys[FULL_ROWS] = np.nan
    ys[3, 0] = np.nan
    ys[8, p - 1] = np.nan
    if p > 2:
        ys[6, [2, p - 3]] = np.nan
    return ys


def _full_rows(ys):
    """the rows of a punched y with nothing observed"""
    return [int(i) for i in np.flatnonzero(np.isnan(ys).all(axis=1))]


def _ref(oracle, obs, m, tv, alg, ys, N, dr, ra, rf, ot, **kw):
    tv = tv or {}
    return MS.pf_run_mv_missing(oracle, obs, m.pack({}), ys, N, dr["z_init"], dr["z_trans"], dr["u_res"], b_t=tv.get("b"), h0_t=tv.get("h0"),
                                H_t=tv.get("H"), algorithm=alg, resample_algorithm=ra, resample_fn=rf, obs_times=ot, move_sd=0.3,
                                z_move=dr.get("z_move"), u_move=dr.get("u_move"), **kw)


def _bar(res, ref):
    """tests/test_gpu_mv_obs.py's bar: its _compare, and the weights history at 1e-9"""
    TO._compare(res, ref)
    np.testing.assert_allclose(res["weights_history"], ref["weights_history"], rtol=1e-9, atol=1e-300)


# ---- 1. parity on injected draws --------------------------------------------------------------------------------------------
RA_RF = {(1, 1): ("SISAR", "stratified"), (3, 2): ("SISAR", "systematic"), (8, 8): ("SISR", "stratified")}


@pytest.mark.parametrize("d,p", SHAPES)
@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("obs", FAMILIES)
def test_parity_with_the_restatement_on_injected_draws(B, ctx, oracle, obs, alg, d, p):
    ra, rf = RA_RF[(d, p)]
    rng = np.random.default_rng(1000 * d + 10 * p + FAMILIES.index(obs))
    q = TO._pieces(rng, d, p)
    ys = _punch(_simulate(rng, obs, q, d, p, OT), p)
    dr = TO._draws(rng, alg, N_PAR, d, rf, OT, oracle)
    m = B.models.linear_gaussian_mv(d, p, obs=obs, missing="skip", **q)
    thr = {"threshold": 0.95 * N_PAR} if ra == "SISAR" else {}       # (as in test_gpu_mv_obs.py: SISAR takes both decisions)
    res = TO._run(B, m, alg, ys, N_PAR, obs_times=OT, resample_algorithm=ra, resample_fn=rf, return_particles=True, return_ancestors=True,
                  draws=dr, ctx=ctx, **thr)
    ref = _ref(oracle, obs, m, None, alg, ys, N_PAR, dr, ra, rf, OT, return_particles=True, **thr)
    print("%s %s (%d, %d): loglike %.12g (restated %.12g), ESS min %.1f" % (obs, alg, d, p, res["loglike"], ref["loglike"], res["ess"][1:].min()))
    _bar(res, ref)
    assert res["_extras"]["early_return_step"] == 0 and ref["n_res_calls"] > 0
    assert res["_extras"]["n_res_calls"] == ref["n_res_calls"]
    assert (res["_extras"]["ancestors"][0] == ref["ancestors"][0]).all()                  # the first resampling: bit-exact
    incr = np.diff(np.concatenate([[0.0], res["loglike_history"]]))
    assert _full_rows(ys) == (FULL_ROWS if p > 1 else sorted(FULL_ROWS + [3, 8]))
    for i in _full_rows(ys):                                                              # nothing observed: exactly 0.0, uniform weights
        assert incr[i] == 0.0 and np.all(res["weights_history"][i + 1] == 1.0 / N_PAR), i
    # a kernel that ignored the mask would read the placeholder: the run with 0.0 in place of NaN is another run
    zero = TO._run(B, m, alg, np.where(np.isnan(ys), 0.0, ys), N_PAR, obs_times=OT, resample_algorithm=ra, resample_fn=rf,
                   return_particles=False, draws=dr, ctx=ctx, **thr)
    assert zero["loglike"] != res["loglike"]


@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("obs", FAMILIES)
def test_parity_with_time_varying_h0_and_H(B, ctx, oracle, obs, alg):
    """OT has a gap of 3 and a repeated time; h0 / H are read by observation row, missing or not"""
    d, p = 3, 2
    rng = np.random.default_rng(77 + FAMILIES.index(obs))
    q = TO._pieces(rng, d, p)
    tv = TO._varying(rng, q, d, p, OT[-1])
    ys = _punch(_simulate(rng, obs, q, d, p, OT, tv), p)
    ra, rf = ("SISAR", "stratified") if alg != "RMPF" else ("SISR", "systematic")
    dr = TO._draws(rng, alg, N_PAR, d, rf, OT, oracle)
    m = B.models.linear_gaussian_mv(d, p, obs=obs, time_varying=tv, missing="skip", **q)
    res = TO._run(B, m, alg, ys, N_PAR, obs_times=OT, resample_algorithm=ra, resample_fn=rf, return_particles=True, draws=dr, ctx=ctx)
    ref = _ref(oracle, obs, m, tv, alg, ys, N_PAR, dr, ra, rf, OT, return_particles=True)
    _bar(res, ref)
    flat = _ref(oracle, obs, m, dict(tv, h0=None, H=None), alg, ys, N_PAR, dr, ra, rf, OT)      # (the rows are read: the block's differ)
    assert flat["loglike"] != ref["loglike"]


@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
def test_every_row_missing(B, ctx, oracle, alg):
    """nothing is ever observed: the log-likelihood is exactly 0.0 at every row, the ESS is N, and the filter still runs its whole
    sequence (SISR resamples at every row from uniform weights; the RMPF accepts every proposal)"""
    d, p, obs = 3, 2, "poisson"
    rng = np.random.default_rng(3)
    q = TO._pieces(rng, d, p)
    ys = np.full((T, p), np.nan)
    dr = TO._draws(rng, alg, N_PAR, d, "stratified", OT, oracle)
    m = B.models.linear_gaussian_mv(d, p, obs=obs, missing="skip", **q)
    res = TO._run(B, m, alg, ys, N_PAR, obs_times=OT, resample_algorithm="SISR", resample_fn="stratified", return_particles=True, draws=dr, ctx=ctx)
    ref = _ref(oracle, obs, m, None, alg, ys, N_PAR, dr, "SISR", "stratified", OT, return_particles=True)
    _bar(res, ref)
    assert res["loglike"] == 0.0 and np.all(res["loglike_history"] == 0.0) and np.all(res["ess"][1:] == N_PAR)     # (SISR: ESS = N as resampled)
    assert res["_extras"]["n_res_calls"] == ref["n_res_calls"] >= T and np.all(res["weights_history"] == 1.0 / N_PAR)


# ---- 2. a NaN-free y: the default descriptor, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("obs", FAMILIES)
def test_without_nan_skip_is_the_default_descriptor_bitwise(B, ctx, obs, alg):
    d, p = 3, 2
    rng = np.random.default_rng(5)
    q = TO._pieces(rng, d, p)
    ys = _simulate(rng, obs, q, d, p, OT)
    a, b = [TO._run(B, B.models.linear_gaussian_mv(d, p, obs=obs, **kw, **q), alg, ys, N_PAR, obs_times=OT, resample_algorithm="SISAR",
                    resample_fn="stratified", return_particles=True, return_ancestors=True, seed=11, stream=2, ctx=ctx)
            for kw in ({}, {"missing": "skip"})]
    TO._same_bits(a, b, keys=("loglike_history", "ess", "state_est", "particles_history", "weights_history"))
    np.testing.assert_array_equal(a["_extras"]["ancestors"], b["_extras"]["ancestors"])
    np.testing.assert_array_equal(a["_extras"]["resampled"], b["_extras"]["resampled"])
    if alg == "BPF":
        for N in (7, 777, B.batch_max_particles(d)):
            o0, o1 = [B.bootstrap_filter_batch(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, [m.pack({})] * 3, 4, [0, 1, 2],
                                               obs_times=OT, ctx=ctx)
                      for m in (B.models.linear_gaussian_mv(d, p, obs=obs, **q), B.models.linear_gaussian_mv(d, p, obs=obs, missing="skip", **q))]
            for k in ("loglike", "loglike_history", "ess", "state_est", "early_return_step", "n_res_calls", "status"):
                np.testing.assert_array_equal(o0[k], o1[k], err_msg="%s at N = %d" % (k, N))


# ---- 3. the generator run equals its own dump -------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,obs", [("BPF", "gaussian"), ("APF", "poisson"), ("RMPF", "logvar")])
def test_generator_run_equals_its_dump(B, ctx, alg, obs):
    d, p, N = 3, 2, N_PAR
    rng = np.random.default_rng(21)
    q = TO._pieces(rng, d, p)
    ys = _punch(_simulate(rng, obs, q, d, p, OT), p)
    m = B.models.linear_gaussian_mv(d, p, obs=obs, missing="skip", **q)
    kw = dict(obs_times=OT, resample_algorithm="SISAR", resample_fn="stratified", return_particles=False, ctx=ctx)
    a = TO._run(B, m, alg, ys, N, seed=77, stream=5, **kw)
    dr = B.dump_draws(alg, T, N, "stratified", 77, 5, obs_times=OT, ctx=ctx, dim=d)
    b = TO._run(B, m, alg, ys, N, draws=dr, **kw)
    TO._same_bits(a, b)
    assert a["_extras"]["early_return_step"] == 0 and np.isfinite(a["loglike"])


# ---- 4. batched equals single runs ------------------------------------------------------------------------------------------
PARAMS, SEEDS, STREAMS = TO.PARAMS[:3], TO.SEEDS[:3], TO.STREAMS[:3]


def _assert_batch_equals_singles(B, ctx, models, params, seeds, streams, d, out, ys, N, ot, ra, rf, threshold=None):
    assert np.all(out["status"] == 0)
    for k, par in enumerate(params):
        m = models[k]
        one = B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, obs_times=ot, resample_algorithm=ra,
                                 resample_fn=rf, threshold=threshold, return_particles=False, seed=seeds[k], stream=streams[k], ctx=ctx, **par)
        assert out["loglike"][k] == one["loglike"], (k, ra, out["loglike"][k], one["loglike"])
        np.testing.assert_array_equal(out["loglike_history"][k], one["loglike_history"])
        np.testing.assert_array_equal(out["ess"][k], one["ess"])
        np.testing.assert_array_equal(out["state_est"][k], np.asarray(one["state_est"]).reshape(-1, d))
        assert out["n_res_calls"][k] == one["_extras"]["n_res_calls"]
        assert out["early_return_step"][k] == one["_extras"]["early_return_step"] == 0


@pytest.mark.parametrize("N", [1, 7, 385, 1000, "max"])             # (385: the first N past the in-order exact sums)
@pytest.mark.parametrize("d,p", SHAPES)
@pytest.mark.parametrize("obs", FAMILIES)
def test_batch_equals_single_runs(B, ctx, obs, d, p, N):
    """three filters with distinct blocks, seeds and streams under SIS, SISR and SISAR: every returned array equals the single runs'"""
    N = B.batch_max_particles(d) if N == "max" else N
    rng = np.random.default_rng(300 + 10 * d + p)
    m, full = TO._batch_model(B, rng, obs, d, p, missing="skip")
    ys = _punch(_simulate(rng, obs, full, d, p, OT), p)
    for ra, rf in (("SIS", "stratified"), ("SISR", "systematic"), ("SISAR", "stratified")):
        thr = 0.95 * N if ra == "SISAR" else None
        out = B.bootstrap_filter_batch(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS, SEEDS, STREAMS, obs_times=OT,
                                       resample_algorithm=ra, resample_fn=rf, threshold=thr, ctx=ctx)
        _assert_batch_equals_singles(B, ctx, [m] * 3, PARAMS, SEEDS, STREAMS, d, out, ys, N, OT, ra, rf, thr)
        incr = np.diff(np.concatenate([np.zeros((3, 1)), out["loglike_history"]], axis=1), axis=1)
        assert np.all(incr[:, _full_rows(ys)] == 0.0) and (N == 1 or len(set(out["loglike"])) == 3)


@pytest.mark.parametrize("obs", FAMILIES)
def test_batch_with_two_array_sets_over_six_filters(B, ctx, obs):
    """the same through bssm_pf_run_batch_tv: two sets of b / h0 / H, filter k reading set tv_set[k]"""
    d, p, N = 3, 2, 385
    rng = np.random.default_rng(41)
    m, full = TO._batch_model(B, rng, obs, d, p, missing="skip")
    sets = [TO._varying(rng, full, d, p, OT[-1]) for _ in range(2)]
    ys = _punch(_simulate(rng, obs, full, d, p, OT, sets[0]), p)
    tv_set = [0, 1, 0, 1, 1, 0]
    params, seeds, streams = TO.PARAMS + [{"a": 0.8, "h": 0.1}], TO.SEEDS + [5], TO.STREAMS + [4]
    out = B.bootstrap_filter_batch(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, params, seeds, streams, obs_times=OT,
                                   resample_algorithm="SISAR", resample_fn="stratified", threshold=0.95 * N, ctx=ctx,
                                   time_varying={k: np.stack([s[k] for s in sets]) for k in ("b", "h0", "H")}, tv_set=tv_set)
    per_set = [TO._batch_model(B, np.random.default_rng(41), obs, d, p, time_varying=s, missing="skip")[0] for s in sets]
    _assert_batch_equals_singles(B, ctx, [per_set[g] for g in tv_set], params, seeds, streams, d, out, ys, N, OT, "SISAR", "stratified", 0.95 * N)
    assert out["n_res_calls"].max() > 0 and len(set(out["loglike"])) == 6


# ---- 5. the exact Kalman filter with missing data ---------------------------------------------------------------------------
def test_kalman_with_missing_data(B):
    """tests/test_gpu_mv.py's Kalman check (its model, N = 2^18, SISR / systematic, its tolerances) with about a third of the
    entries missing: the exact filter updates with the observed rows of H only"""
    import test_gpu_mv as TM
    rng = np.random.default_rng(7)
    d, p, n_obs, N = 3, 2, 30, 1 << 18
    q = TM._model(rng, d, p)
    ys = TM._simulate(rng, q, d, p, n_obs)
    gone = rng.random((n_obs, p)) < 1.0 / 3.0
    gone[4], gone[11, 0], gone[11, 1], gone[17, 0], gone[17, 1] = True, True, False, False, True      # a full row, both partial kinds
    ys[gone] = np.nan
    assert 0.25 < gone.mean() < 0.45 and gone.all(axis=1).any()
    m = B.models.linear_gaussian_mv(d, p, missing="skip", **q)
    cx = B.Context(0, N, d)
    try:
        a = B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, seed=1405, stream=2, resample_algorithm="SISR",
                               resample_fn="systematic", return_particles=False, ctx=cx)
    finally:
        cx.close()
    ll, means = MS.kalman_missing(R.unpack(m.pack({})), ys)
    print("loglike %.6f, Kalman %.6f; max |mean error| %.4f" % (a["loglike"], ll, np.max(np.abs(a["state_est"][1:] - means))))
    assert abs(a["loglike"] - ll) < 0.25, (a["loglike"], ll)
    np.testing.assert_allclose(a["state_est"][1:], means, atol=0.03)


# ---- 6. SIS: rows with nothing observed equal rows that are not there -------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True])
def test_sis_rows_with_nothing_observed_equal_rows_that_are_not_there(B, ctx, batched):
    """tests/test_mv_missing_cpu.py's identity on the device generator: rows {3, 4, 9} fully missing against the series without
    them and obs_times naming the kept times.  The transition calls keep their numbers, so the particles are the same; a row with
    nothing observed adds (0 + log(N)) - log(N) = 0.0: BIT equality of the final log-likelihood and of the kept rows' estimates."""
    d = p = 2
    rng = np.random.default_rng(31)
    q = TO._pieces(rng, d, p)
    n_obs, N = 12, (777 if batched else N_PAR)
    ys = _simulate(rng, "gaussian", q, d, p, list(range(1, n_obs + 1)))
    gone = np.array([3, 4, 9]) - 1
    keep = np.setdiff1d(np.arange(n_obs), gone)
    ys_m = ys.copy(); ys_m[gone] = np.nan
    m = B.models.linear_gaussian_mv(d, p, missing="skip", **q)
    if batched:
        run = lambda y, ot: {k: v[0] for k, v in B.bootstrap_filter_batch(   # noqa: E731
            y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, [m.pack({})], 9, [3], obs_times=ot, resample_algorithm="SIS", ctx=ctx).items()
            if k in ("loglike", "state_est", "loglike_history")}
    else:
        run = lambda y, ot: B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, obs_times=ot,   # noqa: E731
                                               resample_algorithm="SIS", return_particles=False, seed=9, stream=3, ctx=ctx)
    a, b = run(ys_m, None), run(ys[keep], list(keep + 1))
    assert a["loglike"] == b["loglike"] and np.isfinite(a["loglike"]), (a["loglike"], b["loglike"])
    np.testing.assert_array_equal(np.asarray(a["state_est"])[keep + 1], np.asarray(b["state_est"])[1:])
    np.testing.assert_array_equal(np.asarray(a["loglike_history"])[keep], np.asarray(b["loglike_history"]))


# ---- 7. closure mode --------------------------------------------------------------------------------------------------------
class _MaskedClosures(TO._Closures):
    """the family as Python closures that capture the mask: y carries 0.0 where nothing was seen, and the log-likelihoods leave
    those components out -- indexed by the time t the core hands them (strictly increasing times: t names the row)"""

    def __init__(self, obs, q, z_init, z_trans, seen, ot):
        super().__init__(obs, q, z_init, z_trans)
        self.seen = {int(t): np.asarray(s, dtype=bool) for t, s in zip(ot, seen)}

    def _masked(self, y, t):
        return np.where(self.seen[int(t)], np.atleast_1d(np.asarray(y, dtype=np.float64)), np.nan)

    def log_likelihood_fn(self, y, particles, t):
        x = np.asarray(particles, dtype=np.float64).reshape(-1, self.q["d"]).T
        return MS.loglik_skip(self.obs, self.q, self._masked(y, t), x)

    def aux_log_likelihood_fn(self, y, particles, t):
        x = np.asarray(particles, dtype=np.float64).reshape(-1, self.q["d"]).T
        return MS.loglik_skip(self.obs, self.q, self._masked(y, t), R.mean_of_transition(self.q, x))


@pytest.mark.parametrize("alg", ["BPF", "APF"])
@pytest.mark.parametrize("d,p", [(1, 1), (3, 2)])
def test_descriptor_agrees_with_closure_mode(B, ctx, oracle, alg, d, p):
    """the bar of tests/test_gpu_mv_obs.py::test_poisson_descriptor_agrees_with_closure_mode"""
    rng = np.random.default_rng(40 + d)
    N, ot, obs = 500, INCR, "poisson"
    q = TO._pieces(rng, d, p)
    ys = _punch(_simulate(rng, obs, q, d, p, ot), p)
    seen = ~np.isnan(ys)
    y0 = np.where(seen, ys, 0.0)                                     # closure mode refuses NaN: 0.0 as a placeholder
    m = B.models.linear_gaussian_mv(d, p, obs=obs, missing="skip", **q)
    for ra, rf in (("SISAR", "stratified"), ("SISR", "systematic")):
        dr = TO._draws(rng, alg, N, d, rf, ot, oracle)
        dev = TO._run(B, m, alg, ys, N, obs_times=ot, resample_algorithm=ra, resample_fn=rf, return_particles=False, draws=dr, ctx=ctx)
        cl = _MaskedClosures(obs, R.unpack(m.pack({})), dr["z_init"], dr["z_trans"], seen, ot)
        u_list = [np.atleast_1d(u) for u in dr["u_res"]]
        yy = y0[:, 0] if p == 1 else y0
        if alg == "BPF":
            host = B.bootstrap_filter(yy, N, cl.init_fn, cl.transition_fn, cl.log_likelihood_fn, obs_times=ot, resample_algorithm=ra,
                                      resample_fn=rf, return_particles=False, u_res=u_list, ctx=ctx)
        else:
            host = B.auxiliary_filter(yy, N, cl.init_fn, cl.transition_fn, cl.log_likelihood_fn, cl.aux_log_likelihood_fn, obs_times=ot,
                                      resample_algorithm=ra, resample_fn=rf, return_particles=False, u_res=u_list, ctx=ctx)
        assert abs(dev["loglike"] - host["loglike"]) <= 1e-6 * abs(host["loglike"])
        np.testing.assert_allclose(dev["loglike_history"], host["loglike_history"], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(dev["ess"], host["ess"], rtol=1e-6)
        np.testing.assert_allclose(np.asarray(dev["state_est"]).reshape(-1), np.asarray(host["state_est"]).reshape(-1), rtol=1e-6, atol=1e-8)
        # identical decisions, read off the host's ESS (== N exactly after a resampling) as that test does -- where something was
        # observed: uniform weights give ESS == N without a resampling, so at the rows with nothing observed the device's own
        # record is checked instead (SISAR: ESS = N is not below the threshold; SISR resamples always)
        some = seen.any(axis=1)
        assert ((np.asarray(host["ess"])[1:] == N) == (dev["_extras"]["resampled"] == 1))[some].all()
        assert (dev["_extras"]["resampled"][~some] == (1 if ra == "SISR" else 0)).all() and (np.asarray(host["ess"])[1:][~some] == N).all()


# ---- 8. pmmh ----------------------------------------------------------------------------------------------------------------
def test_pmmh_poisson_with_missing_rows_lockstep_equals_sequential(B):
    """tests/test_gpu_mv_obs.py's pmmh case and settings (_pmmh) with counts that were not reported: two whole rows and two
    single entries"""
    m0, ys = TO._pmmh_case(B)
    ys = ys.copy()
    ys[[5, 6]] = np.nan
    ys[12, 0] = ys[17, 1] = np.nan
    m = B.models.linear_gaussian_mv(2, 2, obs="poisson", missing="skip", build=m0.build, param_names=("mu",),
                                    **{k: m0.pieces[k] for k in ("A", "L", "H", "h0")})
    a, again, b = TO._pmmh(B, m, ys), TO._pmmh(B, m, ys), TO._pmmh(B, m, ys, batch_chains=False)
    assert a["_extras"]["batched"] is True and a["_extras"]["batched_launches"] > 0 and b["_extras"]["batched"] is False
    assert a["_extras"]["single_filter_runs"] == 0
    mu = np.asarray(a["theta_chain"]["mu"])
    assert mu.shape == (100,) and np.all(np.isfinite(mu)) and len(np.unique(mu)) > 3
    np.testing.assert_array_equal(mu, np.asarray(again["theta_chain"]["mu"]))             # repeats exactly for the same seed
    np.testing.assert_array_equal(mu, np.asarray(b["theta_chain"]["mu"]))                 # and equals the one-at-a-time run draw for draw
    with pytest.raises(ValueError, match="non-finite|missing values"):                    # the default descriptor still refuses this y
        TO._pmmh(B, m0, ys)


# ---- 9. the C ABI -----------------------------------------------------------------------------------------------------------
def test_the_option_through_the_abi(B, ctx):
    from bayesssm_amd import _lib
    lib = _lib.load()
    p_ = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    N, n_obs, F, d, p = 100, 5, 2, 3, 2
    MISSING = "Assertion on 'y' failed: Contains missing values"

    def call(model_id, y, how, dims=(d, p)):
        th = B.models.linear_gaussian_mv(*dims).pack({}) if model_id >= 3 else np.array([0.8, 1.0, 1.0])
        ths = np.ascontiguousarray([th] * F)
        y = np.ascontiguousarray(y, dtype=np.float64)
        cfg = _lib.PfConfig(model_id, _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN["stratified"], N, n_obs,
                            float("nan"), None if how != "run" else p_(th), int(th.size), p_(y), None, 1, 0, None, None, None, 0, 0, 0.0, None, None)
        if how == "run":
            se, ess, llh, ll = np.zeros((n_obs + 1, dims[0])), np.zeros(n_obs + 1), np.zeros(n_obs), np.zeros(1)
            res = _lib.PfResult(p_(se), p_(ess), p_(llh), p_(ll), None, None, None, None, None, None, None, None)
            rc = lib.bssm_pf_run(ctx.handle, C.byref(cfg), C.byref(res))
            return rc, lib.bssm_last_error().decode(), ll
        ll, st = np.zeros(F), np.zeros(F, np.int32)
        seeds, streams = np.array([1, 1], dtype=np.uint64), np.array([0, 1], dtype=np.uint64)
        res = _lib.PfBatchResult(p_(ll), None, None, None, None, None, p_(st), None)
        if how == "batch":
            rc = lib.bssm_pf_run_batch(ctx.handle, C.byref(cfg), F, p_(ths), p_(seeds), p_(streams), C.byref(res))
        else:
            h0 = np.zeros((n_obs, dims[1]))
            sets = _lib.MvTvBatch(0, 1, None, None, 0, p_(h0), 0, None, 0)
            rc = lib.bssm_pf_run_batch_tv(ctx.handle, C.byref(cfg), F, p_(ths), p_(seeds), p_(streams), C.byref(sets), C.byref(res))
        return rc, lib.bssm_last_error().decode(), ll

    y_nan, y_inf = np.ones((n_obs, p)), np.ones((n_obs, p))
    y_nan[3, 1] = np.nan; y_nan[1] = np.nan
    y_inf[3, 1] = np.nan; y_inf[2, 0] = np.inf
    y_neg = y_nan.copy(); y_neg[0, 0] = -1.0
    try:
        for how in ("run", "batch", "batch_tv"):
            for fam in FAMILIES:
                mid = _lib.MV_OBS_MODEL[fam]
                ctx.set_option("mv_y_missing", 0)
                rc, msg, _ = call(mid, y_nan, how)
                assert rc == _lib.ERR_ARG and msg == MISSING, (how, fam, rc, msg)                    # refused exactly as before
                ctx.set_option("mv_y_missing", 1)
                rc, msg, ll = call(mid, y_nan, how)
                assert rc == _lib.OK and np.all(np.isfinite(ll)) and np.all(ll != 0.0), (how, fam, rc, msg, ll)
                rc, msg, _ = call(mid, y_inf, how)
                assert rc == _lib.ERR_ARG and msg == MISSING, (how, fam, rc, msg)                    # +-inf stays refused
            rc, msg, _ = call(_lib.MV_OBS_MODEL["poisson"], y_neg, how)                              # observed counts are still checked
            assert rc == _lib.ERR_ARG and "non-negative integers" in msg, (how, rc, msg)
        # the scalar models ignore the option
        y1 = np.ones(n_obs); y1[2] = np.nan
        for how in ("run", "batch"):
            rc, msg, _ = call(_lib.MODEL["lg"], y1, how, dims=(1, 1))
            assert rc == _lib.ERR_ARG and msg == MISSING, (how, rc, msg)
    finally:
        ctx.set_option("mv_y_missing", 0)
    # a Python call that raises inside the library (sd = 0 is the library's own refusal) leaves the option at 0: the same context
    # refuses NaN again
    bad = B.models.linear_gaussian_mv(d, p, missing="skip", sd=[0.0, 1.0])
    with pytest.raises(_lib.BssmError, match="observation sd must be positive"):
        B.bootstrap_filter(y_nan, N, bad.init_fn, bad.transition_fn, bad.log_likelihood_fn, ctx=ctx)
    with pytest.raises(_lib.BssmError, match="observation sd must be positive"):
        B.bootstrap_filter_batch(y_nan, N, bad.init_fn, bad.transition_fn, bad.log_likelihood_fn, [bad.pack({})] * 2, 1, [0, 1], ctx=ctx)
    for how in ("run", "batch"):
        rc, msg, _ = call(_lib.MV_OBS_MODEL["gaussian"], y_nan, how)
        assert rc == _lib.ERR_ARG and msg == MISSING, (how, rc, msg)
