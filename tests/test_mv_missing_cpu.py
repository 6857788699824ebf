"""CPU checks of missing and partially observed y for the multivariate family (models.linear_gaussian_mv(..., missing="skip"));
no GPU needed.

tests/mv_missing_restated.py is what the device is compared with when y holds NaN.  Without NaN it must be
tests/mv_obs_restated.py exactly; a row with nothing observed must add exactly 0.0 to the log-likelihood and leave uniform weights;
under SIS, rows with nothing observed must be the same as rows that are not there; and the descriptor and the filters' host checks
let NaN (never +-inf) through for "skip" alone, before any context is created."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402
import mv_missing_restated as MS  # noqa: E402
import mv_obs_restated as OB  # noqa: E402

GAPS = [1, 2, 2, 4, 5, 7, 8, 9, 10, 10, 11, 14]          # T = 12: gaps and repeated times


def _theta(rng, d, p):
    A = 0.6 * np.eye(d) + 0.1 * rng.standard_normal((d, d))
    Lq = np.tril(0.3 * rng.standard_normal((d, d))) + 0.7 * np.eye(d)
    L0 = np.tril(0.2 * rng.standard_normal((d, d))) + np.eye(d)
    return np.concatenate([[d, p], rng.standard_normal(d), L0.ravel(), A.ravel(), 0.1 * rng.standard_normal(d), Lq.ravel(), [0.5],
                           0.3 * rng.standard_normal(p * d), 0.2 * rng.standard_normal(p), 0.5 + rng.random(p)])


def _inputs(rng, oracle, alg, d, T, N, ot, ra=None, rf=None):
    ra0, rf0 = {"BPF": ("SISR", "stratified"), "APF": ("SISAR", "stratified"), "RMPF": ("SISR", "systematic")}[alg]
    ra, rf = ra or ra0, rf or rf0
    mt, mr = oracle.noise_shape(alg, T, ot)
    zi, zt = rng.standard_normal((d, N)), rng.standard_normal((max(mt, 1), d, N))
    ur = rng.random(max(mr, 1)) if rf == "systematic" else rng.random((max(mr, 1), N))
    kw = dict(algorithm=alg, resample_algorithm=ra, resample_fn=rf, obs_times=ot, return_particles=True)
    if alg == "RMPF":
        kw.update(move_sd=0.3, z_move=rng.standard_normal((T, d, N)), u_move=rng.random((T, N)))
    return zi, zt, ur, kw


def _ys(rng, obs, T, p):
    return rng.poisson(2.0, size=(T, p)).astype(np.float64) if obs == "poisson" else rng.standard_normal((T, p))


@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("obs", OB.OBS)
@pytest.mark.parametrize("d,p,ot", [(1, 1, None), (3, 2, GAPS)])
def test_without_nan_it_is_the_existing_restatement_bitwise(oracle, obs, alg, d, p, ot):
    rng = np.random.default_rng(100 * d + p)
    T, N = 12, 300
    theta = _theta(rng, d, p)
    ys = _ys(rng, obs, T, p)
    zi, zt, ur, kw = _inputs(rng, oracle, alg, d, T, N, ot)
    tv = dict(h0_t=0.3 * rng.standard_normal((T, p)), H_t=0.5 * rng.standard_normal((T, p, d)))
    a = OB.pf_run_mv_obs(oracle, obs, theta, ys, N, zi, zt, ur, **tv, **kw)
    b = MS.pf_run_mv_missing(oracle, obs, theta, ys, N, zi, zt, ur, **tv, **kw)
    assert a["loglike"] == b["loglike"] and a["n_res_calls"] == b["n_res_calls"] > 0
    for key in ("loglike_history", "ess", "state_est", "ancestors", "resampled", "particles_history", "weights_history"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
    assert R.loglik.__module__ == "mv_apf_rmpf_restated"          # (the skipping function is in place for the call only)


def test_p_zero_is_the_constant():
    q = R.unpack(_theta(np.random.default_rng(0), 2, 0))
    assert np.array_equal(MS.loglik_skip("gaussian", q, np.zeros(0), np.zeros((2, 7))), np.full(7, 0.5))


@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("obs", OB.OBS)
def test_a_row_with_nothing_observed_adds_exactly_zero(oracle, obs, alg):
    """rows 1, 6 and the last fully missing: the history's increment there is exactly 0.0, the weights are uniform (1 / N for
    every particle), the ESS is N, and the RMPF accepts every proposal; a partially observed row is neither"""
    rng = np.random.default_rng(9)
    d, p, T, N = 3, 2, 12, 257
    theta = _theta(rng, d, p)
    ys = _ys(rng, obs, T, p)
    gone = [0, 5, T - 1]
    ys[gone] = np.nan
    ys[3, 0] = np.nan                                              # partial rows: only k = 0, only k = p - 1 missing
    ys[8, p - 1] = np.nan
    zi, zt, ur, kw = _inputs(rng, oracle, alg, d, T, N, GAPS, ra="SIS" if alg == "BPF" else None)
    r = MS.pf_run_mv_missing(oracle, obs, theta, ys, N, zi, zt, ur, **kw)
    assert r["early_return_step"] == 0 and np.isfinite(r["loglike"])
    incr = np.diff(np.concatenate([[0.0], r["loglike_history"]]))
    for i in gone:
        assert incr[i] == 0.0, (i, incr[i])                        # (the APF's second-stage weights are 0 - aux[idx] = 0 - 0 too)
        assert np.all(r["weights_history"][i + 1] == 1.0 / N) and r["ess"][i + 1] == N
    for i in (3, 8):
        assert incr[i] != 0.0
        if alg == "BPF":                                           # (SIS: the weights stay as normalised)
            assert not np.all(r["weights_history"][i + 1] == 1.0 / N)
    if alg == "RMPF":                                              # every proposal is accepted at a fully missing row, whatever
        u2 = kw["u_move"].copy()                                   # its uniform: other uniforms there change nothing
        u2[gone] = rng.random((len(gone), N))
        r2 = MS.pf_run_mv_missing(oracle, obs, theta, ys, N, zi, zt, ur, **dict(kw, u_move=u2))
        assert r2["loglike"] == r["loglike"] and np.array_equal(r2["particles_history"], r["particles_history"])
        u2[3] = rng.random(N)                                      # (at a partially observed row they do)
        r3 = MS.pf_run_mv_missing(oracle, obs, theta, ys, N, zi, zt, ur, **dict(kw, u_move=u2))
        assert not np.array_equal(r3["particles_history"], r["particles_history"])
    # the missing components are skipped, not read as numbers: any placeholder in their place would change the run
    ys0 = np.where(np.isnan(ys), 0.0, ys)
    r0 = MS.pf_run_mv_missing(oracle, obs, theta, ys0, N, zi, zt, ur, **kw)
    assert r0["loglike"] != r["loglike"]


def test_sis_rows_with_nothing_observed_equal_rows_that_are_not_there(oracle):
    """SIS with the bootstrap filter, T = 12, d = p = 2: rows {3, 4, 9} (1-based) fully missing against the same series with
    those rows dropped and obs_times naming the kept times.  The particles see the same transitions with the same draws (the
    gap loop runs them), the kept rows' weights come from the same log-weights, and a fully missing row adds
    (0 + log(N)) - log(N) = 0.0 exactly: the restatement gives BIT equality, so that is asserted."""
    rng = np.random.default_rng(31)
    d, p, T, N = 2, 2, 12, 300
    theta = _theta(rng, d, p)
    ys = rng.standard_normal((T, p))
    gone = np.array([3, 4, 9]) - 1
    keep = np.setdiff1d(np.arange(T), gone)
    ys_m = ys.copy(); ys_m[gone] = np.nan
    zi, zt = rng.standard_normal((d, N)), rng.standard_normal((T, d, N))
    ur = np.zeros((1, N))
    kw = dict(algorithm="BPF", resample_algorithm="SIS", resample_fn="stratified")
    a = MS.pf_run_mv_missing(oracle, "gaussian", theta, ys_m, N, zi, zt, ur, **kw)
    b = MS.pf_run_mv_missing(oracle, "gaussian", theta, ys[keep], N, zi, zt, ur, obs_times=list(keep + 1), **kw)
    assert a["n_trans_calls"] == b["n_trans_calls"] == T and a["n_res_calls"] == b["n_res_calls"] == 0
    assert a["loglike"] == b["loglike"] and np.isfinite(a["loglike"])
    assert np.array_equal(a["state_est"][keep + 1], b["state_est"][1:])
    assert np.array_equal(a["loglike_history"][keep], b["loglike_history"])
    assert np.array_equal(a["state_est"][0], b["state_est"][0])


def test_kalman_missing_equals_the_full_filter_without_nan():
    import mv_tv_restated as TV
    rng = np.random.default_rng(2)
    q = R.unpack(_theta(rng, 3, 2))
    ys = rng.standard_normal((10, 2))
    a, b = MS.kalman_missing(q, ys), TV.kalman_tv(q, ys)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0]) and np.allclose(a[1], b[1], rtol=1e-12, atol=1e-14)
    ys[4] = np.nan                                                 # a row with nothing observed: the prediction step alone
    ll, means = MS.kalman_missing(q, ys)
    assert np.allclose(means[4], q["A"] @ means[3] + q["b"], rtol=1e-13, atol=1e-15) and np.isfinite(ll)


def test_constructor():
    import bayesssm_amd as B
    assert B.models.linear_gaussian_mv(2, 2).missing == "refuse"
    assert B.models.linear_gaussian_mv(2, 2, missing="skip").missing == "skip"
    assert B.models.linear_gaussian_mv(2, 0, missing="skip").p == 0            # p == 0: accepted, nothing to skip
    for bad in ("drop", None, True, "Skip"):
        with pytest.raises(ValueError) as e:
            B.models.linear_gaussian_mv(2, 2, missing=bad)
        assert str(e.value) == "linear_gaussian_mv: missing must be one of 'refuse', 'skip'"
    a, b = B.models.linear_gaussian_mv(3, 2, sd=[0.4, 0.9]), B.models.linear_gaussian_mv(3, 2, sd=[0.4, 0.9], missing="skip")
    assert np.array_equal(a.pack({}), b.pack({}))                               # the packed block does not know about it
    from bayesssm_amd import _lib
    assert _lib.Context.OPTIONS["mv_y_missing"] == 13


def _all_entry_points(B, m, y):
    yield lambda: B.bootstrap_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn)
    yield lambda: B.auxiliary_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn)
    yield lambda: B.resample_move_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.1))
    yield lambda: B.bootstrap_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, [m.pack({})] * 2, 1, [0, 1])


@pytest.mark.parametrize("obs", OB.OBS)
def test_host_checks(obs):
    import bayesssm_amd as B
    good = np.ones((5, 2))
    skip, refuse = B.models.linear_gaussian_mv(2, 2, obs=obs, missing="skip"), B.models.linear_gaussian_mv(2, 2, obs=obs)
    y_nan, y_row = good.copy(), good.copy()
    y_nan[3, 1] = np.nan
    y_row[2] = np.nan
    for bad in (np.inf, -np.inf):                                  # +-inf: refused by both
        y = y_nan.copy(); y[1, 0] = bad
        for m in (skip, refuse):
            for call in _all_entry_points(B, m, y):
                with pytest.raises(ValueError, match="missing values|non-finite"):
                    call()
    for y in (y_nan, y_row):                                       # NaN: refused by the default, with the existing message
        for call in _all_entry_points(B, refuse, y):
            with pytest.raises(ValueError, match="non-finite" if obs == "poisson" else "Assertion on 'y' failed: Contains missing values"):
                call()
    if obs == "poisson":                                           # observed counts are still checked
        for bad, match in ((-1.0, "negative"), (0.5, "fractional")):
            y = y_nan.copy(); y[0, 0] = bad
            for call in _all_entry_points(B, skip, y):
                with pytest.raises(ValueError, match=match):
                    call()


def test_pmmh_host_check():
    import bayesssm_amd as B
    mk = lambda **kw: B.models.linear_gaussian_mv(2, 2, build=lambda mu: {"b": [mu, mu]}, param_names=("mu",), **kw)   # noqa: E731
    y = np.ones((5, 2)); y[3, 1] = np.nan
    args = lambda m, yy: (B.bootstrap_filter, yy, 10, m.init_fn, m.transition_fn, m.log_likelihood_fn, {"mu": B.prior_normal(0.0, 1.0)},   # noqa: E731
                          [{"mu": 0.1}], 2)
    with pytest.raises(ValueError, match="Assertion on 'y' failed: Contains missing values"):
        B.pmmh(*args(mk(), y), num_chains=1, verbose=False, print_result=False)
    yi = y.copy(); yi[0, 0] = np.inf
    with pytest.raises(ValueError, match="Assertion on 'y' failed: Contains missing values"):
        B.pmmh(*args(mk(missing="skip"), yi), num_chains=1, verbose=False, print_result=False)
    # with "skip" the NaN passes that check: the next one speaks (burn_in = 2 is fine, m = 0 is not)
    with pytest.raises(ValueError, match="Assertion on 'm' failed"):
        B.pmmh(B.bootstrap_filter, y, 0, *args(mk(missing="skip"), y)[3:], num_chains=1, verbose=False, print_result=False)


def test_nan_passes_the_host_checks_with_skip(monkeypatch):
    """with "skip" a NaN gets past every host check: the call reaches the library (here a stub in place of the context, which
    records that the option was 1 during the call and is restored after it, also when the call raises)"""
    import bayesssm_amd as B
    from bayesssm_amd import _lib, filters
    log = []

    class Boom(Exception):
        pass

    class FakeCtx:
        handle = None
        _set_options = {}
        set_option = lambda self, name, v: (log.append((name, int(v))), self._set_options.__setitem__(name, int(v)))[0]   # noqa: E731
        mv_y_missing = _lib.Context.mv_y_missing
        require = lambda self, *a: self   # noqa: E731

    class FakeLib:
        def bssm_pf_noise_shape(self, alg, T, ot, mt, mr):
            mt._obj.value, mr._obj.value = T, T
            return 0

        def _run(self, *a):
            log.append("run")
            raise Boom()
        bssm_pf_run = bssm_pf_run_batch = bssm_pf_run_batch_tv = _run

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    y = np.ones((5, 2)); y[3, 1] = np.nan; y[1] = np.nan
    for obs in OB.OBS:
        m = B.models.linear_gaussian_mv(2, 2, obs=obs, missing="skip")
        for call in (lambda: B.bootstrap_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, ctx=FakeCtx()),
                     lambda: B.auxiliary_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, ctx=FakeCtx()),
                     lambda: B.resample_move_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.1), ctx=FakeCtx()),
                     lambda: filters.bootstrap_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, [m.pack({})] * 2, 1, [0, 1],
                                                            ctx=FakeCtx()),
                     lambda: filters.bootstrap_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, [m.pack({})] * 2, 1, [0, 1],
                                                            ctx=FakeCtx(), time_varying={"h0": np.zeros((2, 5, 2))})):
            del log[:]
            FakeCtx._set_options.clear()
            with pytest.raises(Boom):
                call()
            assert log == [("mv_y_missing", 1), "run", ("mv_y_missing", 0)], log
    # the default descriptor never touches the option
    m = B.models.linear_gaussian_mv(2, 2)
    del log[:]
    with pytest.raises(Boom):
        B.bootstrap_filter(np.ones((5, 2)), 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, ctx=FakeCtx())
    assert log == ["run"]
    # r_seed / r_stream stay refused for the family
    m = B.models.linear_gaussian_mv(2, 2, missing="skip")
    with pytest.raises(ValueError, match="r_seed / r_stream"):
        B.auxiliary_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, r_seed=1)
    with pytest.raises(ValueError, match="r_seed / r_stream"):
        B.resample_move_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.1), r_stream=object())
