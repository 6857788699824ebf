"""CPU checks of the multivariate family's time-varying pieces (no GPU needed).

tests/mv_tv_restated.py is what the device is compared with when b, h0, H vary with time.  With the arrays filled with the
block's own constant b, h0, H it must be tests/mv_apf_rmpf_restated.py exactly: only where a coefficient is read from changes,
never an operation.  Then the descriptor's validation of the arrays (models.linear_gaussian_mv(time_varying=...))."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402
import mv_tv_restated as TV  # noqa: E402

GAPS = [1, 2, 2, 4, 5, 7, 8, 9, 10, 10, 11, 14]          # T = 12: gaps and repeated times


def _theta(rng, d, p):
    A = 0.6 * np.eye(d) + 0.1 * rng.standard_normal((d, d))
    Lq = np.tril(0.3 * rng.standard_normal((d, d))) + 0.7 * np.eye(d)
    L0 = np.tril(0.2 * rng.standard_normal((d, d))) + np.eye(d)
    return np.concatenate([[d, p], rng.standard_normal(d), L0.ravel(), A.ravel(), 0.1 * rng.standard_normal(d), Lq.ravel(), [0.5],
                           rng.standard_normal(p * d), 0.2 * rng.standard_normal(p), 0.5 + rng.random(p)])


@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("d,p,ot", [(1, 1, None), (3, 2, GAPS), (8, 8, None), (2, 0, GAPS)])
def test_constant_arrays_reproduce_the_constant_restatement_bitwise(oracle, alg, d, p, ot):
    rng = np.random.default_rng(100 * d + p)
    T, N = 12, 700
    theta = _theta(rng, d, p)
    q = R.unpack(theta)
    ys = rng.standard_normal((T, p))
    ra, rf = {"BPF": ("SISR", "stratified"), "APF": ("SISAR", "stratified"), "RMPF": ("SISR", "systematic")}[alg]
    mt, mr = oracle.noise_shape(alg, T, ot)
    zi, zt = rng.standard_normal((d, N)), rng.standard_normal((max(mt, 1), d, N))
    ur = rng.random(mr) if rf == "systematic" else rng.random((mr, N))
    kw = dict(algorithm=alg, resample_algorithm=ra, resample_fn=rf, obs_times=ot, return_particles=True)
    if alg == "RMPF":
        kw.update(move_sd=0.3, z_move=rng.standard_normal((T, d, N)), u_move=rng.random((T, N)))
    n_times = ot[-1] if ot is not None else T
    tv = dict(b_t=np.tile(q["b"], (n_times, 1)))
    if p > 0:
        tv.update(h0_t=np.tile(q["h0"], (T, 1)), H_t=np.tile(q["H"], (T, 1, 1)))
    a = R.pf_run_mv(oracle, theta, ys, N, zi, zt, ur, **kw)
    b = TV.pf_run_mv_tv(oracle, theta, ys, N, zi, zt, ur, **tv, **kw)
    assert a["n_res_calls"] == b["n_res_calls"] > 0 and a["n_trans_calls"] == b["n_trans_calls"]
    assert a["loglike"] == b["loglike"] and a["early_return_step"] == b["early_return_step"] == 0
    for key in ("loglike_history", "ess", "state_est", "ancestors", "resampled", "particles_history", "weights_history"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key


def test_varying_b_enters_at_the_time_reached(oracle):
    """x' = x + b_t[tau - 1] without noise (L = 0, L0 = 0): the state at observation i is sum(b_t[:obs_time_i]) whatever the
    gaps, for the BPF; the APF transitions once more with the observation time's row (R/particle_filter_core.R:159)."""
    d, T, N = 1, 4, 8
    ot = [2, 3, 3, 6]
    b_t = np.array([1.0, 10.0, 100.0, 1000.0, 1e4, 1e5]).reshape(-1, 1)
    theta = np.concatenate([[1, 0], [0.0], [0.0], [1.0], [0.0], [0.0], [0.0]])      # d, p, m0, L0, A, b, L, c0
    mt, mr = oracle.noise_shape("APF", T, ot)
    z = dict(z_init=np.zeros((d, N)), z_trans=np.zeros((mt, d, N)), u_res=np.full(mr, 0.5))
    r = TV.pf_run_mv_tv(oracle, theta, np.zeros(T), N, b_t=b_t, algorithm="BPF", resample_fn="systematic", obs_times=ot, **z)
    np.testing.assert_array_equal(r["state_est"], [0.0, 11.0, 111.0, 111.0, 111111.0])
    r = TV.pf_run_mv_tv(oracle, theta, np.zeros(T), N, b_t=b_t, algorithm="APF", resample_fn="systematic", obs_times=ot, **z)
    np.testing.assert_array_equal(r["state_est"], [0.0, 21.0, 221.0, 321.0, 211321.0])


def _kalman_means_constant(A, b, L, H, h0, sd, m0, P0, ys):
    """the textbook Kalman filter of the constant model, written out on its own"""
    m, P, Q, Rm, means = m0.copy(), P0.copy(), L @ L.T, np.diag(sd ** 2), []
    for yv in ys:
        m, P = A @ m + b, A @ P @ A.T + Q
        S = H @ P @ H.T + Rm
        K = P @ H.T @ np.linalg.inv(S)
        m, P = m + K @ (yv - (h0 + H @ m)), (np.eye(len(m)) - K @ H) @ P
        means.append(m.copy())
    return np.array(means)


def test_kalman_tv_reduces_to_the_constant_kalman():
    rng = np.random.default_rng(3)
    d, p, T = 3, 2, 9
    q = R.unpack(_theta(rng, d, p))
    ys = rng.standard_normal((T, p))
    ll, means = TV.kalman_tv(q, ys, b_t=np.tile(q["b"], (T, 1)), h0_t=np.tile(q["h0"], (T, 1)), H_t=np.tile(q["H"], (T, 1, 1)))
    np.testing.assert_allclose(means, _kalman_means_constant(q["A"], q["b"], q["L"], q["H"], q["h0"], q["sd"], q["m0"], q["L0"] @ q["L0"].T, ys),
                               rtol=1e-12)
    assert np.isfinite(ll)


def test_descriptor_validates_the_time_varying_arrays():
    import bayesssm_amd as B
    mk = B.models.linear_gaussian_mv
    T = 6
    ok = {"b": np.zeros((T, 3)), "h0": np.zeros((T, 2)), "H": np.zeros((T, 2, 3))}
    m = mk(3, 2, time_varying=ok)
    n_times, b, h0, H = m.tv_arrays(T)
    assert n_times == T and b.shape == (T, 3) and h0.shape == (T, 2) and H.shape == (T, 2, 3)
    assert all(a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] for a in (b, h0, H))
    assert mk(3, 2).tv_arrays(T) is None and mk(3, 2, time_varying={}).tv_arrays(T) is None
    assert mk(1, 1, time_varying={"b": np.zeros(T), "h0": np.zeros(T)}).tv_arrays(T)[1].shape == (T, 1)     # vectors at d = p = 1
    assert mk(2, 1, time_varying={"H": np.zeros((T, 2))}).tv_arrays(T)[3].shape == (T, 1, 2)                # covariate rows at p = 1
    # shapes against (d, p)
    for bad in ({"b": np.zeros((T, 2))}, {"b": np.zeros(T)}, {"h0": np.zeros((T, 3))}, {"H": np.zeros((T, 3, 2))}, {"H": np.zeros((T, 6))},
                {"b": np.zeros((0, 3))}):
        with pytest.raises(ValueError, match="must have shape"):
            mk(3, 2, time_varying=bad)
    # finiteness
    for k in ok:
        bad = {k2: v.copy() for k2, v in ok.items()}
        bad[k].reshape(-1)[-1] = np.nan
        with pytest.raises(ValueError, match="non-finite"):
            mk(3, 2, time_varying=bad)
    # only b, h0, H vary; observation pieces need observation components
    with pytest.raises(TypeError, match="unknown time-varying piece"):
        mk(3, 2, time_varying={"A": np.zeros((T, 3, 3))})
    with pytest.raises(TypeError, match="must be a dict"):
        mk(3, 2, time_varying=np.zeros((T, 3)))
    with pytest.raises(ValueError, match="p == 0"):
        mk(3, 0, time_varying={"h0": np.zeros((T, 0))})
    with pytest.raises(TypeError, match="unknown piece"):                     # (the fixed pieces' own check is unchanged)
        mk(3, 2, time_varying=ok, nonsense=1.0)
    # n_times against the observation times; one row of h0 / H per observation
    with pytest.raises(ValueError, match="last observation time is 7"):
        m.tv_arrays(T, [1, 2, 3, 4, 5, 7])
    with pytest.raises(ValueError, match="last observation time is 7"):
        m.tv_arrays(7)
    assert mk(3, 2, time_varying={"b": np.zeros((9, 3))}).tv_arrays(T, [1, 2, 3, 4, 5, 9])[0] == 9
    with pytest.raises(ValueError, match="one row each"):
        mk(3, 2, time_varying={"h0": np.zeros((T + 1, 2))}).tv_arrays(T)
    # the filters refuse before any context is created
    with pytest.raises(ValueError, match="last observation time is 8"):
        B.bootstrap_filter(np.zeros((8, 2)), 100, m.init_fn, m.transition_fn, m.log_likelihood_fn)


def test_config_mirror_keeps_positional_constructions():
    """bssm_pf_config.mv_tv is the LAST field and defaults to NULL: every existing positional construction is unchanged, and the
    config embedded by value in bssm_pmmh_config grows with it."""
    import ctypes as C
    from bayesssm_amd import _lib
    assert _lib.PfConfig._fields_[-1][0] == "mv_tv" and _lib.PfConfig._fields_[-2][0] == "u_move"
    cfg = _lib.PfConfig(3, 0, 1, 0, 100, 5, 0.5, None, 0, None, None, 1, 2, None, None, None, 0, 0, 0.0, None, None)
    assert cfg.mv_tv is None and cfg.u_move is None
    assert _lib.PfConfig.mv_tv.offset + C.sizeof(C.c_void_p) == C.sizeof(_lib.PfConfig)
    assert _lib.PmmhConfig.m.offset == C.sizeof(_lib.PfConfig)
    assert [f[0] for f in _lib.MvTv._fields_] == ["n_times", "b_t", "h0_t", "H_t"]
