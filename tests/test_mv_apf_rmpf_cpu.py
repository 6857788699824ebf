"""CPU checks of the multivariate family's auxiliary and resample-move filters (no GPU needed).

The restatement in tests/mv_apf_rmpf_restated.py is what the device's APF / RMPF runs are compared with.  At d = p = 1 (A = phi,
b = 0, H = 1, h0 = 0) the family's arithmetic is the scalar linear-Gaussian model's operation for operation, so the restatement
must reproduce the oracle's own APF / RMPF (oracle/bssm_oracle.c, orc_pf_run) on the same draws."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402


def _theta_lg(phi, sx, sy):
    return np.array([1, 1, 0.0, 1.0, phi, 0.0, sx, 0.0, 1.0, 0.0, sy])      # d, p, m0, L0, A, b, L, c0, H, h0, sd


@pytest.mark.parametrize("alg,ra,rf,ot", [
    ("APF", "SISAR", "stratified", None), ("APF", "SISR", "systematic", None), ("APF", "SIS", "stratified", [1, 2, 2, 4, 5, 7, 8, 9, 10, 11]),
    ("RMPF", "SISR", "stratified", None), ("RMPF", "SISR", "systematic", [1, 2, 2, 4, 5, 7, 8, 9, 10, 11]),
])
def test_restatement_reduces_to_the_scalar_oracle(oracle, alg, ra, rf, ot):
    rng = np.random.default_rng(11)
    T, N = 10, 3000
    phi, sx, sy = 0.8, 1.1, 0.7
    ys = rng.standard_normal(T)
    mt, mr = oracle.noise_shape(alg, T, ot)
    zi, zt = rng.standard_normal(N), rng.standard_normal((mt, N))
    ur = rng.random(mr) if rf == "systematic" else rng.random((mr, N))
    zm, um = rng.standard_normal((T, N)), rng.random((T, N))
    kw = dict(algorithm=alg, resample_algorithm=ra, resample_fn=rf, obs_times=ot)
    if alg == "RMPF":
        kw.update(move_sd=0.3, z_move=zm, u_move=um)
    a = oracle.pf_run("lg", (phi, sx, sy), ys, N, zi, zt, ur, return_ancestors=True, **kw)
    b = R.pf_run_mv(oracle, _theta_lg(phi, sx, sy), ys.reshape(-1, 1), N, zi.reshape(1, N), zt.reshape(mt, 1, N), ur,
                    **dict(kw, z_move=zm.reshape(T, 1, N) if alg == "RMPF" else None))
    k = a["n_res_calls"]
    assert k == b["n_res_calls"] and (a["resampled"] == b["resampled"]).all()
    assert (np.asarray(a["ancestors"])[:k] == b["ancestors"][:k]).all()
    assert a["early_return_step"] == b["early_return_step"] == 0
    assert abs(a["loglike"] - b["loglike"]) <= 1e-12 * abs(a["loglike"])
    for key in ("loglike_history", "ess", "state_est"):
        np.testing.assert_allclose(np.asarray(b[key]).reshape(-1), np.asarray(a[key]).reshape(-1), rtol=1e-12, atol=1e-300, err_msg=key)


def kalman_means(A, b, L, H, h0, sd, m0, P0, ys, transitions_per_obs=1):
    """exact filtering means; transitions_per_obs = 2 gives those of the reference's auxiliary filter, which transitions once
    more after its first-stage resampling (R/particle_filter_core.R:125-136, 159)"""
    m, P, Q, Rm, means = m0.copy(), P0.copy(), L @ L.T, np.diag(sd ** 2), []
    for yv in ys:
        for _ in range(transitions_per_obs):
            m, P = A @ m + b, A @ P @ A.T + Q
        S = H @ P @ H.T + Rm
        K = P @ H.T @ np.linalg.inv(S)
        m, P = m + K @ (yv - (h0 + H @ m)), (np.eye(len(m)) - K @ H) @ P
        means.append(m.copy())
    return np.array(means)


def test_restated_apf_against_kalman_means(oracle):
    """d = 2, p = 2: the restated APF's state estimates follow the exact filtering means of the dynamics it runs (two
    transitions per observation) -- a statistical check of the aux definition and the second-stage correction."""
    rng = np.random.default_rng(5)
    d, p, T, N = 2, 2, 12, 40000
    # (state noise small against the observation noise: the look-ahead at the transition mean is then close to the predictive
    #  density and the second-stage weights stay even -- with a wide state noise they are heavy-tailed and the error is Monte Carlo's)
    A = np.array([[0.7, 0.2], [-0.1, 0.5]]); L = np.array([[0.32, 0.0], [0.12, 0.24]]); H = np.array([[1.0, 0.5], [0.0, 1.0]])
    sd, b, h0 = np.array([0.6, 0.9]), np.array([0.1, -0.2]), np.array([0.0, 0.3])
    theta = np.concatenate([[d, p], np.zeros(2), np.eye(2).ravel(), A.ravel(), b, L.ravel(), [0.0], H.ravel(), h0, sd])
    x = rng.standard_normal(2)
    ys = np.zeros((T, p))
    for t in range(T):
        for _ in range(2):
            x = A @ x + b + L @ rng.standard_normal(2)
        ys[t] = h0 + H @ x + sd * rng.standard_normal(2)
    means = kalman_means(A, b, L, H, h0, sd, np.zeros(2), np.eye(2), ys, transitions_per_obs=2)
    mt, mr = oracle.noise_shape("APF", T)
    r = R.pf_run_mv(oracle, theta, ys, N, rng.standard_normal((d, N)), rng.standard_normal((mt, d, N)), rng.random(mr),
                    algorithm="APF", resample_algorithm="SISR", resample_fn="systematic")
    np.testing.assert_allclose(r["state_est"][1:], means, atol=0.03)


def test_descriptors_of_the_family():
    import bayesssm_amd as B
    m = B.models.linear_gaussian_mv(2, 1, build=lambda phi: {"b": [phi, phi]}, param_names=("phi",))
    aux = m.aux_log_likelihood_fn
    assert aux.model == "lgmv" and aux.role == "aux_log_likelihood" and aux.owner is m
    assert aux.formals() == ["y", "particles", "phi"]
    mv = m.rw_move_fn(0.25)
    assert mv.model == "lgmv" and mv.sd == 0.25 and mv.formals() == ["particle", "y", "phi"]
    assert B.models.linear_gaussian().rw_move_fn(0.1).formals() == ["particle", "y", "sigma_y"]     # (unchanged for the scalar models)
    assert B.models.resolve(m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn) == "lgmv"


def test_host_side_rejections():
    """A scalar model's move with this family, and r_seed / r_stream with it, are refused before any context is created."""
    import bayesssm_amd as B
    m = B.models.linear_gaussian_mv(2, 2)
    y = np.zeros((5, 2))
    with pytest.raises(ValueError, match="move_fn belongs to a different model"):
        B.resample_move_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, B.models.linear_gaussian().rw_move_fn(0.1))
    with pytest.raises(ValueError, match="r_seed / r_stream"):
        B.resample_move_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.1), r_seed=1)
    with pytest.raises(ValueError, match="r_seed / r_stream"):
        B.auxiliary_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, r_seed=1)
