"""CPU restatement of .particle_filter_core (R/particle_filter_core.R:19-267) for the multivariate family with MISSING and partially
observed y (models.linear_gaussian_mv(..., missing="skip"); the context option mv_y_missing), for the three observation families
and BPF, APF and RMPF -- the reference the device's pf_run_mv / k_pf_batch_mv are compared with when y holds NaN.

A NaN in y[i, k] means that component k of observation i was not observed.  In the reference the user's log_likelihood_fn returns
0 for what was not seen; here that is the family's log-likelihood with the missing components left out of its sum:

  log-likelihood of a particle: l = 0.0;  l = l + density_k  for the OBSERVED k, in increasing k    (p == 0: the constant c0)
  a row with nothing observed:  l = 0.0 for every particle; the core then does what it always does (normalisation, log-likelihood
                                increment log(N) - log(N) = 0, ESS = N, resample decision, resampling, the move accepts every
                                proposal because log(u) < 0 - 0)

The filter is tests/mv_tv_restated.py's pf_run_mv_tv, unedited, run with mv_apf_rmpf_restated.loglik replaced for the call by
loglik_skip below -- the technique tests/mv_obs_restated.py uses for the families (its note on how the two files reach that
function applies here word for word).  eta_k and the densities are that file's, operation for operation."""
import contextlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402
import mv_obs_restated as OB  # noqa: E402
import mv_tv_restated as TV  # noqa: E402


def loglik_skip(obs, q, y, x):
    """mv_obs_restated.obs_loglik (mv_apf_rmpf_restated.loglik for obs == "gaussian") over the observed components of y only"""
    assert obs in OB.OBS
    if q["p"] == 0:
        return np.full(x.shape[1], q["c0"])
    l = np.zeros(x.shape[1])
    for k in range(q["p"]):
        yk = float(y[k])
        if math.isnan(yk):                                         # not observed: neither eta_k nor a density
            continue
        eta = np.full(x.shape[1], q["h0"][k])
        for c in range(q["d"]):
            eta = eta + q["H"][k, c] * x[c]
        if obs == "gaussian":
            l = l + R.dnorm_log(yk, eta, q["sd"][k], np.log(q["sd"][k]))
        elif obs == "poisson":
            l = l + OB.dpois_log_eta(yk, eta, math.lgamma(yk + 1.0))
        else:
            l = l + OB.dlogvar_log_eta(yk, eta)
    return l


@contextlib.contextmanager
def _skipping(obs):
    saved = R.loglik
    R.loglik = lambda q, y, x: loglik_skip(obs, q, y, x)
    try:
        yield
    finally:
        R.loglik = saved


def pf_run_mv_missing(oracle, obs, theta, y, N, z_init, z_trans, u_res, **kw):
    """mv_obs_restated.pf_run_mv_obs (same arguments and result) for a y that may hold NaN"""
    assert not np.any(np.isinf(np.asarray(y, dtype=np.float64))), "+-inf is refused everywhere"
    with _skipping(obs):
        return TV.pf_run_mv_tv(oracle, theta, y, N, z_init, z_trans, u_res, **kw)


def kalman_missing(q, ys, obs_times=None):
    """Exact Kalman filter of the constant Gaussian model with missing data: the update of observation i uses the observed rows of
    H (and of h0, sd) only; a row with nothing observed is a prediction step alone.  Returns (log-likelihood, filtering means
    [T][d]); q: the unpacked block (mv_apf_rmpf_restated.unpack)."""
    d = q["d"]
    m, P = q["m0"].astype(np.float64).copy(), q["L0"] @ q["L0"].T
    Q = q["L"] @ q["L"].T
    ll, means, prev_t = 0.0, [], 0
    for i in range(1, len(ys) + 1):
        ot = int(obs_times[i - 1]) if obs_times is not None else i
        for _ in range(prev_t + 1, ot + 1):
            m, P = q["A"] @ m + q["b"], q["A"] @ P @ q["A"].T + Q
        prev_t = ot
        yi = np.atleast_1d(ys[i - 1])
        seen = ~np.isnan(yi)
        if seen.any():
            H, h0, Rm = q["H"][seen], q["h0"][seen], np.diag(q["sd"][seen] ** 2)
            S = H @ P @ H.T + Rm
            e = yi[seen] - (h0 + H @ m)
            ll += -0.5 * (len(e) * np.log(2 * np.pi) + np.linalg.slogdet(S)[1] + e @ np.linalg.solve(S, e))
            K = P @ H.T @ np.linalg.inv(S)
            m, P = m + K @ e, (np.eye(d) - K @ H) @ P
        means.append(m.copy())
    return float(ll), np.array(means)
