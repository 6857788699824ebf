"""CPU restatement of .particle_filter_core (R/particle_filter_core.R:19-267) for the multivariate family with the Poisson and
log-variance observation densities (BSSM_MODEL_LGMV_POIS / BSSM_MODEL_LGMV_LOGVAR), with time-varying b, h0, H, for BPF, APF and
RMPF -- the reference the device's pf_run_mv / k_pf_batch_mv are compared with when models.linear_gaussian_mv(..., obs=...) is not
"gaussian".

The filter itself is tests/mv_tv_restated.py's pf_run_mv_tv, unedited: it evaluates the model through mv_apf_rmpf_restated.loglik
(directly, in aux_loglik at the transition mean, and twice in the move), so running it with THAT ONE FUNCTION replaced by the
family's (obs_loglik below) restates all three filters for the family; the replacement lasts for the call only.  Every family
shares the linear predictor, accumulated in the kernels' order (mv.hip.h, mv_obs_log):

  eta_k = (h0_k + H_k0 x_0) + H_k1 x_1 + ...
  gaussian   dnorm(y_k, eta_k, sd_k, log = TRUE), as mv_apf_rmpf_restated.dnorm_log
  poisson    lambda = exp(eta_k);  -inf unless lambda < +inf;  y_k == 0: -lambda;  else (y_k eta_k - lambda) - lgamma(y_k + 1)
  logvar     (-log(sqrt(2 pi)) - 0.5 eta_k) - (0.5 (y_k y_k)) exp(-eta_k);  the last term 0 when 0.5 (y_k y_k) == 0;  -inf for a
             non-finite eta_k
  log-likelihood of a particle: l = 0.0;  l = l + density_k  for k = 0 .. p-1
"""
import contextlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402
import mv_tv_restated as TV  # noqa: E402

OBS = ("gaussian", "poisson", "logvar")


def dpois_log_eta(y, eta, lgy):
    """dpois(y, exp(eta), log = TRUE) in the device's order of operations; y and lgy = lgamma(y + 1) scalars, eta an array"""
    eta = np.asarray(eta, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        lam = np.exp(eta)
        out = -lam if y == 0.0 else (y * eta - lam) - lgy
    return np.where(lam < np.inf, out, -np.inf)


def dlogvar_log_eta(y, eta):
    """dnorm(y, 0, exp(eta / 2), log = TRUE) in the device's order of operations; y a scalar, eta an array"""
    eta = np.asarray(eta, dtype=np.float64)
    hq = 0.5 * (y * y)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.zeros_like(eta) if hq == 0.0 else hq * np.exp(-eta)
        out = (-R.LN_SQRT_2PI - 0.5 * eta) - t
    return np.where(np.isfinite(eta), out, -np.inf)


def obs_loglik(obs, q, y, x):
    """mv_apf_rmpf_restated.loglik for the family `obs`"""
    assert obs in OBS
    if obs == "gaussian":
        return R.loglik(q, y, x)
    assert q["p"] > 0, "the Poisson / log-variance families need p >= 1"
    l = np.zeros(x.shape[1])
    for k in range(q["p"]):
        eta = np.full(x.shape[1], q["h0"][k])
        for c in range(q["d"]):
            eta = eta + q["H"][k, c] * x[c]
        yk = float(y[k])
        l = l + (dpois_log_eta(yk, eta, math.lgamma(yk + 1.0)) if obs == "poisson" else dlogvar_log_eta(yk, eta))
    return l


@contextlib.contextmanager
def _family(obs):
    """mv_apf_rmpf_restated.loglik = the family's, inside the with block.
    This relies on how the two imported files reach that function: mv_tv_restated calls `R.loglik(...)` on the module object and
    mv_apf_rmpf_restated.aux_loglik calls the module global `loglik`, both looked up at call time, so rebinding the module attribute
    reaches the log-likelihood, the APF's aux log-likelihood and the move's two evaluations.  A `from ... import loglik` in either
    file would bind the Gaussian function for good; test_mv_obs_cpu.py::test_families_run_through_the_three_filters_and_differ_from_gaussian
    would then fail (every family would give the Gaussian run)."""
    saved = R.loglik
    if obs != "gaussian":
        R.loglik = lambda q, y, x: obs_loglik(obs, q, y, x)
    try:
        yield
    finally:
        R.loglik = saved


def pf_run_mv_obs(oracle, obs, theta, y, N, z_init, z_trans, u_res, **kw):
    """mv_tv_restated.pf_run_mv_tv (same arguments and result; b_t / h0_t / H_t optional) for the observation family `obs`"""
    assert obs in OBS
    with _family(obs):
        return TV.pf_run_mv_tv(oracle, theta, y, N, z_init, z_trans, u_res, **kw)
