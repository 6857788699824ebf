"""What negative-binomial observations add to the numpy restatement of the reaction-network family (tests/rnet_restated.py with
tests/rnet_inc_restated.py's counters and missing observations and tests/rnet_tv_restated.py's rate schedules), from the definition in
DESIGN.md section 1d alone.

  block      BSSM_MODEL_RNET's with size[p] directly after G[p][d], in front of the optional tails.
  density    component k: mu = lambda_k as the Poisson family forms it (0.0 + G_k0 x_0 + ..., for the look-ahead at the Euler mean and
             clamped at 0.0), r = size_k, c = (lgamma(y + r) - lgamma(r)) - lgamma(y + 1), and in this order
               if not mu > 0:  0.0 if (y == 0 and mu == 0) else -inf
               s = r + mu;  lr = log(r / s) if r < mu else log1p(-(mu / s))
               if y == 0:  r * lr
               (c + r * lr) + y * log(mu / s)
             summed from 0.0 over the observed components (a NaN y_k is one that was not observed).

The transition is rnet_tv_restated's, untouched.  The restatements offer no hook for the density, so the two log-likelihood loops are
restated here.  counts (rnet_restated.make) additionally collects, over log-likelihood and look-ahead calls alike:
  "lr_log", "lr_log1p"   how often each branch of lr was taken
  "y0"                   how often y == 0 was met on an observed component
  "mu0_inf"              how often the -inf case (mu == 0, y > 0) was met
  "clamped"              how often the look-ahead's clamp acted (a negative mu at the Euler mean)
and "n_inf" is, per log_likelihood call, the number of particles whose log-weight is -inf (as rnet_restated's)."""
import contextlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_inc_restated as RI  # noqa: E402
import rnet_restated as RN  # noqa: E402
import rnet_tv_restated as RT  # noqa: E402
from rnet_restated import R, TV  # noqa: E402

KEYS = ("lr_log", "lr_log1p", "y0", "mu0_inf", "clamped")


def table_c(y, r):
    """the host's table entry c(t, k)"""
    return (math.lgamma(y + r) - math.lgamma(r)) - math.lgamma(y + 1.0)


def dnbinom_log(y, mu, r, c=None, counts=None):
    """dnbinom(y, size = r, mu = mu, log = TRUE) in the definition's order; c: the table entry (computed when not given)"""
    if counts is not None and y == 0.0:
        counts["y0"] += 1
    if not mu > 0.0:
        if y == 0.0 and mu == 0.0:
            return 0.0
        if counts is not None and mu == 0.0:
            counts["mu0_inf"] += 1
        return -math.inf
    s = r + mu
    if r < mu:
        lr = math.log(r / s)
    else:
        lr = math.log1p(-(mu / s))
    if counts is not None:
        counts["lr_log" if r < mu else "lr_log1p"] += 1
    if y == 0.0:
        return r * lr
    if c is None:
        c = table_c(y, r)
    return (c + r * lr) + y * math.log(mu / s)


def split(theta):
    """(BSSM_MODEL_RNET's block: the negative-binomial block without size[p], tails kept;  size[p])"""
    th = np.asarray(theta, dtype=np.float64)
    d, nr, p = int(th[0]), int(th[1]), int(th[2])
    n = 3 + d + 3 * nr + nr * d + p * d
    assert th.size >= n + p
    return np.concatenate([th[:n], th[n + p:]]), th[n:n + p].copy()


def make(oracle, seed, stream, size, reset, first, M, calls, aux_times, counts=None):
    """rnet_tv_restated.make's transition with the negative-binomial densities"""
    transition = RT.make(oracle, seed, stream, reset, first, M, calls, aux_times, counts)[0]
    if counts is not None:
        for key in KEYS:
            counts.setdefault(key, 0)
    seen = {"aux": 0}

    def _ll(q, y, x, tau):
        """tau: None for log_likelihood; the observation's time for the look-ahead (the rates of its propensities)"""
        aux = tau is not None
        if aux and M is not None:
            q = dict(q, k=q["k"] * M[tau - 1])
        y = np.asarray(y, dtype=np.float64)
        out = np.empty(x.shape[1])
        for j in range(x.shape[1]):
            xj = [float(v) for v in x[:, j]]
            if aux:
                a = RN.propensities(q, xj)
                m = []
                for c in range(q["d"]):
                    v = xj[c]
                    for r in range(q["R"]):
                        v = v + float(q["nu"][r, c]) * a[r]
                    m.append(v)
                xj = m
            l = 0.0
            for k in range(q["p"]):
                yk = float(y[k])
                if yk != yk:                                   # not observed
                    continue
                mu = 0.0
                for c in range(q["d"]):
                    mu = mu + float(q["G"][k, c]) * xj[c]
                if aux:
                    if counts is not None and mu < 0.0:
                        counts["clamped"] += 1
                    mu = mu if mu > 0.0 else 0.0
                l = l + dnbinom_log(yk, mu, float(size[k]), None, counts)
            out[j] = l
        if counts is not None and not aux:
            counts["n_inf"].append(int(np.sum(out == -math.inf)))
        return out

    def loglik(q, y, x):
        return _ll(q, y, x, None)

    def aux_loglik(q, y, x):
        i = seen["aux"]; seen["aux"] += 1
        return _ll(q, y, x, aux_times[i])

    return transition, loglik, aux_loglik


@contextlib.contextmanager
def _family(*args, **kw):
    saved = (R.unpack, R.transition, R.loglik, R.aux_loglik)
    R.unpack = RN.unpack
    R.transition, R.loglik, R.aux_loglik = make(*args, **kw)
    try:
        yield
    finally:
        R.unpack, R.transition, R.loglik, R.aux_loglik = saved


def pf_run_rn(oracle, theta, y, N, u_res, seed=0, stream=0, algorithm="BPF", counts=None, **kw):
    """rnet_tv_restated.pf_run_rn for a negative-binomial block (with or without the tails)"""
    assert algorithm in ("BPF", "APF")
    pois, size = split(theta)
    base, reset, M = RT.split(pois)
    q = RN.unpack(base)
    assert size.shape == (q["p"],) and np.all(size > 0)
    y = np.asarray(y, dtype=np.float64).reshape(-1, q["p"])
    T = y.shape[0]
    ot = kw.get("obs_times")
    last = (int(ot[-1]) if ot is not None else T) if T else 0
    assert M is None or M.shape[0] >= last, "the schedule must reach the last observation time"
    ncalls = last + T + 1
    z_trans = np.repeat(np.arange(ncalls, dtype=np.float64), q["d"] * N).reshape(ncalls, q["d"], N)
    calls, aux_times = RT.call_times(T, ot, algorithm)
    if reset is not None and not reset.any():
        reset = None
    with _family(oracle, int(seed), int(stream), size, reset, RI.first_calls(T, ot, algorithm), M, calls, aux_times, counts):
        return TV.pf_run_mv_tv(oracle, base, y, N, np.zeros((q["d"], N)), z_trans, u_res, algorithm=algorithm, **kw)
