"""What counter species and missing observations add to the numpy restatement of the reaction-network family (tests/rnet_restated.py),
from the definition in DESIGN.md section 1d and rnet.hip.h alone:

  counters   transition_fn(particles, t) sets every counter component to 0.0 before its Gillespie loop if and only if it is the first
             call of the gap loop of R/particle_filter_core.R:125-136 (step == 1).  The restated transition learns its call number
             from z (rnet_restated), so the set of such call numbers is computed from obs_times and the algorithm: the gap loop of
             observation i starts at the running call count when gap >= 1; a repeated time (gap <= 0) has no such call; the auxiliary
             filter's second-stage transition (:159) takes one more call per observation and never resets.
  missing    a NaN in y_k is a component that was not observed: the log-likelihood (and the look-ahead) is rnet_restated's over the
             observed components alone, in their order; a row with nothing observed gives 0.0.

The packed block may end in the tail reset[d] of 0.0 / 1.0; rnet_restated.unpack takes the block without it."""
import contextlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_restated as RN  # noqa: E402
from rnet_restated import R, TV  # noqa: E402


def split(theta):
    """(the block in rnet_restated's layout, reset[d] or None)"""
    th = np.asarray(theta, dtype=np.float64)
    d, nr, p = int(th[0]), int(th[1]), int(th[2])
    n = 3 + d + 3 * nr + nr * d + p * d
    assert th.size in (n, n + d)
    return th[:n], (th[n:] if th.size == n + d else None)


def first_calls(T, obs_times, algorithm):
    """the transition-call numbers that are the first of a gap loop"""
    out, k, prev_t = set(), 0, 0
    for i in range(1, T + 1):
        ot = int(obs_times[i - 1]) if obs_times is not None else i
        gap = ot - prev_t
        prev_t = ot
        if gap >= 1:
            out.add(k)
        k += max(gap, 0)
        if algorithm == "APF":
            k += 1                                                 # :159, never a first step
    return out


def make(oracle, seed, stream, reset, first, counts=None):
    """rnet_restated.make with the counters' reset in front of the transition and the densities over the observed components"""
    trans, ll, aux = RN.make(oracle, seed, stream, counts)

    def transition(q, x, z):
        if reset is not None and int(z[0, 0]) in first:
            x = np.array(x, dtype=np.float64)
            x[reset != 0.0] = 0.0
        return trans(q, x, z)

    def observed(f):
        def g(q, y, x):
            seen = ~np.isnan(np.asarray(y, dtype=np.float64))
            return f(dict(q, p=int(seen.sum()), G=q["G"][seen]), np.asarray(y)[seen], x)      # (p = 0: the sum from 0.0 over nothing)
        return g

    return transition, observed(ll), observed(aux)


@contextlib.contextmanager
def _family(oracle, seed, stream, reset, first, counts=None):
    saved = (R.unpack, R.transition, R.loglik, R.aux_loglik)
    R.unpack = RN.unpack
    R.transition, R.loglik, R.aux_loglik = make(oracle, seed, stream, reset, first, counts)
    try:
        yield
    finally:
        R.unpack, R.transition, R.loglik, R.aux_loglik = saved


def pf_run_rn(oracle, theta, y, N, u_res, seed=0, stream=0, algorithm="BPF", counts=None, **kw):
    """rnet_restated.pf_run_rn for a block with or without the tail and a y that may hold NaN"""
    assert algorithm in ("BPF", "APF")
    base, reset = split(theta)
    q = RN.unpack(base)
    y = np.asarray(y, dtype=np.float64).reshape(-1, q["p"])
    T = y.shape[0]
    ot = kw.get("obs_times")
    ncalls = (int(ot[-1]) if ot is not None and T else T) + T + 1
    z_trans = np.repeat(np.arange(ncalls, dtype=np.float64), q["d"] * N).reshape(ncalls, q["d"], N)
    with _family(oracle, int(seed), int(stream), reset, first_calls(T, ot, algorithm), counts):
        return TV.pf_run_mv_tv(oracle, base, y, N, np.zeros((q["d"], N)), z_trans, u_res, algorithm=algorithm, **kw)
