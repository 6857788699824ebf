"""What a rate schedule adds to the numpy restatement of the reaction-network family (tests/rnet_restated.py, with
tests/rnet_inc_restated.py's counters and missing observations), from the definition in DESIGN.md section 1d alone:

  schedule   M[n_times][R] of multipliers.  The transition TO absolute time tau uses row tau - 1: the propensity of reaction r
             starts from  k_r * M[tau - 1][r]  and goes on as rnet_restated.propensities does (times x[s1], times x[s2], not > 0
             counts as 0.0).  Here the row enters as the rate vector k * M[tau - 1] handed to the unchanged routines: the one
             new multiplication, in front of the others.
  tau        prev_t + step in the gap loop of R/particle_filter_core.R:125-136; the observation's time for the auxiliary filter's
             second-stage transition (:159) and for the propensities of its look-ahead (the Euler mean).  The restated transition
             learns its call number from z (rnet_restated), so the map call -> (tau, kind) is computed from obs_times and the
             algorithm; the look-ahead is called once per observation, in order.

The packed block may end in reset[d] (rnet_inc_restated) and then n_times, M[n_times][R].
counts (rnet_restated.make) additionally collects "rows": one (kind, call, row) per schedule row read, kind in "gap" | "second" |
"aux" (call is the observation number for "aux")."""
import contextlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_inc_restated as RI  # noqa: E402
import rnet_restated as RN  # noqa: E402
from rnet_restated import R, TV  # noqa: E402


def split(theta):
    """(the block in rnet_restated's layout, reset[d] or None, M[n_times][R] or None)"""
    th = np.asarray(theta, dtype=np.float64)
    d, nr, p = int(th[0]), int(th[1]), int(th[2])
    n = 3 + d + 3 * nr + nr * d + p * d
    if th.size in (n, n + d):
        base, reset = RI.split(th)
        return base, reset, None
    nt = int(th[n + d])
    assert nt >= 1 and th.size == n + d + 1 + nt * nr
    return th[:n], th[n:n + d], th[n + d + 1:].reshape(nt, nr)


def call_times(T, obs_times, algorithm):
    """({transition call number: (tau, "gap" | "second")}, [tau of the look-ahead at observation 1 .. T])"""
    calls, aux, k, prev_t = {}, [], 0, 0
    for i in range(1, T + 1):
        ot = int(obs_times[i - 1]) if obs_times is not None else i
        for step in range(1, ot - prev_t + 1):
            calls[k] = (prev_t + step, "gap"); k += 1
        prev_t = ot
        aux.append(ot)
        if algorithm == "APF":
            calls[k] = (ot, "second"); k += 1                      # :159
    return calls, aux


def make(oracle, seed, stream, reset, first, M, calls, aux_times, counts=None):
    """rnet_inc_restated.make with the rates of the moment"""
    trans, ll, aux = RI.make(oracle, seed, stream, reset, first, counts)
    if counts is not None:
        counts.setdefault("rows", [])
    seen = {"aux": 0}

    def at(q, tau):
        assert tau >= 1
        return q if M is None else dict(q, k=q["k"] * M[tau - 1])

    def transition(q, x, z):
        call = int(z[0, 0])
        tau, kind = calls[call]
        if counts is not None and M is not None:
            counts["rows"].append((kind, call, tau - 1))
        return trans(at(q, tau), x, z)

    def aux_loglik(q, y, x):
        i = seen["aux"]; seen["aux"] += 1
        if counts is not None and M is not None:
            counts["rows"].append(("aux", i + 1, aux_times[i] - 1))
        return aux(at(q, aux_times[i]), y, x)

    return transition, ll, aux_loglik


@contextlib.contextmanager
def _family(oracle, seed, stream, reset, first, M, calls, aux_times, counts=None):
    saved = (R.unpack, R.transition, R.loglik, R.aux_loglik)
    R.unpack = RN.unpack
    R.transition, R.loglik, R.aux_loglik = make(oracle, seed, stream, reset, first, M, calls, aux_times, counts)
    try:
        yield
    finally:
        R.unpack, R.transition, R.loglik, R.aux_loglik = saved


def pf_run_rn(oracle, theta, y, N, u_res, seed=0, stream=0, algorithm="BPF", counts=None, **kw):
    """rnet_inc_restated.pf_run_rn for a block with or without the tails"""
    assert algorithm in ("BPF", "APF")
    base, reset, M = split(theta)
    q = RN.unpack(base)
    y = np.asarray(y, dtype=np.float64).reshape(-1, q["p"])
    T = y.shape[0]
    ot = kw.get("obs_times")
    last = (int(ot[-1]) if ot is not None else T) if T else 0
    assert M is None or M.shape[0] >= last, "the schedule must reach the last observation time"
    ncalls = last + T + 1
    z_trans = np.repeat(np.arange(ncalls, dtype=np.float64), q["d"] * N).reshape(ncalls, q["d"], N)
    calls, aux_times = call_times(T, ot, algorithm)
    if reset is not None and not reset.any():
        reset = None
    with _family(oracle, int(seed), int(stream), reset, RI.first_calls(T, ot, algorithm), M, calls, aux_times, counts):
        return TV.pf_run_mv_tv(oracle, base, y, N, np.zeros((q["d"], N)), z_trans, u_res, algorithm=algorithm, **kw)
