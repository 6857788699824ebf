"""What tau-leaping (models.reaction_network(..., method="tau_leap", leaps=K)) puts in the place of Gillespie's direct method in the
numpy restatement of the reaction-network family (tests/rnet_restated.py and what rnet_inc_restated.py, rnet_tv_restated.py and
rnet_nb_restated.py add to it), from the definition in DESIGN.md section 1d alone.  fp64, in the order written.

  transition   one unit of time for one particle, after the counters' reset (rnet_inc_restated, unchanged): for leap l = 0 .. K-1
                 a[0 .. R) = the propensities at the current x (rnet_restated.propensities with the rates of the moment)
                 for r = 0 .. R-1 in order:
                   lam = a[r] / K;  n = rpois(lam)
                   cap = min of x[c] over the species c with nu[r][c] < 0 (no cap if the reaction consumes nothing);  n = min(n, cap)
                   x[c] = x[c] + nu[r][c] * n  for every c
               The propensities are not recomputed inside a leap; the cap sees the x that the earlier reactions of the leap changed.
  rpois(lam)   for reaction r in leap l of call `call` and particle j, attempt a uses the Philox block at
                 (j, call, DRAW_TRANS | (((l * RNR + r) << 6 | a) << 8), stream),  u1 = u01(q.x, q.y),  u2 = u01(q.z, q.w),  RNR = 8
               not lam > 0: 0.0.   lam < 10: inversion by sequential search on u1 of attempt 0
                 p = exp(-lam); F = p; k = 0;  while u1 > F and k < 128: k = k + 1; p = p * lam / k; F = F + p;  return k
               lam >= 10: Hoermann's transformed rejection with squeeze (PTRS, 1993)
                 slam = sqrt(lam); loglam = log(lam); b = 0.931 + 2.53 slam; a_ = -0.059 + 0.02483 b
                 invalpha = 1.1239 + 1.1328 / (b - 3.4); vr = 0.9277 - 3.6224 / (b - 2)
                 attempts a = 0 .. 63:  U = u1 - 0.5; V = u2; us = 0.5 - |U|; k = floor((2 a_ / us + b) U + lam + 0.43)
                   accept if us >= 0.07 and V <= vr;  reject if k < 0 or (us < 0.013 and V > us)
                   accept if log(V) + log(invalpha) - log(a_ / us^2 + b) <= -lam + k loglam - lgamma(k + 1)
                 after 64 rejections floor(lam)

Everything else -- densities, look-ahead, counters, missing observations, schedule rows, the filter core -- is the other restatements',
untouched: they reach the transition through rnet_restated.make, which leaping(K) rebinds for the length of a with block.

counts (rnet_restated.make) additionally collects
  "zero", "inv", "ptrs"    draws by branch (not lam > 0, inversion, PTRS)
  "squeeze", "full"        PTRS accepts by the squeeze and by the full test
  "rejected"               PTRS attempts that were rejected
  "fallback"               PTRS draws that ran out of attempts
  "cap"                    draws that the cap cut"""
import contextlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_nb_restated as NB  # noqa: E402
import rnet_restated as RN  # noqa: E402
import rnet_tv_restated as RT  # noqa: E402
from rnet_restated import DRAW_TRANS, stream_word, u01_from_bits  # noqa: E402

RNR = 8
KEYS = ("zero", "inv", "ptrs", "squeeze", "full", "rejected", "fallback", "cap")


def new_counts():
    return {k: 0 for k in KEYS}


def rpois(oracle, key, sw, j, call, leap, r, lam, counts=None):
    """one draw; key: the two seed words, sw: the stream word"""
    def uniforms(a):
        w = oracle.philox4x32_10([j, call, DRAW_TRANS | ((((leap * RNR + r) << 6) | a) << 8), sw], key)
        return u01_from_bits(w[0], w[1]), u01_from_bits(w[2], w[3])

    def count(name):
        if counts is not None:
            counts[name] = counts.get(name, 0) + 1

    if not lam > 0.0:
        count("zero")
        return 0.0
    if lam < 10.0:
        count("inv")
        u1, _ = uniforms(0)
        p = math.exp(-lam)
        F = p
        k = 0.0
        while u1 > F and k < 128.0:
            k = k + 1.0
            p = p * lam / k
            F = F + p
        return k
    count("ptrs")
    slam = math.sqrt(lam)
    loglam = math.log(lam)
    b = 0.931 + 2.53 * slam
    a_ = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    for a in range(64):
        u1, u2 = uniforms(a)
        U = u1 - 0.5
        V = u2
        us = 0.5 - abs(U)
        k = math.floor((2.0 * a_ / us + b) * U + lam + 0.43)
        if us >= 0.07 and V <= vr:
            count("squeeze")
            return float(k)
        if k < 0.0 or (us < 0.013 and V > us):
            count("rejected")
            continue
        if math.log(V) + math.log(invalpha) - math.log(a_ / (us * us) + b) <= -lam + k * loglam - math.lgamma(k + 1.0):
            count("full")
            return float(k)
        count("rejected")
    count("fallback")
    return float(math.floor(lam))


def sample(oracle, seed, stream, call, leap, r, lam, counts=None):
    """what bssm_dump_rpois returns: the draws that particles 0 .. len(lam)-1 take for (call, leap, r)"""
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    sw = stream_word(stream)
    return np.array([rpois(oracle, key, sw, j, call, leap, r, float(v), counts) for j, v in enumerate(lam)])


_gillespie_make = RN.make


def make(K, oracle, seed, stream, counts=None):
    """rnet_restated.make with the tau-leap transition of K leaps; the densities are rnet_restated's"""
    _, ll, aux = _gillespie_make(oracle, seed, stream, counts)
    if counts is not None:
        for name in KEYS:
            counts.setdefault(name, 0)
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    sw = stream_word(stream)

    def transition(q, x, z):
        call = int(z[0, 0])
        x = np.array(x, dtype=np.float64)
        d, nr = q["d"], q["R"]
        nu = [[float(q["nu"][r, c]) for c in range(d)] for r in range(nr)]
        for j in range(x.shape[1]):
            xj = [float(v) for v in x[:, j]]
            for leap in range(K):
                a = RN.propensities(q, xj)
                for r in range(nr):
                    lam = a[r] / float(K)
                    n = rpois(oracle, key, sw, j, call, leap, r, lam, counts)
                    cap = math.inf
                    for c in range(d):
                        if nu[r][c] < 0.0 and xj[c] < cap:
                            cap = xj[c]
                    if cap < n:
                        n = cap
                        if counts is not None:
                            counts["cap"] += 1
                    for c in range(d):
                        xj[c] = xj[c] + nu[r][c] * n
            x[:, j] = xj
        return x

    return transition, ll, aux


@contextlib.contextmanager
def leaping(K):
    """inside, every restatement of the family (rnet_restated and the modules that build on its make) runs the tau-leap transition"""
    assert isinstance(K, int) and 1 <= K <= 1024
    saved = RN.make
    RN.make = lambda oracle, seed, stream, counts=None: make(K, oracle, seed, stream, counts)
    try:
        yield
    finally:
        RN.make = saved


def pf_run_rn(oracle, theta, y, N, u_res, K, nb=False, **kw):
    """rnet_tv_restated.pf_run_rn (nb: rnet_nb_restated.pf_run_rn, for a negative-binomial block) with K leaps per unit of time"""
    with leaping(K):
        return (NB if nb else RT).pf_run_rn(oracle, theta, y, N, u_res, **kw)
