"""CPU restatement of the reaction-network family's closures (include/bayesssm_amd.h, BSSM_MODEL_RNET) in numpy, from the
definitions alone, plugged into tests/mv_tv_restated.py's restated .particle_filter_core the way mv_obs_restated.py plugs its
densities in: the core reaches unpack / transition / loglik / aux_loglik through the module object mv_apf_rmpf_restated, looked
up at call time, so rebinding them inside a with block swaps the model.

Draws: one Philox4x32-10 block (the oracle's independent C restatement) per event at the counter
(particle, call, DRAW_TRANS | event << 8, stream) under the key (seed low, seed high); u01 from a pair of words as rng.h's
u01_from_bits.  The core hands transition() the injected normals of the call; here every entry of z_trans[k] is k, which is how
the transition learns its call number.  z_init is zeros over L0 = 0, so the core's init gives x0."""
import contextlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402
import mv_tv_restated as TV  # noqa: E402

DRAW_TRANS = 2


def u01_from_bits(lo, hi):
    b = (int(hi) << 32) | int(lo)
    return (float(b >> 11) + 0.5) * 2.0 ** -53


def stream_word(stream):
    return (stream & 0xFFFFFFFF) ^ (((stream >> 32) * 0x9E3779B9) & 0xFFFFFFFF)


def unpack(theta):
    th = np.asarray(theta, dtype=np.float64)
    d, nr, p = int(th[0]), int(th[1]), int(th[2])
    o = 3
    q = {"d": d, "R": nr, "p": p}
    q["x0"] = th[o:o + d]; o += d
    q["k"] = th[o:o + nr]; o += nr
    q["s1"] = th[o:o + nr].astype(int); o += nr
    q["s2"] = th[o:o + nr].astype(int); o += nr
    q["nu"] = th[o:o + nr * d].reshape(nr, d); o += nr * d
    q["G"] = th[o:o + p * d].reshape(p, d); o += p * d
    assert o == th.size
    q["m0"], q["L0"] = q["x0"], np.zeros((d, d))          # the core's init: x0 + 0 z
    return q


def propensities(q, x):
    a = []
    for r in range(q["R"]):
        v = float(q["k"][r])
        if q["s1"][r] >= 0:
            v = v * x[q["s1"][r]]
        if q["s2"][r] >= 0:
            v = v * x[q["s2"][r]]
        a.append(v if v > 0.0 else 0.0)
    return a


def dpois_log(y, lam, lgy):
    if lam <= 0.0:
        return 0.0 if (y == 0.0 and lam == 0.0) else -math.inf
    if y == 0.0:
        return -lam
    return y * math.log(lam) - lam - lgy


def make(oracle, seed, stream, counts=None):
    """(transition, loglik, aux_loglik) in the signatures of mv_apf_rmpf_restated, drawing under (seed, stream).
    counts: a dict that, when given, collects "fired" (how often each reaction index was chosen, over all particles and calls)
    and "n_inf" (per log_likelihood call, the number of particles whose log-weight is -inf)"""
    if counts is not None:
        counts.setdefault("fired", {})
        counts.setdefault("n_inf", [])
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    sw = stream_word(stream)

    def transition(q, x, z):
        call = int(z[0, 0])
        x = np.array(x, dtype=np.float64)
        d, nr = q["d"], q["R"]
        for j in range(x.shape[1]):
            xj = [float(v) for v in x[:, j]]
            t, ev = 0.0, 0
            while t < 1.0 and ev < (1 << 20):
                a = propensities(q, xj)
                total = a[0]
                for r in range(1, nr):
                    total = total + a[r]
                if total <= 0.0:
                    break
                w = oracle.philox4x32_10([j, call, DRAW_TRANS | (ev << 8), sw], key)
                dt = -math.log(u01_from_bits(w[0], w[1])) / total
                if t + dt > 1.0:
                    break
                t = t + dt
                u = u01_from_bits(w[2], w[3])
                rsel, cum = nr - 1, a[0]
                for r in range(nr - 1):
                    if r > 0:
                        cum = cum + a[r]
                    if u < cum / total:
                        rsel = r
                        break
                for c in range(d):
                    xj[c] = xj[c] + float(q["nu"][rsel, c])
                if counts is not None:
                    counts["fired"][rsel] = counts["fired"].get(rsel, 0) + 1
                ev += 1
            x[:, j] = xj
        return x

    def _ll(q, y, x, aux):
        out = np.empty(x.shape[1])
        for j in range(x.shape[1]):
            xj = [float(v) for v in x[:, j]]
            if aux:
                a = propensities(q, xj)
                m = []
                for c in range(q["d"]):
                    v = xj[c]
                    for r in range(q["R"]):
                        v = v + float(q["nu"][r, c]) * a[r]
                    m.append(v)
                xj = m
            l = 0.0
            for k in range(q["p"]):
                lam = 0.0
                for c in range(q["d"]):
                    lam = lam + float(q["G"][k, c]) * xj[c]
                if aux:
                    lam = lam if lam > 0.0 else 0.0
                yk = float(y[k])
                l = l + dpois_log(yk, lam, math.lgamma(yk + 1.0))
            out[j] = l
        if counts is not None and not aux:
            counts["n_inf"].append(int(np.sum(out == -math.inf)))
        return out

    return transition, (lambda q, y, x: _ll(q, y, x, False)), (lambda q, y, x: _ll(q, y, x, True))


@contextlib.contextmanager
def _family(oracle, seed, stream, counts=None):
    saved = (R.unpack, R.transition, R.loglik, R.aux_loglik)
    R.unpack = unpack
    R.transition, R.loglik, R.aux_loglik = make(oracle, seed, stream, counts)
    try:
        yield
    finally:
        R.unpack, R.transition, R.loglik, R.aux_loglik = saved


def pf_run_rn(oracle, theta, y, N, u_res, seed=0, stream=0, algorithm="BPF", counts=None, **kw):
    """mv_tv_restated.pf_run_mv_tv for a reaction network's packed block; u_res injected, the Gillespie draws keyed by (seed, stream);
    counts: see make()"""
    assert algorithm in ("BPF", "APF")
    q = unpack(theta)
    y = np.asarray(y, dtype=np.float64).reshape(-1, q["p"])
    T = y.shape[0]
    ot = kw.get("obs_times")
    ncalls = (int(ot[-1]) if ot is not None and T else T) + T + 1
    z_trans = np.repeat(np.arange(ncalls, dtype=np.float64), q["d"] * N).reshape(ncalls, q["d"], N)
    with _family(oracle, int(seed), int(stream), counts):
        return TV.pf_run_mv_tv(oracle, theta, y, N, np.zeros((q["d"], N)), z_trans, u_res, algorithm=algorithm, **kw)
