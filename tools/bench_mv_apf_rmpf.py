"""Bench tool: the multivariate linear-Gaussian family's bootstrap, auxiliary and resample-move filters on the device
(pf_run_mv), against the same auxiliary / resample-move runs in closure mode (closures.py: the model on the host, the particles
across PCIe at every observation) -- the route these models had before the device forms existed.

    python tools/bench_mv_apf_rmpf.py [N] [T]        (default N = 2^20, T = 100)

Device legs: particle-steps/s = N T / device_ms (the run's own event timing), median of 3 runs after a warm-up.  Closure legs:
wall time of one run.  The closure-mode move calls move_fn once per particle (R/particle_filter_core.R:226-234), so the RMPF
closure leg runs T_closure_rmpf = 2 observations and is reported per particle-step like the others.
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import bayesssm_amd as b  # noqa: E402

T_CLOSURE_RMPF = 2


def model(d, p, seed=5):
    rng = np.random.default_rng(seed)
    q = dict(m0=np.zeros(d), L0=np.eye(d), A=0.8 * np.eye(d) + 0.05 * rng.standard_normal((d, d)), b=np.zeros(d),
             L=np.tril(0.1 * rng.standard_normal((d, d))) + 0.4 * np.eye(d), c0=0.0, H=rng.standard_normal((p, d)), h0=np.zeros(p),
             sd=1.0 + rng.random(p))
    return b.models.linear_gaussian_mv(d, p, **q), q


def data(q, d, p, T, seed=6):
    rng = np.random.default_rng(seed)
    x, ys = np.zeros(d), np.zeros((T, p))
    for t in range(T):
        x = q["A"] @ x + q["L"] @ rng.standard_normal(d)
        ys[t] = q["H"] @ x + q["sd"] * rng.standard_normal(p)
    return ys


def closures(q, d, p, sd_move=0.1):
    rng = np.random.default_rng(7)
    A, L, H, sdo = q["A"], q["L"], q["H"], q["sd"]
    lsd = np.log(sdo)

    def init_fn(num_particles):
        return rng.standard_normal((num_particles, d))

    def transition_fn(particles):
        return particles @ A.T + rng.standard_normal(particles.shape) @ L.T

    def loglik(y, x):
        m = x @ H.T
        return np.sum(-(0.918938533204672741780329736406 + 0.5 * ((y - m) / sdo) ** 2 + lsd), axis=-1)

    def log_likelihood_fn(y, particles):
        return loglik(y, particles)

    def aux_log_likelihood_fn(y, particles):
        return loglik(y, particles @ A.T)

    def move_fn(particle, y):
        prop = particle + sd_move * rng.standard_normal(d)
        return prop if np.log(rng.random()) < loglik(y, prop) - loglik(y, particle) else particle

    return init_fn, transition_fn, log_likelihood_fn, aux_log_likelihood_fn, move_fn


def device_leg(m, alg, ys, N, ctx):
    kw = dict(resample_algorithm="SISAR", resample_fn="stratified", return_particles=False, ctx=ctx)
    ms = []
    for r in range(4):
        kw.update(seed=1405, stream=r)
        if alg == "BPF":
            res = b.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw)
        elif alg == "APF":
            res = b.auxiliary_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, **kw)
        else:
            kw.pop("resample_algorithm", None)
            res = b.resample_move_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.1), **kw)
        if r:                                              # (run 0: warm-up)
            ms.append(res["_extras"]["device_ms"])
    return float(np.median(ms))


def closure_leg(q, d, p, alg, ys, N):
    init_fn, transition_fn, ll_fn, aux_fn, move_fn = closures(q, d, p)
    t0 = time.perf_counter()
    if alg == "APF":
        b.auxiliary_filter(ys, N, init_fn, transition_fn, ll_fn, aux_fn, resample_fn="stratified", return_particles=False)
    else:
        b.resample_move_filter(ys, N, init_fn, transition_fn, ll_fn, move_fn, resample_fn="stratified", return_particles=False)
    return (time.perf_counter() - t0) * 1e3


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    ctx = b.Context(0, N, 8)
    print("N = %d, T = %d; particle-steps/s (device: median device_ms of 3 runs; closure mode: one run's wall time)" % (N, T))
    for d, p in ((3, 2), (8, 8)):
        m, q = model(d, p)
        ys = data(q, d, p, T)
        dev = {alg: device_leg(m, alg, ys, N, ctx) for alg in ("BPF", "APF", "RMPF")}
        rate = {alg: N * T / (dev[alg] * 1e-3) for alg in dev}
        line = "(d, p) = (%d, %d)  device: " % (d, p) + ", ".join("%s %.3e (%.2f ms/obs)" % (a, rate[a], dev[a] / T) for a in dev)
        line += "  | APF/BPF %.2fx, RMPF/BPF %.2fx" % (dev["APF"] / dev["BPF"], dev["RMPF"] / dev["BPF"])
        print(line, flush=True)
        for alg, Tc in (("APF", T), ("RMPF", T_CLOSURE_RMPF)):
            wall = closure_leg(q, d, p, alg, ys[:Tc], N)
            cr = N * Tc / (wall * 1e-3)
            print("(d, p) = (%d, %d)  closure mode %s: %.3e particle-steps/s (%.1f ms/obs over T = %d)  -> device is %.0fx" %
                  (d, p, alg, cr, wall / Tc, Tc, rate[alg] / cr), flush=True)


if __name__ == "__main__":
    main()
