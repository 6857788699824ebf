"""Dev tool: what a rate schedule costs the reaction-network family (models.reaction_network(rate_schedule=)).
  python tools/bench_rnet_tv.py plain [--reps 5]     the no-schedule path: bootstrap_filter on the prevalence SEIR (d = 4, R = 3, no counters) and on
                                                     the SIR instance, N = 2^18, T = 50, SISAR / stratified -- run it once per library build
                                                     (BAYESSSM_AMD_LIB) to compare a commit with its parent
  python tools/bench_rnet_tv.py sched [--reps 5]     the same SEIR with a non-trivial schedule against without: one filter (N = 2^18, T = 50) and
                                                     512 batched filters x N = 1000, T = 1000 from prepacked blocks (device_ms and the call's wall time)
  python tools/bench_rnet_tv.py closure [--n 4096]   one SEIR-with-schedule bootstrap filter through a t-dependent host closure (closure mode)
                                                     against the device path, wall time
Every timed case: one warm-up call, then the median of `reps` calls.  Data: counts from the network's own rate equations.  Prints one
JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEIR_PAR = dict(beta=0.001, sigma=0.5, gamma=0.2)
X0 = (430, 0, 70, 0)


def season(T, R=3):
    """a seasonal transmission rate with a lockdown: column 0 moves, the others are 1.0"""
    M = np.ones((T, R))
    t = np.arange(T)
    M[:, 0] = (1.0 + 0.3 * np.sin(2 * np.pi * t / 25.0)) * np.where((t >= 20) & (t < 35), 0.4, 1.0)
    return M


def seir(B, sched=None):
    return B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                            ({"I": 1}, {"R": 1}, "gamma")], x0=X0, observe={"I": 0.6}, rate_schedule=sched)


def sir(B):
    return B.models.reaction_network(("S", "I"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {}, "gamma")], x0=(430, 70), observe={"I": 1.0})


def seir_counts(T, M=None, rho=0.6):
    """round(rho I) along the rate equations, one Euler step of 1/16 of a unit at a time"""
    s, e, i, r = [float(v) for v in X0]
    out = []
    for t in range(T):
        b = SEIR_PAR["beta"] * (M[t, 0] if M is not None else 1.0)
        for _ in range(16):
            inf, on, rec = b * s * i / 16, SEIR_PAR["sigma"] * e / 16, SEIR_PAR["gamma"] * i / 16
            s, e, i, r = s - inf, e + inf - on, i + on - rec, r + rec
        out.append(round(rho * i))
    return np.array(out, dtype=np.float64)


def sir_counts(T):
    s, i = 430.0, 70.0
    out = []
    for _ in range(T):
        for _ in range(16):
            inf, rec = 0.001 * s * i / 16, 0.2 * i / 16
            s, i = s - inf, i + inf - rec
        out.append(round(i))
    return np.array(out, dtype=np.float64)


def timed(fn, reps):
    """(median device_ms, median wall ms, last result) over reps calls after one warm-up"""
    dev, wall, res = [], [], None
    for k in range(reps + 1):
        t0 = time.perf_counter()
        res = fn(k)
        w = (time.perf_counter() - t0) * 1e3
        if k:
            wall.append(w); dev.append(res["device_ms"] if "device_ms" in res else res["_extras"]["device_ms"])
    return float(np.median(dev)), float(np.median(wall)), res


def plain(B, reps):
    N, T = 1 << 18, 50
    for name, m, par, y in (("seir", seir(B), SEIR_PAR, seir_counts(T)), ("sir", sir(B), dict(beta=0.001, gamma=0.2), sir_counts(T))):
        dev, wall, res = timed(lambda k: B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SISAR",
                                                            resample_fn="stratified", return_particles=False, seed=1, stream=7, **par), reps)
        print(json.dumps({"case": "plain_" + name, "lib": os.path.basename(os.environ.get("BAYESSSM_AMD_LIB", "")) or "this build", "N": N, "T": T, "median_device_ms": dev,
                          "median_wall_ms": wall, "loglike": res["loglike"]}), flush=True)


def sched(B, reps):
    N, T = 1 << 18, 50
    M = season(T)
    y = seir_counts(T, M)
    for name, m in (("none", seir(B)), ("ones", seir(B, np.ones((T, 3)))), ("season", seir(B, M))):
        dev, wall, res = timed(lambda k: B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SISAR",
                                                            resample_fn="stratified", return_particles=False, seed=1, stream=7, **SEIR_PAR), reps)
        print(json.dumps({"case": "single_" + name, "N": N, "T": T, "median_device_ms": dev, "median_wall_ms": wall, "loglike": res["loglike"]}), flush=True)
    F, N, T = 512, 1000, 1000
    M = season(T)
    y = seir_counts(T, M)
    for name, m in (("none", seir(B)), ("season", seir(B, M))):
        blocks = np.ascontiguousarray(np.stack([m.pack(SEIR_PAR)] * F))
        dev, wall, res = timed(lambda k: B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, blocks, 1, None), reps)
        print(json.dumps({"case": "batch_" + name, "F": F, "N": N, "T": T, "block_bytes": int(blocks.nbytes), "median_device_ms": dev,
                          "median_wall_ms": wall, "finite": int(np.isfinite(res["loglike"]).sum())}), flush=True)


def closure(B, n, reps):
    """closure mode: the same SEIR with the schedule read through `t` by a host Gillespie loop, one particle at a time (numpy's own draws)"""
    T = 10
    M = season(50)[15:25]                               # (the lockdown starts half way)
    y = seir_counts(T, M)
    nu = np.array([[-1, 1, 0, 0], [0, -1, 1, 0], [0, 0, -1, 1]], dtype=np.float64)
    rng = np.random.default_rng(3)

    def init_fn(num_particles):
        return np.tile(np.array(X0, dtype=np.float64), (num_particles, 1))

    def transition_fn(particles, t, beta, sigma, gamma):
        out = np.array(particles, dtype=np.float64)
        b = beta * M[t - 1, 0]
        for j in range(out.shape[0]):
            x, clock = out[j], 0.0
            while True:
                a = (b * x[0] * x[2], sigma * x[1], gamma * x[2])
                total = a[0] + a[1] + a[2]
                if total <= 0.0:
                    break
                clock += rng.exponential(1.0 / total)
                if clock > 1.0:
                    break
                u = rng.random() * total
                x += nu[0 if u < a[0] else 1 if u < a[0] + a[1] else 2]
        return out

    def log_likelihood_fn(y, particles):
        lam = 0.6 * particles[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(lam > 0, y * np.log(lam) - lam, np.where(y == 0, 0.0, -np.inf))

    t0 = time.perf_counter()
    res = B.bootstrap_filter(y, n, init_fn, transition_fn, log_likelihood_fn, return_particles=False, **SEIR_PAR)
    host = (time.perf_counter() - t0) * 1e3
    m = seir(B, M)
    _, wall, dres = timed(lambda k: B.bootstrap_filter(y, n, m.init_fn, m.transition_fn, m.log_likelihood_fn, return_particles=False, seed=1, stream=k,
                                                       **SEIR_PAR), reps)
    print(json.dumps({"case": "closure_vs_device", "N": n, "T": T, "closure_wall_ms": host, "device_wall_ms": wall, "ratio": host / wall,
                      "closure_loglike_up_to_a_constant": res["loglike"], "device_loglike": dres["loglike"]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("plain", "sched", "closure"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    a = ap.parse_args()
    import bayesssm_amd as B
    if a.what == "plain":
        plain(B, a.reps)
    elif a.what == "sched":
        sched(B, a.reps)
    else:
        closure(B, a.n, a.reps)
