"""Dev tool: Gillespie's direct method against tau-leaping (models.reaction_network(method="tau_leap", leaps=K)) as the population grows.
An SEIR (d = 4, R = 3, p = 1, y ~ Poisson(rho I)) with x0 scaled to a population n and beta scaled by 1 / n:
  single    one bootstrap filter, N = 2^16, T = 50, SISAR / stratified: device time per observation
  batched   512 filters x N = 1000, T = 50 in k_pf_batch_rn: device time per observation
  bound     Gillespie only, in the numpy restatement (tests/rnet_restated.py) with one particle: the events of each unit of time along one
            path, and whether any unit reached the 2^20-event bound at which rn_transition stops without a flag
  bias      the log-likelihood estimate over --seeds seeds (N = 4096, T = 20) under Gillespie and under K in {1, 4, 16, 64}: mean and
            spread of each, and the difference of the means in units of Gillespie's spread
  python tools/bench_rnet_leap.py --mode single|batched|bound|bias [--pops 1e3,1e5,1e6] [--methods gillespie,4,16] [--reps 3] [--warmup 1]
With --methods gillespie the tool uses nothing this feature added, so it also runs against the parent's build (BAYESSSM_AMD_LIB).
Every timed call's device_ms is printed with the median.  Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA, GAMMA, RHO = 0.5, 0.2, 0.6


def seir(B, n, method):
    kw = {} if method == "gillespie" else dict(method="tau_leap", leaps=int(method))
    return B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                            ({"I": 1}, {"R": 1}, "gamma")], x0=(round(0.86 * n), 0, round(0.14 * n), 0), observe={"I": RHO}, **kw)


def par(n):
    return dict(beta=0.5 / n, sigma=SIGMA, gamma=GAMMA)


def counts_of_i(n, T):
    """round(rho I) along the rate equations (1/16 of a unit per Euler step)"""
    s, e, i = 0.86 * n, 0.0, 0.14 * n
    out = []
    for _ in range(T):
        for _ in range(16):
            inf, on, rec = 0.5 / n * s * i / 16, SIGMA * e / 16, GAMMA * i / 16
            s, e, i = s - inf, e + inf - on, i + on - rec
        out.append(round(RHO * i))
    return np.array(out, dtype=np.float64)


def lib_name():
    return os.path.basename(os.path.dirname(os.environ.get("BAYESSSM_AMD_LIB", ""))) or "this build"


def timed(cases, reps, warmup, T, **more):
    """cases: name -> fn() returning a result dict; they alternate call by call"""
    dev = {k: [] for k in cases}
    for k in range(warmup + reps):
        for name, fn in cases.items():
            res = fn()
            if k >= warmup:
                dev[name].append(res["device_ms"] if "device_ms" in res else res["_extras"]["device_ms"])
    for name, v in dev.items():
        print(json.dumps(dict({"method": name, "lib": lib_name(), "device_ms": [round(x, 3) for x in v], "median_device_ms": float(np.median(v)),
                               "T": T, "us_per_observation": float(np.median(v)) * 1e3 / T}, **more)), flush=True)


def single(B, pops, methods, reps, warmup):
    N, T = 1 << 16, 50
    for n in pops:
        y = counts_of_i(n, T)
        ms = {k: seir(B, n, k) for k in methods}
        timed({k: (lambda m=m: B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SISAR", resample_fn="stratified",
                                                  return_particles=False, seed=1, stream=7, **par(n))) for k, m in ms.items()}, reps, warmup, T, case="single", pop=n, N=N)


def batched(B, pops, methods, reps, warmup):
    F, N, T = 512, 1000, 50
    for n in pops:
        y = counts_of_i(n, T)
        ms = {k: seir(B, n, k) for k in methods}
        draws = [dict(par(n), beta=(0.45 + 0.1 * f / F) / n) for f in range(F)]
        timed({k: (lambda m=m: B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, draws, 1, None)) for k, m in ms.items()},
              reps, warmup, T, case="batched", pop=n, F=F, N=N)


def bound(B, pops, units):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rnet_restated as RN
    from oracle import oracle as orc
    orc.build()
    for n in pops:
        m = seir(B, n, "gillespie")
        q = RN.unpack(m.pack(par(n)))
        x = np.array(q["x0"], dtype=np.float64).reshape(-1, 1)
        events, t0 = [], time.perf_counter()
        for call in range(units):
            c = {}
            x = RN.make(orc, 1, 7, c)[0](q, x, np.full((1, 1), float(call)))
            events.append(int(sum(c["fired"].values())))
        print(json.dumps({"case": "bound", "pop": n, "units": units, "events_per_unit": events, "reached_2_20": bool(max(events) >= (1 << 20)),
                          "restatement_s": round(time.perf_counter() - t0, 1)}), flush=True)


def bias(B, pops, seeds):
    N, T = 4096, 20
    for n in pops:
        y = counts_of_i(n, T)
        out = {}
        for k in ("gillespie", "1", "4", "16", "64"):
            m = seir(B, n, k)
            out[k] = np.array([B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SISAR", resample_fn="stratified",
                                                  return_particles=False, seed=100 + s, stream=s, **par(n))["loglike"] for s in range(seeds)])
        g = out["gillespie"]
        for k, v in out.items():
            print(json.dumps({"case": "bias", "pop": n, "N": N, "T": T, "seeds": seeds, "method": k, "mean_loglike": float(v.mean()), "sd_loglike": float(v.std(ddof=1)),
                              "mean_minus_gillespie_in_gillespie_sd": float((v.mean() - g.mean()) / g.std(ddof=1))}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("single", "batched", "bound", "bias"), required=True)
    ap.add_argument("--pops", default="1e3,1e5,1e6")
    ap.add_argument("--methods", default="gillespie,4,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--units", type=int, default=3)
    a = ap.parse_args()
    pops = [int(float(v)) for v in a.pops.split(",")]
    import bayesssm_amd as B
    if a.mode == "single":
        single(B, pops, a.methods.split(","), a.reps, a.warmup)
    elif a.mode == "batched":
        batched(B, pops, a.methods.split(","), a.reps, a.warmup)
    elif a.mode == "bound":
        bound(B, pops, a.units)
    else:
        bias(B, pops, a.seeds)
