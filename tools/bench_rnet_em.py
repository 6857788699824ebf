"""Dev tool: Euler-multinomial leaps (models.reaction_network(method="euler_multinomial", leaps=K)) against tau-leaping at the same K, on
tools/bench_rnet_leap.py's SEIR (d = 4, R = 3, p = 1, x0 scaled to a population n, beta scaled by 1 / n) and with its timing loop:
  single    one bootstrap filter, N = 2^16, T = 50, SISAR / stratified: device time per observation
  batched   512 filters x N = 1000, T = 50 in k_pf_batch_rn: device time per observation
  bias      the log-likelihood estimate over --seeds seeds (N = 4096, T = 20) under Gillespie and, for K in {4, 16, 64}, under tau-leaping and
            under Euler-multinomial leaps from the same seeds: mean and spread of each, and the difference of the means to Gillespie's in
            units of Gillespie's spread
  python tools/bench_rnet_em.py --mode single|batched|bias [--pops 1e6] [--methods tau:16,em:16] [--reps 3] [--warmup 1]
A method is gillespie, tau:K or em:K.  The existing Gillespie and tau-leap filters are measured against the parent commit's library with
tools/bench_rnet_leap.py itself (BAYESSSM_AMD_LIB), which uses nothing this feature added.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_rnet_leap as L  # noqa: E402


def seir(B, n, method):
    if method == "gillespie" or not method.startswith("em:"):
        return L.seir(B, n, method.split(":")[-1])
    return B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                            ({"I": 1}, {"R": 1}, "gamma")], x0=(round(0.86 * n), 0, round(0.14 * n), 0), observe={"I": L.RHO},
                                     method="euler_multinomial", leaps=int(method[3:]))


def single(B, pops, methods, reps, warmup):
    N, T = 1 << 16, 50
    for n in pops:
        y = L.counts_of_i(n, T)
        ms = {k: seir(B, n, k) for k in methods}
        L.timed({k: (lambda m=m: B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SISAR", resample_fn="stratified",
                                                    return_particles=False, seed=1, stream=7, **L.par(n))) for k, m in ms.items()}, reps, warmup, T, case="single", pop=n, N=N)


def batched(B, pops, methods, reps, warmup):
    F, N, T = 512, 1000, 50
    for n in pops:
        y = L.counts_of_i(n, T)
        ms = {k: seir(B, n, k) for k in methods}
        draws = [dict(L.par(n), beta=(0.45 + 0.1 * f / F) / n) for f in range(F)]
        L.timed({k: (lambda m=m: B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, draws, 1, None)) for k, m in ms.items()},
                reps, warmup, T, case="batched", pop=n, F=F, N=N)


def bias(B, pops, seeds, leaps):
    N, T = 4096, 20
    for n in pops:
        y = L.counts_of_i(n, T)
        out = {}
        for k in ["gillespie"] + ["%s:%d" % (f, K) for K in leaps for f in ("tau", "em")]:
            m = seir(B, n, k)
            out[k] = np.array([B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SISAR", resample_fn="stratified",
                                                  return_particles=False, seed=100 + s, stream=s, **L.par(n))["loglike"] for s in range(seeds)])
        g = out["gillespie"]
        for k, v in out.items():
            print(json.dumps({"case": "bias", "pop": n, "N": N, "T": T, "seeds": seeds, "method": k, "mean_loglike": float(v.mean()), "sd_loglike": float(v.std(ddof=1)),
                              "mean_minus_gillespie_in_gillespie_sd": float((v.mean() - g.mean()) / g.std(ddof=1))}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("single", "batched", "bias"), required=True)
    ap.add_argument("--pops", default="1e6")
    ap.add_argument("--methods", default="tau:16,em:16")
    ap.add_argument("--leaps", default="4,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seeds", type=int, default=20)
    a = ap.parse_args()
    pops = [int(float(v)) for v in a.pops.split(",")]
    import bayesssm_amd as B
    if a.mode == "single":
        single(B, pops, a.methods.split(","), a.reps, a.warmup)
    elif a.mode == "batched":
        batched(B, pops, a.methods.split(","), a.reps, a.warmup)
    else:
        bias(B, pops, a.seeds, [int(v) for v in a.leaps.split(",")])
