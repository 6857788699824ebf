"""Dev tool: the reaction-network family's SIR instance against the built-in SIR on the same data, and SEIR's time.
  python tools/bench_rnet.py [--reps 7]
Shapes: C4's (N = 2^18, T = 200, auxiliary filter) and 512 filters x N = 1000, T = 200 through the batched kernel.  Every timed
case runs in a fresh process (one warm-up call, then the median of `reps` calls of the filter's device_ms).  Prints one line per
case and the ratios generic / built-in; informational, the built-in SIR stays the C4 path."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def models(B):
    n_total, i0 = 500, 70
    net = B.models.reaction_network(("S", "I"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {}, "gamma")], x0=(n_total - i0, i0),
                                    observe={"I": 1.0}, build=lambda lam, gamma: {"rates": {"beta": lam / n_total, "gamma": gamma}},
                                    param_names=("lam", "gamma"))
    seir = B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                            ({"I": 1}, {"R": 1}, "gamma")], x0=(n_total - i0, 0, i0, 0), observe={"I": 1.0})
    return {"sir": (B.models.sir(n_total, i0), {"lambda_": 0.5, "gamma": 0.2}, [[0.5, 0.2, n_total, n_total - i0, i0]]),
            "rnet_sir": (net, {"lam": 0.5, "gamma": 0.2}, [{"lam": 0.5, "gamma": 0.2}]),
            "rnet_seir": (seir, {"beta": 0.5 / n_total, "sigma": 0.5, "gamma": 0.2}, [{"beta": 0.5 / n_total, "sigma": 0.5, "gamma": 0.2}])}


def one(case, shape, reps):
    import numpy as np
    import bayesssm_amd as B
    m, par, theta = models(B)[case]
    rng = np.random.default_rng(4)
    T = 200
    y = np.round(70 + 60 * np.sin(np.arange(T) / 40.0) ** 2 + rng.random(T) * 5)
    times = []
    for k in range(reps + 1):
        if shape == "c4":
            r = B.auxiliary_filter(y, 1 << 18, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn,
                                   return_particles=False, seed=1, stream=k, **par)
            ms = r["_extras"]["device_ms"]
        else:
            th = theta * 512 if isinstance(theta[0], dict) else np.array(theta * 512)
            ms = B.bootstrap_filter_batch(y, 1000, m.init_fn, m.transition_fn, m.log_likelihood_fn, th, 1, None)["device_ms"]
        if k:
            times.append(ms)
    print(json.dumps({"case": case, "shape": shape, "median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times))}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--one", nargs=2)
    a = ap.parse_args()
    if a.one:
        one(a.one[0], a.one[1], a.reps)
        sys.exit(0)
    got = {}
    for shape in ("c4", "batch"):
        for case in ("sir", "rnet_sir", "rnet_seir"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one", case, shape],
                                 capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1]
            print(out)
            got[(case, shape)] = json.loads(out)["median_ms"]
        print("ratio generic / built-in (%s): %.3f" % (shape, got[("rnet_sir", shape)] / got[("sir", shape)]))
