"""Dev tool: what negative-binomial observations cost the reaction-network family (models.reaction_network(obs="negbin", size=)).
The same SEIR with the onsets counted (d = 5, R = 3, p = 1, counter C, y ~ rho C) under Poisson and under negative-binomial observations:
  single    one bootstrap filter, N = 2^16, T = 50, SISAR / stratified
  batched   512 filters x N = 1000, T = 100 from prepacked blocks (every filter its own size), with the host's time for the
            [F][T][p] tables c(t, k) (bssm_rn_nb_tables, what bssm_pf_run_batch calls) reported separately
  python tools/bench_rnet_nb.py [--mode single|batched|both] [--obs poisson|negbin|both] [--reps 5] [--warmup 2]
With --obs poisson the tool uses nothing this feature added, so it also runs against the parent's build (BAYESSSM_AMD_LIB) to compare
a commit with its parent.  Every case: `warmup` calls, then `reps` timed calls, the observation families alternating call by call;
every timed call's device_ms is printed (the spread is the point), with the median.  Prints one JSON line per case."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAR = dict(beta=0.001, sigma=0.5, gamma=0.2)
X0 = (430, 0, 70, 0, 0)
RHO = 0.6


def seir_c(B, **kw):
    return B.models.reaction_network(("S", "E", "I", "R", "C"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1, "C": 1}, "sigma"),
                                                                 ({"I": 1}, {"R": 1}, "gamma")], x0=X0, observe={"C": RHO}, counters=("C",), **kw)


def onset_counts(T):
    """round(rho * onsets of the day) along the rate equations (1/16 of a unit per Euler step), every fifth day doubled: overdispersed"""
    s, e, i = float(X0[0]), float(X0[1]), float(X0[2])
    out = []
    for t in range(T):
        c = 0.0
        for _ in range(16):
            inf, on, rec = PAR["beta"] * s * i / 16, PAR["sigma"] * e / 16, PAR["gamma"] * i / 16
            s, e, i, c = s - inf, e + inf - on, i + on - rec, c + on
        out.append(round(RHO * c * (2.0 if t % 5 == 4 else 1.0)))
    return np.array(out, dtype=np.float64)


def alternate(cases, reps, warmup):
    """cases: name -> fn() returning a result dict; the cases alternate call by call.  name -> (device_ms per timed call, wall ms per call, last result)"""
    dev, wall, last = {k: [] for k in cases}, {k: [] for k in cases}, {}
    for k in range(warmup + reps):
        for name, fn in cases.items():
            t0 = time.perf_counter()
            res = fn()
            w = (time.perf_counter() - t0) * 1e3
            last[name] = res
            if k >= warmup:
                wall[name].append(w)
                dev[name].append(res["device_ms"] if "device_ms" in res else res["_extras"]["device_ms"])
    return {k: (dev[k], wall[k], last[k]) for k in cases}


def report(case, obs, dev, wall, **more):
    print(json.dumps(dict({"case": case, "obs": obs, "lib": os.path.basename(os.path.dirname(os.environ.get("BAYESSSM_AMD_LIB", ""))) or "this build",
                           "device_ms": [round(v, 4) for v in dev], "median_device_ms": float(np.median(dev)), "min_device_ms": float(np.min(dev)),
                           "max_device_ms": float(np.max(dev)), "median_wall_ms": float(np.median(wall))}, **more)), flush=True)


def nets(B, which):
    out = {}
    if which in ("poisson", "both"):
        out["poisson"] = seir_c(B)                       # (no keyword: the parent's descriptor)
    if which in ("negbin", "both"):
        out["negbin"] = seir_c(B, obs="negbin", size="r")
    return out


def single(B, which, reps, warmup):
    N, T = 1 << 16, 50
    y = onset_counts(T)
    ms = nets(B, which)
    cases = {obs: (lambda m=m, obs=obs: B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SISAR",
                                                           resample_fn="stratified", return_particles=False, seed=1, stream=7,
                                                           **(dict(PAR, r=10.0) if obs == "negbin" else PAR))) for obs, m in ms.items()}
    got = alternate(cases, reps, warmup)
    for obs, (dev, wall, res) in got.items():
        report("single", obs, dev, wall, N=N, T=T, loglike=res["loglike"])
    if len(got) == 2:
        print(json.dumps({"case": "single", "negbin_over_poisson_median_device_ms": float(np.median(got["negbin"][0]) / np.median(got["poisson"][0]))}), flush=True)


def batched(B, which, reps, warmup):
    from bayesssm_amd import _lib
    F, N, T = 512, 1000, 100
    y = onset_counts(T)
    ms = nets(B, which)
    sizes = 2.0 + 0.05 * np.arange(F)                     # every filter its own size: F distinct tables
    blocks = {obs: np.ascontiguousarray(np.stack([m.pack(dict(PAR, r=float(sizes[f])) if obs == "negbin" else PAR) for f in range(F)])) for obs, m in ms.items()}
    cases = {obs: (lambda m=m, obs=obs: B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, blocks[obs], 1, None))
             for obs, m in ms.items()}
    got = alternate(cases, reps, warmup)
    more = {}
    if "negbin" in ms:                                     # the host's share: the tables alone, as pf_run_batch_rn fills them
        lib, m, blk = _lib.load(), ms["negbin"], blocks["negbin"]
        o_size = 3 + m.dim + 3 * m.R + m.R * m.dim + m.p * m.dim
        out = np.zeros((F, T, m.p))
        y2 = np.ascontiguousarray(y.reshape(T, m.p))
        host = []
        for k in range(warmup + reps):
            t0 = time.perf_counter()
            rc = lib.bssm_rn_nb_tables(y2.ctypes.data_as(C.c_void_p), T, m.p, F, C.c_void_p(blk.ctypes.data + 8 * o_size), blk.shape[1],
                                       out.ctypes.data_as(C.c_void_p))
            if k >= warmup:
                host.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        more = {"host_tables_ms": [round(v, 4) for v in host], "median_host_tables_ms": float(np.median(host)), "table_bytes": int(out.nbytes)}
    for obs, (dev, wall, res) in got.items():
        report("batched", obs, dev, wall, F=F, N=N, T=T, finite=int(np.isfinite(res["loglike"]).sum()), **(more if obs == "negbin" else {}))
    if len(got) == 2:
        print(json.dumps({"case": "batched", "negbin_over_poisson_median_device_ms": float(np.median(got["negbin"][0]) / np.median(got["poisson"][0])),
                          "negbin_over_poisson_median_wall_ms": float(np.median(got["negbin"][1]) / np.median(got["poisson"][1]))}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("single", "batched", "both"), default="both")
    ap.add_argument("--obs", choices=("poisson", "negbin", "both"), default="both")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import bayesssm_amd as B
    if a.mode in ("single", "both"):
        single(B, a.obs, a.reps, a.warmup)
    if a.mode in ("batched", "both"):
        batched(B, a.obs, a.reps, a.warmup)
