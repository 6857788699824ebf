"""Dev/bench tool: what the Poisson and log-variance observation densities of the multivariate family cost against the Gaussian
one (models.linear_gaussian_mv(..., obs=...)), at tools/bench_mv_tv.py's shapes, (d, p) = (3, 2), SISAR + stratified:
  batch   512 filters x N = 1000, T = 1000 in one launch of k_pf_batch_mv (bootstrap_filter_batch)
  large   one filter at N = 2^20, T = 100 through pf_run_mv (bootstrap_filter): device time per observation
Every family filters data simulated from itself over the same latent model (bench_mv_tv.pieces with H scaled by 0.3, so that
exp(eta) stays moderate).  Device times are the HIP-event times the library reports; medians with the range over the repeats.
The checksum line of a leg compares two builds of the library on the same inputs.

    python tools/bench_mv_obs.py [repeats] [--gaussian-only] [--no-large]
(--gaussian-only: the Gaussian legs only -- for a build of the library that predates the families, selected with BAYESSSM_AMD_LIB)
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import bayesssm_amd as b  # noqa: E402
from bench_mv_tv import D, P, pieces, stats  # noqa: E402

F, N, T = 512, 1000, 1000
N_LARGE, T_LARGE = 1 << 20, 100


def model_pieces():
    q = pieces()
    q["H"] = 0.3 * q["H"]
    return q


def data(q, obs, n_obs, seed=6):
    rng = np.random.default_rng(seed)
    x, ys = np.zeros(D), np.zeros((n_obs, P))
    for t in range(n_obs):
        x = q["A"] @ x + q["b"] + q["L"] @ rng.standard_normal(D)
        eta = q["h0"] + q["H"] @ x
        ys[t] = (eta + q["sd"] * rng.standard_normal(P) if obs == "gaussian" else rng.poisson(np.exp(eta)) if obs == "poisson"
                 else np.exp(0.5 * eta) * rng.standard_normal(P))
    return ys


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 7
    families = ("gaussian",) if "--gaussian-only" in sys.argv else ("gaussian", "poisson", "logvar")
    print("library: %s" % b._lib.LIB_PATH)
    q = model_pieces()
    ctx_b, ctx_l = b.Context(0, 2048, 8), (None if "--no-large" in sys.argv else b.Context(0, N_LARGE, 8))
    med = {}
    for obs in families:
        m = b.models.linear_gaussian_mv(D, P, obs=obs, **q)
        y = data(q, obs, T)
        thetas = np.array([m.pack({})] * F)

        def run_batch():
            return b.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, thetas, 1, resample_algorithm="SISAR",
                                            resample_fn="stratified", ctx=ctx_b)
        run_batch()                                                   # warm-up
        outs = [run_batch() for _ in range(repeats)]
        med["batch", obs] = float(np.median([o["device_ms"] for o in outs]))
        print("batch %-8s %d filters x N = %d, T = %d: device %s" % (obs, F, N, T, stats([o["device_ms"] for o in outs])), flush=True)
        print("batch %-8s loglike sha256 %s (filter 0: %.12f; early returns: %d)" % (
            obs, hashlib.sha256(outs[-1]["loglike"].tobytes()).hexdigest()[:16], outs[-1]["loglike"][0], int(np.count_nonzero(outs[-1]["early_return_step"]))))
        if ctx_l is None:
            continue

        def run_large():
            return b.bootstrap_filter(y[:T_LARGE], N_LARGE, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SISAR",
                                      resample_fn="stratified", return_particles=False, seed=1, stream=0, ctx=ctx_l)
        run_large()
        outs = [run_large() for _ in range(repeats)]
        dev = [o["_extras"]["device_ms"] for o in outs]
        med["large", obs] = float(np.median(dev))
        print("large %-8s N = 2^20, T = %d: device %s = %.1f us per observation; loglike %.12f" % (
            obs, T_LARGE, stats(dev), 1e3 * med["large", obs] / T_LARGE, outs[-1]["loglike"]), flush=True)
    for leg in ("batch", "large"):
        for obs in families[1:]:
            if (leg, obs) in med:
                print("%s: %s / gaussian = %.4f" % (leg, obs, med[leg, obs] / med[leg, "gaussian"]))
    ctx_b.close()
    if ctx_l is not None:
        ctx_l.close()
