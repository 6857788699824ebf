"""Dev/bench tool: batched small filters of the multivariate linear-Gaussian family (bssm_pf_run_batch, k_pf_batch_mv) vs one
bssm_pf_run at a time on the same work, and the wall time of the reference's multi-dimensional PMMH call
(tests/testthat/test-pmmh.R:619-668) with and without batch_chains.

    python tools/bench_batch_mv.py [T]        (T: observations of the filter legs, default 1000)
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import bayesssm_amd as b  # noqa: E402


def model(d, p, seed=5):
    rng = np.random.default_rng(seed)
    q = dict(m0=np.zeros(d), L0=np.eye(d), A=0.8 * np.eye(d) + 0.05 * rng.standard_normal((d, d)), b=np.zeros(d),
             L=np.tril(0.2 * rng.standard_normal((d, d))) + 0.8 * np.eye(d), c0=1.0, H=rng.standard_normal((p, d)), h0=np.zeros(p),
             sd=1.0 + rng.random(p))
    A0 = q.pop("A")
    return b.models.linear_gaussian_mv(d, p, build=lambda a: {"A": a * A0}, param_names=("a",), **q), A0, q


def data(d, p, T, A0, q, seed=6):
    rng = np.random.default_rng(seed)
    x, ys = np.zeros(d), np.zeros((T, p))
    for t in range(T):
        x = A0 @ x + q["L"] @ rng.standard_normal(d)
        ys[t] = q["H"] @ x + q["sd"] * rng.standard_normal(p)
    return ys if p > 0 else np.zeros(T)


def leg(d, p, N, F, T, nsingle=4):
    m, A0, q = model(d, p)
    y = data(d, p, T, A0, q)
    ctx = b.Context(0, 2048, 8)
    kw = dict(resample_algorithm="SISAR", resample_fn="stratified", ctx=ctx)
    thetas = [{"a": 1.0}] * F
    b.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, thetas[:2], 1, **kw)     # warm-up
    t0 = time.perf_counter()
    out = b.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, thetas, 1, **kw)
    dt = time.perf_counter() - t0
    b.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, return_particles=False, seed=1, stream=0, a=1.0, **kw)
    t1 = time.perf_counter()
    for k in range(nsingle):
        r = b.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, return_particles=False, seed=1, stream=k, a=1.0, **kw)
        assert r["loglike"] == out["loglike"][k]
    ds = (time.perf_counter() - t1) / nsingle
    ctx.close()
    print("(d, p) = (%d, %d)  N=%5d F=%4d T=%d: batch %.1f ms (device %.1f ms) = %.1f filters/s, %.3f G particle-steps/s;"
          " one at a time %.2f ms/filter = %.1f filters/s, %.4f G particle-steps/s -> x%.0f"
          % (d, p, N, F, T, 1e3 * dt, out["device_ms"], F / dt, N * T * F / dt / 1e9, 1e3 * ds, 1 / ds, N * T / ds / 1e9, ds / (dt / F)),
          flush=True)


def pmmh_case():
    """tests/testthat/test-pmmh.R:619-668: 2-d random walk with mean phi, constant log-likelihood, phi ~ N(0, 1), m = 500, two chains"""
    m = b.models.linear_gaussian_mv(2, 0, c0=1.0, build=lambda phi: {"b": [phi, phi]}, param_names=("phi",))
    outs = {}
    for bc in (True, False):
        t0 = time.perf_counter()
        out = b.pmmh(b.bootstrap_filter, np.zeros(20), 500, m.init_fn, m.transition_fn, m.log_likelihood_fn, {"phi": b.prior_normal(0.0, 1.0)},
                     [{"phi": 0.8}, {"phi": 0.5}], 100, num_chains=2, param_transform={"phi": "identity"}, seed=1405, print_result=False,
                     batch_chains=bc)
        outs[bc] = (time.perf_counter() - t0, out)
    same = np.array_equal(np.asarray(outs[True][1]["theta_chain"]["phi"]), np.asarray(outs[False][1]["theta_chain"]["phi"]))
    print("pmmh test-pmmh.R:619-668 (m = 500, 2 chains, pilot_m = 2000, pilot_reps = 100, T = 20): batch_chains=True %.2f s (%d launches),"
          " batch_chains=False %.2f s -> x%.1f; theta_chain identical: %s"
          % (outs[True][0], outs[True][1]["_extras"]["batched_launches"], outs[False][0], outs[False][0] / outs[True][0], same), flush=True)


if __name__ == "__main__":
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    for d, p in ((2, 0), (3, 2), (8, 8)):
        leg(d, p, 1000, 512, T)
    leg(3, 2, 100, 100, T)                   # the pilot's shape: pilot_reps = 100 filters at pilot_n = 100
    pmmh_case()
