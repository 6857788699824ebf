"""Dev/bench tool: what the time-varying b / h0 / H of the multivariate linear-Gaussian family cost.  Its `batch` leg is the
(d, p) = (3, 2) leg of tools/bench_batch_mv.py (the same pieces, F, N, T and settings), which cannot pass the arrays.

Two shapes at (d, p) = (3, 2), each WITHOUT and WITH the arrays (all three given, genuinely varying), repeated:
  batch   512 filters x N = 1000, T = 1000 through bootstrap_filter_batch (k_pf_batch_mv)
  large   one bootstrap filter, N = 2^20, T = 100 (k_step_mv and the scalar path's kernels)
and the same time-varying model as t-dependent closures in closure mode (N = 2^20, a few observations): the path such a
model took before.  Device times are the HIP-event times the library reports; medians with the range over the repeats.

    python tools/bench_mv_tv.py [repeats] [--no-tv] [--no-closures]
(--no-tv: only the legs without arrays -- for a build of the library that predates them, selected with BAYESSSM_AMD_LIB)
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import bayesssm_amd as b  # noqa: E402

D, P = 3, 2


def pieces(seed=5):
    rng = np.random.default_rng(seed)
    return dict(m0=np.zeros(D), L0=np.eye(D), A=0.8 * np.eye(D) + 0.05 * rng.standard_normal((D, D)), b=np.zeros(D),
                L=np.tril(0.2 * rng.standard_normal((D, D))) + 0.8 * np.eye(D), H=rng.standard_normal((P, D)), h0=np.zeros(P),
                sd=1.0 + rng.random(P))


def arrays(q, T, seed=7):
    rng = np.random.default_rng(seed)
    return {"b": 0.3 * rng.standard_normal((T, D)), "h0": 0.3 * rng.standard_normal((T, P)), "H": q["H"] + 0.2 * rng.standard_normal((T, P, D))}


def data(q, tv, T, seed=6):
    rng = np.random.default_rng(seed)
    x, ys = np.zeros(D), np.zeros((T, P))
    for t in range(T):
        x = q["A"] @ x + tv["b"][t] + q["L"] @ rng.standard_normal(D)
        ys[t] = tv["h0"][t] + tv["H"][t] @ x + q["sd"] * rng.standard_normal(P)
    return ys


def stats(v):
    v = np.sort(np.asarray(v))
    return "median %.3f ms (min %.3f, max %.3f, n = %d)" % (np.median(v), v[0], v[-1], v.size)


def leg(name, T, with_tv, repeats, run):
    q = pieces()
    tv = arrays(q, T)
    y = data(q, tv, T)
    m = b.models.linear_gaussian_mv(D, P, time_varying=tv if with_tv else None, **q)
    run(m, y)                                                     # warm-up
    dev, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        dev.append(run(m, y))
        wall.append(1e3 * (time.perf_counter() - t0))
    print("%-6s T=%4d %-14s device %s; wall %s" % (name, T, "with arrays" if with_tv else "without arrays", stats(dev), stats(wall)), flush=True)
    return float(np.median(dev))


def closures_leg(T, N):
    """the same model as t-dependent closures (vectorised numpy): host model evaluation, particles across PCIe per observation"""
    q = pieces()
    tv = arrays(q, T)
    y = data(q, tv, T)
    rng = np.random.default_rng(1)

    def init_fn(num_particles):
        return q["m0"] + rng.standard_normal((num_particles, D)) @ q["L0"].T

    def transition_fn(particles, t):
        return particles @ q["A"].T + tv["b"][t - 1] + rng.standard_normal(particles.shape) @ q["L"].T

    def log_likelihood_fn(y, particles, t):
        z = (y - (tv["h0"][t - 1] + particles @ tv["H"][t - 1].T)) / q["sd"]
        return -(0.918938533204672741780329736406 * P + 0.5 * (z * z).sum(axis=1) + np.log(q["sd"]).sum())

    t0 = time.perf_counter()
    b.bootstrap_filter(y, N, init_fn, transition_fn, log_likelihood_fn, return_particles=False)
    dt = time.perf_counter() - t0
    print("closure mode, the same time-varying model: N=%d T=%d: %.1f ms = %.2f ms per observation" % (N, T, 1e3 * dt, 1e3 * dt / T), flush=True)
    return 1e3 * dt / T


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 7
    modes = (False,) if "--no-tv" in sys.argv else (False, True)
    print("library: %s" % b._lib.LIB_PATH)
    ctx_b, ctx_l = b.Context(0, 2048, 8), b.Context(0, 1 << 20, 8)
    res = {}

    def run_batch(m, y):
        thetas = np.array([m.pack({})] * 512)
        return b.bootstrap_filter_batch(y, 1000, m.init_fn, m.transition_fn, m.log_likelihood_fn, thetas, 1, resample_algorithm="SISAR",
                                        resample_fn="stratified", ctx=ctx_b)["device_ms"]

    def run_large(m, y):
        return b.bootstrap_filter(y, 1 << 20, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SISAR",
                                  resample_fn="stratified", return_particles=False, seed=1, stream=0, ctx=ctx_l)["_extras"]["device_ms"]

    for with_tv in modes:
        res["batch", with_tv] = leg("batch", 1000, with_tv, repeats, run_batch)
        res["large", with_tv] = leg("large", 100, with_tv, repeats, run_large)
    if len(modes) == 2:
        for k in ("batch", "large"):
            print("%s: with arrays / without = %.4f" % (k, res[k, True] / res[k, False]))
    if "--no-closures" not in sys.argv:
        per_obs = closures_leg(5, 1 << 20)
        if ("large", True) in res:
            print("large, per observation: device descriptor %.3f ms, closure mode %.1f ms -> x%.0f" % (res["large", True] / 100, per_obs, per_obs / (res["large", True] / 100)))
    ctx_b.close(); ctx_l.close()
