"""Dev tool: record the outputs of the single-filter runners behind bssm_pf_run (scalar models, multivariate family, reaction
networks) that tests/test_gpu_runner_golden.py holds a later build to, bit for bit.  Run it on a GPU with the build whose results
are the reference -- the commit BEFORE a change to the runners' host code (BAYESSSM_AMD_LIB selects another build of the library):
    python tools/record_runner_golden.py [OUT_DIR, default tests/golden]
One small .npz per case: loglike, loglike_history, ess, state_est, resampled and the early-return step of the run and, where the
case asks for them, ancestors, particles_history and weights_history.

Every case: N = 4096 + 777 (three scan workgroups, the last one partly filled), T = 6 at the times 1, 1, 3, 4, 4, 7 (a repeated
time twice, a gap of 2, a gap of 3).  The cases named dead_* make their second observation impossible (every log-weight below
-1e8, or a positive count of a species that is always 0): the run returns early at step 2, which the recorder asserts."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, T = 4096 + 777, 6
OBS_TIMES = np.array([1, 1, 3, 4, 4, 7], dtype=np.int32)
SEED = 1405
SCALARS = ("loglike", "loglike_history", "ess", "state_est")
LG_PAR = dict(phi=0.8, sigma_x=1.0, sigma_y=0.7)


def series(cols=None, counts=False):
    """T observations (a vector, or T x cols), the same for every case of a kind: an AR(1) path plus noise, or counts around 6"""
    rng = np.random.default_rng(SEED)
    shape = (T,) if cols is None else (T, cols)
    if counts:
        return rng.poisson(6.0, size=shape).astype(np.float64)
    x = np.cumsum(rng.standard_normal(shape), axis=0) * 0.5
    return x + 0.7 * rng.standard_normal(shape)


def lg_case(B, cx, algorithm="BPF", ra="SISR", rf="stratified", fused=None, hist=False, anc=False, inject=False, dead=False):
    m = B.models.linear_gaussian()
    y = series()
    if dead:
        y[1] = 1e6 * LG_PAR["sigma_y"]
    kw = dict(obs_times=OBS_TIMES, resample_fn=rf, return_particles=hist, return_ancestors=anc, seed=SEED, stream=3, ctx=cx, **LG_PAR)
    if inject:
        kw["draws"] = B.dump_draws(algorithm, T, N, rf, SEED, 5, obs_times=OBS_TIMES, ctx=cx)
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    if fused is not None:
        cx.set_option("fused", fused)
    try:
        if algorithm == "BPF":
            return B.bootstrap_filter(y, N, *fns, resample_algorithm=ra, **kw)
        if algorithm == "APF":
            return B.auxiliary_filter(y, N, *fns, m.aux_log_likelihood_fn, resample_algorithm=ra, **kw)
        # (resample_move_filter drops resample_algorithm, as the reference does; the core takes it, and the library must force SISR)
        return B.particle_filter_core(y, N, "lg", [LG_PAR[k] for k in ("phi", "sigma_x", "sigma_y")], "RMPF", OBS_TIMES, ra, rf, None, hist,
                                      anc, SEED, 3, kw.get("draws"), cx, move_sd=0.3)
    finally:
        if fused is not None:
            cx.set_option("fused", 1)


def sir_case(B, cx):
    m = B.models.sir(500, 70)
    y = np.array([70, 75, 90, 100, 95, 120], dtype=np.float64)
    return B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, obs_times=OBS_TIMES, resample_algorithm="SISAR",
                              resample_fn="systematic", return_particles=False, seed=SEED, stream=4, ctx=cx, **{"lambda": 0.6, "gamma": 0.2})


def mv_model(B, d, p, obs="gaussian", tv=False):
    rng = np.random.default_rng(SEED + 10 * d + p)
    A = 0.7 * np.eye(d) + 0.05 * rng.standard_normal((d, d))
    L = np.tril(0.3 * rng.standard_normal((d, d))) + 0.5 * np.eye(d)
    H = 0.3 * rng.standard_normal((p, d)) + np.eye(p, d) * (0.5 if obs != "gaussian" else 1.0)
    time_varying = None
    if tv:
        time_varying = {"b": 0.2 * rng.standard_normal((int(OBS_TIMES[-1]), d)), "h0": 0.1 * rng.standard_normal((T, p)),
                        "H": H[None] + 0.05 * rng.standard_normal((T, p, d))}
    return B.models.linear_gaussian_mv(d, p, obs=obs, time_varying=time_varying, A=A, L=L, H=H, b=0.1 * np.ones(d),
                                       h0=(1.0 if obs == "poisson" else 0.0) * np.ones(p), sd=0.8 * np.ones(p))


def mv_case(B, cx, d=3, p=2, algorithm="BPF", obs="gaussian", tv=False, hist=False, dead=False):
    m = mv_model(B, d, p, obs, tv)
    y = series(p, counts=obs == "poisson")
    if dead:
        y[1] = 1e6 * 0.8
    kw = dict(obs_times=OBS_TIMES, resample_fn="stratified", return_particles=hist, seed=SEED, stream=6, ctx=cx)
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    if algorithm == "BPF":
        return B.bootstrap_filter(y, N, *fns, resample_algorithm="SISAR", **kw)
    if algorithm == "APF":
        return B.auxiliary_filter(y, N, *fns, m.aux_log_likelihood_fn, resample_algorithm="SISAR", **kw)
    return B.resample_move_filter(y, N, *fns, m.rw_move_fn(0.3), **kw)


def rn_case(B, cx, algorithm="BPF", method="gillespie", obs="poisson", schedule=False, dead=False):
    """S + I -> E + I, E -> I, I -> 0 on (S, E, I).  dead: no infection and no one exposed, so E is 0 for ever, and E is observed"""
    kw = {}
    if method != "gillespie":
        kw.update(method=method, leaps=4)
    if obs == "negbin":
        kw.update(obs="negbin", size=5.0)
    if schedule:
        kw["rate_schedule"] = {"beta": np.array([1.0, 1.0, 0.5, 0.5, 1.5, 1.5, 1.0])}
    x0, observe = (300, 4, 12), {"I": 0.5}
    y = series(counts=True)
    if dead:
        x0, observe = (300, 0, 12), [{"I": 0.5}, {"E": 1.0}]
        y = np.stack([y, np.zeros(T)], axis=1)
        y[1, 1] = 3.0
    m = B.models.reaction_network(("S", "E", "I"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"), ({"I": 1}, {}, "gamma")],
                                  x0=x0, observe=observe, **kw)
    par = dict(beta=0.0 if dead else 0.002, sigma=0.5, gamma=0.3)
    run = dict(obs_times=OBS_TIMES, resample_algorithm="SISAR", resample_fn="systematic", return_particles=dead, seed=SEED, stream=7, ctx=cx, **par)
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    if algorithm == "APF":
        return B.auxiliary_filter(y, N, *fns, m.aux_log_likelihood_fn, **run)
    return B.bootstrap_filter(y, N, *fns, **run)


# name -> (runner, keywords)
CASES = {}
for _alg in ("BPF", "APF", "RMPF"):
    for _ra in ("SIS", "SISR", "SISAR"):
        for _rf in ("stratified", "systematic"):
            CASES["lg_%s_%s_%s" % (_alg, _ra, _rf)] = (lg_case, dict(algorithm=_alg, ra=_ra, rf=_rf))
CASES["lg_fused2"] = (lg_case, dict(fused=2))
CASES["lg_fused0"] = (lg_case, dict(fused=0))
CASES["lg_histories"] = (lg_case, dict(ra="SISAR", hist=True, anc=True))
CASES["lg_injected"] = (lg_case, dict(inject=True))
CASES["dead_lg"] = (lg_case, dict(hist=True, dead=True))
CASES["sir_BPF"] = (sir_case, {})
for _alg in ("BPF", "APF", "RMPF"):
    CASES["mv_gaussian_%s" % _alg] = (mv_case, dict(algorithm=_alg))
CASES["mv_poisson"] = (mv_case, dict(obs="poisson"))
CASES["mv_logvar"] = (mv_case, dict(obs="logvar"))
CASES["mv_tv"] = (mv_case, dict(tv=True))
CASES["mv_histories"] = (mv_case, dict(hist=True))
CASES["dead_mv"] = (mv_case, dict(hist=True, dead=True))
CASES["dead_mv_d1"] = (mv_case, dict(d=1, p=1, hist=True, dead=True))
for _alg in ("BPF", "APF"):
    for _method in ("gillespie", "tau_leap", "euler_multinomial"):
        CASES["rn_%s_%s" % (_alg, _method)] = (rn_case, dict(algorithm=_alg, method=_method))
CASES["rn_negbin"] = (rn_case, dict(obs="negbin"))
CASES["rn_schedule"] = (rn_case, dict(schedule=True))
CASES["dead_rn"] = (rn_case, dict(dead=True))


def golden_path(name, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), "runner_%s.npz" % name)


def run_case(B, cx, name):
    """the outputs of one case as arrays: floating-point ones as float64, the others as int32"""
    fn, kw = CASES[name]
    res = fn(B, cx, **kw)
    out = {k: np.atleast_1d(np.asarray(res[k], dtype=np.float64)) for k in SCALARS}
    out["resampled"] = np.asarray(res["_extras"]["resampled"], dtype=np.int32)
    out["early_return_step"] = np.array([res["_extras"]["early_return_step"]], dtype=np.int32)
    if "ancestors" in res["_extras"]:
        out["ancestors"] = np.asarray(res["_extras"]["ancestors"], dtype=np.int32)
    for k in ("particles_history", "weights_history"):
        if k in res:
            out[k] = np.asarray(res[k], dtype=np.float64)
    return out


def context(B):
    return B.Context(0, 1 << 13, 3)


def main():
    import bayesssm_amd as B
    out_dir = sys.argv[1] if len(sys.argv) > 1 else None
    cx = context(B)
    for name in CASES:
        out = run_case(B, cx, name)
        early = int(out["early_return_step"][0])
        print("%-28s loglike %.17g  early return %d  resampled %s  %s" % (
            name, out["loglike"][0], early, out["resampled"].tolist(), " ".join("%s%s" % (k, out[k].shape) for k in out if k not in SCALARS)), flush=True)
        assert early == (2 if name.startswith("dead_") else 0), "%s: early return at %d" % (name, early)
        np.savez_compressed(golden_path(name, out_dir), **out)
    cx.close()


if __name__ == "__main__":
    main()
