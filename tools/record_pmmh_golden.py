"""Dev tool: record what bayesssm_amd/pmmh.py computes, prints, warns about and refuses, for tests/test_pmmh_golden.py (no GPU) and
tests/test_gpu_pmmh_golden.py to hold a later build to.  Run it with the build whose results are the reference -- the commit BEFORE a
change to pmmh.py:
    python tools/record_pmmh_golden.py cpu|refusals|gpu|all [--check] [OUT_DIR, default tests/golden]
--check writes nothing: it runs the cases, compares with the fixtures and prints every difference (exit status 1 if there is one).
One pmmh_<case>.npz per case (arrays; text as 0-d string arrays under "text/...") and pmmh_refusals.json.

cpu      run_pilot_chain / run_pilot_chains_lockstep / run_chain_host / run_chains_host_lockstep over a synthetic filter: a smooth
         log-likelihood plus a perturbation hashed from (theta, n, tag or call count, chain), NaN / -Inf at chosen calls.  Recorded:
         every returned array, the sequence of filter calls, how many draws every generator gave and its next draw, stdout, the error.
refusals every argument check of pmmh() broken one at a time (a few two at a time) for a built-in model, Python closures, an lgmv and an
         rnet descriptor: exception type and text, warnings.  All of them refuse before any device call.
gpu      one tiny pmmh() call per route through the dispatcher (T = 8, m = 10, pilot_m = 12, pilot_n = 64, pilot_reps = 4).

Everything is compared byte for byte, text by equality (stdout of a case whose chains run on worker threads: as a multiset of lines).
PILOT_COV_RTOL: the relative tolerance for "pilot_theta_cov" alone (np.cov goes through BLAS); 0 means exact, which the parent build
met on the hosts where `cpu --check` was run on it (see profiles/README.md, r21_a)."""
import contextlib
import hashlib
import importlib
import io
import json
import os
import struct
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 1405
PILOT_M, PILOT_N, PILOT_REPS, MAIN_M = 12, 64, 4, 16
PILOT_COV_RTOL = 0.0


# ---------------------------------------------------------------- the synthetic filter and the counting generators

def _hash01(theta, *ints):
    """a number in [0, 1) from the bytes of theta and some integers: the same on every host"""
    h = hashlib.sha256(np.asarray(theta, dtype=np.float64).tobytes() + struct.pack("<%dq" % len(ints), *[int(v) for v in ints])).digest()
    return int.from_bytes(h[:6], "little") / float(1 << 48)


def _smooth(theta):
    return -2.0 * sum((float(t) - 0.5) * (float(t) - 0.5) for t in theta)          # (+, -, * only: exact on every host)


class _Counting:
    """a generator that counts the calls made to it"""

    def __init__(self, g):
        self.g, self.normals, self.uniforms = g, 0, 0

    def standard_normal(self, p):
        self.normals += 1
        return self.g.standard_normal(p)

    def random(self):
        self.uniforms += 1
        return self.g.random()


class _Calls:
    """the sequence of filter calls: one row per filter, `call` numbers the calls of the user's function"""

    def __init__(self):
        self.rows, self.n_calls = [], 0

    def add(self, thetas, ns, tags, who, batch):
        for th, n, tag, k in zip(thetas, ns, tags, who):
            self.rows.append((np.array(th, dtype=np.float64), int(n), int(tag), int(k), self.n_calls, int(batch)))
        self.n_calls += 1

    def arrays(self, p):
        out = {"calls/theta": np.array([r[0] for r in self.rows], dtype=np.float64).reshape(len(self.rows), p)}
        for j, k in enumerate(("n", "tag", "who", "call", "batch")):
            out["calls/" + k] = np.array([r[j + 1] for r in self.rows], dtype=np.int64)
        out["calls/count"] = np.array([self.n_calls], dtype=np.int64)
        return out


def _capture(fn):
    """(result or None, stdout, 'Type: text' of the exception or '')"""
    buf, res, err = io.StringIO(), None, ""
    with contextlib.redirect_stdout(buf):
        try:
            res = fn()
        except Exception as e:          # noqa: BLE001 -- the refusal is what the case records
            err = "%s: %s" % (type(e).__name__, e)
    return res, buf.getvalue(), err


_PILOT_SET = {      # transform(s) -> (priors as (kind, a, b), start, proposal_sd)
    ("identity",): ([("uniform", -0.2, 0.9)], [0.3], 0.5),
    ("log",): ([("uniform", 0.2, 1.4)], [0.6], 0.5),
    ("logit",): ([("uniform", 0.35, 0.65)], [0.5], 0.5),
    ("log", "logit"): ([("uniform", 0.2, 1.4), ("uniform", 0.35, 0.65)], [0.6, 0.5], [0.5, 0.3]),
    ("identity", "log"): ([("normal", 0.0, 1.0), ("exponential", 1.0, 0.0)], [0.3, 0.6], 0.4),
}


def pilot_case(kind, tr, K=1, batch=False, special=False, na=False, verbose=True, bad_init=False):
    """kind "single": run_pilot_chain (with pf_batch when `batch`); "lockstep": run_pilot_chains_lockstep with K chains.
    special: tag 3 gives NaN, tags 5 and 8 give -Inf; na: repetition 1 of .pilot_run gives -Inf ("May not be NA")"""
    P = importlib.import_module("bayesssm_amd.pmmh")      # (the package's attribute `pmmh` is the function)
    spec, init, sd = _PILOT_SET[tuple(tr)]
    priors, p = [P.Prior(*s) for s in spec], len(tr)
    inits = [[v + 0.01 * k for v in init] for k in range(K)]
    if bad_init:
        inits[-1][0] = 5.0
    calls = _Calls()

    def one(theta, n, tag, k):
        if special and tag == 3:
            return float("nan")
        if (special and tag in (5, 8)) or (na and tag == 10_000_001):
            return -np.inf
        return _smooth(theta) + (_hash01(theta, n, tag, k) - 0.5) * (6.0 if tag >= 10_000_000 else 0.6)

    def pf(theta, n, tag):
        calls.add([theta], [n], [tag], [0], False)
        return one(theta, n, tag, 0)

    def pf_batch1(theta, n, tags):
        calls.add([theta] * len(tags), [n] * len(tags), tags, [0] * len(tags), True)
        return np.array([one(theta, n, t, 0) for t in tags])

    def pf_batch(thetas, n, tags, who):
        calls.add(thetas, [n] * len(tags), tags, who, True)
        return np.array([one(th, n, t, k) for th, t, k in zip(thetas, tags, who)])

    rngs = [_Counting(np.random.default_rng([SEED, k])) for k in range(K)]
    message = lambda s: print("message: " + s)      # noqa: E731
    if kind == "single":
        run = lambda: [P.run_pilot_chain(pf, PILOT_M, PILOT_N, PILOT_REPS, priors, sd, list(tr), inits[0], rngs[0], verbose, message,     # noqa: E731
                                         pf_batch=pf_batch1 if batch else None)]
    else:
        run = lambda: P.run_pilot_chains_lockstep(pf_batch, inits, rngs, PILOT_M, PILOT_N, PILOT_REPS, priors, sd, list(tr), verbose, message)   # noqa: E731
    res, stdout, err = _capture(run)
    out = calls.arrays(p)
    for k, r in enumerate(res or []):
        out["chain%d/keys" % k] = " ".join(sorted(r))
        for key, v in r.items():
            out["chain%d/%s" % (k, key)] = np.atleast_1d(np.asarray(v, dtype=np.int64 if key == "target_n" else np.float64))
    out["rng/normals"] = np.array([g.normals for g in rngs], dtype=np.int64)
    out["rng/uniforms"] = np.array([g.uniforms for g in rngs], dtype=np.int64)
    out["rng/next"] = np.array([g.g.random() for g in rngs])
    out["text/stdout"], out["text/error"] = stdout, err
    return out


_MAIN_LOGIT_PRIOR = (0.34, 0.66)
_MAIN_COV = {"diag": np.diag([0.15, 0.04]), "dense": np.array([[0.15, 0.03], [0.03, 0.04]])}


def main_case(kind, cov, K=1, r_stream=False, lapack=False, latent=False):
    """kind "single": run_chain_host; "lockstep": run_chains_host_lockstep with K chains.  p = 2, transforms (log, logit), narrow uniform
    priors: many proposals have no prior support, so they run no filter.  r_stream: the generators are _RStreamRng over an rrng.RRandom per
    chain and the filter draws one uniform from its chain's generator too.  The 3rd filter run of every chain gives NaN."""
    P = importlib.import_module("bayesssm_amd.pmmh")      # (the package's attribute `pmmh` is the function)
    from bayesssm_amd.rrng import RRandom
    tr, p = ["log", "logit"], 2
    priors = [P.prior_uniform(0.5, 1.6), P.prior_uniform(*_MAIN_LOGIT_PRIOR)]
    inits = [[0.9 + 0.02 * k, 0.5 - 0.02 * k] for k in range(K)]
    ns = [50 + 10 * k for k in range(K)]
    gens = [RRandom(SEED + k) for k in range(K)] if r_stream else [np.random.default_rng([SEED, 7, k]) for k in range(K)]
    rngs = [_Counting(P._RStreamRng(g) if r_stream else g) for g in gens]
    calls, runs = _Calls(), [0] * K

    def one(theta, n, k):
        runs[k] += 1
        ll = _smooth(theta) + (_hash01(theta, n, runs[k], k) - 0.5)
        if r_stream:
            ll += gens[k].unif_rand() - 0.5
        if runs[k] == 3:
            ll = float("nan")
        return ll, np.array([float(theta[0]) * j + runs[k] for j in range(5)])

    def pf(theta):
        calls.add([theta], [ns[0]], [runs[0]], [0], False)
        ll, se = one(theta, ns[0], 0)
        return {"loglike": ll, "state_est": se}

    def pf_batch(thetas, ns_, who):
        calls.add(thetas, ns_, [runs[k] for k in who], who, True)
        return [one(th, n, k) for th, n, k in zip(thetas, ns_, who)]

    mv = P._mvrnorm_lapack if lapack else None
    if kind == "single":
        run = lambda: [P.run_chain_host(pf, MAIN_M, inits[0], _MAIN_COV[cov], tr, priors, rngs[0], latent, mvrnorm=mv)]      # noqa: E731
    else:
        kw = {"mvrnorm": mv} if lapack else {}
        run = lambda: P.run_chains_host_lockstep(pf_batch, inits, [_MAIN_COV[cov]] * K, ns, tr, priors, rngs, MAIN_M, latent, **kw)   # noqa: E731
    res, stdout, err = _capture(run)
    out = calls.arrays(p)
    for k, r in enumerate(res or []):
        out["chain%d/keys" % k] = " ".join(sorted(r))
        for key, v in r.items():
            if v is not None:
                out["chain%d/%s" % (k, key)] = np.atleast_1d(np.asarray(v, dtype=np.int64 if key == "accepted" else np.float64))
    out["rng/normals"] = np.array([g.normals for g in rngs], dtype=np.int64)
    out["rng/uniforms"] = np.array([g.uniforms for g in rngs], dtype=np.int64)
    out["rng/next"] = np.array([g.g.random() for g in rngs])
    out["text/stdout"], out["text/error"] = stdout, err
    return out


# ---------------------------------------------------------------- pmmh() on the device

def _lg_series(T=8, cols=None):
    rng = np.random.default_rng(SEED)
    shape = (T,) if cols is None else (T, cols)
    return np.cumsum(rng.standard_normal(shape), axis=0) * 0.5 + 0.7 * rng.standard_normal(shape)


def _tune(B, **kw):
    return B.default_tune_control(pilot_m=PILOT_M, pilot_burn_in=2, pilot_n=PILOT_N, pilot_reps=PILOT_REPS, **kw)


def _lg_args(B, chains=3, model="lg"):
    m = B.models.linear_gaussian() if model == "lg" else B.models.ar1_sin()
    return dict(pf_wrapper=B.bootstrap_filter, y=_lg_series(), m=10, init_fn=m.init_fn, transition_fn=m.transition_fn,
                log_likelihood_fn=m.log_likelihood_fn,
                log_priors={"phi": B.prior_uniform(0.0, 1.0), "sigma_x": B.prior_exponential(1.0), "sigma_y": B.prior_exponential(1.0)},
                pilot_init_params=[{"phi": 0.7 + 0.05 * c, "sigma_x": 1.0, "sigma_y": 0.6 + 0.1 * c} for c in range(chains)], burn_in=2,
                num_chains=chains, param_transform={"phi": "logit", "sigma_x": "log", "sigma_y": "log"}, tune_control=_tune(B), verbose=True,
                seed=SEED)


def gpu_builtin(B, chains=3, model="lg", **kw):
    runner_calls = []
    if kw.pop("inject_runner", False):
        from bayesssm_amd.pmmh import run_chain_device

        def runner(**a):
            runner_calls.append(int(a["chain_index"]))
            print("injected runner: chain %d, %d particles" % (a["chain_index"], a["num_particles"]))
            return run_chain_device(**a)
        kw["_chain_runner"] = runner
    if kw.pop("large", False):
        kw.update(num_particles=4096, proposal_cov=np.diag([0.01, 0.01, 0.01]))
    return B.pmmh(**dict(_lg_args(B, chains, model), **kw))


def gpu_sir(B):
    m = B.models.sir(500, 70)
    y = np.array([70, 75, 90, 100, 95, 120, 110, 100], dtype=np.float64)
    return B.pmmh(B.auxiliary_filter, y, 10, m.init_fn, m.transition_fn, m.log_likelihood_fn,
                  {"lambda": B.prior_halfnormal(1.0), "gamma": B.prior_halfnormal(2.0)},
                  [{"lambda": 0.5, "gamma": 0.2}, {"lambda": 0.6, "gamma": 0.25}], 2, num_chains=2, param_transform={"lambda": "log", "gamma": "log"},
                  tune_control=_tune(B, pilot_proposal_sd=0.1), verbose=True, seed=SEED, aux_log_likelihood_fn=m.aux_log_likelihood_fn)


def gpu_closures(B, r_stream=False, latent=False):
    """the linear-Gaussian model as Python closures; their normals come from a generator of their own, or from the call's R stream"""
    from bayesssm_amd import resampling as rs
    from bayesssm_amd.rrng import rnorm_vec
    rng = np.random.default_rng(SEED + 1)
    draw = (lambda n: rnorm_vec(rs._rng, int(n))) if r_stream else (lambda n: rng.standard_normal(int(n)))      # noqa: E731

    def init_fn(num_particles):
        return draw(num_particles)

    def transition_fn(particles, phi, sigma_x):
        return phi * particles + sigma_x * draw(particles.shape[0])

    def log_likelihood_fn(y, particles, sigma_y):
        z = (y - particles) / sigma_y
        return -(0.918938533204672741780329736406 + 0.5 * z * z + np.log(sigma_y))

    a = _lg_args(B, 2)
    a.update(init_fn=init_fn, transition_fn=transition_fn, log_likelihood_fn=log_likelihood_fn, return_latent_state_est=latent)
    if r_stream:
        a["r_stream"] = True
    return B.pmmh(**a)


def gpu_lgmv(B, **kw):
    d, p = 3, 2
    m = B.models.linear_gaussian_mv(d, p, build=lambda a: {"A": a * np.eye(d)}, param_names=("a",))
    return B.pmmh(B.bootstrap_filter, _lg_series(8, p), 10, m.init_fn, m.transition_fn, m.log_likelihood_fn, {"a": B.prior_uniform(0.0, 1.0)},
                  [{"a": 0.5}, {"a": 0.7}, {"a": 0.6}], 2, num_chains=3, param_transform={"a": "logit"}, tune_control=_tune(B), verbose=True, seed=SEED,
                  **kw)


def _seir(B, **kw):
    return B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                          ({"I": 1}, {"R": 1}, "gamma")], x0=[180.0, 8.0, 12.0, 0.0], observe=[{"I": 0.6, "S": 0.01}], **kw)


SEIR_PAR = dict(beta=0.004, sigma=0.5, gamma=0.3)
Y_SEIR = np.array([8, 9, 12, 13, 17, 19, 20, 24], dtype=np.float64)


def gpu_rnet(B):
    m = _seir(B)
    priors = {"beta": B.prior_exponential(100.0), "sigma": B.prior_exponential(1.0), "gamma": B.prior_exponential(1.0)}
    return B.pmmh(B.bootstrap_filter, Y_SEIR, 10, m.init_fn, m.transition_fn, m.log_likelihood_fn, priors,
                  [dict(SEIR_PAR), dict(beta=0.0045, sigma=0.45, gamma=0.33)], 2, num_chains=2, param_transform={k: "log" for k in priors},
                  tune_control=_tune(B, pilot_proposal_sd=0.05), verbose=True, seed=7)


def flatten_pmmh(res):
    """a pmmh() result as named arrays and strings; device_ms is left out"""
    out = {"post/" + k: np.asarray(v) for k, v in res["theta_chain"].items()}
    for what in ("ess", "rhat"):
        for name, v in res["diagnostics"][what].items():
            out["diag/%s/%s" % (what, name)] = np.array([v], dtype=np.float64)
    ex = res["_extras"]
    out["seeds"] = np.asarray(ex["seeds"], dtype=np.int64)
    out["extras/keys"] = " ".join(sorted(ex))
    for k, v in ex.items():
        if k not in ("local_chains", "seeds"):
            out["extras/" + k] = np.array([int(v)], dtype=np.int64)
    out["keys"] = " ".join(sorted(res))
    for c, ch in sorted(ex["local_chains"].items()):
        out["chain%d/keys" % c] = " ".join(sorted(ch))
        for k, v in ch.items():
            if k in ("device_ms", "pilot") or v is None:
                continue
            out["chain%d/%s" % (c, k)] = np.atleast_1d(np.asarray(v, dtype=np.float64 if k.endswith("_chain") else np.int64))
        if ch.get("pilot") is not None:
            out["chain%d/pilot/keys" % c] = " ".join(sorted(ch["pilot"]))
            for k, v in ch["pilot"].items():
                out["chain%d/pilot/%s" % (c, k)] = np.atleast_1d(np.asarray(v, dtype=np.int64 if k == "target_n" else np.float64))
    for c, v in sorted(res.get("latent_state_chain", {}).items()):
        out["latent/%d" % c] = np.asarray(v, dtype=np.float64)
    return out


def gpu_case(fn, **kw):
    import bayesssm_amd as B
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res, stdout, err = _capture(lambda: fn(B, **kw))
    if res is None:
        raise RuntimeError(err)
    out = flatten_pmmh(res)
    out["text/stdout"] = stdout
    out["text/warnings"] = "\n---\n".join("%s: %s" % (x.category.__name__, x.message) for x in w)
    return out


# name -> (kind, runner, keywords); kind "cpu" | "gpu" | "gpu-threads" (stdout compared as a multiset of lines)
CASES = {}
for _tr in (("identity",), ("log",), ("logit",), ("log", "logit")):
    _n = "_".join(_tr)
    CASES["pilot_single_" + _n] = ("cpu", pilot_case, dict(kind="single", tr=_tr))
    CASES["pilot_single_batch_" + _n] = ("cpu", pilot_case, dict(kind="single", tr=_tr, batch=True))
    CASES["pilot_lockstep1_" + _n] = ("cpu", pilot_case, dict(kind="lockstep", tr=_tr, K=1))
    CASES["pilot_lockstep3_" + _n] = ("cpu", pilot_case, dict(kind="lockstep", tr=_tr, K=3))
for _k, _kw in (("single", dict(kind="single")), ("single_batch", dict(kind="single", batch=True)), ("lockstep1", dict(kind="lockstep", K=1)),
                ("lockstep3", dict(kind="lockstep", K=3))):
    CASES["pilot_%s_nan_inf" % _k] = ("cpu", pilot_case, dict(tr=("identity", "log"), special=True, **_kw))
    CASES["pilot_%s_na_refused" % _k] = ("cpu", pilot_case, dict(tr=("identity", "log"), na=True, **_kw))
    CASES["pilot_%s_quiet" % _k] = ("cpu", pilot_case, dict(tr=("identity", "log"), verbose=False, **_kw))
CASES["pilot_single_bad_init"] = ("cpu", pilot_case, dict(kind="single", tr=("log",), bad_init=True))
CASES["pilot_lockstep3_bad_init"] = ("cpu", pilot_case, dict(kind="lockstep", tr=("log",), K=3, bad_init=True))
for _cov in ("diag", "dense"):
    for _rs in (False, True):
        _lat = (_cov == "dense") != _rs                  # latent estimates on for (dense, numpy) and (diag, r_stream)
        _n = "%s_%s" % (_cov, "rstream" if _rs else "numpy")
        CASES["main_single_" + _n] = ("cpu", main_case, dict(kind="single", cov=_cov, r_stream=_rs, lapack=_rs, latent=_lat))
        CASES["main_lockstep1_" + _n] = ("cpu", main_case, dict(kind="lockstep", cov=_cov, K=1, r_stream=_rs, latent=_lat))
        CASES["main_lockstep3_" + _n] = ("cpu", main_case, dict(kind="lockstep", cov=_cov, K=3, r_stream=_rs, latent=_lat))
CASES["main_single_dense_numpy_lapack"] = ("cpu", main_case, dict(kind="single", cov="dense", lapack=True))

CASES["gpu_lg_lockstep"] = ("gpu", gpu_case, dict(fn=gpu_builtin))
CASES["gpu_lg_lockstep_latent"] = ("gpu", gpu_case, dict(fn=gpu_builtin, return_latent_state_est=True))
CASES["gpu_lg_one_at_a_time"] = ("gpu", gpu_case, dict(fn=gpu_builtin, batch_chains=False, chains_per_gpu=1))
CASES["gpu_lg_one_chain"] = ("gpu", gpu_case, dict(fn=gpu_builtin, chains=1))
CASES["gpu_lg_large_streams"] = ("gpu-threads", gpu_case, dict(fn=gpu_builtin, large=True, chains_per_gpu=2))
CASES["gpu_lg_large_lockstep"] = ("gpu-threads", gpu_case, dict(fn=gpu_builtin, large=True, lockstep_large=True))
CASES["gpu_sir_apf"] = ("gpu", gpu_case, dict(fn=gpu_sir))
CASES["gpu_lg_chain_runner"] = ("gpu", gpu_case, dict(fn=gpu_builtin, chains=2, inject_runner=True))
CASES["gpu_ar1sin_r_stream"] = ("gpu", gpu_case, dict(fn=gpu_builtin, chains=2, model="ar1sin", r_stream=True))
CASES["gpu_ar1sin_r_stream_latent"] = ("gpu", gpu_case, dict(fn=gpu_builtin, chains=2, model="ar1sin", r_stream=True, return_latent_state_est=True))
CASES["gpu_closures"] = ("gpu", gpu_case, dict(fn=gpu_closures))
CASES["gpu_closures_latent"] = ("gpu", gpu_case, dict(fn=gpu_closures, latent=True))
CASES["gpu_closures_r_stream"] = ("gpu", gpu_case, dict(fn=gpu_closures, r_stream=True))
CASES["gpu_lgmv_batched"] = ("gpu", gpu_case, dict(fn=gpu_lgmv))
CASES["gpu_lgmv_batched_latent"] = ("gpu", gpu_case, dict(fn=gpu_lgmv, return_latent_state_est=True))
CASES["gpu_lgmv_one_at_a_time"] = ("gpu", gpu_case, dict(fn=gpu_lgmv, batch_chains=False))
CASES["gpu_rnet_batched"] = ("gpu", gpu_case, dict(fn=gpu_rnet))


def golden_path(name, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), "pmmh_%s" % name + ("" if name.endswith(".json") else ".npz"))


def run_case(name):
    """the outputs of one case: name -> array, or str for text"""
    _, fn, kw = CASES[name]
    return fn(**kw)


def load_case(name, out_dir=None):
    with np.load(golden_path(name, out_dir)) as z:
        return {k: (str(z[k][()]) if z[k].dtype.kind == "U" else z[k]) for k in z.files}


def differences(name, got, want):
    """every way in which `got` is not the recording `want`: arrays by shape, dtype and bytes, text by equality"""
    kind = CASES[name][0]
    out = []
    if set(got) != set(want):
        out.append("keys: %s only in this run, %s only in the recording" % (sorted(set(got) - set(want)), sorted(set(want) - set(got))))
    for k in sorted(set(got) & set(want)):
        g, w = got[k], want[k]
        if isinstance(w, str) or isinstance(g, str):
            if k == "text/stdout" and kind == "gpu-threads":
                g, w = sorted(str(g).splitlines()), sorted(str(w).splitlines())
            if g != w:
                out.append("%s: %r, recorded %r" % (k, g, w))
            continue
        if g.shape != w.shape or g.dtype != w.dtype:
            out.append("%s: shape %s dtype %s, recorded %s %s" % (k, g.shape, g.dtype, w.shape, w.dtype))
            continue
        if k.endswith("pilot_theta_cov") and PILOT_COV_RTOL > 0:
            if not np.allclose(g, w, rtol=PILOT_COV_RTOL, atol=0.0, equal_nan=True):
                out.append("%s: beyond rtol %g: %r, recorded %r" % (k, PILOT_COV_RTOL, g, w))
            continue
        gb, wb = np.ascontiguousarray(g).view(np.uint8).ravel(), np.ascontiguousarray(w).view(np.uint8).ravel()
        if not np.array_equal(gb, wb):
            bad = np.unique(np.flatnonzero(gb != wb) // g.dtype.itemsize)
            rel = ""
            if g.dtype.kind == "f":
                with np.errstate(all="ignore"):
                    rel = ", largest relative difference %.3g" % np.nanmax(np.abs(g - w) / np.abs(w))
            out.append("%s: %d of %d differ, first at %d: %r, recorded %r%s" % (k, bad.size, g.size, bad[0], g.ravel()[bad[0]], w.ravel()[bad[0]], rel))
    return out


def happened(name, out):
    """what a case is there for has happened in it (asserted when recording, and on the recording by the tests)"""
    if name.startswith("pilot_"):
        if name.endswith("bad_init"):
            assert out["text/error"].startswith("ValueError: Initial parameter values are invalid"), out["text/error"]
        elif name.endswith("na_refused"):
            assert out["text/error"] == "ValueError: Assertion on 'num_particles' failed: May not be NA.", out["text/error"]
        else:
            assert out["text/error"] == "" and "Using " in out["text/stdout"]
            if "nan_inf" in name:
                assert np.all(out["rng/uniforms"] == PILOT_M - 1)                      # the NaN / -Inf runs are rejected, the chain goes on
            elif "quiet" not in name:
                assert np.all(out["rng/normals"] > PILOT_M - 1), out["rng/normals"]    # the redraw loop has iterated
    elif name.startswith("main_"):
        K = int(out["rng/normals"].size)
        sizes = np.bincount(out["calls/call"])                                         # filters per call of the user's function
        assert out["text/error"] == "" and np.all(out["rng/normals"] == MAIN_M - 1)
        assert np.all(out["rng/uniforms"] < MAIN_M - 1), out["rng/uniforms"]            # some proposals ran no filter and drew no uniform
        assert np.all(np.bincount(out["calls/who"], minlength=K) >= 4)                  # (the NaN of run 3 was reached)
        if K > 1:
            assert np.any(sizes[1:] < K) and sizes.size - 1 < MAIN_M - 1, sizes         # `who` a strict subset; at least once empty (no call)


# ---------------------------------------------------------------- pmmh()'s refusals

def _refusal_base(B, family):
    a = _lg_args(B, 2)
    a.update(verbose=False, print_result=False)
    if family == "closures":
        a.update(init_fn=lambda num_particles: np.zeros(num_particles), transition_fn=lambda particles, phi, sigma_x: particles,
                 log_likelihood_fn=lambda y, particles, sigma_y: np.zeros(particles.shape[0]))
    elif family in ("lgmv", "rnet"):
        if family == "lgmv":
            m, y, init = B.models.linear_gaussian_mv(3, 2, build=lambda a: {"A": a * np.eye(3)}, param_names=("a",)), _lg_series(8, 2), [{"a": 0.5}, {"a": 0.7}]
            priors = {"a": B.prior_uniform(0.0, 1.0)}
        else:
            m, y, init = _seir(B), Y_SEIR.copy(), [dict(SEIR_PAR), dict(SEIR_PAR)]
            priors = {k: B.prior_exponential(1.0) for k in SEIR_PAR}
        a.update(y=y, init_fn=m.init_fn, transition_fn=m.transition_fn, log_likelihood_fn=m.log_likelihood_fn, log_priors=priors,
                 pilot_init_params=init, param_transform={k: "log" for k in priors})
    return a


def _drop_last(d):
    return {k: d[k] for k in list(d)[:-1]}


def _with_nan(y):
    y = np.array(y, dtype=np.float64)
    y[(1,) + (0,) * (y.ndim - 1)] = np.nan
    return y


# name -> function(arguments of a valid call) -> the arguments that break a rule
_BREAKS = {
    "num_chains_zero": lambda a: dict(a, num_chains=0),
    "num_chains_float": lambda a: dict(a, num_chains=2.0),
    "y_nan": lambda a: dict(a, y=_with_nan(a["y"])),
    "m_zero": lambda a: dict(a, m=0),
    "m_float": lambda a: dict(a, m=10.0),
    "burn_in_negative": lambda a: dict(a, burn_in=-1),
    "burn_in_m": lambda a: dict(a, burn_in=a["m"]),
    "burn_in_float": lambda a: dict(a, burn_in=2.0),
    "init_length": lambda a: dict(a, pilot_init_params=a["pilot_init_params"][:1]),
    "init_not_a_list": lambda a: dict(a, pilot_init_params=a["pilot_init_params"][0]),
    "init_names_differ": lambda a: dict(a, pilot_init_params=[a["pilot_init_params"][0], dict(reversed(list(a["pilot_init_params"][1].items())), extra=1.0)]),
    "init_empty": lambda a: dict(a, pilot_init_params=[{}, {}]),
    "fn_params_not_in_init": lambda a: dict(a, pilot_init_params=[dict(_drop_last(q), other=1.0) for q in a["pilot_init_params"]]),
    "fn_params_not_in_priors": lambda a: dict(a, log_priors=_drop_last(a["log_priors"])),
    "resample_algorithm": lambda a: dict(a, resample_algorithm="XYZ"),
    "resample_fn": lambda a: dict(a, resample_fn="residual"),
    "param_transform_not_a_dict": lambda a: dict(a, param_transform="log"),
    "param_transform_entry_missing": lambda a: dict(a, param_transform=_drop_last(a["param_transform"])),
    "r_stream_without_seed": lambda a: dict(a, r_stream=True, seed=None),
    "transform_warning_then_r_stream_without_seed": lambda a: dict(a, param_transform=dict(a["param_transform"], **{list(a["log_priors"])[0]: "sqrt"}),
                                                                   r_stream=True, seed=None),
    # two rules at once: the earlier check speaks
    "m_zero_and_burn_in_negative": lambda a: dict(a, m=0, burn_in=-1),
    "y_nan_and_m_zero": lambda a: dict(a, y=_with_nan(a["y"]), m=0),
    "init_length_and_m_zero": lambda a: dict(a, pilot_init_params=a["pilot_init_params"][:1], m=0),
    "resample_algorithm_and_param_transform": lambda a: dict(a, resample_algorithm="XYZ", param_transform="log"),
    "fn_params_not_in_priors_and_resample_fn": lambda a: dict(a, log_priors=_drop_last(a["log_priors"]), resample_fn="residual"),
    "num_chains_zero_and_y_nan": lambda a: dict(a, num_chains=0, y=_with_nan(a["y"])),
}


def _ar1sin_transition(B):
    return B.models.ar1_sin().transition_fn


_BREAKS_BUILTIN = {
    "two_models": lambda a, B: dict(a, transition_fn=_ar1sin_transition(B)),
    "role_mismatch": lambda a, B: dict(a, transition_fn=a["init_fn"]),
    "log_priors_order": lambda a, B: dict(a, log_priors=dict(reversed(list(a["log_priors"].items())))),
    "transform_warning_then_log_priors_order": lambda a, B: dict(a, log_priors=dict(reversed(list(a["log_priors"].items()))),
                                                                 param_transform=dict(a["param_transform"], phi="sqrt")),
    "r_stream_with_overrides": lambda a, B: dict(a, r_stream=True, num_particles=100, proposal_cov=np.eye(3)),
    "r_stream_with_auxiliary_filter": lambda a, B: dict(a, r_stream=True, pf_wrapper=B.auxiliary_filter),
    "r_stream_with_chain_runner": lambda a, B: dict(a, r_stream=True, _chain_runner=lambda **kw: None),
}
_BREAKS_CLOSURES = {          # (closures, lgmv, rnet)
    "num_particles_override": lambda a, B: dict(a, num_particles=100),
    "proposal_cov_override": lambda a, B: dict(a, proposal_cov=np.eye(len(a["log_priors"]))),
    "override_and_m_zero": lambda a, B: dict(a, num_particles=100, m=0),
}


def _short_schedule(a, B):
    m = _seir(B, rate_schedule=np.ones((5, 3)))
    return dict(a, init_fn=m.init_fn, transition_fn=m.transition_fn, log_likelihood_fn=m.log_likelihood_fn)


_BREAKS_RNET = {
    "rate_schedule_short": _short_schedule,
    "rate_schedule_short_with_obs_times": lambda a, B: dict(_short_schedule(a, B), obs_times=np.array([1, 2, 3, 4, 5, 5, 6, 9])),
    "rate_schedule_short_and_param_transform": lambda a, B: dict(_short_schedule(a, B), param_transform="log"),
    "resample_fn_and_rate_schedule_short": lambda a, B: dict(_short_schedule(a, B), resample_fn="residual"),
}


def refusal_names():
    names = []
    for fam in ("builtin", "closures", "lgmv", "rnet"):
        names += ["%s/%s" % (fam, k) for k in _BREAKS]
        names += ["%s/%s" % (fam, k) for k in (_BREAKS_BUILTIN if fam == "builtin" else _BREAKS_CLOSURES)]
        if fam == "rnet":
            names += ["rnet/" + k for k in _BREAKS_RNET]
    return names


def run_refusal(name):
    """{"type", "text", "warnings"} of the pmmh() call `name`; the call must refuse"""
    import bayesssm_amd as B
    fam, what = name.split("/")
    a = _refusal_base(B, fam)
    if what in _BREAKS:
        a = _BREAKS[what](a)
    else:
        a = {**_BREAKS_BUILTIN, **_BREAKS_CLOSURES, **_BREAKS_RNET}[what](a, B)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            B.pmmh(**a)
        except Exception as e:          # noqa: BLE001 -- the refusal is what is recorded
            return {"type": type(e).__name__, "text": str(e), "warnings": ["%s: %s" % (x.category.__name__, x.message) for x in w]}
    raise AssertionError("%s: pmmh() did not refuse" % name)


def main():
    args = [a for a in sys.argv[1:] if a != "--check"]
    check = "--check" in sys.argv[1:]
    what, out_dir = (args[0] if args else "all"), (args[1] if len(args) > 1 else None)
    bad = 0
    for name, (kind, _, _) in CASES.items():
        if what != "all" and not kind.startswith(what):
            continue
        out = run_case(name)
        happened(name, out)
        if check:
            diffs = differences(name, out, load_case(name, out_dir))
            bad += bool(diffs)
            print("%-44s %s" % (name, "; ".join(diffs) or "equal"), flush=True)
            continue
        np.savez_compressed(golden_path(name, out_dir), **out)
        print("%-44s %d entries  %s" % (name, len(out), out.get("text/error") or out["text/stdout"].splitlines()[-1:]), flush=True)
    if what in ("all", "refusals"):
        got = {name: run_refusal(name) for name in refusal_names()}
        if check:
            want = json.load(open(golden_path("refusals.json", out_dir)))
            diff = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
            bad += bool(diff)
            print("refusals: %d calls, %s" % (len(got), "; ".join("%s: %r, recorded %r" % (k, got.get(k), want.get(k)) for k in diff) or "equal"))
        else:
            with open(golden_path("refusals.json", out_dir), "w") as f:
                json.dump(got, f, indent=1, sort_keys=True)
                f.write("\n")
            for k, v in got.items():
                print("%-64s %s: %s%s" % (k, v["type"], v["text"][:90], "  [+%d warnings]" % len(v["warnings"]) if v["warnings"] else ""))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
