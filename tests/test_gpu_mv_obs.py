"""Poisson and log-variance observations of the multivariate family on the device (models.linear_gaussian_mv(..., obs=...);
BSSM_MODEL_LGMV_POIS / BSSM_MODEL_LGMV_LOGVAR through pf_run_mv and k_pf_batch_mv).

  1. parity with tests/mv_obs_restated.py on injected draws at the family's bar (tests/test_gpu_mv_apf_rmpf.py::_compare, plus
     the weights history at 1e-9), both families x BPF / APF / RMPF x the three register-array sizes, with time-varying rows once;
  2. bit equalities: generator run = run on its dump; batched filters = single runs (shared arrays, and array sets through
     bssm_pf_run_batch_tv); obs="gaussian" given explicitly = the default descriptor;
  3. exact answers at H = 0 (constant weights) and the all -inf early return at h0 = 800;
  4. closure mode on the same draws;  5. pmmh (lock-step batched = sequential; APF one at a time);  6. refusals through the C ABI."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402
import mv_obs_restated as OB  # noqa: E402

pytestmark = pytest.mark.gpu

T = 12
OT = [1, 2, 5, 6, 6, 7, 8, 9, 10, 11, 12, 13]          # a gap of 3, one repeated time (the weight-only launch)
INCR = [1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]       # closure mode: strictly increasing
N_PAR = 2048 + 513                                      # two scan blocks with a ragged tail, odd
FAMILIES = ["poisson", "logvar"]


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    cx = B.Context(0, 1 << 13, 8)
    yield cx
    cx.close()


def _pieces(rng, d, p):
    """a stationary state of unit scale and a small H: |eta| stays within about 4, the weights are not degenerate"""
    A = 0.6 * np.eye(d) + 0.1 * rng.standard_normal((d, d)) / np.sqrt(d)
    Lq = 0.5 * (np.tril(0.3 * rng.standard_normal((d, d))) + 0.7 * np.eye(d))
    L0 = 0.5 * (np.tril(0.2 * rng.standard_normal((d, d))) + np.eye(d))
    return dict(m0=0.3 * rng.standard_normal(d), L0=L0, A=A, b=0.1 * rng.standard_normal(d), L=Lq,
                H=0.8 * rng.standard_normal((p, d)) / np.sqrt(d), h0=0.5 + 0.3 * rng.standard_normal(p), sd=0.5 + rng.random(p))


def _varying(rng, q, d, p, n_times):
    return {"b": q["b"] + 0.3 * rng.standard_normal((n_times, d)), "h0": q["h0"] + 0.3 * rng.standard_normal((T, p)),
            "H": q["H"] + 0.3 * rng.standard_normal((T, p, d)) / np.sqrt(d)}


def _simulate(rng, obs, q, d, p, ot, tv=None):
    x = q["m0"] + q["L0"] @ rng.standard_normal(d)
    ys, prev = np.zeros((len(ot), p)), 0
    for i, t in enumerate(ot):
        for tau in range(prev + 1, t + 1):
            x = q["A"] @ x + (tv["b"][tau - 1] if tv else q["b"]) + q["L"] @ rng.standard_normal(d)
        prev = t
        eta = (tv["h0"][i] + tv["H"][i] @ x) if tv else (q["h0"] + q["H"] @ x)
        ys[i] = rng.poisson(np.exp(eta)) if obs == "poisson" else np.exp(0.5 * eta) * rng.standard_normal(p)
    return ys


def _draws(rng, alg, N, d, rf, ot, oracle):
    mt, mr = oracle.noise_shape(alg, T, ot)
    dr = {"z_init": rng.standard_normal((d, N)), "z_trans": rng.standard_normal((max(mt, 1), d, N)),
          "u_res": rng.random(mr) if rf == "systematic" else rng.random((mr, N))}
    if alg == "RMPF":
        dr["z_move"], dr["u_move"] = rng.standard_normal((T, d, N)), rng.random((T, N))
    return dr


def _run(B, m, alg, ys, N, **kw):
    if alg == "BPF":
        return B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw)
    if alg == "APF":
        return B.auxiliary_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, **kw)
    kw.pop("resample_algorithm", None)
    return B.resample_move_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.3), **kw)


def _ref(oracle, obs, m, tv, alg, ys, N, dr, ra, rf, ot, **kw):
    tv = tv or {}
    return OB.pf_run_mv_obs(oracle, obs, m.pack({}), ys, N, dr["z_init"], dr["z_trans"], dr["u_res"], b_t=tv.get("b"), h0_t=tv.get("h0"),
                            H_t=tv.get("H"), algorithm=alg, resample_algorithm=ra, resample_fn=rf, obs_times=ot, move_sd=0.3,
                            z_move=dr.get("z_move"), u_move=dr.get("u_move"), **kw)


def _compare(res, ref):
    """the bar of tests/test_gpu_mv_apf_rmpf.py::_compare (a non-finite log-likelihood must be equal)"""
    assert res["_extras"]["early_return_step"] == ref["early_return_step"]
    if np.isfinite(ref["loglike"]):
        assert abs(res["loglike"] - ref["loglike"]) <= 1e-6 * abs(ref["loglike"])
    else:
        assert res["loglike"] == ref["loglike"]
    np.testing.assert_allclose(res["loglike_history"], ref["loglike_history"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(res["ess"], ref["ess"], rtol=1e-6)
    np.testing.assert_allclose(np.asarray(res["state_est"]).reshape(-1), np.asarray(ref["state_est"]).reshape(-1), rtol=1e-6, atol=1e-8)
    assert (res["_extras"]["resampled"] == ref["resampled"]).all()


def _same_bits(a, b, keys=("loglike_history", "ess", "state_est")):
    assert a["loglike"] == b["loglike"]
    for k in keys:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


# ---- 1. parity on injected draws --------------------------------------------------------------------------------------------
# (ra, rf) by (d, p): both resamplers and SISAR / SISR for every family and algorithm (the RMPF resamples at every step anyway)
PARITY = [(1, 1, "SISAR", "stratified"), (2, 1, "SISR", "systematic"), (3, 2, "SISAR", "systematic"), (8, 8, "SISR", "stratified")]


@pytest.mark.parametrize("d,p,ra,rf", PARITY)
@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("obs", FAMILIES)
def test_parity_with_the_restatement_on_injected_draws(B, ctx, oracle, obs, alg, d, p, ra, rf):
    rng = np.random.default_rng(1000 * d + 10 * p + FAMILIES.index(obs))
    q = _pieces(rng, d, p)
    ys = _simulate(rng, obs, q, d, p, OT)
    dr = _draws(rng, alg, N_PAR, d, rf, OT, oracle)
    m = B.models.linear_gaussian_mv(d, p, obs=obs, **q)
    thr = {"threshold": 0.95 * N_PAR} if ra == "SISAR" else {}       # (|eta| <= 4 keeps the ESS above N / 2: resample below 0.95 N instead,
    res = _run(B, m, alg, ys, N_PAR, obs_times=OT, resample_algorithm=ra, resample_fn=rf, return_particles=True, return_ancestors=True,
               draws=dr, ctx=ctx, **thr)                            #  so that SISAR takes both decisions)
    ref = _ref(oracle, obs, m, None, alg, ys, N_PAR, dr, ra, rf, OT, return_particles=True, **thr)
    print("%s %s (%d, %d): loglike %.12g (restated %.12g), ESS min %.1f" % (obs, alg, d, p, res["loglike"], ref["loglike"], res["ess"][1:].min()))
    _compare(res, ref)
    assert res["_extras"]["early_return_step"] == 0 and ref["n_res_calls"] > 0
    assert res["_extras"]["n_res_calls"] == ref["n_res_calls"]
    assert (res["_extras"]["ancestors"][0] == ref["ancestors"][0]).all()                  # the first resampling: bit-exact
    np.testing.assert_allclose(res["weights_history"], ref["weights_history"], rtol=1e-9, atol=1e-300)
    g = _run(B, B.models.linear_gaussian_mv(d, p, **q), alg, ys, N_PAR, obs_times=OT, resample_algorithm=ra, resample_fn=rf,
             return_particles=False, draws=dr, ctx=ctx, **thr)
    assert g["loglike"] != res["loglike"]                                                 # (the family is not the Gaussian one)


@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("obs", FAMILIES)
def test_parity_with_time_varying_h0_and_H(B, ctx, oracle, obs, alg):
    d, p = 3, 2
    rng = np.random.default_rng(77 + FAMILIES.index(obs))
    q = _pieces(rng, d, p)
    tv = _varying(rng, q, d, p, OT[-1])
    ys = _simulate(rng, obs, q, d, p, OT, tv)
    ra, rf = ("SISAR", "stratified") if alg != "RMPF" else ("SISR", "systematic")
    dr = _draws(rng, alg, N_PAR, d, rf, OT, oracle)
    m = B.models.linear_gaussian_mv(d, p, obs=obs, time_varying=tv, **q)
    res = _run(B, m, alg, ys, N_PAR, obs_times=OT, resample_algorithm=ra, resample_fn=rf, return_particles=True, draws=dr, ctx=ctx)
    ref = _ref(oracle, obs, m, tv, alg, ys, N_PAR, dr, ra, rf, OT, return_particles=True)
    _compare(res, ref)
    np.testing.assert_allclose(res["weights_history"], ref["weights_history"], rtol=1e-9, atol=1e-300)
    flat = _ref(oracle, obs, m, dict(tv, h0=None, H=None), alg, ys, N_PAR, dr, ra, rf, OT)      # (the rows are read: the block's differ)
    assert flat["loglike"] != ref["loglike"]


# ---- 2. bit equalities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("obs", FAMILIES)
def test_generator_run_equals_its_dump(B, ctx, oracle, obs, alg):
    d, p, N = 3, 2, N_PAR
    rng = np.random.default_rng(21)
    q = _pieces(rng, d, p)
    ys = _simulate(rng, obs, q, d, p, OT)
    m = B.models.linear_gaussian_mv(d, p, obs=obs, **q)
    kw = dict(obs_times=OT, resample_algorithm="SISAR", resample_fn="stratified", return_particles=False, ctx=ctx)
    a = _run(B, m, alg, ys, N, seed=77, stream=5, **kw)
    dr = B.dump_draws(alg, T, N, "stratified", 77, 5, obs_times=OT, ctx=ctx, dim=d)
    b = _run(B, m, alg, ys, N, draws=dr, **kw)
    _same_bits(a, b)
    assert a["_extras"]["early_return_step"] == 0 and np.isfinite(a["loglike"])


PARAMS = [{"a": 1.0, "h": 0.0}, {"a": 0.7, "h": 0.3}, {"a": 1.2, "h": -0.4}, {"a": 0.4, "h": 0.6}, {"a": 0.9, "h": -0.2}]
SEEDS, STREAMS = [1405, 7, 7, 99, 3], [0, 1, 2, 3, 9]


def _batch_model(B, rng, obs, d, p, **extra):
    q = _pieces(rng, d, p)
    A0, h00 = q.pop("A"), q.pop("h0")
    m = B.models.linear_gaussian_mv(d, p, obs=obs, build=lambda a, h: {"A": a * A0, "h0": h00 + h}, param_names=("a", "h"), **extra, **q)
    return m, dict(q, A=A0, h0=h00)


def _assert_batch_equals_singles(B, ctx, models, d, out, ys, N, ot, ra, rf, threshold=None):
    assert np.all(out["status"] == 0)
    for k, par in enumerate(PARAMS):
        m = models[k]
        one = B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, obs_times=ot, resample_algorithm=ra,
                                 resample_fn=rf, threshold=threshold, return_particles=False, seed=SEEDS[k], stream=STREAMS[k], ctx=ctx, **par)
        assert out["loglike"][k] == one["loglike"], (k, out["loglike"][k], one["loglike"])
        np.testing.assert_array_equal(out["loglike_history"][k], one["loglike_history"])
        np.testing.assert_array_equal(out["ess"][k], one["ess"])
        np.testing.assert_array_equal(out["state_est"][k], np.asarray(one["state_est"]).reshape(-1, d))
        assert out["n_res_calls"][k] == one["_extras"]["n_res_calls"]
        assert out["early_return_step"][k] == one["_extras"]["early_return_step"] == 0


@pytest.mark.parametrize("N", [777, "max"])
@pytest.mark.parametrize("d,p", [(2, 1), (3, 2), (8, 8)])
@pytest.mark.parametrize("obs", FAMILIES)
def test_batch_equals_single_runs(B, ctx, oracle, obs, d, p, N):
    """F = 5 filters with distinct blocks, seeds and streams: every returned array equals the single runs', bit for bit"""
    N = B.batch_max_particles(d) if N == "max" else N
    rng = np.random.default_rng(300 + 10 * d + p)
    m, full = _batch_model(B, rng, obs, d, p)
    ys = _simulate(rng, obs, full, d, p, OT)
    ra, rf = ("SISAR", "stratified") if d != 3 else ("SISR", "systematic")
    thr = 0.95 * N if ra == "SISAR" else None                      # (as in the parity test: SISAR takes both decisions)
    out = B.bootstrap_filter_batch(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS, SEEDS, STREAMS, obs_times=OT,
                                   resample_algorithm=ra, resample_fn=rf, threshold=thr, ctx=ctx)
    _assert_batch_equals_singles(B, ctx, [m] * 5, d, out, ys, N, OT, ra, rf, thr)
    assert len(set(out["loglike"])) == 5 and out["n_res_calls"].max() > 0


@pytest.mark.parametrize("obs", FAMILIES)
def test_batch_with_two_array_sets_equals_single_runs(B, ctx, oracle, obs):
    """the same through bssm_pf_run_batch_tv: two sets of b / h0 / H, filter k reading set tv_set[k]"""
    d, p, N = 3, 2, 777
    rng = np.random.default_rng(41)
    m, full = _batch_model(B, rng, obs, d, p)
    sets = [_varying(rng, full, d, p, OT[-1]) for _ in range(2)]
    ys = _simulate(rng, obs, full, d, p, OT, sets[0])
    tv_set = [0, 1, 0, 1, 1]
    out = B.bootstrap_filter_batch(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS, SEEDS, STREAMS, obs_times=OT,
                                   resample_algorithm="SISAR", resample_fn="stratified", threshold=0.95 * N, ctx=ctx,
                                   time_varying={k: np.stack([s[k] for s in sets]) for k in ("b", "h0", "H")}, tv_set=tv_set)
    per_set = [_batch_model(B, np.random.default_rng(41), obs, d, p, time_varying=s)[0] for s in sets]
    _assert_batch_equals_singles(B, ctx, [per_set[g] for g in tv_set], d, out, ys, N, OT, "SISAR", "stratified", 0.95 * N)
    assert out["n_res_calls"].max() > 0


@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
def test_explicit_gaussian_is_the_default_descriptor_bitwise(B, ctx, alg):
    d, p = 3, 2
    rng = np.random.default_rng(5)
    q = _pieces(rng, d, p)
    ys = rng.standard_normal((T, p))
    a, b = [_run(B, B.models.linear_gaussian_mv(d, p, **kw, **q), alg, ys, N_PAR, obs_times=OT, resample_algorithm="SISAR",
                 resample_fn="stratified", return_particles=True, seed=11, stream=2, ctx=ctx) for kw in ({}, {"obs": "gaussian"})]
    _same_bits(a, b, keys=("loglike_history", "ess", "state_est", "particles_history", "weights_history"))
    if alg == "BPF":
        m0, m1 = B.models.linear_gaussian_mv(d, p, **q), B.models.linear_gaussian_mv(d, p, obs="gaussian", **q)
        o0, o1 = [B.bootstrap_filter_batch(ys, 777, m.init_fn, m.transition_fn, m.log_likelihood_fn, [m.pack({})] * 3, 4, [0, 1, 2],
                                           obs_times=OT, ctx=ctx) for m in (m0, m1)]
        for k in ("loglike", "loglike_history", "ess", "state_est"):
            np.testing.assert_array_equal(o0[k], o1[k])


# ---- 3. exact answers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("obs", FAMILIES)
def test_constant_weights_give_the_exact_log_likelihood(B, ctx, obs, alg):
    """H = 0: every particle has the same weight, so the log-likelihood is the sum of the observation log-densities at eta = h0
    (the APF's second-stage weights are log g - aux = 0: its log-likelihood is 0) and the ESS is N"""
    d, p, N = 3, 2, 1024
    rng = np.random.default_rng(8)
    q = _pieces(rng, d, p)
    q["H"] = np.zeros((p, d))
    h0 = q["h0"]
    ys = rng.poisson(np.exp(h0), size=(T, p)).astype(np.float64) if obs == "poisson" else np.exp(0.5 * h0) * rng.standard_normal((T, p))
    ys[3, 0] = 0.0                                              # (the y == 0 branch of both densities)
    m = B.models.linear_gaussian_mv(d, p, obs=obs, **q)
    res = _run(B, m, alg, ys, N, obs_times=OT, resample_algorithm="SISAR", resample_fn="stratified", return_particles=False, seed=3,
               stream=1, ctx=ctx)
    if obs == "poisson":
        terms = [[yk * h - math.exp(h) - math.lgamma(yk + 1.0) for yk, h in zip(row, h0)] for row in ys]      # dpois(y, exp(h0), log = TRUE)
    else:
        terms = [[-0.5 * math.log(2.0 * math.pi) - 0.5 * h - 0.5 * (yk / math.exp(0.5 * h)) ** 2 for yk, h in zip(row, h0)]
                 for row in ys]                                                                                 # dnorm(y, 0, exp(h0 / 2), log = TRUE)
    want = 0.0 if alg == "APF" else float(np.sum(terms))
    print("%s %s: loglike %.15g exact %.15g" % (obs, alg, res["loglike"], want))
    np.testing.assert_allclose(res["loglike"], want, rtol=1e-12, atol=1e-12 if alg == "APF" else 0.0)
    if alg != "APF":
        np.testing.assert_allclose(res["loglike_history"], np.cumsum(np.sum(terms, axis=1)), rtol=1e-12)
    np.testing.assert_allclose(res["ess"], np.full(T + 1, float(N)), rtol=1e-12)


def test_all_weights_minus_infinity_returns_at_the_first_observation(B, ctx, oracle):
    """Poisson with h0 = 800: exp(eta) = +inf for every particle, every log-weight is -inf at observation 1.  The single and
    the batched run return there (early_return_step == 1) with the restatement's outputs."""
    d, p, N = 3, 2, 777
    rng = np.random.default_rng(13)
    m, full = _batch_model(B, rng, "poisson", d, p)
    ys = _simulate(rng, "poisson", full, d, p, OT)
    params = [dict(q, h=800.0) if k in (1, 4) else q for k, q in enumerate(PARAMS)]
    out = B.bootstrap_filter_batch(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, params, SEEDS, STREAMS, obs_times=OT,
                                   resample_algorithm="SISAR", resample_fn="stratified", ctx=ctx)
    assert list(out["early_return_step"]) == [0, 1, 0, 0, 1] and np.all(out["status"] == 0)
    for k in (1, 4):
        dr = B.dump_draws("BPF", T, N, "stratified", SEEDS[k], STREAMS[k], obs_times=OT, ctx=ctx, dim=d)
        one = B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, obs_times=OT, resample_algorithm="SISAR",
                                 resample_fn="stratified", return_particles=False, seed=SEEDS[k], stream=STREAMS[k], ctx=ctx, **params[k])
        ref = OB.pf_run_mv_obs(oracle, "poisson", m.pack(params[k]), ys, N, dr["z_init"], dr["z_trans"], dr["u_res"], obs_times=OT)
        assert ref["early_return_step"] == 1 and ref["loglike"] == -np.inf
        _compare(one, ref)
        assert "resample_algorithm" not in one
        assert out["loglike"][k] == one["loglike"] == -np.inf
        np.testing.assert_array_equal(out["loglike_history"][k], one["loglike_history"])
        np.testing.assert_array_equal(out["ess"][k], one["ess"])
        np.testing.assert_array_equal(out["state_est"][k], np.asarray(one["state_est"]).reshape(-1, d))
        assert np.all(np.isnan(out["state_est"][k][1:])) and np.all(out["ess"][k][1:] == 0.0)
    assert np.all(np.isfinite(out["loglike"][[0, 2, 3]]))


# ---- 4. closure mode --------------------------------------------------------------------------------------------------------
class _Closures:
    """the Poisson model as Python closures, drawing from the injected normals in call order and summing as the kernels do"""

    def __init__(self, obs, q, z_init, z_trans):
        self.obs, self.q, self.zi, self.zt, self.k = obs, q, z_init, z_trans, 0

    def init_fn(self, num_particles):
        q, d = self.q, self.q["d"]
        x = np.empty((d, num_particles))
        for c in range(d):
            v = np.full(num_particles, q["m0"][c])
            for j in range(c + 1):
                v = v + q["L0"][c, j] * self.zi[j]
            x[c] = v
        return x.T

    def transition_fn(self, particles, t):
        z = self.zt[self.k]; self.k += 1
        x = np.asarray(particles, dtype=np.float64).reshape(len(z[0]), -1).T
        return R.transition(self.q, x, z).T

    def log_likelihood_fn(self, y, particles, t):
        x = np.asarray(particles, dtype=np.float64).reshape(-1, self.q["d"]).T
        return OB.obs_loglik(self.obs, self.q, np.atleast_1d(y), x)

    def aux_log_likelihood_fn(self, y, particles, t):
        x = np.asarray(particles, dtype=np.float64).reshape(-1, self.q["d"]).T
        return OB.obs_loglik(self.obs, self.q, np.atleast_1d(y), R.mean_of_transition(self.q, x))


@pytest.mark.parametrize("alg", ["BPF", "APF"])
@pytest.mark.parametrize("d,p", [(1, 1), (3, 2)])
def test_poisson_descriptor_agrees_with_closure_mode(B, ctx, oracle, alg, d, p):
    rng = np.random.default_rng(40 + d)
    N, ot, obs = 500, INCR, "poisson"
    q = _pieces(rng, d, p)
    ys = _simulate(rng, obs, q, d, p, ot)
    m = B.models.linear_gaussian_mv(d, p, obs=obs, **q)
    for ra, rf in (("SISAR", "stratified"), ("SISR", "systematic")):
        dr = _draws(rng, alg, N, d, rf, ot, oracle)
        dev = _run(B, m, alg, ys, N, obs_times=ot, resample_algorithm=ra, resample_fn=rf, return_particles=False, draws=dr, ctx=ctx)
        cl = _Closures(obs, R.unpack(m.pack({})), dr["z_init"], dr["z_trans"])
        u_list = [np.atleast_1d(u) for u in dr["u_res"]]
        yy = ys[:, 0] if p == 1 else ys
        if alg == "BPF":
            host = B.bootstrap_filter(yy, N, cl.init_fn, cl.transition_fn, cl.log_likelihood_fn, obs_times=ot, resample_algorithm=ra,
                                      resample_fn=rf, return_particles=False, u_res=u_list, ctx=ctx)
        else:
            host = B.auxiliary_filter(yy, N, cl.init_fn, cl.transition_fn, cl.log_likelihood_fn, cl.aux_log_likelihood_fn, obs_times=ot,
                                      resample_algorithm=ra, resample_fn=rf, return_particles=False, u_res=u_list, ctx=ctx)
        assert abs(dev["loglike"] - host["loglike"]) <= 1e-6 * abs(host["loglike"])
        np.testing.assert_allclose(dev["loglike_history"], host["loglike_history"], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(dev["ess"], host["ess"], rtol=1e-6)
        np.testing.assert_allclose(np.asarray(dev["state_est"]).reshape(-1), np.asarray(host["state_est"]).reshape(-1), rtol=1e-6, atol=1e-8)
        assert ((np.asarray(host["ess"])[1:] == N) == (dev["_extras"]["resampled"] == 1)).all()       # identical decisions


# ---- 5. pmmh ----------------------------------------------------------------------------------------------------------------
def _pmmh_case(B):
    """(d, p) = (2, 2), Poisson counts, the drift mu entering b through build; T = 20"""
    rng = np.random.default_rng(6)
    q = dict(A=np.array([[0.7, 0.1], [0.0, 0.6]]), L=0.4 * np.eye(2), H=np.array([[0.8, 0.0], [0.3, 0.6]]), h0=[0.5, 0.2])
    m = B.models.linear_gaussian_mv(2, 2, obs="poisson", build=lambda mu: {"b": [mu, 0.5 * mu]}, param_names=("mu",), **q)
    x, ys = np.zeros(2), []
    for _ in range(20):
        x = q["A"] @ x + np.array([0.4, 0.2]) + q["L"] @ rng.standard_normal(2)
        ys.append(rng.poisson(np.exp(np.asarray(q["h0"]) + q["H"] @ x)))
    return m, np.array(ys, dtype=np.float64)


def _pmmh(B, m, ys, wrapper=None, **kw):
    """2 chains of 60 iterations.  The family refuses a num_particles override (pmmh takes the count from its pilot for descriptor
    models of this family), so 300 particles is what the PILOT's filters run (pilot_n); the main chains run the count the tuner
    derives from them (target_n, between 50 and 1000), which the lock-step test checks against the batched kernel's capacity."""
    tc = B.default_tune_control(pilot_m=30, pilot_n=300, pilot_reps=10, pilot_burn_in=10, pilot_proposal_sd=0.2)
    return B.pmmh(wrapper or B.bootstrap_filter, ys, 60, m.init_fn, m.transition_fn, m.log_likelihood_fn, {"mu": B.prior_normal(0.0, 1.0)},
                  [{"mu": 0.3}, {"mu": 0.6}], 10, num_chains=2, param_transform={"mu": "identity"}, seed=1405, verbose=False,
                  print_result=False, tune_control=tc, **kw)


def test_pmmh_poisson_lockstep_equals_sequential(B):
    m, ys = _pmmh_case(B)
    a, again, b = _pmmh(B, m, ys), _pmmh(B, m, ys), _pmmh(B, m, ys, batch_chains=False)
    assert a["_extras"]["batched"] is True and a["_extras"]["batched_launches"] > 0 and b["_extras"]["batched"] is False
    targets = [ch["pilot"]["target_n"] for ch in a["_extras"]["local_chains"].values()]
    assert len(targets) == 2 and all(50 <= n <= B.batch_max_particles(2) for n in targets), targets      # the main chains fit the batched
    assert a["_extras"]["single_filter_runs"] == 0                                                        # kernel: no filter ran alone
    mu = np.asarray(a["theta_chain"]["mu"])
    assert mu.shape == (100,) and np.all(np.isfinite(mu)) and len(np.unique(mu)) > 3
    np.testing.assert_array_equal(mu, np.asarray(again["theta_chain"]["mu"]))             # repeats exactly for the same seed
    np.testing.assert_array_equal(mu, np.asarray(b["theta_chain"]["mu"]))                 # and equals the one-at-a-time run draw for draw


def test_pmmh_poisson_over_the_auxiliary_filter(B):
    m, ys = _pmmh_case(B)
    a, b = [_pmmh(B, m, ys, wrapper=B.auxiliary_filter, aux_log_likelihood_fn=m.aux_log_likelihood_fn) for _ in range(2)]
    assert a["_extras"]["batched"] is False                                                # the one-at-a-time path
    mu = np.asarray(a["theta_chain"]["mu"])
    assert mu.shape == (100,) and np.all(np.isfinite(mu))
    np.testing.assert_array_equal(mu, np.asarray(b["theta_chain"]["mu"]))


# ---- 6. refusals through the C ABI ------------------------------------------------------------------------------------------
def test_refusals_through_the_abi(B, ctx):
    """the descriptor checks y and p itself; here the library's own checks speak (bssm_pf_run and bssm_pf_run_batch)"""
    from bayesssm_amd import _lib
    lib = _lib.load()
    p_ = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    N, n_obs, F = 100, 5, 2

    def call(model_id, d, p, y, batch):
        th = B.models.linear_gaussian_mv(d, p).pack({})
        ths = np.ascontiguousarray([th] * F)
        y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
        cfg = _lib.PfConfig(model_id, _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN["stratified"], N, n_obs,
                            float("nan"), None if batch else p_(th), int(th.size), p_(y), None, 1, 0, None, None, None, 0, 0, 0.0, None, None)
        if batch:
            ll, st = np.zeros(F), np.zeros(F, np.int32)
            seeds, streams = np.array([1, 1], dtype=np.uint64), np.array([0, 1], dtype=np.uint64)
            res = _lib.PfBatchResult(p_(ll), None, None, None, None, None, p_(st), None)
            rc = lib.bssm_pf_run_batch(ctx.handle, C.byref(cfg), F, p_(ths), p_(seeds), p_(streams), C.byref(res))
            return rc, lib.bssm_last_error().decode(), ll
        se, ess, llh, ll = np.zeros((n_obs + 1, d)), np.zeros(n_obs + 1), np.zeros(n_obs), np.zeros(1)
        res = _lib.PfResult(p_(se), p_(ess), p_(llh), p_(ll), None, None, None, None, None, None, None, None)
        rc = lib.bssm_pf_run(ctx.handle, C.byref(cfg), C.byref(res))
        return rc, lib.bssm_last_error().decode(), ll

    good = np.ones((n_obs, 2))
    for batch in (False, True):
        who = "bssm_pf_run_batch: " if batch else "bssm_pf_run: "
        for bad in (-1.0, 0.5, np.nan, np.inf):
            y = good.copy(); y[3, 1] = bad
            rc, msg, _ = call(_lib.MV_OBS_MODEL["poisson"], 3, 2, y, batch)
            assert rc == _lib.ERR_ARG, (batch, bad, rc, msg)
            assert ("Contains missing values" in msg) if not np.isfinite(bad) else msg.startswith(who) and "non-negative integers" in msg
            if np.isfinite(bad):                           # (the log-variance family takes any finite y)
                rc, msg, ll = call(_lib.MV_OBS_MODEL["logvar"], 3, 2, y, batch)
                assert rc == _lib.OK and np.all(np.isfinite(ll)), (batch, bad, rc, msg)
        for o in ("poisson", "logvar"):
            rc, msg, _ = call(_lib.MV_OBS_MODEL[o], 3, 0, None, batch)
            assert rc == _lib.ERR_ARG and msg.startswith(who) and "p >= 1" in msg, (batch, o, rc, msg)
        rc, msg, ll = call(_lib.MV_OBS_MODEL["poisson"], 3, 2, good, batch)               # and a valid call through the same door
        assert rc == _lib.OK and np.all(np.isfinite(ll)), (rc, msg)
