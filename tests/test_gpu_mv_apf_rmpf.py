"""Auxiliary and resample-move filters of the multivariate linear-Gaussian family on the device (pf_run_mv with BSSM_APF /
BSSM_RMPF; models.linear_gaussian_mv's aux_log_likelihood_fn and rw_move_fn).

Parity: against the CPU restatement in tests/mv_apf_rmpf_restated.py (pinned to the oracle's scalar APF / RMPF by
tests/test_mv_apf_rmpf_cpu.py) on identical injected draws, at the bar of tests/test_gpu_mv.py -- log-likelihood within 1e-6
relative, ESS / state estimates within 1e-6, resample decisions equal, the first resampling's ancestors bit-exact; the d = p = 1
cases also against the oracle's own scalar filters.  Then: generator runs equal their own dumps bit for bit, statistics against
the exact Kalman filter, the reference's two APF / RMPF tests in two dimensions, pmmh over both filters, and the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    return B.Context(0, 1 << 18, 8)


def _model(rng, d, p, noise=1.0):
    A = 0.6 * np.eye(d) + 0.1 * rng.standard_normal((d, d))
    Lq = noise * (np.tril(0.3 * rng.standard_normal((d, d))) + 0.7 * np.eye(d))
    L0 = np.tril(0.2 * rng.standard_normal((d, d))) + np.eye(d)
    H = rng.standard_normal((p, d))
    return dict(m0=rng.standard_normal(d), L0=L0, A=A, b=0.1 * rng.standard_normal(d), L=Lq, H=H, h0=0.2 * rng.standard_normal(p),
                sd=0.5 + rng.random(p))


def _simulate(rng, q, d, p, T, transitions_per_obs=1):
    x = q["m0"] + q["L0"] @ rng.standard_normal(d)
    ys = np.zeros((T, p))
    for t in range(T):
        for _ in range(transitions_per_obs):
            x = q["A"] @ x + q["b"] + q["L"] @ rng.standard_normal(d)
        ys[t] = q["h0"] + q["H"] @ x + q["sd"] * rng.standard_normal(p)
    return ys


def _compare(res, ref):
    assert res["_extras"]["early_return_step"] == ref["early_return_step"]
    assert abs(res["loglike"] - ref["loglike"]) <= 1e-6 * abs(ref["loglike"])
    np.testing.assert_allclose(res["loglike_history"], ref["loglike_history"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(res["ess"], ref["ess"], rtol=1e-6)
    np.testing.assert_allclose(np.asarray(res["state_est"]).reshape(-1), np.asarray(ref["state_est"]).reshape(-1), rtol=1e-6, atol=1e-8)
    assert (res["_extras"]["resampled"] == ref["resampled"]).all()


def _draws(rng, alg, T, N, d, rf, ot, oracle):
    mt, mr = oracle.noise_shape(alg, T, ot)
    dr = {"z_init": rng.standard_normal((d, N)), "z_trans": rng.standard_normal((max(mt, 1), d, N)),
          "u_res": rng.random(mr) if rf == "systematic" else rng.random((mr, N))}
    if alg == "RMPF":
        dr["z_move"], dr["u_move"] = rng.standard_normal((T, d, N)), rng.random((T, N))
    return dr


def _run(B, m, alg, ys, N, **kw):
    if alg == "APF":
        kw.pop("move_fn", None)
        return B.auxiliary_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, **kw)
    kw.pop("resample_algorithm", None)
    mv = kw.pop("move_fn", None) or m.rw_move_fn(0.3)
    return B.resample_move_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, mv, **kw)


GAPS = [1, 2, 2, 5, 6, 6, 9, 10]
CASES = [
    ("APF", 1, 1, 3000, "SISAR", "stratified", None), ("APF", 2, 2, 3000, "SISR", "systematic", None),
    ("APF", 3, 1, 20000, "SIS", "stratified", None), ("APF", 8, 8, 5000, "SISAR", "systematic", None),
    ("APF", 2, 0, 2048, "SISR", "stratified", None), ("APF", 3, 2, 4097, "SISAR", "stratified", GAPS),
    ("RMPF", 1, 1, 3000, "SISR", "systematic", None), ("RMPF", 2, 2, 3000, "SISR", "stratified", None),
    ("RMPF", 3, 1, 20000, "SISR", "systematic", None), ("RMPF", 8, 8, 5000, "SISR", "stratified", None),
    ("RMPF", 2, 0, 2048, "SISR", "systematic", None), ("RMPF", 3, 2, 4097, "SISR", "systematic", GAPS),
]


@pytest.mark.parametrize("alg,d,p,N,ra,rf,ot", CASES)
def test_mv_apf_rmpf_against_restatement_injected_draws(B, ctx, oracle, alg, d, p, N, ra, rf, ot):
    rng = np.random.default_rng(1000 * d + 10 * p + (alg == "RMPF"))
    q = _model(rng, d, p, noise=0.5)
    T = len(ot) if ot is not None else 10
    ys = _simulate(rng, q, d, p, T)
    dr = _draws(rng, alg, T, N, d, rf, ot, oracle)
    m = B.models.linear_gaussian_mv(d, p, **q)
    hist = N < 10000
    res = _run(B, m, alg, ys, N, obs_times=ot, resample_algorithm=ra, resample_fn=rf, return_particles=hist, return_ancestors=True,
               draws=dr, ctx=ctx)
    ref = R.pf_run_mv(oracle, m.pack({}), ys, N, dr["z_init"], dr["z_trans"], dr["u_res"], algorithm=alg, resample_algorithm=ra,
                      resample_fn=rf, obs_times=ot, move_sd=0.3, z_move=dr.get("z_move"), u_move=dr.get("u_move"), return_particles=hist)
    _compare(res, ref)
    assert res["state_est"].shape == ((T + 1, d) if d > 1 else (T + 1,))
    assert res["_extras"]["n_res_calls"] == ref["n_res_calls"]
    assert ref["n_res_calls"] > 0 and (res["_extras"]["ancestors"][0] == ref["ancestors"][0]).all()   # the first resampling: bit-exact
    if hist:
        assert res["particles_history"].shape == (T + 1, N * d) and res["weights_history"].shape == (T + 1, N)
        np.testing.assert_allclose(res["weights_history"], ref["weights_history"], rtol=1e-9, atol=1e-300)
        assert (res["particles_history"] == ref["particles_history"]).mean() > 0.99
    if d == 1 and p == 1:                    # the scalar linear-Gaussian model's own APF / RMPF (oracle/bssm_oracle.c)
        phi, sx, sy = float(q["A"][0, 0]), float(q["L"][0, 0]), float(q["sd"][0])
        m1 = B.models.linear_gaussian_mv(1, 1, A=[[phi]], L=[[sx]], sd=[sy])      # (m0 = 0, L0 = 1, b = 0, H = 1, h0 = 0)
        r1 = _run(B, m1, alg, ys, N, obs_times=ot, resample_algorithm=ra, resample_fn=rf, return_particles=False, return_ancestors=True,
                  draws=dr, ctx=ctx)
        kw = dict(move_sd=0.3, z_move=dr["z_move"].reshape(T, N), u_move=dr["u_move"]) if alg == "RMPF" else {}
        o = oracle.pf_run("lg", (phi, sx, sy), ys[:, 0], N, dr["z_init"].reshape(-1), dr["z_trans"].reshape(-1, N), dr["u_res"],
                          algorithm=alg, resample_algorithm="SISR" if alg == "RMPF" else ra, resample_fn=rf, obs_times=ot,
                          return_ancestors=True, **kw)
        _compare(r1, o)
        assert (r1["_extras"]["ancestors"][0] == o["ancestors"][0]).all()


@pytest.mark.parametrize("alg", ["APF", "RMPF"])
def test_mv_generator_equals_its_dump(B, ctx, oracle, alg):
    """Throughput mode: a generator run equals the injected-draws run on the generator's own dump, bit for bit (normals via
    bssm_dump_normals_mv, move draws via bssm_dump_move_draws_mv)."""
    rng = np.random.default_rng(21)
    d, p, T, N = 3, 2, 12, 5000
    q = _model(rng, d, p)
    ys = _simulate(rng, q, d, p, T)
    m = B.models.linear_gaussian_mv(d, p, **q)
    kw = dict(resample_algorithm="SISAR", resample_fn="stratified", return_particles=False, ctx=ctx)
    a = _run(B, m, alg, ys, N, seed=77, stream=5, **kw)
    dr = B.dump_draws(alg, T, N, "stratified", 77, 5, ctx=ctx, dim=d)
    b = _run(B, m, alg, ys, N, draws=dr, **kw)
    assert a["loglike"] == b["loglike"] and (a["state_est"] == b["state_est"]).all() and (a["ess"] == b["ess"]).all()
    ref = R.pf_run_mv(oracle, m.pack({}), ys, N, dr["z_init"], dr["z_trans"], dr["u_res"], algorithm=alg, resample_algorithm="SISAR",
                      move_sd=0.3, z_move=dr.get("z_move"), u_move=dr.get("u_move"))
    _compare(a, ref)


@pytest.mark.parametrize("alg", ["APF", "RMPF"])
def test_mv_d1_generator_run_equals_scalar_model(B, ctx, alg):
    """At d = p = 1 the family's draws are the scalar models' (the move draws at component 0 are bssm_dump_move_draws' exactly);
    where the scalar transition keys coincide too, the lgmv generator run is the scalar lg run for the same seed and stream."""
    import ctypes as C
    from bayesssm_amd import _lib
    lib = _lib.load()
    T, N, seed, stream = 15, 4096, 1405, 3
    phi, sx, sy = 0.8, 0.9, 0.7
    rng = np.random.default_rng(4)
    ys = rng.standard_normal(T)
    for i in range(1, T + 1):
        z1, u1, zd, ud = np.empty(N), np.empty(N), np.empty(N), np.empty(N)
        _lib.check(lib.bssm_dump_move_draws(ctx.handle, seed, stream, i, N, z1.ctypes.data_as(C.c_void_p), u1.ctypes.data_as(C.c_void_p)))
        _lib.check(lib.bssm_dump_move_draws_mv(ctx.handle, seed, stream, i, N, 1, zd.ctypes.data_as(C.c_void_p), ud.ctypes.data_as(C.c_void_p)))
        assert (z1 == zd).all() and (u1 == ud).all()
    sc = B.dump_draws(alg, T, N, "systematic", seed, stream, ctx=ctx)
    mv = B.dump_draws(alg, T, N, "systematic", seed, stream, ctx=ctx, dim=1)
    keys_coincide = all(np.array_equal(np.asarray(sc[k]).reshape(-1), np.asarray(mv[k]).reshape(-1)) for k in sc)
    assert keys_coincide
    m1 = B.models.linear_gaussian_mv(1, 1, A=[[phi]], L=[[sx]], sd=[sy])
    ml = B.models.linear_gaussian()
    kw = dict(resample_fn="systematic", return_particles=False, seed=seed, stream=stream, ctx=ctx)
    if alg == "APF":
        a = B.auxiliary_filter(ys, N, m1.init_fn, m1.transition_fn, m1.log_likelihood_fn, m1.aux_log_likelihood_fn, resample_algorithm="SISAR", **kw)
        b = B.auxiliary_filter(ys, N, ml.init_fn, ml.transition_fn, ml.log_likelihood_fn, ml.aux_log_likelihood_fn, resample_algorithm="SISAR",
                               phi=phi, sigma_x=sx, sigma_y=sy, **kw)
    else:
        a = B.resample_move_filter(ys, N, m1.init_fn, m1.transition_fn, m1.log_likelihood_fn, m1.rw_move_fn(0.2), **kw)
        b = B.resample_move_filter(ys, N, ml.init_fn, ml.transition_fn, ml.log_likelihood_fn, ml.rw_move_fn(0.2),
                                   phi=phi, sigma_x=sx, sigma_y=sy, **kw)
    assert (a["_extras"]["resampled"] == b["_extras"]["resampled"]).all()
    assert a["loglike"] == b["loglike"] and (a["loglike_history"] == b["loglike_history"]).all()
    np.testing.assert_allclose(a["state_est"], b["state_est"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(a["ess"], b["ess"], rtol=1e-12)


def test_mv_apf_state_estimates_against_kalman(B, ctx):
    """APF, SISR, N = 2^18, (d, p) = (3, 2): the filtering means follow the exact Kalman filter of the dynamics the reference's
    APF runs -- it transitions once more after its first-stage resampling (R/particle_filter_core.R:125-136,159), two transitions
    per observation.  (Its log-likelihood omits the first-stage normaliser log(sum(exp(aux)) / N): not a likelihood estimate, so
    it is not compared.  The state noise is small against the observation noise, so the look-ahead at the transition mean stays
    close to the predictive density and the second-stage weights stay even.)"""
    rng = np.random.default_rng(9)
    d, p, T, N = 3, 2, 25, 1 << 18
    q = _model(rng, d, p, noise=0.4)
    ys = _simulate(rng, q, d, p, T, transitions_per_obs=2)
    m = B.models.linear_gaussian_mv(d, p, **q)
    a = _run(B, m, "APF", ys, N, resample_algorithm="SISR", resample_fn="systematic", return_particles=False, seed=1405, stream=2, ctx=ctx)
    mm, P, Q, Rm, means = q["m0"].copy(), q["L0"] @ q["L0"].T, q["L"] @ q["L"].T, np.diag(q["sd"] ** 2), []
    for yv in ys:
        for _ in range(2):
            mm, P = q["A"] @ mm + q["b"], q["A"] @ P @ q["A"].T + Q
        S = q["H"] @ P @ q["H"].T + Rm
        K = P @ q["H"].T @ np.linalg.inv(S)
        mm, P = mm + K @ (yv - (q["h0"] + q["H"] @ mm)), (np.eye(d) - K @ q["H"]) @ P
        means.append(mm.copy())
    np.testing.assert_allclose(a["state_est"][1:], np.array(means), atol=0.03)


def _reference_case(rng, T, sigma, d=2):
    x = np.zeros((T + 1, d))
    y = np.zeros((T, d))
    x[0] = rng.standard_normal(d)
    for t in range(T):
        x[t + 1] = x[t] + 1.0 + rng.standard_normal(d)                 # x' = x + rnorm(mean = mu), mu = 1
        y[t] = x[t + 1] + sigma * rng.standard_normal(d)
    return x, y


@pytest.mark.parametrize("alg,sigma", [("APF", 0.1), ("RMPF", 0.05)])
def test_reference_apf_rmpf_tests_in_two_dimensions(B, ctx, alg, sigma):
    """tests/testthat/test-auxiliary_filter.R ("APF outperforms BPF under informative observations") and
    test-resample_move_filter.R ("RMPF outperforms BPF under strong particle degeneracy") in two dimensions: x' = x + mu + noise,
    y = x + N(0, sigma^2 I), N = 20, T = 50, move sd 0.1.  The reference asserts one seeded run; here the mean squared error is
    averaged over 32 (seed, stream) pairs."""
    T, N = 50, 20
    m = B.models.linear_gaussian_mv(2, 2, b=np.ones(2), sd=np.full(2, sigma))
    mse = {"BPF": [], alg: []}
    for s in range(32):
        x, y = _reference_case(np.random.default_rng(500 + s), T, sigma)
        kw = dict(seed=1405 + s, stream=s, return_particles=False, ctx=ctx)
        bpf = B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw)
        other = _run(B, m, alg, y, N, move_fn=m.rw_move_fn(0.1), **kw)
        for k, r in (("BPF", bpf), (alg, other)):
            assert r["_extras"]["early_return_step"] == 0
            mse[k].append(np.mean((r["state_est"] - x) ** 2))
    assert np.mean(mse[alg]) < np.mean(mse["BPF"]), {k: np.mean(v) for k, v in mse.items()}


@pytest.mark.parametrize("alg", ["APF", "RMPF"])
def test_pmmh_over_mv_apf_rmpf(B, alg):
    """tests/testthat/test-pmmh.R:619-668 (two-dimensional random walk with drift phi, constant log-likelihood, phi ~ N(0, 1): the
    posterior is the prior) through pmmh(auxiliary_filter) / pmmh(resample_move_filter): both run, stay in the band of
    test_gpu_mv.py::test_reference_multi_dim_pmmh_case, and repeat exactly for the same seed."""
    m = B.models.linear_gaussian_mv(2, 0, c0=1.0, build=lambda phi: {"b": [phi, phi]}, param_names=("phi",))
    y = np.zeros(20)
    if alg == "APF":
        wrapper, extra = B.auxiliary_filter, {"aux_log_likelihood_fn": m.aux_log_likelihood_fn}
    else:
        wrapper, extra = B.resample_move_filter, {"move_fn": m.rw_move_fn(0.1)}

    def run():
        return B.pmmh(wrapper, y, 300, m.init_fn, m.transition_fn, m.log_likelihood_fn, {"phi": B.prior_normal(0.0, 1.0)},
                      [{"phi": 0.8}, {"phi": 0.5}], 60, num_chains=2, param_transform={"phi": "identity"}, seed=1405, verbose=False,
                      print_result=False, **extra)
    out = run()
    phi = np.asarray(out["theta_chain"]["phi"])
    assert phi.shape == (480,) and abs(phi.mean()) < 0.4 and 0.5 < phi.std() < 1.5
    again = run()
    assert (np.asarray(again["theta_chain"]["phi"]) == phi).all()


def test_mv_apf_rmpf_refusals(B, ctx):
    m = B.models.linear_gaussian_mv(2, 2)
    y = np.zeros((5, 2))
    with pytest.raises(Exception, match="stratified / systematic"):
        B.auxiliary_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, resample_fn="multinomial", ctx=ctx)
    with pytest.raises(Exception, match="stratified / systematic"):
        B.resample_move_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.1), resample_fn="multinomial", ctx=ctx)
    th = [m.pack({}), m.pack({})]
    with pytest.raises(Exception, match="the multivariate family runs the bootstrap filter"):
        B.auxiliary_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, th, ctx=ctx)
    with pytest.raises(Exception, match="the multivariate family runs the bootstrap filter"):
        B.resample_move_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.1), th, ctx=ctx)
    with pytest.raises(ValueError, match="move_fn belongs to a different model"):
        B.resample_move_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, B.models.linear_gaussian().rw_move_fn(0.1), ctx=ctx)
