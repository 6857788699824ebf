"""CPU checks of the multivariate family's Poisson and log-variance observation densities (no GPU needed).

tests/mv_obs_restated.py is what the device is compared with for models.linear_gaussian_mv(..., obs=...).  With obs="gaussian" it
must be tests/mv_tv_restated.py exactly; its Poisson formula must be dpois; the packed block does not depend on obs; and the
descriptor and the filters refuse what the families cannot take before any context is created."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402
import mv_obs_restated as OB  # noqa: E402
import mv_tv_restated as TV  # noqa: E402

GAPS = [1, 2, 2, 4, 5, 7, 8, 9, 10, 10, 11, 14]          # T = 12: gaps and repeated times


def _theta(rng, d, p):
    A = 0.6 * np.eye(d) + 0.1 * rng.standard_normal((d, d))
    Lq = np.tril(0.3 * rng.standard_normal((d, d))) + 0.7 * np.eye(d)
    L0 = np.tril(0.2 * rng.standard_normal((d, d))) + np.eye(d)
    return np.concatenate([[d, p], rng.standard_normal(d), L0.ravel(), A.ravel(), 0.1 * rng.standard_normal(d), Lq.ravel(), [0.5],
                           0.3 * rng.standard_normal(p * d), 0.2 * rng.standard_normal(p), 0.5 + rng.random(p)])


def _inputs(rng, oracle, alg, d, p, T, N, ot):
    ra, rf = {"BPF": ("SISR", "stratified"), "APF": ("SISAR", "stratified"), "RMPF": ("SISR", "systematic")}[alg]
    mt, mr = oracle.noise_shape(alg, T, ot)
    zi, zt = rng.standard_normal((d, N)), rng.standard_normal((max(mt, 1), d, N))
    ur = rng.random(mr) if rf == "systematic" else rng.random((mr, N))
    kw = dict(algorithm=alg, resample_algorithm=ra, resample_fn=rf, obs_times=ot, return_particles=True)
    if alg == "RMPF":
        kw.update(move_sd=0.3, z_move=rng.standard_normal((T, d, N)), u_move=rng.random((T, N)))
    return zi, zt, ur, kw


@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
@pytest.mark.parametrize("d,p,ot", [(1, 1, None), (3, 2, GAPS), (2, 0, GAPS)])
def test_gaussian_family_is_the_existing_restatement_bitwise(oracle, alg, d, p, ot):
    rng = np.random.default_rng(100 * d + p)
    T, N = 12, 500
    theta = _theta(rng, d, p)
    ys = rng.standard_normal((T, p))
    zi, zt, ur, kw = _inputs(rng, oracle, alg, d, p, T, N, ot)
    tv = dict(b_t=0.3 * rng.standard_normal((ot[-1] if ot is not None else T, d)))
    if p > 0:
        tv.update(h0_t=0.3 * rng.standard_normal((T, p)), H_t=rng.standard_normal((T, p, d)))
    a = TV.pf_run_mv_tv(oracle, theta, ys, N, zi, zt, ur, **tv, **kw)
    b = OB.pf_run_mv_obs(oracle, "gaussian", theta, ys, N, zi, zt, ur, **tv, **kw)
    assert a["loglike"] == b["loglike"] and a["n_res_calls"] == b["n_res_calls"] > 0
    for key in ("loglike_history", "ess", "state_est", "ancestors", "resampled", "particles_history", "weights_history"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
    assert R.loglik.__module__ == "mv_apf_rmpf_restated"          # (the family's function is in place for the call only)


@pytest.mark.parametrize("obs", ["poisson", "logvar"])
@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
def test_families_run_through_the_three_filters_and_differ_from_gaussian(oracle, obs, alg):
    """the restatement runs for both families (finite log-likelihoods, resampling happens), is not the Gaussian run, and leaves
    mv_apf_rmpf_restated as it found it"""
    rng = np.random.default_rng(5)
    d, p, T, N = 3, 2, 12, 400
    theta = _theta(rng, d, p)
    ys = rng.poisson(2.0, size=(T, p)).astype(np.float64) if obs == "poisson" else rng.standard_normal((T, p))
    zi, zt, ur, kw = _inputs(rng, oracle, alg, d, p, T, N, GAPS)
    a = OB.pf_run_mv_obs(oracle, obs, theta, ys, N, zi, zt, ur, **kw)
    g = OB.pf_run_mv_obs(oracle, "gaussian", theta, ys, N, zi, zt, ur, **kw)
    assert np.isfinite(a["loglike"]) and a["early_return_step"] == 0 and a["n_res_calls"] > 0
    assert a["loglike"] != g["loglike"]
    assert R.loglik.__module__ == "mv_apf_rmpf_restated"


def test_poisson_formula_is_dpois():
    """(y eta - exp(eta)) - lgamma(y + 1) against y log(lambda) - lambda - lgamma(y + 1) at lambda = exp(eta): within 1e-13
    relative over eta in [-20, 20], y in {0, 1, 7, 400}; y == 0 gives -lambda exactly"""
    eta = np.linspace(-20.0, 20.0, 4001)
    for y in (0.0, 1.0, 7.0, 400.0):
        lgy = math.lgamma(y + 1.0)
        got = OB.dpois_log_eta(y, eta, lgy)
        lam = np.exp(eta)
        want = np.array([y * math.log(l) - l - lgy for l in lam])
        assert np.all(np.abs(got - want) <= 1e-13 * np.abs(want)), (y, np.max(np.abs(got - want) / np.abs(want)))
        if y == 0.0:
            assert np.array_equal(got, -lam)
    assert OB.dpois_log_eta(3.0, np.array([800.0]), math.lgamma(4.0))[0] == -np.inf          # exp(eta) = +inf
    assert OB.dpois_log_eta(0.0, np.array([800.0]), 0.0)[0] == -np.inf


def test_logvar_formula_is_dnorm_at_sd_exp_half_eta():
    eta = np.linspace(-20.0, 20.0, 801)
    for y in (0.0, 0.3, -2.5, 40.0):
        got = OB.dlogvar_log_eta(y, eta)
        sd = np.exp(0.5 * eta)
        want = -0.5 * math.log(2.0 * math.pi) - np.log(sd) - 0.5 * (y / sd) ** 2
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert OB.dlogvar_log_eta(0.0, np.array([-800.0]))[0] == -R.LN_SQRT_2PI + 400.0          # no 0 * inf at y == 0
    assert OB.dlogvar_log_eta(1.0, np.array([-800.0]))[0] == -np.inf
    assert OB.dlogvar_log_eta(1.0, np.array([np.inf]))[0] == -np.inf


def test_pack_does_not_depend_on_obs():
    import bayesssm_amd as B
    rng = np.random.default_rng(1)
    pieces = dict(m0=rng.standard_normal(3), A=0.5 * np.eye(3), H=rng.standard_normal((2, 3)), h0=rng.standard_normal(2), sd=[0.4, 0.9])
    blocks = [B.models.linear_gaussian_mv(3, 2, obs=o, **pieces).pack({}) for o in ("gaussian", "poisson", "logvar")]
    assert np.array_equal(blocks[0], B.models.linear_gaussian_mv(3, 2, **pieces).pack({}))
    assert np.array_equal(blocks[0], blocks[1]) and np.array_equal(blocks[0], blocks[2])
    m = B.models.linear_gaussian_mv(3, 2, obs="poisson", **pieces)
    assert m.obs == "poisson" and B.models.linear_gaussian_mv(3, 2).obs == "gaussian"
    assert m.init_fn.model == m.log_likelihood_fn.model == m.rw_move_fn(0.1).model == "lgmv"     # the descriptors' name stays


def test_refusals_without_a_gpu():
    import bayesssm_amd as B
    from bayesssm_amd import _lib
    assert _lib.MV_OBS_MODEL == {"gaussian": 3, "poisson": 4, "logvar": 5} and _lib.MODEL["lgmv"] == 3
    with pytest.raises(ValueError, match="obs must be one of"):
        B.models.linear_gaussian_mv(2, 2, obs="binomial")
    for o in ("poisson", "logvar"):
        with pytest.raises(ValueError, match="p >= 1"):
            B.models.linear_gaussian_mv(2, 0, obs=o)
    assert B.models.linear_gaussian_mv(2, 0, obs="gaussian").p == 0
    m = B.models.linear_gaussian_mv(2, 2, obs="poisson")
    good = np.ones((5, 2))
    for bad, match in ((-1.0, "negative"), (0.5, "fractional"), (np.nan, "non-finite"), (np.inf, "non-finite")):
        y = good.copy(); y[3, 1] = bad
        with pytest.raises(ValueError, match=match):
            B.bootstrap_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn)
        with pytest.raises(ValueError, match=match):
            B.auxiliary_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn)
        with pytest.raises(ValueError, match=match):
            B.resample_move_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.1))
        with pytest.raises(ValueError, match=match):
            B.bootstrap_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, [m.pack({})] * 2, 1, [0, 1])
    # r_seed / r_stream stay refused for the family
    for o in ("poisson", "logvar"):
        mm = B.models.linear_gaussian_mv(2, 2, obs=o)
        with pytest.raises(ValueError, match="r_seed / r_stream"):
            B.auxiliary_filter(good, 100, mm.init_fn, mm.transition_fn, mm.log_likelihood_fn, mm.aux_log_likelihood_fn, r_seed=1)
        with pytest.raises(ValueError, match="r_seed / r_stream"):
            B.resample_move_filter(good, 100, mm.init_fn, mm.transition_fn, mm.log_likelihood_fn, mm.rw_move_fn(0.1), r_seed=1)
