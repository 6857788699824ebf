"""Many small filters of the multivariate linear-Gaussian family per launch (k_pf_batch_mv, bssm_pf_run_batch with
BSSM_MODEL_LGMV): every batched filter equals bootstrap_filter(..., seed=, stream=) on the same packed block bit for bit --
and bootstrap_filter on this family is held to the oracle (orc_pf_run_mv) by tests/test_gpu_mv.py.  PMMH on this family
(the reference's multi-dimensional case, tests/testthat/test-pmmh.R:619-668) then runs its pilot repetitions, pilot chains
and main chains through the batched kernel and returns the same numbers as its one-filter-at-a-time path."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_OBS = np.array([1, 2, 2, 5, 6, 6, 7, 9, 10, 11, 13, 14], dtype=np.int32)     # a gap of 3 and two repeated times
SEEDS = [1405, (1 << 33) + 7, 99, (1 << 40) + 3, 5]
STREAMS = [0, (1 << 35) + 1, 7, 3, 1 << 32]


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


def _pieces(d, p, seed=11):
    rng = np.random.default_rng(seed + 10 * d + p)
    A = 0.6 * np.eye(d) + 0.15 * rng.standard_normal((d, d))
    return dict(m0=rng.standard_normal(d), L0=np.tril(0.2 * rng.standard_normal((d, d))) + np.eye(d), A=A,
                b=0.1 * rng.standard_normal(d), L=np.tril(0.3 * rng.standard_normal((d, d))) + 0.7 * np.eye(d),
                c0=-0.3, H=rng.standard_normal((p, d)), h0=0.2 * rng.standard_normal(p), sd=0.5 + rng.random(p))


def _model(B, d, p):
    """general A (scaled by the parameter a), lower-triangular L0 / L, dense H, unequal sd (scaled by s)"""
    q = _pieces(d, p)
    A0, sd0 = q.pop("A"), q.pop("sd")
    return B.models.linear_gaussian_mv(d, p, build=lambda a, s: {"A": a * A0, "sd": s * sd0}, param_names=("a", "s"), **q)


def _data(d, p, T, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, p)) if p > 0 else np.zeros(T)


PARAMS = [{"a": 1.0, "s": 1.0}, {"a": 0.7, "s": 1.3}, {"a": 1.2, "s": 0.8}, {"a": 0.4, "s": 2.0}, {"a": 0.9, "s": 0.6}]


def _single(B, m, y, N, params, seed, stream, **kw):
    return B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, return_particles=False, seed=seed,
                              stream=stream, **kw, **params)


def _assert_same(B, m, d, out, y, N, **kw):
    for k, params in enumerate(PARAMS):
        ref = _single(B, m, y, N, params, SEEDS[k], STREAMS[k], **kw)
        assert out["loglike"][k] == ref["loglike"], (k, out["loglike"][k], ref["loglike"])
        np.testing.assert_array_equal(out["loglike_history"][k], ref["loglike_history"])
        np.testing.assert_array_equal(out["ess"][k], ref["ess"])
        np.testing.assert_array_equal(out["state_est"][k], np.asarray(ref["state_est"]).reshape(-1, d))
        assert out["n_res_calls"][k] == ref["_extras"]["n_res_calls"]
        assert out["early_return_step"][k] == ref["_extras"]["early_return_step"]


@pytest.mark.parametrize("ra", ["SISAR", "SISR", "SIS"])
@pytest.mark.parametrize("rf", ["stratified", "systematic"])
@pytest.mark.parametrize("N", [1, 7, 100, 384, 385, 1000, "max"])
@pytest.mark.parametrize("dp", [(1, 1), (2, 0), (3, 2), (8, 8)])
def test_batch_mv_equals_single_runs(B, dp, N, rf, ra):
    d, p = dp
    N = B.batch_max_particles(d) if N == "max" else N
    m = _model(B, d, p)
    y = _data(d, p, T_OBS.size)
    out = B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS, SEEDS, STREAMS, obs_times=T_OBS,
                                   resample_algorithm=ra, resample_fn=rf)
    assert out["state_est"].shape == (len(PARAMS), T_OBS.size + 1, d)
    assert np.all(out["status"] == 0)
    _assert_same(B, m, d, out, y, N, obs_times=T_OBS, resample_algorithm=ra, resample_fn=rf)


def test_batch_mv_packed_blocks_and_matrix_y(B):
    """thetas as an (F, n_theta) array of packed blocks equals the list of parameter dicts; y without obs_times"""
    d, p = 3, 2
    m = _model(B, d, p)
    y = _data(d, p, 20)
    blocks = np.array([m.pack(q) for q in PARAMS])
    a = B.bootstrap_filter_batch(y, 300, m.init_fn, m.transition_fn, m.log_likelihood_fn, blocks, SEEDS, STREAMS)
    b = B.bootstrap_filter_batch(y, 300, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS, SEEDS, STREAMS)
    for k in ("loglike", "state_est", "ess", "loglike_history"):
        np.testing.assert_array_equal(a[k], b[k])
    _assert_same(B, m, d, a, y, 300)


def test_batch_mv_in_order_and_record_paths_agree(B):
    """the in-order exact sums (N <= batch_literal_max) and the record machinery are both exact: moving the threshold
    changes no bit"""
    d, p = 3, 2
    m = _model(B, d, p)
    y = _data(d, p, T_OBS.size)
    cx = B.Context(0, 4096, 8)
    outs = []
    try:
        for lim in (0, 100000):
            cx.set_option("batch_literal_max", lim)
            outs.append([B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS, SEEDS, STREAMS,
                                                  obs_times=T_OBS, resample_algorithm=ra, resample_fn=rf, ctx=cx)
                         for N in (5, 64, 333, 1500, 2048) for rf in ("systematic", "stratified") for ra in ("SISR", "SISAR")])
    finally:
        cx.close()
    for a, c in zip(*outs):
        for k in ("loglike", "state_est", "ess", "loglike_history", "n_res_calls"):
            np.testing.assert_array_equal(a[k], c[k])


@pytest.mark.parametrize("dp", [(1, 1), (2, 1), (4, 3)])
def test_batch_mv_degenerate_early_return(B, dp):
    """every log-weight below -1e8 at observation 6 (sd = 1e-3, y far from the state): the reference returns at once --
    same step, NaN rows for d > 1 (0 for d = 1), ESS 0, log-likelihood history 0 -- as the one-at-a-time run"""
    d, p = dp
    q = _pieces(d, p)
    q["sd"] = np.full(p, 1e-3)
    m = B.models.linear_gaussian_mv(d, p, build=lambda a, s: {"b": np.full(d, 0.1 * a)}, param_names=("a", "s"), **q)
    y = _data(d, p, 10)
    y[5] = 1e3
    out = B.bootstrap_filter_batch(y, 200, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS, SEEDS, STREAMS)
    assert np.all(out["early_return_step"] == 6)
    _assert_same(B, m, d, out, y, 200)
    rows = out["state_est"][:, 6:, :]
    assert np.all(np.isnan(rows)) if d > 1 else np.all(rows == 0.0)
    assert np.all(out["ess"][:, 6:] == 0.0) and np.all(out["loglike_history"][:, 6:] == 0.0)


def test_batch_mv_capacity_and_rejections(B):
    from bayesssm_amd import _lib
    for d in range(1, 9):
        cap = B.batch_max_particles(d)
        assert cap >= (2048 if d <= 4 else 1000)
        m = _model(B, d, 1)
        y = _data(d, 1, 5)
        with pytest.raises(_lib.BssmError):
            B.bootstrap_filter_batch(y, cap + 1, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS[:2], 1, [0, 1])
    m = _model(B, 2, 1)
    y = _data(2, 1, 5)
    with pytest.raises(_lib.BssmError, match="stratified / systematic"):
        B.bootstrap_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS[:2], 1, [0, 1], resample_fn="multinomial")
    # rows of another (d, p) in one call: refused by the Python layer, and by the C ABI itself
    other = _model(B, 3, 0).pack(PARAMS[0])
    blocks = np.array([m.pack(PARAMS[0]), m.pack(PARAMS[1])])
    mixed = blocks.copy()
    mixed[1, 0] = 1.0
    with pytest.raises(ValueError):
        B.bootstrap_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, mixed, 1, [0, 1])
    with pytest.raises(ValueError):
        B.bootstrap_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, [blocks[0], other], 1, [0, 1])
    lib = _lib.load()
    cx = B.Context(0, 4096, 8)
    try:
        yv = np.ascontiguousarray(y, dtype=np.float64)
        F = 2
        ll, se = np.zeros(F), np.zeros((F, 6, 2))
        ess, llh, ers, nres, st, ms = np.zeros((F, 6)), np.zeros((F, 5)), np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(1)
        seeds, streams = np.ones(F, np.uint64), np.arange(F, dtype=np.uint64)
        p_ = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        res = _lib.PfBatchResult(p_(ll), p_(se), p_(ess), p_(llh), p_(ers), p_(nres), p_(st), p_(ms))

        def run(th):
            th = np.ascontiguousarray(th)
            cfg = _lib.PfConfig(_lib.MODEL["lgmv"], _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN["stratified"],
                                100, 5, float("nan"), None, int(th.shape[1]), p_(yv), None, 0, 0, None, None, None, 0, 0, 0.0, None, None)
            return lib.bssm_pf_run_batch(cx.handle, C.byref(cfg), F, p_(th), p_(seeds), p_(streams), C.byref(res))

        assert run(blocks) == _lib.OK and np.all(st == 0)
        assert run(mixed) != _lib.OK and b"same (d, p)" in lib.bssm_last_error()
    finally:
        cx.close()


def _pmmh_pair(B, args, kw):
    outs = []
    for bc in (True, False):
        outs.append(B.pmmh(*args, batch_chains=bc, return_latent_state_est=True, print_result=False, **kw))
    return outs


def _assert_pmmh_same(a, b, names):
    for k in names:
        np.testing.assert_array_equal(np.asarray(a["theta_chain"][k]), np.asarray(b["theta_chain"][k]))
    la, lb = a["_extras"]["local_chains"], b["_extras"]["local_chains"]
    assert sorted(la) == sorted(lb)
    for c in la:
        pa, pb = la[c]["pilot"], lb[c]["pilot"]
        assert pa["target_n"] == pb["target_n"]
        for k in ("pilot_theta_mean", "pilot_theta_cov", "pilot_theta_chain", "pilot_loglike_chain"):
            np.testing.assert_array_equal(pa[k], pb[k])
        assert pa["variance_estimate"] == pb["variance_estimate"] or (np.isnan(pa["variance_estimate"]) and np.isnan(pb["variance_estimate"]))
        assert la[c]["accepted"] == lb[c]["accepted"]
    assert sorted(a["latent_state_chain"]) == sorted(b["latent_state_chain"])
    for c in a["latent_state_chain"]:
        np.testing.assert_array_equal(a["latent_state_chain"][c], b["latent_state_chain"][c])
    assert a["_extras"]["batched"] is True and a["_extras"]["batched_launches"] > 0
    assert b["_extras"]["batched"] is False


def test_pmmh_reference_multi_dim_case_batched_equals_sequential(B):
    """tests/testthat/test-pmmh.R:619-668 (2-d random walk, constant log-likelihood, phi ~ N(0, 1)), small m / pilot_m"""
    m = B.models.linear_gaussian_mv(2, 0, c0=1.0, build=lambda phi: {"b": [phi, phi]}, param_names=("phi",))
    tc = B.default_tune_control(pilot_m=30, pilot_reps=20, pilot_burn_in=10)
    args = (B.bootstrap_filter, np.zeros(20), 40, m.init_fn, m.transition_fn, m.log_likelihood_fn, {"phi": B.prior_normal(0.0, 1.0)},
            [{"phi": 0.8}, {"phi": 0.5}], 10)
    a, b = _pmmh_pair(B, args, dict(num_chains=2, param_transform={"phi": "identity"}, seed=1405, tune_control=tc))
    _assert_pmmh_same(a, b, ["phi"])
    assert a["_extras"]["single_filter_runs"] == 0
    assert a["latent_state_chain"][0].shape == (30, 21, 2)


def test_pmmh_3x2_model_batched_equals_sequential(B):
    """(d, p) = (3, 2), build maps two parameters into A and sd; proposals outside the prior's support included"""
    q = _pieces(3, 2)
    A0, sd0 = q.pop("A"), q.pop("sd")
    m = B.models.linear_gaussian_mv(3, 2, build=lambda rho, s: {"A": rho * A0, "sd": s * sd0}, param_names=("rho", "s"), **q)
    rng = np.random.default_rng(8)
    x, ys = q["m0"].copy(), []
    for _ in range(25):
        x = 0.8 * A0 @ x + q["b"] + q["L"] @ rng.standard_normal(3)
        ys.append(q["h0"] + q["H"] @ x + sd0 * rng.standard_normal(2))
    tc = B.default_tune_control(pilot_m=30, pilot_n=100, pilot_reps=20, pilot_burn_in=10, pilot_proposal_sd=0.3)
    args = (B.bootstrap_filter, np.array(ys), 40, m.init_fn, m.transition_fn, m.log_likelihood_fn,
            {"rho": B.prior_uniform(0.0, 1.2), "s": B.prior_exponential(1.0)}, [{"rho": 0.5, "s": 1.0}, {"rho": 0.9, "s": 0.7},
                                                                               {"rho": 0.7, "s": 1.5}], 10)
    a, b = _pmmh_pair(B, args, dict(num_chains=3, param_transform={"rho": "identity", "s": "log"}, seed=77, tune_control=tc))
    _assert_pmmh_same(a, b, ["rho", "s"])
    assert a["latent_state_chain"][2].shape == (30, 26, 3)
