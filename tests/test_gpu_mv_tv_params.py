"""Time-varying b / h0 / H of the multivariate linear-Gaussian family that depend on the sampled parameters (an input gain
b_t = g u_t, a seasonal amplitude h0_t = a s_t): `build` returns them per draw, the single filters take the draw's arrays, the
batched kernel reads one array SET per draw (bssm_pf_run_batch_tv, k_pf_batch_mv) and PMMH's lock-step path stays bit-identical
to its one-filter-at-a-time path.  Everything is compared bit for bit with paths that tests/test_gpu_mv_tv.py holds to the
restated arithmetic: a descriptor constructed with the evaluated arrays, and bootstrap_filter on one draw."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_OBS = np.array([1, 2, 2, 5, 6, 6, 7, 9, 10, 11, 13, 14], dtype=np.int32)     # a gap of 3 and two repeated times
T = T_OBS.size
NB = 16                                                                       # rows of b: more than the last time
SEEDS = [1405, (1 << 33) + 7, 99, (1 << 40) + 3, 5, 77]
STREAMS = [0, (1 << 35) + 1, 7, 3, 1 << 32, 12]
GAINS = [1.0, 1.25, 1.5, 1.75, 2.0, 2.25]                                      # g of filter k = 1 + k / 4 (k is read back from g)
PARAMS = [{"g": g, "a": a} for g, a in zip(GAINS, [0.4, -1.3, 0.9, 2.0, 0.1, -0.6])]
FIELDS = ("loglike", "loglike_history", "ess", "state_est")


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


def _pieces(d, p, seed=23):
    """general A, lower-triangular L0 / L, dense H; H small and sd large enough that the offsets of b below (hundreds) leave
    the filters alive (no log-weight falls below the reference's -1e8)"""
    rng = np.random.default_rng(seed + 10 * d + p)
    return dict(m0=rng.standard_normal(d), L0=np.tril(0.2 * rng.standard_normal((d, d))) + np.eye(d),
                A=0.6 * np.eye(d) + 0.1 * rng.standard_normal((d, d)), b=0.1 * rng.standard_normal(d),
                L=np.tril(0.3 * rng.standard_normal((d, d))) + 0.7 * np.eye(d), c0=-0.3, H=0.1 * rng.standard_normal((p, d)),
                h0=0.2 * rng.standard_normal(p), sd=2.0 + rng.random(p))


def _arrays(d, p, seed=5):
    rng = np.random.default_rng(seed + 10 * d + p)
    return rng.standard_normal((NB, d)), rng.standard_normal((T, p)), 0.1 * rng.standard_normal((T, p, d))


def _b_of(U, g):
    """filter k's (g = 1 + k / 4) row r of b is offset by 100 k + r: a wrong stride or a wrong set cannot give the right numbers"""
    k = int(round(4 * (g - 1.0)))
    return g * U + (100.0 * k + np.arange(U.shape[0]))[:, None]


def _model(B, d, p, pieces=("b", "h0"), **kw):
    """build returns the per-draw arrays named in `pieces`:  b = g U + offsets,  h0 = a S,  H = g H0"""
    U, S, H0 = _arrays(d, p)
    make = {"b": lambda g, a: _b_of(U, g), "h0": lambda g, a: a * S, "H": lambda g, a: g * H0}
    return B.models.linear_gaussian_mv(d, p, build=lambda g, a: {"sd": (1.0 + 0.1 * abs(a)) * _pieces(d, p)["sd"],
                                                                 "time_varying": {k: make[k](g, a) for k in pieces}},
                                       param_names=("g", "a"), **dict(_pieces(d, p), **kw))


def _data(p, n=T, seed=3):
    return np.random.default_rng(seed).standard_normal((n, p))


def _assert_equal_runs(a, b, d):
    """two single-filter results, bit for bit"""
    for k in FIELDS:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
    assert a["_extras"]["n_res_calls"] == b["_extras"]["n_res_calls"]
    assert a["_extras"]["early_return_step"] == b["_extras"]["early_return_step"]


def _assert_batch_equals_singles(B, m, d, out, y, N, params, **kw):
    assert np.all(out["status"] == 0)
    for k, q in enumerate(params):
        ref = B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, return_particles=False, seed=SEEDS[k],
                                 stream=STREAMS[k], **kw, **q)
        assert out["loglike"][k] == ref["loglike"], (k, out["loglike"][k], ref["loglike"])
        np.testing.assert_array_equal(out["loglike_history"][k], ref["loglike_history"])
        np.testing.assert_array_equal(out["ess"][k], ref["ess"])
        np.testing.assert_array_equal(out["state_est"][k], np.asarray(ref["state_est"]).reshape(-1, d))
        assert out["n_res_calls"][k] == ref["_extras"]["n_res_calls"]
        assert out["early_return_step"][k] == ref["_extras"]["early_return_step"]


def _assert_batches_equal(a, b):
    for k in FIELDS + ("n_res_calls", "early_return_step", "status"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- one filter at a time ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["bootstrap", "auxiliary", "resample_move"])
def test_single_filter_takes_the_draws_arrays(B, which):
    """filter(..., g=1.7, a=0.4) on the parameter-dependent descriptor == the same call on a descriptor constructed with
    time_varying= holding the evaluated arrays"""
    d, p, N = 3, 2, 3000
    U, S, H0 = _arrays(d, p)
    q = _pieces(d, p)
    m = B.models.linear_gaussian_mv(d, p, build=lambda g, a: {"A": q["A"], "time_varying": {"b": g * U, "h0": a * S}},
                                    param_names=("g", "a"), time_varying={"H": H0, "h0": np.zeros((T, p))}, **q)
    fixed = B.models.linear_gaussian_mv(d, p, build=lambda g, a: {"A": q["A"]}, param_names=("g", "a"),
                                        time_varying={"b": 1.7 * U, "h0": 0.4 * S, "H": H0}, **q)
    y = _data(p)

    def run(mm):
        kw = dict(obs_times=T_OBS, return_particles=False, seed=SEEDS[1], stream=STREAMS[1], g=1.7, a=0.4)
        fns = (mm.init_fn, mm.transition_fn, mm.log_likelihood_fn)
        if which == "bootstrap":
            return B.bootstrap_filter(y, N, *fns, **kw)
        if which == "auxiliary":
            return B.auxiliary_filter(y, N, *fns, mm.aux_log_likelihood_fn, **kw)
        return B.resample_move_filter(y, N, *fns, mm.rw_move_fn(0.3), **kw)

    a, b = run(m), run(fixed)
    _assert_equal_runs(a, b, d)
    assert a["_extras"]["early_return_step"] == 0 and np.isfinite(a["loglike"])
    other = B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, obs_times=T_OBS, return_particles=False,
                               seed=SEEDS[1], stream=STREAMS[1], g=1.7, a=0.5)
    assert which != "bootstrap" or other["loglike"] != a["loglike"]            # (the draw's arrays are read, not the first draw's)


# ---- batched -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ra", ["SISAR", "SISR", "SIS"])
@pytest.mark.parametrize("rf", ["stratified", "systematic"])
@pytest.mark.parametrize("N", [1, 7, 385, 1000, "max"])
@pytest.mark.parametrize("dp", [(1, 1), (3, 2), (8, 8)])
def test_batch_equals_single_runs(B, dp, N, rf, ra):
    d, p = dp
    N = B.batch_max_particles(d) if N == "max" else N
    m = _model(B, d, p)
    y = _data(p)
    out = B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS[:5], SEEDS[:5], STREAMS[:5],
                                   obs_times=T_OBS, resample_algorithm=ra, resample_fn=rf)
    assert out["state_est"].shape == (5, T + 1, d)
    assert np.all(out["early_return_step"] == 0) and np.all(np.isfinite(out["loglike"]))     # (the filters run to the end)
    assert len(set(out["loglike"])) == 5
    _assert_batch_equals_singles(B, m, d, out, y, N, PARAMS[:5], obs_times=T_OBS, resample_algorithm=ra, resample_fn=rf)


@pytest.mark.parametrize("dp", [(1, 1), (3, 2), (8, 8)])
def test_batch_only_b_per_set(B, dp):
    """b per set, h0 one shared array (the constructor's), H from the blocks"""
    d, p = dp
    m = _model(B, d, p, pieces=("b",), time_varying={"h0": _arrays(d, p)[1]})
    y = _data(p)
    out = B.bootstrap_filter_batch(y, 500, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS[:5], SEEDS[:5], STREAMS[:5], obs_times=T_OBS)
    _assert_batch_equals_singles(B, m, d, out, y, 500, PARAMS[:5], obs_times=T_OBS)


@pytest.mark.parametrize("dp", [(1, 1), (3, 2), (8, 8)])
def test_batch_only_H_per_set(B, dp):
    d, p = dp
    m = _model(B, d, p, pieces=("H",))
    y = _data(p)
    out = B.bootstrap_filter_batch(y, 500, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS[:5], SEEDS[:5], STREAMS[:5], obs_times=T_OBS)
    assert len(set(out["loglike"])) == 5
    _assert_batch_equals_singles(B, m, d, out, y, 500, PARAMS[:5], obs_times=T_OBS)


def test_batch_without_observations(B):
    """T = 0: nothing is read from the sets; the t = 0 row as the single filters return it"""
    d, p = 3, 2
    m = _model(B, d, p, pieces=("b",))
    y = np.zeros((0, p))
    out = B.bootstrap_filter_batch(y, 300, m.init_fn, m.transition_fn, m.log_likelihood_fn, PARAMS[:5], SEEDS[:5], STREAMS[:5])
    assert out["state_est"].shape == (5, 1, d)
    _assert_batch_equals_singles(B, m, d, out, y, 300, PARAMS[:5])


# ---- sets ----------------------------------------------------------------------------------------------------------

def test_set_indirection_equals_repeated_arrays(B):
    """F = 6 filters on G = 2 sets through tv_set == the F = 6, G = 6 call with the arrays repeated; the list-of-dicts form
    with repeated dicts == the explicit form"""
    d, p, N = 3, 2, 700
    m = _model(B, d, p)
    U, S, _ = _arrays(d, p)
    y = _data(p)
    tv_set = [0, 1, 1, 0, 1, 0]
    two = [PARAMS[1], PARAMS[4]]
    dicts = [two[s] for s in tv_set]
    blocks = np.array([m.pack(q) for q in dicts])
    b2, h2 = np.stack([_b_of(U, q["g"]) for q in two]), np.stack([q["a"] * S for q in two])
    args = (y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn)
    by_set = B.bootstrap_filter_batch(*args, blocks, SEEDS, STREAMS, obs_times=T_OBS, time_varying={"b": b2, "h0": h2}, tv_set=tv_set)
    repeated = B.bootstrap_filter_batch(*args, blocks, SEEDS, STREAMS, obs_times=T_OBS, time_varying={"b": b2[tv_set], "h0": h2[tv_set]})
    by_dicts = B.bootstrap_filter_batch(*args, dicts, SEEDS, STREAMS, obs_times=T_OBS)
    _assert_batches_equal(by_set, repeated)
    _assert_batches_equal(by_set, by_dicts)
    _assert_batch_equals_singles(B, m, d, by_set, y, N, dicts, obs_times=T_OBS)
    assert by_set["loglike"][0] != by_set["loglike"][1]


# ---- the C ABI's refusals --------------------------------------------------------------------------------------------

def test_c_abi_refusals_then_a_valid_call(B):
    from bayesssm_amd import _lib
    d, p, N, F, G = 3, 2, 200, 3, 2
    m = _model(B, d, p)
    U, S, _ = _arrays(d, p)
    set_of = np.array([0, 1, 1], dtype=np.int32)
    blocks = np.ascontiguousarray([m.pack(PARAMS[k]) for k in set_of])          # (filter f: the block AND the arrays of draw set_of[f])
    y = np.ascontiguousarray(_data(p))
    b_sets = np.ascontiguousarray(np.stack([_b_of(U, PARAMS[k]["g"]) for k in range(G)]))
    h_sets = np.ascontiguousarray(np.stack([PARAMS[k]["a"] * S for k in range(G)]))
    ll, se = np.zeros(F), np.zeros((F, T + 1, d))
    ess, llh, ers, nres, st, ms = np.zeros((F, T + 1)), np.zeros((F, T)), np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(1)
    seeds, streams = np.array(SEEDS[:F], dtype=np.uint64), np.array(STREAMS[:F], dtype=np.uint64)
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    res = _lib.PfBatchResult(p_(ll), p_(se), p_(ess), p_(llh), p_(ers), p_(nres), p_(st), p_(ms))
    lib = _lib.load()
    cx = B.Context(0, 4096, 8)

    def run(n_times=NB, b=b_sets, b_stride=NB * d, h0=h_sets, sets=set_of, n_sets=G, mv_tv=None):
        cfg = _lib.PfConfig(_lib.MODEL["lgmv"], _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN["stratified"],
                            N, T, float("nan"), None, int(blocks.shape[1]), p_(y), p_(T_OBS), 0, 0, None, None, None, 0, 0, 0.0, None, None,
                            C.cast(C.pointer(mv_tv), C.c_void_p) if mv_tv is not None else None)
        tv = _lib.MvTvBatch(n_times, n_sets, p_(sets), p_(b), b_stride, p_(h0), T * p, None, 0)
        return lib.bssm_pf_run_batch_tv(cx.handle, C.byref(cfg), F, p_(blocks), p_(seeds), p_(streams), C.byref(tv), C.byref(res))

    def refused(**kw):
        rc = run(**kw)
        msg = lib.bssm_last_error().decode()
        assert rc == _lib.ERR_ARG and msg.startswith("bssm_pf_run_batch_tv: mv_tv:"), (kw.keys(), rc, msg)
        return msg

    try:
        assert "n_times" in refused(n_times=13, b=np.ascontiguousarray(b_sets[:, :13]), b_stride=13 * d)       # the last time is 14
        nan1 = h_sets.copy()
        nan1[1, 7, 1] = np.nan
        assert "h0_t contains non-finite" in refused(h0=nan1)                                                  # in set 1 only
        assert "stride" in refused(b_stride=1)
        assert "set_of" in refused(sets=np.array([0, 1, G], dtype=np.int32))
        assert "cfg->mv_tv must be NULL" in refused(mv_tv=_lib.MvTv(NB, p_(b_sets), None, None))
        assert run() == _lib.OK and np.all(st == 0)                                                            # the same context, a valid call
        out = {"loglike": ll, "loglike_history": llh, "ess": ess, "state_est": se, "n_res_calls": nres, "early_return_step": ers, "status": st}
        _assert_batch_equals_singles(B, m, d, out, y, N, [PARAMS[s] for s in set_of], obs_times=T_OBS)
    finally:
        cx.close()


# ---- PMMH ------------------------------------------------------------------------------------------------------------

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


def test_pmmh_learns_gain_and_amplitude_batched_equals_sequential(B):
    """(d, p) = (2, 1): an input gain g (b_t = g u_t) and a seasonal amplitude a (h0_t = a sin(t / 2)) as sampled parameters"""
    n = 25
    rng = np.random.default_rng(8)
    u = rng.standard_normal((n, 2))
    s = np.sin(0.5 * np.arange(1, n + 1)).reshape(n, 1)
    q = dict(A=np.array([[0.7, 0.1], [0.0, 0.5]]), L=0.5 * np.eye(2), H=np.array([[1.0, 0.5]]), sd=[0.7])
    m = B.models.linear_gaussian_mv(2, 1, build=lambda g, a: {"time_varying": {"b": g * u, "h0": a * s}}, param_names=("g", "a"), **q)
    x, ys = np.zeros(2), []
    for i in range(n):
        x = q["A"] @ x + 1.0 * u[i] + q["L"] @ rng.standard_normal(2)
        ys.append(0.8 * s[i] + q["H"] @ x + 0.7 * rng.standard_normal(1))
    tc = B.default_tune_control(pilot_m=30, pilot_n=100, pilot_reps=20, pilot_burn_in=10)
    args = (B.bootstrap_filter, np.array(ys), 40, m.init_fn, m.transition_fn, m.log_likelihood_fn,
            {"g": B.prior_normal(0.0, 2.0), "a": B.prior_exponential(1.0)}, [{"g": 0.8, "a": 1.0}, {"g": 1.2, "a": 0.5}, {"g": 1.0, "a": 0.8}], 10)
    kw = dict(num_chains=3, param_transform={"g": "identity", "a": "log"}, seed=77, tune_control=tc)
    a, b = [B.pmmh(*args, batch_chains=bc, return_latent_state_est=True, print_result=False, **kw) for bc in (True, False)]
    _assert_pmmh_same(a, b, ["g", "a"])
    assert a["_extras"]["single_filter_runs"] == 0
    assert a["latent_state_chain"][2].shape == (30, n + 1, 2)
    assert len(np.unique(np.asarray(a["theta_chain"]["g"]))) > 3               # (proposals were accepted: the arrays did change)
