"""GPU tests of the genealogy smoother on the device (bssm_pf_run_smooth, smooth.hip.h) against its numpy
restatement (tests/smooth_restated.py) on the histories and ancestors of the same run.

    n_lineages, trajectory_index, trajectories     equal exactly
    smoothed_state_est[t, c]                       within  N 2^-52 sum_j |W[j] x_t,c[b_t(j)]|  of the fsum value: the bound of any
                                                   summation order of N fp64 terms (the products themselves are the same doubles on
                                                   both sides: the library is built without contraction)
Shapes: N in {1, 2, 100, one scan block = 2048, 2049, 5000}, T in {1, 12}, K in {1, 7, 300}."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_restated as SR  # noqa: E402

pytestmark = pytest.mark.gpu

EB = 2048                                           # NT * EL: the particles of one scan block
GAPS = [1, 2, 5, 5, 6, 7, 8, 9, 10, 11, 12, 13]     # a gap of 3 and a repeated time
LG = dict(phi=0.8, sigma_x=0.5, sigma_y=2.0)
# mostly flat weights (sigma_y is large against the state's spread: ESS near N, carried under SISAR) and two far-out
# observations (ESS / N about exp(-(6 / 4)^2 0.7) = 0.2: resampled)
Y_LG = np.array([0.3, -0.2, 6.0, 0.1, 0.4, -0.5, -6.0, 0.2, 0.0, 0.6, -0.1, 0.3])
Y_SIR = np.array([76, 89, 93, 101, 117, 120, 135, 128, 140, 139, 131, 150], dtype=np.float64)
SIR_PAR = {"lambda": 0.5, "gamma": 0.2}
SEIR_PAR = dict(beta=0.004, sigma=0.5, gamma=0.3)
Y_SEIR = np.array([8, 9, 12, 13, 17, 19, 20, 24, 25, 27, 26, 30], dtype=np.float64)
FIELDS = ("loglike", "loglike_history", "ess", "state_est")


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 13, 8)
    yield c
    c.close()


def run(B, m, alg, y, N, **kw):
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    if alg == "APF":
        return B.auxiliary_filter(y, N, *fns, m.aux_log_likelihood_fn, **kw)
    if alg == "RMPF":
        kw.pop("resample_algorithm", None)
        return B.resample_move_filter(y, N, *fns, m.rw_move_fn(0.3), **kw)
    return B.bootstrap_filter(y, N, *fns, **kw)


def check_against_restatement(res, N, T, d, K):
    ex = res["_extras"]
    assert ex["early_return_step"] == 0
    assert ex["call_obs"].shape == (ex["n_res_calls"],) == (ex["ancestors"].shape[0],)
    assert np.all(np.diff(ex["call_obs"]) >= 0) and (ex["n_res_calls"] == 0 or (ex["call_obs"].min() >= 1 and ex["call_obs"].max() <= T))
    ph, wh = res["particles_history"], res["weights_history"]
    ref = SR.smooth(ph, wh, ex["ancestors"], ex["call_obs"], d)
    assert res["n_lineages"].shape == (T + 1,) and np.array_equal(res["n_lineages"], ref["n_lineages"])
    assert res["n_lineages"][T] == N
    assert res["smoothed_state_est"].shape == ((T + 1, d) if d > 1 else (T + 1,))
    got = res["smoothed_state_est"].reshape(T + 1, d)
    err, bound = np.abs(got - ref["smoothed"]), N * 2.0 ** -52 * ref["abs_sum"]
    print("smoothed: max error %.3e, the bound there %.3e" % (err.max(), bound.reshape(-1)[err.argmax()]))
    assert np.all(err <= bound)
    u = ex["trajectory_u"]
    assert u.shape == (K,) and np.all((u > 0) & (u < 1))
    idx = SR.terminal_indices(wh[T], u)
    assert np.array_equal(ex["trajectory_index"], idx)
    assert res["trajectories"].shape == (K, T + 1, d)
    assert np.array_equal(res["trajectories"], SR.paths(ph, ref["b"], idx, d))
    return ref


KW = dict(smooth=True, return_particles=True, return_ancestors=True)

LG_CASES = [
    # alg, N, T, K, resample_algorithm, resample_fn, obs_times
    ("BPF", 1, 1, 1, "SISR", "stratified", None),
    ("BPF", 2, 12, 7, "SISAR", "systematic", None),
    ("BPF", 100, 12, 300, "SISR", "stratified", None),
    ("BPF", EB, 12, 7, "SISR", "systematic", None),
    ("BPF", EB + 1, 1, 300, "SISR", "stratified", None),
    ("BPF", 5000, 12, 7, "SISR", "stratified", GAPS),
    ("BPF", EB + 1, 12, 300, "SISR", "multinomial", None),
    ("BPF", 100, 12, 7, "SISAR", "multinomial", None),
    ("APF", 100, 1, 1, "SISR", "stratified", None),
    ("APF", EB + 1, 12, 7, "SISAR", "stratified", None),
    ("APF", 5000, 12, 300, "SISR", "systematic", GAPS),
    ("RMPF", EB, 12, 7, "SISR", "stratified", None),
    ("RMPF", 5000, 12, 1, "SISR", "systematic", GAPS),
]


@pytest.mark.parametrize("alg,N,T,K,ra,rf,ot", LG_CASES)
def test_lg_device_against_restatement(B, ctx, alg, N, T, K, ra, rf, ot):
    m = B.models.linear_gaussian()
    res = run(B, m, alg, Y_LG[:T], N, trajectories=K, obs_times=None if ot is None else ot[:T], resample_algorithm=ra, resample_fn=rf,
              seed=11, stream=N % 7, ctx=ctx, **KW, **LG)
    check_against_restatement(res, N, T, 1, K)
    if alg == "APF" and ra == "SISR":
        assert res["_extras"]["n_res_calls"] == 2 * T and np.array_equal(res["_extras"]["call_obs"], np.repeat(np.arange(1, T + 1), 2))


@pytest.mark.parametrize("N", [100, EB + 1])
def test_sis_keeps_every_lineage(B, ctx, N):
    """SIS never resamples: identity lineages, n_lineages is N at every t, the smoothed means are the final weights on every history row"""
    m = B.models.linear_gaussian()
    res = run(B, m, "BPF", Y_LG, N, trajectories=7, resample_algorithm="SIS", seed=5, stream=1, ctx=ctx, **KW, **LG)
    ref = check_against_restatement(res, N, 12, 1, 7)
    assert res["_extras"]["n_res_calls"] == 0 and np.all(res["n_lineages"] == N)
    assert np.array_equal(ref["b"], np.tile(np.arange(N), (13, 1)))


@pytest.mark.parametrize("N", [100, 5000])
def test_sisar_mixes_resampled_and_carried_steps(B, ctx, N):
    m = B.models.linear_gaussian()
    res = run(B, m, "BPF", Y_LG, N, trajectories=7, resample_algorithm="SISAR", resample_fn="stratified", seed=5, stream=2, ctx=ctx, **KW, **LG)
    resampled = np.asarray(res["_extras"]["resampled"], dtype=bool)
    assert resampled.any() and (~resampled).any(), resampled
    assert np.array_equal(res["_extras"]["call_obs"], np.flatnonzero(resampled) + 1)
    check_against_restatement(res, N, 12, 1, 7)


@pytest.mark.parametrize("N,T,K,ra,ot", [(EB + 1, 12, 7, "SISAR", None), (100, 12, 300, "SISR", GAPS), (2, 1, 1, "SISR", None)])
def test_sir_two_components(B, ctx, N, T, K, ra, ot):
    m = B.models.sir()
    res = run(B, m, "BPF", Y_SIR[:T], N, trajectories=K, obs_times=None if ot is None else ot[:T], resample_algorithm=ra, seed=3, stream=4, ctx=ctx,
              **KW, **SIR_PAR)
    check_against_restatement(res, N, T, 2, K)


def _mv_model(rng, d, p):
    A = 0.6 * np.eye(d) + 0.1 * rng.standard_normal((d, d))
    Lq = np.tril(0.3 * rng.standard_normal((d, d))) + 0.7 * np.eye(d)
    L0 = np.tril(0.2 * rng.standard_normal((d, d))) + np.eye(d)
    q = dict(m0=rng.standard_normal(d), L0=L0, A=A, b=0.1 * rng.standard_normal(d), L=Lq, H=rng.standard_normal((p, d)),
             h0=0.2 * rng.standard_normal(p), sd=0.5 + rng.random(p))
    x, ys = q["m0"] + L0 @ rng.standard_normal(d), np.zeros((12, p))
    for t in range(12):
        x = A @ x + q["b"] + Lq @ rng.standard_normal(d)
        ys[t] = q["h0"] + q["H"] @ x + q["sd"] * rng.standard_normal(p)
    return q, ys


MV_CASES = [
    ("BPF", 3, 2, EB + 1, 12, 7, "SISAR", None), ("APF", 3, 2, 5000, 12, 300, "SISR", GAPS), ("RMPF", 3, 2, 100, 12, 1, "SISR", None),
    ("BPF", 8, 8, 5000, 12, 1, "SISR", GAPS), ("APF", 8, 8, EB, 12, 7, "SISAR", None), ("RMPF", 8, 8, EB + 1, 1, 300, "SISR", None),
    ("BPF", 3, 2, 1, 12, 7, "SISR", None), ("APF", 8, 8, 2, 1, 1, "SISR", None),
]


@pytest.mark.parametrize("alg,d,p,N,T,K,ra,ot", MV_CASES)
def test_lgmv_device_against_restatement(B, ctx, alg, d, p, N, T, K, ra, ot):
    q, ys = _mv_model(np.random.default_rng(100 * d + p), d, p)
    m = B.models.linear_gaussian_mv(d, p, **q)
    res = run(B, m, alg, ys[:T], N, trajectories=K, obs_times=None if ot is None else ot[:T], resample_algorithm=ra, resample_fn="systematic",
              seed=8, stream=d, ctx=ctx, **KW)
    check_against_restatement(res, N, T, d, K)


def _seir(B):
    return B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                            ({"I": 1}, {"R": 1}, "gamma")], x0=[180.0, 8.0, 12.0, 0.0], observe=[{"I": 0.6}])


@pytest.mark.parametrize("alg,N,T,K,ra,ot", [("BPF", EB + 1, 12, 7, "SISAR", None), ("APF", 5000, 12, 300, "SISR", GAPS), ("BPF", 100, 1, 1, "SISR", None),
                                             ("APF", 2, 12, 7, "SISAR", None)])
def test_rnet_seir_device_against_restatement(B, ctx, alg, N, T, K, ra, ot):
    res = run(B, _seir(B), alg, Y_SEIR[:T], N, trajectories=K, obs_times=None if ot is None else ot[:T], resample_algorithm=ra, seed=23, stream=4,
              ctx=ctx, **KW, **SEIR_PAR)
    check_against_restatement(res, N, T, 4, K)


# ---- 2. the filter's own outputs do not move --------------------------------------------------------------------------------------
def _same_filter_outputs(a, b):
    for k in FIELDS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    assert a["_extras"]["n_res_calls"] == b["_extras"]["n_res_calls"]


@pytest.mark.parametrize("alg", ["BPF", "APF", "RMPF"])
def test_filter_outputs_unchanged_small(B, ctx, alg):
    m = B.models.linear_gaussian()
    kw = dict(resample_algorithm="SISAR", resample_fn="stratified", seed=9, stream=3, ctx=ctx, return_particles=False, **LG)
    _same_filter_outputs(run(B, m, alg, Y_LG, 100, smooth=True, **kw), run(B, m, alg, Y_LG, 100, **kw))
    q, ys = _mv_model(np.random.default_rng(302), 3, 2)
    mv = B.models.linear_gaussian_mv(3, 2, **q)
    kw = dict(resample_algorithm="SISAR", resample_fn="systematic", seed=9, stream=3, ctx=ctx, return_particles=False)
    _same_filter_outputs(run(B, mv, alg, ys, 100, trajectories=3, **kw), run(B, mv, alg, ys, 100, **kw))
    if alg != "RMPF":
        kw = dict(resample_algorithm="SISAR", seed=9, stream=3, ctx=ctx, return_particles=False, **SEIR_PAR)
        _same_filter_outputs(run(B, _seir(B), alg, Y_SEIR, 100, smooth=True, **kw), run(B, _seir(B), alg, Y_SEIR, 100, **kw))
    if alg == "BPF":
        kw = dict(seed=9, stream=3, ctx=ctx, return_particles=False, **SIR_PAR)
        _same_filter_outputs(run(B, B.models.sir(), alg, Y_SIR, 100, smooth=True, **kw), run(B, B.models.sir(), alg, Y_SIR, 100, **kw))


def test_filter_outputs_unchanged_where_the_default_path_is_the_one_launch_step(B):
    """The smallest N whose default path is the fused one-launch step (more than FZ_MINB = 256 scan blocks): 256 * 2048 + 1, T = 3.
    The plain call runs there; the smoothing call runs the path return_particles / return_ancestors select.  Same outputs."""
    N = 256 * EB + 1
    big = B.Context(0, N, 1)
    try:
        m = B.models.linear_gaussian()
        kw = dict(resample_algorithm="SISR", resample_fn="systematic", seed=4, stream=1, ctx=big, return_particles=False, **LG)
        a = run(B, m, "BPF", Y_LG[:3], N, smooth=True, **kw)
        _same_filter_outputs(a, run(B, m, "BPF", Y_LG[:3], N, **kw))
        assert a["n_lineages"][3] == N and np.all(np.diff(a["n_lineages"]) >= 0) and a["n_lineages"][0] >= 1
        assert np.all(np.isfinite(a["smoothed_state_est"]))
    finally:
        big.close()


# ---- 3, 4. reproducible; the host copy of the histories is not needed ------------------------------------------------------------
def test_reproducible_and_independent_of_the_host_copy(B, ctx):
    q, ys = _mv_model(np.random.default_rng(302), 3, 2)
    m = B.models.linear_gaussian_mv(3, 2, **q)
    kw = dict(trajectories=7, resample_algorithm="SISAR", resample_fn="stratified", seed=6, stream=2, ctx=ctx)
    a = run(B, m, "APF", ys, 5000, return_particles=True, return_ancestors=True, **kw)
    b = run(B, m, "APF", ys, 5000, return_particles=True, return_ancestors=True, **kw)
    c = run(B, m, "APF", ys, 5000, return_particles=False, **kw)
    assert "particles_history" not in c and "ancestors" not in c["_extras"]
    for other in (b, c):
        for k in ("smoothed_state_est", "n_lineages", "trajectories"):
            assert np.array_equal(a[k], other[k]), k
        for k in ("trajectory_u", "trajectory_index", "call_obs"):
            assert np.array_equal(a["_extras"][k], other["_extras"][k]), k
    assert a["_extras"]["smooth_ms"] > 0 and c["_extras"]["smooth_ms"] > 0


def test_keywords_absent_leave_the_result_as_it_was(B, ctx):
    m = B.models.linear_gaussian()
    res = run(B, m, "BPF", Y_LG, 100, seed=1, stream=0, ctx=ctx, **LG)
    assert not {"smoothed_state_est", "n_lineages", "trajectories"} & set(res)
    assert not {"call_obs", "smooth_ms", "trajectory_u", "trajectory_index"} & set(res["_extras"])
    only = run(B, m, "BPF", Y_LG, 100, seed=1, stream=0, smooth=True, ctx=ctx, **LG)
    assert "trajectories" not in only and "trajectory_u" not in only["_extras"] and only["smoothed_state_est"].shape == (13,)


# ---- 5. the exact smoother on the device filter -----------------------------------------------------------------------------------
def test_device_smoother_meets_the_exact_smoothed_means(B, ctx):
    """the CPU test's model, T, N and 32 (seed, stream) pairs: within 5 standard errors of the Rauch-Tung-Striebel means at every t"""
    m = B.models.linear_gaussian()
    reps = [run(B, m, "BPF", SR.EXACT_Y, SR.EXACT_N, smooth=True, return_particles=False, resample_algorithm="SISR", resample_fn="stratified",
                seed=s, stream=k, ctx=ctx, **SR.EXACT)["smoothed_state_est"] for s, k in SR.EXACT_SEEDS]
    ok, z = SR.within_5_se(reps, SR.exact_means())
    print("exact", SR.exact_means(), "mean", np.mean(reps, axis=0), "z", z)
    assert ok.all(), z


# ---- 6. early return -----------------------------------------------------------------------------------------------------------
def test_early_return_is_not_traced(B, ctx):
    m = B.models.linear_gaussian()
    y = np.array([0.3, -0.2, 0.1, 1e6, 0.4])                  # all(log_weights < -1e8) at observation 4
    res = run(B, m, "BPF", y, 100, trajectories=3, seed=1, stream=0, ctx=ctx, **KW, **LG)
    assert res["_extras"]["early_return_step"] == 4 and res["particles_history"].shape[0] == 4
    assert res["smoothed_state_est"] is None and res["n_lineages"] is None and res["trajectories"] is None
    assert res["_extras"]["trajectory_u"] is None and res["_extras"]["trajectory_index"] is None
    assert res["_extras"]["smooth_ms"] == 0.0
    plain = run(B, m, "BPF", y, 100, seed=1, stream=0, ctx=ctx, return_ancestors=True, **LG)
    _same_filter_outputs(res, plain)


# ---- 7. the C ABI ------------------------------------------------------------------------------------------------------------
def test_c_abi(B, ctx):
    from bayesssm_amd import _lib
    lib = _lib.load()
    N, T, K = 100, 12, 7
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    theta, y = np.array([0.8, 0.5, 2.0]), Y_LG.copy()
    se, ess, llh, ll, nres = np.zeros(T + 1), np.zeros(T + 1), np.zeros(T), np.zeros(1), np.zeros(1, dtype=np.int32)
    cfg = _lib.PfConfig(_lib.MODEL["lg"], _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN["stratified"], N, T, float("nan"),
                        p_(theta), 3, p_(y), None, 11, 2, None, None, None, 0, 0, 0.0, None, None)
    res = _lib.PfResult(p_(se), p_(ess), p_(llh), p_(ll), None, p_(nres), None, None, None, None, None, None)
    scfg = _lib.SmoothConfig(K)
    st = lib.bssm_pf_run_smooth(ctx.handle, C.byref(cfg), C.byref(res), C.byref(scfg), None)
    assert st == _lib.ERR_ARG and b"bssm_pf_run_smooth" in lib.bssm_last_error()
    sm, nl, tr, u, idx, co, ms = (np.zeros(T + 1), np.zeros(T + 1, dtype=np.int32), np.zeros((K, T + 1, 1)), np.zeros(K), np.zeros(K, dtype=np.int32),
                                  np.zeros(T, dtype=np.int32), np.zeros(1))
    sres = _lib.SmoothResult(p_(sm), p_(nl), p_(tr), p_(u), p_(idx), p_(co), p_(ms))
    bad = _lib.SmoothConfig(4097)
    assert lib.bssm_pf_run_smooth(ctx.handle, C.byref(cfg), C.byref(res), C.byref(bad), C.byref(sres)) == _lib.ERR_ARG
    _lib.check(lib.bssm_pf_run_smooth(ctx.handle, C.byref(cfg), C.byref(res), C.byref(scfg), C.byref(sres)))
    m = B.models.linear_gaussian()
    py = run(B, m, "BPF", Y_LG, N, trajectories=K, resample_algorithm="SISAR", resample_fn="stratified", seed=11, stream=2, ctx=ctx,
             return_particles=False, **LG)
    assert ll[0] == py["loglike"] and np.array_equal(se, py["state_est"])
    assert np.array_equal(sm, py["smoothed_state_est"]) and np.array_equal(nl, py["n_lineages"]) and np.array_equal(tr, py["trajectories"])
    assert np.array_equal(u, py["_extras"]["trajectory_u"]) and np.array_equal(idx, py["_extras"]["trajectory_index"])
    assert np.array_equal(co[: nres[0]], py["_extras"]["call_obs"]) and ms[0] > 0
