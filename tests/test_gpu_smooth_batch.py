"""GPU tests of the batched genealogy smoother (bootstrap_smoother_batch, bssm_pf_run_batch_smooth: the recording form of
k_pf_batch_mv / k_pf_batch_rn and k_trace_batch).  The oracle is the single-filter smoother, itself held to the numpy
restatement by tests/test_gpu_smooth.py: for every filter f of a launch

    bootstrap_filter(..., smooth=True, trajectories=K, seed=seeds[f], stream=streams[f])

at the same parameters gives the same smoothed_state_est, n_lineages, trajectory_index and trajectories EXACTLY, and the filter
outputs equal bootstrap_filter_batch's bit for bit.  smoothed is also spot-checked against the math.fsum restatement within
N 2^-52 sum |W x| (the bound of any summation order of N fp64 terms)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_restated as SR  # noqa: E402

pytestmark = pytest.mark.gpu

GAPS = [1, 2, 5, 5, 6, 7, 8, 9, 10, 11, 12, 13]     # a gap of 3 and a repeated time
SEEDS = [1405, (1 << 33) + 7, 99, (1 << 40) + 3, 5]
STREAMS = [0, (1 << 35) + 1, 7, 3, 1 << 32]
PARAMS = [{"a": 1.0, "s": 1.0}, {"a": 0.7, "s": 1.3}, {"a": 1.2, "s": 0.8}, {"a": 0.4, "s": 2.0}, {"a": 0.9, "s": 0.6}]
FILTER_FIELDS = ("loglike", "loglike_history", "ess", "state_est", "n_res_calls", "early_return_step", "status")
# the scalar model of tests/test_gpu_smooth.py as linear_gaussian_mv(1, 1): mostly flat weights (carried under SISAR) and two far-out
# observations (resampled)
Y_LG = np.array([0.3, -0.2, 6.0, 0.1, 0.4, -0.5, -6.0, 0.2, 0.0, 0.6, -0.1, 0.3])
SEIR_PARAMS = [dict(beta=0.004, sigma=0.5, gamma=0.3), dict(beta=0.006, sigma=0.4, gamma=0.25), dict(beta=0.003, sigma=0.6, gamma=0.35),
               dict(beta=0.005, sigma=0.5, gamma=0.2), dict(beta=0.004, sigma=0.3, gamma=0.3)]
Y_SEIR = np.array([8, 9, 12, 13, 17, 19, 20, 24, 25, 27, 26, 30], dtype=np.float64)


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 12, 8)
    yield c
    c.close()


def _fns(m):
    return (m.init_fn, m.transition_fn, m.log_likelihood_fn)


def _pieces(d, p, seed=11):
    rng = np.random.default_rng(seed + 10 * d + p)
    return dict(m0=rng.standard_normal(d), L0=np.tril(0.2 * rng.standard_normal((d, d))) + np.eye(d), A=0.6 * np.eye(d) + 0.15 * rng.standard_normal((d, d)),
                b=0.1 * rng.standard_normal(d), L=np.tril(0.3 * rng.standard_normal((d, d))) + 0.7 * np.eye(d),
                H=rng.standard_normal((p, d)), h0=0.2 * rng.standard_normal(p), sd=0.5 + rng.random(p))


def _mv(B, d, p, **kw):
    """general A (scaled by the parameter a), lower-triangular L0 / L, dense H, unequal sd (scaled by s)"""
    q = _pieces(d, p)
    A0, sd0 = q.pop("A"), q.pop("sd")
    if kw.get("obs") == "poisson":                               # eta = h0 + H x stays small; s scales the level instead of an sd
        H0 = 0.2 * q.pop("H")
        return B.models.linear_gaussian_mv(d, p, build=lambda a, s: {"A": a * A0, "H": s * H0}, param_names=("a", "s"), **q, **kw)
    return B.models.linear_gaussian_mv(d, p, build=lambda a, s: {"A": a * A0, "sd": s * sd0}, param_names=("a", "s"), **q, **kw)


def _mv_data(d, p, T, seed=3, counts=False):
    rng = np.random.default_rng(seed + d)
    y = rng.poisson(2.0, (T, p)).astype(np.float64) if counts else rng.standard_normal((T, p))
    if not counts and T >= 8:
        y[2] += 4.0                                              # two far-out rows: a launch holds resampled and carried steps
        y[6] -= 4.0
    return y


def _seir(B, **kw):
    return B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                            ({"I": 1}, {"R": 1}, "gamma")], x0=[180.0, 8.0, 12.0, 0.0], observe=[{"I": 0.6}], **kw)


def _seir_counter(B):
    return B.models.reaction_network(("S", "E", "I", "R", "C"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1, "C": 1}, "sigma"),
                                                                 ({"I": 1}, {"R": 1}, "gamma")], x0=[180.0, 8.0, 12.0, 0.0, 0.0], observe=[{"C": 0.8}],
                                     counters=("C",))


def compare(B, ctx, m, d, y, N, K, params, seeds, streams, restate=False, **kw):
    """one smoothing launch against the plain launch (filter outputs) and against every filter's single-filter smoothing run"""
    T, F = int(np.shape(y)[0]), len(params)
    bat = B.bootstrap_smoother_batch(y, N, *_fns(m), params, seeds, streams, trajectories=K, ctx=ctx, **kw)
    plain = B.bootstrap_filter_batch(y, N, *_fns(m), params, seeds, streams, ctx=ctx, **kw)
    for k in FILTER_FIELDS:
        assert np.array_equal(bat[k], plain[k], equal_nan=True), k
    assert bat["smoothed_state_est"].shape == (F, T + 1, d) and bat["n_lineages"].shape == (F, T + 1)
    assert bat["trajectories"].shape == (F, K, T + 1, d) and bat["_extras"]["trajectory_index"].shape == (F, K)
    assert np.all(bat["traced"] == 1) and np.all(bat["status"] == 0)
    for f in range(F):
        one = B.bootstrap_filter(y, N, *_fns(m), smooth=True, trajectories=K, seed=seeds[f], stream=streams[f], ctx=ctx,
                                 return_particles=restate, return_ancestors=restate, **kw, **params[f])
        assert one["_extras"]["early_return_step"] == 0
        assert np.array_equal(bat["smoothed_state_est"][f], np.asarray(one["smoothed_state_est"]).reshape(T + 1, d)), f
        assert np.array_equal(bat["n_lineages"][f], one["n_lineages"]), f
        assert bat["n_lineages"][f][T] == N
        if K:
            assert np.array_equal(bat["_extras"]["trajectory_u"][f], one["_extras"]["trajectory_u"]), f
            assert np.array_equal(bat["_extras"]["trajectory_index"][f], one["_extras"]["trajectory_index"]), f
            assert np.array_equal(bat["trajectories"][f], one["trajectories"]), f
        if restate:                                               # the spot check against math.fsum on the single run's histories
            ref = SR.smooth(one["particles_history"], one["weights_history"], one["_extras"]["ancestors"], one["_extras"]["call_obs"], d)
            err, bound = np.abs(bat["smoothed_state_est"][f] - ref["smoothed"]), N * 2.0 ** -52 * ref["abs_sum"]
            print("filter %d smoothed: max error %.3e, the bound there %.3e" % (f, err.max(), bound.reshape(-1)[err.argmax()]))
            assert np.all(err <= bound)
            assert np.array_equal(bat["n_lineages"][f], ref["n_lineages"])
    return bat


def _cap(B, d, rnet=False):
    return B.batch_max_particles(d, "rnet") if rnet else B.batch_max_particles(d)


# every N of the list at every (d, p); F, T, K, the resampling rule and the observation clock rotate with the case
MV_CASES = []
for _i, _dp in enumerate([(1, 1), (3, 2), (8, 8)]):
    for _j, _N in enumerate([1, 2, 100, 257, 1000, "cap"]):
        _c = _i + _j
        MV_CASES.append((_dp, _N, [1, 3, 5][_c % 3], [12, 1, 12, 0, 12, 12][_j], [7, 1, 0][_c % 3], ["SISAR", "SISR", "SISAR", "SIS"][(_i + 2 * _j) % 4],
                         ["stratified", "systematic"][_c % 2], _j in (2, 5)))


@pytest.mark.parametrize("dp,N,F,T,K,ra,rf,gaps", MV_CASES)
def test_lgmv_equals_the_single_filter_smoother(B, ctx, dp, N, F, T, K, ra, rf, gaps):
    d, p = dp
    N = _cap(B, d) if N == "cap" else N
    bat = compare(B, ctx, _mv(B, d, p), d, _mv_data(d, p, T), N, K, PARAMS[:F], SEEDS[:F], STREAMS[:F], restate=(N in (2, 257)),
                  resample_algorithm=ra, resample_fn=rf, obs_times=(GAPS[:T] if gaps else None))
    if ra == "SIS":
        assert np.all(bat["n_res_calls"] == 0) and np.all(bat["n_lineages"] == N)


@pytest.mark.parametrize("dp", [(1, 1), (3, 2), (8, 8)])
def test_lgmv_poisson_missing_and_per_draw_sets(B, ctx, dp):
    d, p = dp
    T, N, F = 12, 257, 3
    # Poisson counts
    compare(B, ctx, _mv(B, d, p, obs="poisson"), d, _mv_data(d, p, T, counts=True), N, 7, PARAMS[:F], SEEDS[:F], STREAMS[:F], resample_algorithm="SISAR",
            resample_fn="systematic")
    # missing="skip": a row of all NaN and, where there is more than one component, a row with one
    y = _mv_data(d, p, T)
    y[4] = np.nan
    if p > 1:
        y[7, 0] = np.nan
    compare(B, ctx, _mv(B, d, p, missing="skip"), d, y, N, 1, PARAMS[:F], SEEDS[:F], STREAMS[:F], resample_algorithm="SISAR", resample_fn="stratified")
    # time-varying b and h0 that depend on the draw: one array set per filter
    rng = np.random.default_rng(40 + d)
    U, S = 0.3 * rng.standard_normal((T, d)), 0.3 * rng.standard_normal((T, p))
    q = _pieces(d, p)
    m = B.models.linear_gaussian_mv(d, p, build=lambda a, s: {"time_varying": {"b": a * U, "h0": s * S}}, param_names=("a", "s"), **q)
    compare(B, ctx, m, d, _mv_data(d, p, T), N, 7, PARAMS[:F], SEEDS[:F], STREAMS[:F], resample_algorithm="SISR", resample_fn="systematic")


def test_sis_sisr_sisar_on_carried_and_resampled_steps(B, ctx):
    T, N = 12, 100
    m = B.models.linear_gaussian_mv(1, 1, build=lambda a, s: {"A": [[0.8 * a]], "sd": [2.0 * s]}, param_names=("a", "s"), m0=[0.0], L0=[[1.0]],
                                    b=[0.0], L=[[0.5]], H=[[1.0]], h0=[0.0])
    par = [{"a": 1.0, "s": 1.0}, {"a": 0.9, "s": 1.1}, {"a": 1.1, "s": 0.9}]
    sis = compare(B, ctx, m, 1, Y_LG, N, 7, par, SEEDS[:3], STREAMS[:3], resample_algorithm="SIS")
    assert np.all(sis["n_res_calls"] == 0) and np.all(sis["n_lineages"] == N)
    sisr = compare(B, ctx, m, 1, Y_LG, N, 7, par, SEEDS[:3], STREAMS[:3], resample_algorithm="SISR", resample_fn="systematic")
    assert np.all(sisr["n_res_calls"] == T)
    sisar = compare(B, ctx, m, 1, Y_LG, N, 7, par, SEEDS[:3], STREAMS[:3], restate=True, resample_algorithm="SISAR", resample_fn="stratified")
    print("SISAR resample calls per filter", sisar["n_res_calls"])
    assert np.all(sisar["n_res_calls"] > 0) and np.all(sisar["n_res_calls"] < T)          # the launch holds carried and resampled steps
    compare(B, ctx, m, 1, Y_LG, N, 1, par, SEEDS[:3], STREAMS[:3], resample_algorithm="SISAR", resample_fn="systematic", obs_times=GAPS)


RN_CASES = [("gillespie", 100, 5, 12, 7, "SISAR", False), ("gillespie", "cap", 3, 12, 1, "SISR", True), ("gillespie", 1, 1, 1, 1, "SISR", False),
            ("gillespie", 2, 3, 0, 0, "SISAR", False), ("em_noise", 257, 3, 12, 7, "SISAR", True), ("em_noise", 1000, 1, 12, 0, "SISR", False),
            ("counter", 257, 5, 12, 1, "SISAR", False), ("counter", 1000, 3, 1, 7, "SIS", False)]


@pytest.mark.parametrize("net,N,F,T,K,ra,gaps", RN_CASES)
def test_rnet_equals_the_single_filter_smoother(B, ctx, net, N, F, T, K, ra, gaps):
    par = SEIR_PARAMS[:F]
    if net == "em_noise":
        m = _seir(B, method="euler_multinomial", leaps=4, noise={"beta": "sigma_se"})
        par = [dict(q, sigma_se=0.1 + 0.05 * k) for k, q in enumerate(par)]
    else:
        m = _seir_counter(B) if net == "counter" else _seir(B)
    d = 5 if net == "counter" else 4
    N = _cap(B, d, True) if N == "cap" else N
    compare(B, ctx, m, d, Y_SEIR[:T], N, K, par, SEEDS[:F], STREAMS[:F], restate=(N == 257), resample_algorithm=ra,
            resample_fn="systematic" if gaps else "stratified", obs_times=(GAPS[:T] if gaps else None))


def test_early_return_is_not_traced_and_leaves_the_neighbours_alone(B, ctx):
    """filter 1 of the launch has all(log_weights < -1e8) at observation 4 (y = 1e6 against sd = 2); its neighbours' sd is 1000 times
    that and they run to the end"""
    m = B.models.linear_gaussian_mv(1, 1, build=lambda a, s: {"A": [[0.8 * a]], "sd": [2.0 * s]}, param_names=("a", "s"), m0=[0.0], L0=[[1.0]],
                                    b=[0.0], L=[[0.5]], H=[[1.0]], h0=[0.0])
    y = np.array([0.3, -0.2, 0.1, 1e6, 0.4])
    par = [{"a": 1.0, "s": 1000.0}, {"a": 1.0, "s": 1.0}, {"a": 0.9, "s": 2000.0}]
    T, N, K = 5, 100, 3
    bat = B.bootstrap_smoother_batch(y, N, *_fns(m), par, SEEDS[:3], STREAMS[:3], trajectories=K, ctx=ctx)
    plain = B.bootstrap_filter_batch(y, N, *_fns(m), par, SEEDS[:3], STREAMS[:3], ctx=ctx)
    for k in FILTER_FIELDS:
        assert np.array_equal(bat[k], plain[k], equal_nan=True), k
    assert list(bat["early_return_step"]) == [0, 4, 0] and list(bat["traced"]) == [1, 0, 1]
    assert np.all(np.isnan(bat["smoothed_state_est"][1])) and np.all(np.isnan(bat["trajectories"][1])) and np.all(bat["n_lineages"][1] == 0)
    assert np.all(np.isnan(bat["_extras"]["trajectory_u"][1])) and np.all(bat["_extras"]["trajectory_index"][1] == 0)
    for f in (0, 2):
        one = B.bootstrap_filter(y, N, *_fns(m), trajectories=K, seed=SEEDS[f], stream=STREAMS[f], ctx=ctx, return_particles=False, **par[f])
        assert np.array_equal(bat["smoothed_state_est"][f][:, 0], one["smoothed_state_est"]) and np.array_equal(bat["n_lineages"][f], one["n_lineages"])
        assert np.array_equal(bat["trajectories"][f], one["trajectories"])
        assert np.array_equal(bat["_extras"]["trajectory_index"][f], one["_extras"]["trajectory_index"])


def test_results_do_not_depend_on_the_composition_of_the_batch(B, ctx):
    d, p, T, N, K = 3, 2, 12, 257, 7
    m, y = _mv(B, d, p), _mv_data(d, p, T)
    kw = dict(trajectories=K, ctx=ctx, resample_algorithm="SISAR", resample_fn="systematic")
    among = B.bootstrap_smoother_batch(y, N, *_fns(m), PARAMS, SEEDS, STREAMS, **kw)
    alone = B.bootstrap_smoother_batch(y, N, *_fns(m), [PARAMS[3]], [SEEDS[3]], [STREAMS[3]], **kw)
    other = B.bootstrap_smoother_batch(y, N, *_fns(m), [PARAMS[3], PARAMS[0]], [SEEDS[3], SEEDS[0]], [STREAMS[3], STREAMS[0]], **kw)
    for k in ("smoothed_state_est", "n_lineages", "trajectories", "loglike", "state_est"):
        assert np.array_equal(among[k][3], alone[k][0]) and np.array_equal(among[k][3], other[k][0]), k
        assert np.array_equal(among[k][0], other[k][1]), k
    for k in ("trajectory_u", "trajectory_index"):
        assert np.array_equal(among["_extras"][k][3], alone["_extras"][k][0]), k


def test_one_launch_of_32_filters_meets_the_exact_smoothed_means(B, ctx):
    """SR.EXACT's model, data and 32 (seed, stream) pairs at N = 1024, ONE launch: within 5 standard errors (from the 32 replicates) of the
    Rauch-Tung-Striebel means at every t"""
    q = SR.EXACT
    m = B.models.linear_gaussian_mv(1, 1, m0=[0.0], L0=[[1.0]], A=[[q["phi"]]], b=[0.0], L=[[q["sigma_x"]]], H=[[1.0]], h0=[0.0], sd=[q["sigma_y"]])
    seeds, streams = [s for s, _ in SR.EXACT_SEEDS], [k for _, k in SR.EXACT_SEEDS]
    bat = B.bootstrap_smoother_batch(SR.EXACT_Y, 1024, *_fns(m), [{}] * 32, seeds, streams, ctx=ctx, resample_algorithm="SISR", resample_fn="stratified")
    assert np.all(bat["traced"] == 1) and bat["_extras"]["smooth_ms"] > 0
    ok, z = SR.within_5_se(bat["smoothed_state_est"][:, :, 0], SR.exact_means())
    print("exact", SR.exact_means(), "mean", bat["smoothed_state_est"][:, :, 0].mean(axis=0), "z", z)
    assert ok.all(), z


def test_c_abi(B, ctx):
    from bayesssm_amd import _lib
    lib = _lib.load()
    d, p, T, N, K, F = 3, 2, 12, 100, 7, 3
    m, y = _mv(B, d, p), np.ascontiguousarray(_mv_data(d, p, T))
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    thetas = np.ascontiguousarray(np.array([m.pack(q) for q in PARAMS[:F]]))
    seeds, streams = np.array(SEEDS[:F], dtype=np.uint64), np.array(STREAMS[:F], dtype=np.uint64)

    def call(model, alg, rf, N_, T_, y_, F_, th, K_, sres=True):
        ll, se, ess, llh = np.zeros(F), np.zeros((F, T + 1, d)), np.zeros((F, T + 1)), np.zeros((F, T))
        ers, nres, status, ms = np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(1)
        sm, nl, tr = np.zeros((F, T + 1, d)), np.zeros((F, T + 1), dtype=np.int32), np.zeros((F, K, T + 1, d))
        u, idx, traced, sms = np.zeros((F, K)), np.zeros((F, K), dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(1)
        cfg = _lib.PfConfig(model, _lib.ALGORITHM[alg], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN[rf], N_, T_, float("nan"), None,
                            int(th.shape[1]), p_(y_), None, 0, 0, None, None, None, 0, 0, 0.0, None, None)
        res = _lib.PfBatchResult(p_(ll), p_(se), p_(ess), p_(llh), p_(ers), p_(nres), p_(status), p_(ms))
        keep = (_lib.SmoothConfig(K_), _lib.SmoothBatchResult(p_(sm), p_(nl), p_(tr), p_(u), p_(idx), p_(traced), p_(sms)))
        st = lib.bssm_pf_run_batch_smooth(ctx.handle, C.byref(cfg), F_, p_(th), p_(seeds if F_ == F else np.zeros(F_, dtype=np.uint64)),
                                          p_(streams if F_ == F else np.arange(F_, dtype=np.uint64)), None, C.byref(res),
                                          C.cast(C.pointer(keep[0]), C.c_void_p), C.cast(C.pointer(keep[1]), C.c_void_p) if sres else None)
        return st, dict(loglike=ll, state_est=se, smoothed_state_est=sm, n_lineages=nl, trajectories=tr, trajectory_u=u, trajectory_index=idx,
                        traced=traced, smooth_ms=sms)

    mv_id = _lib.MV_OBS_MODEL["gaussian"]
    st, _ = call(mv_id, "BPF", "stratified", N, T, y, F, thetas, K, sres=False)
    assert st == _lib.ERR_ARG and b"bssm_pf_run_batch_smooth" in lib.bssm_last_error()
    assert call(mv_id, "BPF", "stratified", N, T, y, F, thetas, 4097)[0] == _lib.ERR_ARG
    covers = b"covers the bootstrap filter of the multivariate linear-Gaussian family"
    assert call(_lib.MODEL["lg"], "BPF", "stratified", N, T, y, F, thetas, K)[0] == _lib.ERR_ARG and covers in lib.bssm_last_error()
    assert call(mv_id, "APF", "stratified", N, T, y, F, thetas, K)[0] == _lib.ERR_ARG and covers in lib.bssm_last_error()
    assert call(mv_id, "BPF", "multinomial", N, T, y, F, thetas, K)[0] == _lib.ERR_ARG and covers in lib.bssm_last_error()
    # histories that cannot fit: 1024 filters x 20001 rows x 3 x 2048 doubles = 1 PB, settled by arithmetic before anything is staged
    Fb, Tb = 1024, 20000
    st, _ = call(mv_id, "BPF", "stratified", B.batch_max_particles(d), Tb, np.zeros((Tb, p)), Fb, np.ascontiguousarray(np.tile(thetas[0], (Fb, 1))), 0)
    msg = lib.bssm_last_error().decode()
    assert st == _lib.ERR_CAPACITY and "bssm_pf_run_batch_smooth" in msg and "bytes of device memory" in msg, msg
    need = Fb * ((Tb + 1) * d * B.batch_max_particles(d) * 8 + Tb * (B.batch_max_particles(d) + 1) * 4 + B.batch_max_particles(d) * 8)
    assert int(msg.split(" need ")[1].split(" bytes")[0]) >= need
    st, got = call(mv_id, "BPF", "stratified", N, T, y, F, thetas, K)
    _lib.check(st)
    py = B.bootstrap_smoother_batch(y, N, *_fns(m), PARAMS[:F], SEEDS[:F], STREAMS[:F], trajectories=K, ctx=ctx, resample_algorithm="SISAR",
                                    resample_fn="stratified")
    for k in ("loglike", "state_est", "smoothed_state_est", "n_lineages", "trajectories", "traced"):
        assert np.array_equal(got[k], py[k]), k
    for k in ("trajectory_u", "trajectory_index"):
        assert np.array_equal(got[k], py["_extras"][k]), k
    assert got["smooth_ms"][0] > 0 and np.all(got["traced"] == 1)
