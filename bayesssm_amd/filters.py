"""bootstrap_filter / auxiliary_filter: Python mirror of R/bootstrap_filter.R:129-171,
R/auxiliary_filter.R:163-216 and .particle_filter_core (R/particle_filter_core.R:19-267),
executed on the GPU by bssm_pf_run."""
import contextlib
import ctypes as C

import numpy as np

from . import _lib, models

_RESAMPLE_ALGORITHMS = ("SISAR", "SISR", "SIS")
_RESAMPLE_FNS = ("stratified", "systematic", "multinomial")


def _match_arg(value, choices, name):
    if value is None:
        return choices[0]
    if value not in choices:
        raise ValueError("'%s' should be one of %s" % (name, ", ".join('"%s"' % c for c in choices)))   # match.arg
    return value


_MAX_TRAJECTORIES = 4096


def _refuse_smooth(kwargs, who):
    """smooth= / trajectories= (the genealogy smoother) where it does not run: one ValueError; keywords that ask for nothing are dropped"""
    if kwargs.get("smooth") or kwargs.get("trajectories"):
        raise ValueError("%s: smooth= / trajectories= (the genealogy smoother) run on the single-filter device path only -- bootstrap_filter, "
                         "auxiliary_filter and resample_move_filter on a built-in model with the device generator or injected draws" % who)
    kwargs.pop("smooth", None)
    kwargs.pop("trajectories", None)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _mv_tv_struct(tv):
    """bssm_mv_tv for (n_times, b_t, h0_t, H_t) (LinearGaussianMV.tv_arrays); the caller keeps the struct alive over the call"""
    if tv is None:
        return None
    n_times, b, h0, H = tv
    return _lib.MvTv(int(n_times), _ptr(b), _ptr(h0), _ptr(H))


def noise_shape(algorithm, T, obs_times=None):
    ot = np.ascontiguousarray(obs_times, dtype=np.int32) if obs_times is not None else None
    mt, mr = C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().bssm_pf_noise_shape(_lib.ALGORITHM[algorithm], int(T), _ptr(ot), C.byref(mt), C.byref(mr)))
    return mt.value, mr.value


def particle_filter_core(y, num_particles, model, theta, algorithm="BPF", obs_times=None,
                         resample_algorithm="SISAR", resample_fn="stratified", threshold=None,
                         return_particles=True, return_ancestors=False, seed=0, stream=0, draws=None, ctx=None,
                         move_sd=0.0, mv_owner=None, mv_params=None, rn_owner=None, smooth=False, trajectories=0):
    """.particle_filter_core on the device.  `draws` (parity mode) = dict(z_init, z_trans, u_res)
    of injected random draws; otherwise the device generator keyed by (seed, stream) is used.
    mv_owner: the multivariate family's descriptor, for its time-varying pieces (models.LinearGaussianMV.tv_arrays);
    mv_params: the parameter draw, for the arrays of a descriptor whose `build` returns them (has_param_tv).
    rn_owner: a reaction network's descriptor (models.ReactionNetwork; model == "rnet"), for its dimensions and its checks of y.
    smooth / trajectories: the genealogy smoother on the device (bssm_pf_run_smooth) -- smoothed_state_est [T+1(, d)],
    n_lineages [T+1] and, for trajectories = K > 0 (which implies the trace), trajectories [K, T+1, d]; the histories stay on the
    device unless return_particles / return_ancestors ask for them as well."""
    if not (isinstance(trajectories, (int, np.integer)) and not isinstance(trajectories, bool) and 0 <= trajectories <= _MAX_TRAJECTORIES):
        raise ValueError("trajectories must be an integer in 0 .. %d" % _MAX_TRAJECTORIES)
    n_traj = int(trajectories)
    smooth = bool(smooth) or n_traj > 0
    if not (isinstance(num_particles, (int, np.integer)) and num_particles > 0):
        raise ValueError("Assertion on 'num_particles' failed: Must be a positive count")      # assert_count :33
    y = np.ascontiguousarray(y, dtype=np.float64)
    mv = (model == "lgmv")
    if mv:                                                 # y: a vector (one column, :70) or a T x p matrix
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        mv_d, mv_p = int(theta[0]), int(theta[1])
        if y.ndim == 1:
            y = y.reshape(-1, 1)
        if y.ndim != 2 or (mv_p > 0 and y.shape[1] != mv_p):
            raise ValueError("y must be a vector or a T x %d matrix for this model" % mv_p)
        if mv_p == 0:
            y = np.zeros((y.shape[0], 0))
        if mv_owner is not None:
            mv_owner.check_y(y)                            # (the observation family's own demands, before any context exists)
    elif model == "rnet":                                  # reaction networks: y a vector (p = 1) or a T x p matrix of counts
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        y = _rn_y(rn_owner, y)
    elif y.ndim != 1:
        raise ValueError("this build supports scalar observations (y a vector) for the scalar models")
    y_owner = mv_owner if mv else rn_owner if model == "rnet" else None
    skip = y_owner is not None and y_owner.missing == "skip"               # NaN in y: a component that was not observed
    if not (y_owner.y_ok(y) if skip else np.all(np.isfinite(y))):
        raise ValueError("Assertion on 'y' failed: Contains missing values")                    # assert_numeric :69
    T = int(y.shape[0])
    N = int(num_particles)
    ot = None
    if obs_times is not None:
        ot = np.ascontiguousarray(obs_times, dtype=np.int32)
        if ot.size != T or (T and (ot[0] < 1 or np.any(np.diff(ot) < 0))):
            raise ValueError("Assertion on 'obs_times' failed")                                  # assert_integerish :73
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    dim = mv_d if mv else rn_owner.dim if model == "rnet" else models.dim_of(model)
    tvs = None
    if mv and mv_owner is not None:                        # (checked against T and obs_times)
        tvs = _mv_tv_struct(mv_owner.tv_arrays(T, ot, mv_params) if (mv_params is not None and mv_owner.has_param_tv)
                            else mv_owner.tv_arrays(T, ot))
    ctx = ctx.require(N, dim) if ctx is not None else _lib.default_context(N, dim=dim)
    max_trans, max_res = noise_shape(algorithm, T, ot)
    state_est = np.zeros((T + 1, dim)) if dim > 1 else np.zeros(T + 1)
    ess = np.zeros(T + 1)
    llh = np.zeros(max(T, 1))
    ll = np.zeros(1)
    ers = np.zeros(1, dtype=np.int32)
    nres = np.zeros(1, dtype=np.int32)
    resampled = np.zeros(max(T, 1), dtype=np.int32)
    anc = np.zeros((max(max_res, 1), N), dtype=np.int32) if return_ancestors else None
    ph = np.zeros((T + 1, N * dim)) if return_particles else None
    wh = np.zeros((T + 1, N)) if return_particles else None
    ms = np.zeros(1)
    scan_stats = np.zeros(3, dtype=np.int64)
    zi = zt = ur = None
    if draws is not None:
        ur = np.ascontiguousarray(draws["u_res"], dtype=np.float64)
        assert ur.size >= max_res * (1 if resample_fn == "systematic" else N)
        if model not in ("sir", "rnet"):       # SIR / reaction networks draw a data-dependent number of variates: always the device generator
            zi = np.ascontiguousarray(draws["z_init"], dtype=np.float64)
            zt = np.ascontiguousarray(draws["z_trans"], dtype=np.float64)
            assert zi.size >= N * (dim if mv else 1) and zt.size >= max_trans * N * (dim if mv else 1)       # (lgmv: [d][N] per call, component-major)
    zmv = umv = None
    if draws is not None and algorithm == "RMPF":
        zmv = np.ascontiguousarray(draws["z_move"], dtype=np.float64)
        umv = np.ascontiguousarray(draws["u_move"], dtype=np.float64)
        assert zmv.size >= T * N * (dim if mv else 1) and umv.size >= T * N       # (lgmv: z_move [T][d][N], component-major)
    model_id = _lib.MV_OBS_MODEL[mv_owner.obs] if (mv and mv_owner is not None) else _lib.RN_OBS_MODEL[rn_owner.obs] if model == "rnet" else _lib.MODEL[model]
    cfg = _lib.PfConfig(model_id, _lib.ALGORITHM[algorithm], _lib.RESAMPLE_ALGORITHM[resample_algorithm],
                        _lib.RESAMPLE_FN[resample_fn], N, T, float("nan") if threshold is None else float(threshold),
                        _ptr(theta), int(theta.size), _ptr(y), _ptr(ot), int(seed), int(stream),
                        _ptr(zi), _ptr(zt), _ptr(ur), 1 if return_particles else 0, 1 if return_ancestors else 0,
                        float(move_sd), _ptr(zmv), _ptr(umv), C.cast(C.pointer(tvs), C.c_void_p) if tvs is not None else None)
    res = _lib.PfResult(_ptr(state_est), _ptr(ess), _ptr(llh), _ptr(ll), _ptr(ers), _ptr(nres), _ptr(resampled),
                        _ptr(anc), _ptr(ph), _ptr(wh), _ptr(ms), _ptr(scan_stats))
    with contextlib.ExitStack() as scope:
        scope.enter_context(ctx.mv_y_missing(skip))
        if model == "rnet":                                   # (K leaps per unit of time, or 0: Gillespie's direct method)
            scope.enter_context(ctx.rn_method(rn_owner.rn_method, rn_owner.rn_leaps))
        if smooth:
            sm_se = np.zeros((T + 1, dim)) if dim > 1 else np.zeros(T + 1)
            sm_nlin = np.zeros(T + 1, dtype=np.int32)
            sm_traj = np.zeros((n_traj, T + 1, dim)) if n_traj else None
            sm_u = np.zeros(n_traj) if n_traj else None
            sm_idx = np.zeros(n_traj, dtype=np.int32) if n_traj else None
            sm_call_obs = np.zeros(max(max_res, 1), dtype=np.int32)
            sm_ms = np.zeros(1)
            scfg = _lib.SmoothConfig(n_traj)
            sres = _lib.SmoothResult(_ptr(sm_se), _ptr(sm_nlin), _ptr(sm_traj), _ptr(sm_u), _ptr(sm_idx), _ptr(sm_call_obs), _ptr(sm_ms))
            st = _lib.load().bssm_pf_run_smooth(ctx.handle, C.byref(cfg), C.byref(res), C.byref(scfg), C.byref(sres))
        else:
            st = _lib.load().bssm_pf_run(ctx.handle, C.byref(cfg), C.byref(res))
    if st in (_lib.ERR_NEGATIVE, _lib.ERR_ZERO_SUM):
        raise ValueError(_lib.load().bssm_status_string(st).decode())
    _lib.check(st)
    out = {"state_est": state_est, "ess": ess, "loglike": float(ll[0]), "loglike_history": llh[:T],
           "algorithm": algorithm}
    early = int(ers[0])
    if early == 0:
        out["resample_algorithm"] = "SISR" if algorithm == "RMPF" else resample_algorithm   # absent on the early return (:192-196)
    if return_particles:
        rows = early if early else T + 1                      # histories end where the reference returned
        out["particles_history"] = ph[:rows]
        out["weights_history"] = wh[:rows]
    # extras (not in the reference's list): diagnostics for tests and benches
    out["_extras"] = {"device_ms": float(ms[0]), "n_res_calls": int(nres[0]), "early_return_step": early,
                      "resampled": resampled[:T], "scan_stats": scan_stats}
    if return_ancestors:
        out["_extras"]["ancestors"] = anc[: int(nres[0])]
    if smooth:                                                # a run that returned early is not traced
        traced = early == 0
        out["smoothed_state_est"] = sm_se if traced else None
        out["n_lineages"] = sm_nlin if traced else None
        if n_traj:
            out["trajectories"] = sm_traj if traced else None
            out["_extras"]["trajectory_u"] = sm_u if traced else None
            out["_extras"]["trajectory_index"] = sm_idx if traced else None
        out["_extras"]["call_obs"] = sm_call_obs[: int(nres[0])]
        out["_extras"]["smooth_ms"] = float(sm_ms[0])
    return out


def batch_max_particles(d=1, model=None):
    """Largest num_particles of a batched filter (one workgroup per filter) with d state components: the scalar models
    (d = 1, and the SIR model) and the multivariate family (models.linear_gaussian_mv, d <= 8).  0 for d outside 1..8.
    model="rnet": a reaction network (models.reaction_network) with d species."""
    lib = _lib.load()
    if model == "rnet":
        return int(lib.bssm_pf_batch_max_particles_rn(int(d)))
    return int(lib.bssm_pf_batch_max_particles()) if d == 1 else int(lib.bssm_pf_batch_max_particles_mv(int(d)))


def _rn_y(owner, y):
    """y of a reaction network as a T x p matrix of counts, checked on the host"""
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    if y.ndim != 2 or y.shape[1] != owner.p:
        raise ValueError("y must be a vector or a T x %d matrix for this model" % owner.p)
    owner.check_y(y)
    return np.ascontiguousarray(y)


def _rn_batch_args(owner, y, thetas):
    """y as a T x p matrix and thetas as an (F, n_theta) array of packed blocks for bootstrap_filter_batch on a reaction network;
    thetas is a list of parameter dicts (each packed by the descriptor) or an array of packed blocks."""
    y = _rn_y(owner, np.ascontiguousarray(y, dtype=np.float64))
    if isinstance(thetas, dict):
        raise ValueError("thetas must be a list of parameter dicts or an (n_filters, n_theta) array of packed blocks")
    if isinstance(thetas, (list, tuple)) and len(thetas) and all(isinstance(q, dict) for q in thetas):
        thetas = owner.pack_many(thetas)                               # (refuses draws whose blocks differ in length)
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    d, R, p = owner.dim, owner.R, owner.p
    # d, R, p, x0, k, s1, s2, nu, G [, size] [, reset [, n_times, M]]: the descriptor knows its length (with a schedule from `build`, after a first pack)
    if thetas.ndim != 2 or thetas.shape[0] < 1 or not owner.n_theta_ok(int(thetas.shape[1])):
        n_theta = owner.n_theta() or (owner._base_size() + (d if owner.counters else 0))
        raise ValueError("thetas must be a list of parameter dicts or an (n_filters, %d) array of packed blocks" % n_theta)
    if not (np.all(thetas[:, 0] == d) and np.all(thetas[:, 1] == R) and np.all(thetas[:, 2] == p)):
        raise ValueError("thetas: every packed block must have the descriptor's (d, R, p) = (%d, %d, %d)" % (d, R, p))
    return y, thetas


def _mv_batch_args(owner, y, thetas):
    """y as a T x p matrix and thetas as an (F, n_theta) array of packed blocks for bootstrap_filter_batch on the multivariate
    family; thetas is a list of parameter dicts (each packed by the descriptor) or an array of packed blocks."""
    d, p = owner.dim, owner.p
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    if y.ndim != 2 or (p > 0 and y.shape[1] != p):
        raise ValueError("y must be a vector or a T x %d matrix for this model" % p)
    if p == 0:
        y = np.zeros((y.shape[0], 0))
    owner.check_y(y)
    if not owner.y_ok(y):                                         # (missing="skip": NaN passes, +-inf does not)
        raise ValueError("Assertion on 'y' failed: Contains missing values")
    if isinstance(thetas, dict):
        raise ValueError("thetas must be a list of parameter dicts or an (n_filters, n_theta) array of packed blocks")
    draws = None
    if isinstance(thetas, (list, tuple)) and len(thetas) and all(isinstance(q, dict) for q in thetas):
        draws = list(thetas)
        thetas = [owner.pack(q) for q in thetas]
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    n_theta = 2 + d + 3 * d * d + d + 1 + p * d + 2 * p          # d, p, m0, L0, A, b, L, c0, H, h0, sd
    if thetas.ndim != 2 or thetas.shape[0] < 1 or thetas.shape[1] != n_theta:
        raise ValueError("thetas must be a list of parameter dicts or an (n_filters, %d) array of packed blocks" % n_theta)
    if not (np.all(thetas[:, 0] == d) and np.all(thetas[:, 1] == p)):
        raise ValueError("thetas: every packed block must have the descriptor's (d, p) = (%d, %d)" % (d, p))
    return y, thetas, draws


_TV_NAMES = ("b", "h0", "H")


def _mv_batch_tv(owner, F, T, ot, draws, time_varying, tv_set):
    """The time-varying array sets of bootstrap_filter_batch on the multivariate family: None (the descriptor's own arrays,
    shared by the filters: bssm_pf_run_batch) or (n_times, n_sets, set_of or None, {name: (array, stride in doubles)}) for
    bssm_pf_run_batch_tv.  Every set is checked as a single filter's arrays are (models.LinearGaussianMV.tv_checked)."""
    if time_varying is None:
        if tv_set is not None:
            raise ValueError("tv_set is given without time_varying")
        if not owner.has_param_tv:
            return None
        if draws is None:
            raise ValueError("thetas holds packed blocks and the model's time-varying pieces depend on the parameters: "
                             "pass time_varying= (the arrays of every filter) or a list of parameter dicts")
        keys, set_of = {}, []                                 # equal draws share a set
        for q in draws:
            set_of.append(keys.setdefault(tuple(float(q[k]) for k in owner.param_order), len(keys)))
        firsts = [set_of.index(g) for g in range(len(keys))]
        sets = [owner.tv_arrays(T, ot, draws[k]) for k in firsts]
    else:
        if not isinstance(time_varying, dict):
            raise TypeError("linear_gaussian_mv: time_varying must be a dict with keys among 'b', 'h0', 'H'")
        shared, per_set, G = {}, {}, None
        full = {"b": 2, "h0": 2, "H": 3}                      # dimensions of the documented shapes
        for k, v in time_varying.items():
            if v is None:
                continue
            a = np.asarray(v, dtype=np.float64)
            if k not in full or a.ndim != full[k] + 1:        # one array for all filters (the check names whatever is wrong with it)
                shared.update(owner._check_time_varying({k: a}) or {})
                continue
            per_set[k] = [owner._check_time_varying({k: a[g]})[k] for g in range(a.shape[0])]      # a leading set axis [G, ...]
            if not per_set[k]:
                raise ValueError("time_varying[%r]: the set axis is empty" % k)
            if G is not None and G != len(per_set[k]):
                raise ValueError("time_varying: the arrays with a leading set axis must agree on the number of sets (%d and %d)"
                                 % (G, len(per_set[k])))
            G = len(per_set[k])
        if G is None:
            G = 1
            if tv_set is not None and np.any(np.asarray(tv_set) != 0):
                raise ValueError("tv_set: the arrays have no set axis, every entry must be 0")
        if tv_set is None:
            if G not in (1, F):
                raise ValueError("time_varying: a leading set axis must hold one set per filter (%d) unless tv_set is given, got %d" % (F, G))
            set_of = list(range(F)) if G == F else [0] * F
        else:
            set_of = np.asarray(tv_set)
            if set_of.shape != (F,) or not np.issubdtype(set_of.dtype, np.integer):
                raise ValueError("tv_set must hold one integer set index per filter (%d)" % F)
            if np.any(set_of < 0) or np.any(set_of >= G):
                raise ValueError("tv_set: set indices must lie in [0, %d)" % G)
            set_of = [int(v) for v in set_of]
        base = dict(owner.time_varying or {}, **shared)
        sets = [owner.tv_checked(dict(base, **{k: per_set[k][g] for k in per_set}), T, ot) for g in range(G)]
    if sets[0] is None:
        return None
    if len({s[0] for s in sets}) != 1:
        raise ValueError("time_varying['b']: every set must have the same number of rows (n_times)")
    pieces = {}
    for j, k in enumerate(_TV_NAMES, start=1):
        arrs = [s[j] for s in sets]
        if arrs[0] is None:
            continue
        if all(a is arrs[0] for a in arrs):                   # one array for every filter
            pieces[k] = (arrs[0], 0)
        else:
            pieces[k] = (np.ascontiguousarray(np.stack(arrs)), int(arrs[0].size))
    one_each = len(sets) == F and set_of == list(range(F))
    return sets[0][0], len(sets), (None if (one_each or len(sets) == 1) else np.ascontiguousarray(set_of, dtype=np.int32)), pieces


def auxiliary_filter_batch(y, num_particles, init_fn, transition_fn, log_likelihood_fn, aux_log_likelihood_fn, thetas,
                           seeds=0, streams=None, **kw):
    """bootstrap_filter_batch for auxiliary_filter (R/auxiliary_filter.R:163-216): filter k equals
    auxiliary_filter(..., seed=seeds[k], stream=streams[k], return_particles=False) bit for bit."""
    models.resolve(init_fn, transition_fn, log_likelihood_fn, aux_log_likelihood_fn)
    return bootstrap_filter_batch(y, num_particles, init_fn, transition_fn, log_likelihood_fn, thetas, seeds, streams,
                                  _algorithm="APF", **kw)


def resample_move_filter_batch(y, num_particles, init_fn, transition_fn, log_likelihood_fn, move_fn, thetas,
                               seeds=0, streams=None, **kw):
    """bootstrap_filter_batch for resample_move_filter (R/resample_move_filter.R:190-236) with the built-in random-walk
    Metropolis move: filter k equals resample_move_filter(..., seed=seeds[k], stream=streams[k]) bit for bit."""
    if not isinstance(move_fn, models.MoveFn):
        raise TypeError("move_fn must be the built-in move descriptor (models.<model>.rw_move_fn(sd))")
    return bootstrap_filter_batch(y, num_particles, init_fn, transition_fn, log_likelihood_fn, thetas, seeds, streams,
                                  _algorithm="RMPF", _move_sd=move_fn.sd, **kw)


def bootstrap_filter_batch(y, num_particles, init_fn, transition_fn, log_likelihood_fn, thetas, seeds=0, streams=None,
                           obs_times=None, resample_algorithm=None, resample_fn=None, threshold=None, ctx=None,
                           _algorithm="BPF", _move_sd=0.0, time_varying=None, tv_set=None, smooth=False, trajectories=0, _smooth_k=None):
    """Many independent bootstrap filters in ONE kernel launch (one workgroup per filter, the whole T loop on chip):
    filter k runs with thetas[k] = (phi, sigma_x, sigma_y), seeds[k], streams[k] on the shared data `y`.  Each filter
    returns exactly what bootstrap_filter(..., seed=seeds[k], stream=streams[k], return_particles=False) returns.
    This is the shape of the reference's small-N workloads: the pilot's repeated runs (R/pmmh_tuning.R:111-151) and
    PMMH chains advancing in lock-step (R/pmmh.R:445-457).  num_particles <= batch_max_particles().
    The multivariate family (models.linear_gaussian_mv): thetas is a list of parameter dicts (packed by the descriptor) or
    an (F, n_theta) array of packed blocks, y a vector or a T x p matrix, state_est [F, T+1, d];
    num_particles <= batch_max_particles(d).  The descriptor's time-varying pieces are shared by the filters, as y is.
    Time-varying pieces that differ between the filters (the multivariate family only):  time_varying = {"b": ..., "h0": ...,
    "H": ...}, each array in the descriptor's shape or shorthand (one array for all filters) or in the full shape with a
    leading set axis, [G, n_times, d] / [G, T, p] / [G, T, p, d];  tv_set [F] names each filter's set (default: filter k uses
    set k, G == F).  The arrays replace the descriptor's for this call.  When the descriptor's `build` returns such arrays (has_param_tv) and thetas is a list of
    parameter dicts, the sets are assembled from the draws, equal dicts sharing one; with packed blocks time_varying= is required.
    Returns a dict of arrays: loglike [F], state_est [F, T+1], ess [F, T+1], loglike_history [F, T],
    early_return_step [F], n_res_calls [F], status [F] (0 = ok) and device_ms.
    smooth / trajectories are refused here: the batched smoother is a function of its own, bootstrap_smoother_batch (which
    passes _smooth_k, its number of trajectories)."""
    _refuse_smooth({"smooth": smooth, "trajectories": trajectories}, "bootstrap_filter_batch")
    resample_algorithm = _match_arg(resample_algorithm, _RESAMPLE_ALGORITHMS, "resample_algorithm")
    resample_fn = _match_arg(resample_fn, _RESAMPLE_FNS, "resample_fn")
    if not (isinstance(num_particles, (int, np.integer)) and num_particles > 0):
        raise ValueError("Assertion on 'num_particles' failed: Must be a positive count")
    model = models.resolve(init_fn, transition_fn, log_likelihood_fn)
    if model == "lgmv":
        y, thetas, tv_draws = _mv_batch_args(init_fn.owner, y, thetas)
        dim = init_fn.owner.dim
    elif model == "rnet":
        if time_varying is not None or tv_set is not None:
            raise ValueError("time_varying / tv_set: the multivariate linear-Gaussian family only")
        if _algorithm != "BPF":
            raise ValueError("reaction_network: the batched path runs the bootstrap filter (batched APF / RMPF are not available)")
        if resample_fn == "multinomial":
            raise ValueError("reaction_network: stratified / systematic resampling only")
        y, thetas = _rn_batch_args(init_fn.owner, y, thetas)
        dim = init_fn.owner.dim
        if int(num_particles) > batch_max_particles(dim, "rnet"):
            raise ValueError("reaction_network: a batched filter holds at most batch_max_particles(%d, \"rnet\") particles" % dim)
    else:
        if time_varying is not None or tv_set is not None:
            raise ValueError("time_varying / tv_set: the multivariate linear-Gaussian family only")
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim != 1:
            raise ValueError("this build supports scalar observations (y a vector)")
        if not np.all(np.isfinite(y)):
            raise ValueError("Assertion on 'y' failed: Contains missing values")
    T, N = int(y.shape[0]), int(num_particles)
    ot = None
    if obs_times is not None:
        ot = np.ascontiguousarray(obs_times, dtype=np.int32)
        if ot.size != T or (T and (ot[0] < 1 or np.any(np.diff(ot) < 0))):
            raise ValueError("Assertion on 'obs_times' failed")
    if model == "rnet":
        init_fn.owner.check_times(thetas.shape[1], T, ot)          # (a rate schedule reaches the last observation time)
    if model not in ("lgmv", "rnet"):
        thetas = np.ascontiguousarray(thetas, dtype=np.float64)
        dim = models.dim_of(model)
        if thetas.ndim != 2 or thetas.shape[1] < (5 if model == "sir" else 3):
            raise ValueError("thetas must be an (n_filters, 3) array of (phi, sigma_x, sigma_y) "
                             "[SIR: (n_filters, 5) of (lambda, gamma, n_total, s0, i0)]")
    F = int(thetas.shape[0])
    seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (F,)))
    streams = np.arange(F, dtype=np.uint64) if streams is None else \
        np.ascontiguousarray(np.broadcast_to(np.asarray(streams, dtype=np.uint64), (F,)))
    tvs = tvb = None
    if model == "lgmv":
        tvb = _mv_batch_tv(init_fn.owner, F, T, ot, tv_draws, time_varying, tv_set)
        if tvb is None and time_varying is None and not init_fn.owner.has_param_tv:
            tvs = _mv_tv_struct(init_fn.owner.tv_arrays(T, ot))      # shared by the filters, as y is
    ctx = ctx.require(1, 1) if ctx is not None else _lib.default_context(N, dim=1)
    ll = np.zeros(F)
    se = np.zeros((F, T + 1, dim)) if (dim > 1 or model in ("lgmv", "rnet")) else np.zeros((F, T + 1))
    ess = np.zeros((F, T + 1))
    llh = np.zeros((F, max(T, 1)))
    ers = np.zeros(F, dtype=np.int32)
    nres = np.zeros(F, dtype=np.int32)
    status = np.zeros(F, dtype=np.int32)
    ms = np.zeros(1)
    model_id = _lib.MV_OBS_MODEL[init_fn.owner.obs] if model == "lgmv" else _lib.RN_OBS_MODEL[init_fn.owner.obs] if model == "rnet" else _lib.MODEL[model]
    cfg = _lib.PfConfig(model_id, _lib.ALGORITHM[_algorithm], _lib.RESAMPLE_ALGORITHM[resample_algorithm],
                        _lib.RESAMPLE_FN[resample_fn], N, T, float("nan") if threshold is None else float(threshold),
                        None, int(thetas.shape[1]), _ptr(y), _ptr(ot), 0, 0, None, None, None, 0, 0, float(_move_sd), None, None,
                        C.cast(C.pointer(tvs), C.c_void_p) if tvs is not None else None)
    res = _lib.PfBatchResult(_ptr(ll), _ptr(se), _ptr(ess), _ptr(llh), _ptr(ers), _ptr(nres), _ptr(status), _ptr(ms))
    skip = model in ("lgmv", "rnet") and init_fn.owner.missing == "skip"
    sets = None
    if tvb is not None:                                      # one array set per parameter draw
        n_times, n_sets, set_of, tvp = tvb
        (b, sb), (h0, sh0), (H, sH) = (tvp.get(k, (None, 0)) for k in _TV_NAMES)
        sets = _lib.MvTvBatch(int(n_times), int(n_sets), _ptr(set_of), _ptr(b), sb, _ptr(h0), sh0, _ptr(H), sH)
    if _smooth_k is not None:                                # bootstrap_smoother_batch: the recording launch and the trace
        K = int(_smooth_k)
        sm_se, sm_nlin, traced, sm_ms = np.zeros((F, T + 1, dim)), np.zeros((F, T + 1), dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(1)
        sm_traj, sm_u, sm_idx = np.zeros((F, K, T + 1, dim)), np.zeros((F, K)), np.zeros((F, K), dtype=np.int32)
        scfg = _lib.SmoothConfig(K)
        sres = _lib.SmoothBatchResult(_ptr(sm_se), _ptr(sm_nlin), _ptr(sm_traj) if K else None, _ptr(sm_u) if K else None,
                                      _ptr(sm_idx) if K else None, _ptr(traced), _ptr(sm_ms))
    with contextlib.ExitStack() as scope:
        scope.enter_context(ctx.mv_y_missing(skip))
        if model == "rnet":                                   # (as particle_filter_core)
            scope.enter_context(ctx.rn_method(init_fn.owner.rn_method, init_fn.owner.rn_leaps))
        if _smooth_k is not None:
            st = _lib.load().bssm_pf_run_batch_smooth(ctx.handle, C.byref(cfg), F, _ptr(thetas), _ptr(seeds), _ptr(streams),
                                                      C.cast(C.pointer(sets), C.c_void_p) if sets is not None else None, C.byref(res),
                                                      C.cast(C.pointer(scfg), C.c_void_p), C.cast(C.pointer(sres), C.c_void_p))
        elif sets is not None:
            st = _lib.load().bssm_pf_run_batch_tv(ctx.handle, C.byref(cfg), F, _ptr(thetas), _ptr(seeds), _ptr(streams),
                                                  C.byref(sets), C.byref(res))
        else:
            st = _lib.load().bssm_pf_run_batch(ctx.handle, C.byref(cfg), F, _ptr(thetas), _ptr(seeds), _ptr(streams),
                                               C.byref(res))
    _lib.check(st)
    out = {"loglike": ll, "state_est": se, "ess": ess, "loglike_history": llh[:, :T], "early_return_step": ers,
           "n_res_calls": nres, "status": status, "device_ms": float(ms[0]), "algorithm": _algorithm}
    if _smooth_k is not None:
        out.update(smoothed_state_est=sm_se, n_lineages=sm_nlin, trajectories=sm_traj, traced=traced,
                   _extras={"smooth_ms": float(sm_ms[0]), "trajectory_u": sm_u, "trajectory_index": sm_idx})
    return out


def bootstrap_smoother_batch(y, num_particles, init_fn, transition_fn, log_likelihood_fn, thetas, seeds=0, streams=None, trajectories=0,
                             obs_times=None, resample_algorithm=None, resample_fn=None, threshold=None, time_varying=None, tv_set=None,
                             ctx=None):
    """bootstrap_filter_batch with the genealogy smoother of every filter: the batched launch leaves each filter's
    histories on the device and one more launch traces them, one workgroup per filter (bssm_pf_run_batch_smooth).  The
    multivariate linear-Gaussian family and the reaction networks, with every option bootstrap_filter_batch takes for them.
    The result is bootstrap_filter_batch's dict (bit for bit) plus
        smoothed_state_est [F, T+1, d], n_lineages [F, T+1], trajectories [F, K, T+1, d] (K = trajectories, 0 .. 4096), traced [F],
        _extras: smooth_ms, trajectory_u [F, K], trajectory_index [F, K] (1-based),
    filter k's rows being exactly what bootstrap_filter(..., smooth=True, trajectories=K, seed=seeds[k], stream=streams[k]) returns.
    A filter that returned early on degenerate weights is not traced: traced[k] == 0, NaN in its float rows, 0 in its int rows."""
    if not (isinstance(trajectories, (int, np.integer)) and not isinstance(trajectories, bool) and 0 <= trajectories <= _MAX_TRAJECTORIES):
        raise ValueError("trajectories must be an integer in 0 .. %d" % _MAX_TRAJECTORIES)
    if models.resolve(init_fn, transition_fn, log_likelihood_fn) not in ("lgmv", "rnet"):
        raise ValueError("bootstrap_smoother_batch: the multivariate linear-Gaussian family (models.linear_gaussian_mv) and the reaction "
                         "networks (models.reaction_network) only -- the scalar models' batched kernel keeps no history; "
                         "linear_gaussian_mv(1, 1) and the reaction-network SIR are the same models there")
    return bootstrap_filter_batch(y, num_particles, init_fn, transition_fn, log_likelihood_fn, thetas, seeds, streams, obs_times=obs_times,
                                  resample_algorithm=resample_algorithm, resample_fn=resample_fn, threshold=threshold, ctx=ctx,
                                  time_varying=time_varying, tv_set=tv_set, _smooth_k=int(trajectories))


def bootstrap_filter_multi(y, num_particles, init_fn, transition_fn, log_likelihood_fn, thetas, seeds=0, streams=None, obs_times=None,
                           resample_algorithm=None, resample_fn=None, threshold=None, ctxs=None, smooth=False, trajectories=0):
    """K (<= 4) independent LARGE bootstrap filters in lock-step on one stream (bssm_pf_run_multi): the launches of one filter run
    carry all K filters (blockIdx.y), so independent PMMH chains (R/pmmh.R:511-531) share them.  Filter k runs with thetas[k],
    seeds[k], streams[k] on the shared data and returns exactly what bootstrap_filter(..., seed=seeds[k], stream=streams[k],
    return_particles=False) returns.  ctxs: one Context per filter (created and closed here when None).
    Returns a dict of arrays like bootstrap_filter_batch.  smooth / trajectories are refused (the lock-step filters keep no history)."""
    _refuse_smooth({"smooth": smooth, "trajectories": trajectories}, "bootstrap_filter_multi")
    resample_algorithm = _match_arg(resample_algorithm, _RESAMPLE_ALGORITHMS, "resample_algorithm")
    resample_fn = _match_arg(resample_fn, _RESAMPLE_FNS, "resample_fn")
    model = models.resolve(init_fn, transition_fn, log_likelihood_fn)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 1 or not np.all(np.isfinite(y)):
        raise ValueError("Assertion on 'y' failed")
    T, N = int(y.size), int(num_particles)
    ot = np.ascontiguousarray(obs_times, dtype=np.int32) if obs_times is not None else None
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    F = int(thetas.shape[0])
    if not 1 <= F <= 4:
        raise ValueError("bootstrap_filter_multi: 1 .. 4 filters per call")
    seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (F,)))
    streams = np.arange(F, dtype=np.uint64) if streams is None else np.ascontiguousarray(np.broadcast_to(np.asarray(streams, dtype=np.uint64), (F,)))
    dim = models.dim_of(model)
    own = ctxs is None
    if own:
        ctxs = [_lib.Context(_lib.default_context(1).device, N, dim) for _ in range(F)]
    try:
        ll, se, ess = np.zeros(F), (np.zeros((F, T + 1, dim)) if dim > 1 else np.zeros((F, T + 1))), np.zeros((F, T + 1))
        llh, ers, nres, status, ms = np.zeros((F, max(T, 1))), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(1)
        cfg = _lib.PfConfig(_lib.MODEL[model], _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM[resample_algorithm], _lib.RESAMPLE_FN[resample_fn],
                            N, T, float("nan") if threshold is None else float(threshold), None, int(thetas.shape[1]), _ptr(y), _ptr(ot), 0, 0,
                            None, None, None, 0, 0, 0.0, None, None)
        res = _lib.PfBatchResult(_ptr(ll), _ptr(se), _ptr(ess), _ptr(llh), _ptr(ers), _ptr(nres), _ptr(status), _ptr(ms))
        handles = (C.c_void_p * F)(*[cx.handle for cx in ctxs[:F]])
        lib = _lib.load()
        lib.bssm_pf_run_multi.argtypes = [C.c_void_p, C.c_int, C.POINTER(_lib.PfConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_lib.PfBatchResult)]
        _lib.check(lib.bssm_pf_run_multi(handles, F, C.byref(cfg), _ptr(thetas), _ptr(seeds), _ptr(streams), C.byref(res)))
    finally:
        if own:
            for cx in ctxs:
                cx.close()
    return {"loglike": ll, "state_est": se, "ess": ess, "loglike_history": llh[:, :T], "early_return_step": ers, "n_res_calls": nres,
            "status": status, "device_ms": float(ms[0])}


def bootstrap_filter(y, num_particles, init_fn, transition_fn, log_likelihood_fn, obs_times=None,
                     resample_algorithm=None, resample_fn=None, threshold=None, return_particles=True, **kwargs):
    """bootstrap_filter (R/bootstrap_filter.R:129-171).  Model parameters are passed by name
    (phi=, sigma_x=, sigma_y=), as through `...` in the reference.  Extra keywords of this
    build: seed, stream, draws, ctx, return_ancestors, and smooth / trajectories (the genealogy smoother, DESIGN 1e: the result gains
    smoothed_state_est, n_lineages and, for trajectories = K > 0, trajectories [K, T+1, d])."""
    resample_algorithm = _match_arg(resample_algorithm, _RESAMPLE_ALGORITHMS, "resample_algorithm")
    resample_fn = _match_arg(resample_fn, _RESAMPLE_FNS, "resample_fn")
    from .closures import is_closure_model, particle_filter_closures
    if is_closure_model(init_fn, transition_fn, log_likelihood_fn):
        # plain callables: the model runs on the host, the core's own work on the device (closures.py)
        _refuse_smooth(kwargs, "closure mode")
        extra = {k: kwargs.pop(k) for k in ("ctx", "u_res") if k in kwargs}
        return particle_filter_closures(y, num_particles, init_fn, transition_fn, log_likelihood_fn, None, None, obs_times, "BPF",
                                        resample_algorithm, resample_fn, threshold, return_particles, **extra, **kwargs)
    r_seed = kwargs.pop("r_seed", None)
    r_stream = kwargs.pop("r_stream", None)          # an rrng.RRandom positioned where R's generator stands before this call
    r_guess = kwargs.pop("r_guess", None)            # first guess of the resample decisions (any guess converges; a good one saves rounds)
    ctl = {k: kwargs.pop(k) for k in ("seed", "stream", "draws", "ctx", "return_ancestors", "smooth", "trajectories") if k in kwargs}
    model = models.resolve(init_fn, transition_fn, log_likelihood_fn)
    if model == "lgmv":                      # multivariate linear-Gaussian family: the descriptor packs its matrices for this parameter draw
        theta = init_fn.owner.pack(kwargs)
        return particle_filter_core(y, num_particles, model, theta, "BPF", obs_times, resample_algorithm, resample_fn,
                                    threshold, return_particles, mv_owner=init_fn.owner, mv_params=kwargs, **ctl)
    if model == "rnet":                      # reaction network: the descriptor packs its block for this parameter draw
        if r_seed is not None or r_stream is not None:
            raise ValueError("r_seed / r_stream: the scalar Gaussian-observation models only (closures of the README's form)")
        return _rn_filter("BPF", y, num_particles, init_fn.owner, kwargs, obs_times, resample_algorithm, resample_fn, threshold,
                          return_particles, ctl)
    theta = models.theta_from_kwargs((init_fn, transition_fn, log_likelihood_fn), kwargs)
    if r_seed is not None or r_stream is not None:
        _refuse_smooth(ctl, "r_seed / r_stream")
        if r_seed is not None and r_stream is not None:
            raise ValueError("r_seed and r_stream are mutually exclusive")
        from .rrng import RRandom
        return _r_seeded_bootstrap(y, num_particles, model, theta, obs_times, resample_algorithm, resample_fn, threshold,
                                   return_particles, RRandom(int(r_seed)) if r_seed is not None else r_stream, ctl, r_guess)
    return particle_filter_core(y, num_particles, model, theta, "BPF", obs_times, resample_algorithm, resample_fn,
                                threshold, return_particles, **ctl)


def _r_seeded_bootstrap(y, N, model, theta, obs_times, ra, rf, threshold, return_particles, g, ctl, guess=None):
    """bootstrap_filter(..., r_seed = s) / (..., r_stream = g): the run R makes from the generator's position (after `set.seed(s)`,
    or wherever a longer R session -- a whole pmmh() call -- has left it) when the closures have the README's form
    (rrng.r_stream_draws): the draws come from the R-compatible host generator in R's order and enter through the
    parity mode.  Whether uniforms are consumed at an observation depends on that observation's resample decision, so
    the draw sequence is the fixed point of "assume decisions -> draw -> run -> read decisions" (at most T rounds; one
    round for SIS / SISR); every round starts from the same generator state and the last one leaves the generator exactly where
    R's stands after the call.  R's streams are pinned by R's published known answers, the filter arithmetic by the parity tests,
    and the two together by the README's printed PMMH table (tests/test_gpu_readme_r_stream.py)."""
    from .rrng import r_stream_draws
    if model not in ("lg", "ar1sin"):
        raise ValueError("r_seed / r_stream: the scalar Gaussian-observation models only (closures of the README's form)")
    rf_dev = "multinomial_r" if rf == "multinomial" else rf      # Rcpp::sample's own algorithm on R's unif_rand() stream
    if ctl.get("draws") is not None:
        raise ValueError("r_seed / r_stream and draws are mutually exclusive")
    T = int(np.asarray(y).size)
    dec = np.ones(T, dtype=bool) if ra != "SIS" else np.zeros(T, dtype=bool)
    if guess is not None and ra == "SISAR" and len(guess) == T:
        dec = np.asarray(guess, dtype=bool).copy()
    ctl = {k: v for k, v in ctl.items() if k not in ("seed", "stream", "draws")}
    start = g.snapshot()
    upto_draw = None
    for _ in range(T + 2):
        g.restore(start)
        d = r_stream_draws(g, T, int(N), rf, dec, obs_times, upto=upto_draw)
        res = particle_filter_core(y, N, model, theta, "BPF", obs_times, ra, rf_dev, threshold, return_particles, draws=d, **ctl)
        got = np.asarray(res["_extras"]["resampled"], dtype=bool)
        early = res["_extras"]["early_return_step"]
        upto = (early - 1) if early else T                    # after a degenerate early return nothing more is drawn
        if np.array_equal(got[:upto], dec[:upto]):
            if early and upto_draw != early:                  # (one more round so that the generator stops where R's does)
                upto_draw = early
                continue
            res["_extras"]["r_seed_decisions"] = dec[:upto].copy()
            return res
        upto_draw = None
        k = int(np.flatnonzero(got[:upto] != dec[:upto])[0])  # everything before the first disagreement was drawn right
        dec[:k + 1] = got[:k + 1]
        dec[k + 1:] = got[k + 1:]
    raise RuntimeError("r_seed: the resample decisions did not reach a fixed point")


def auxiliary_filter(y, num_particles, init_fn, transition_fn, log_likelihood_fn, aux_log_likelihood_fn,
                     obs_times=None, resample_algorithm=None, resample_fn=None, threshold=None,
                     return_particles=True, **kwargs):
    """auxiliary_filter (R/auxiliary_filter.R:163-216)."""
    resample_fn = _match_arg(resample_fn, _RESAMPLE_FNS, "resample_fn")
    resample_algorithm = _match_arg(resample_algorithm, _RESAMPLE_ALGORITHMS, "resample_algorithm")
    from .closures import is_closure_model, particle_filter_closures
    if is_closure_model(init_fn, transition_fn, log_likelihood_fn, aux_log_likelihood_fn):
        _refuse_smooth(kwargs, "closure mode")
        extra = {k: kwargs.pop(k) for k in ("ctx", "u_res") if k in kwargs}
        return particle_filter_closures(y, num_particles, init_fn, transition_fn, log_likelihood_fn, aux_log_likelihood_fn, None,
                                        obs_times, "APF", resample_algorithm, resample_fn, threshold, return_particles,
                                        **extra, **kwargs)
    ctl = {k: kwargs.pop(k) for k in ("seed", "stream", "draws", "ctx", "return_ancestors", "smooth", "trajectories") if k in kwargs}
    model = models.resolve(init_fn, transition_fn, log_likelihood_fn, aux_log_likelihood_fn)
    if model == "lgmv":                      # multivariate linear-Gaussian family: the descriptor packs its matrices for this parameter draw
        _mv_no_r_stream(kwargs)
        return particle_filter_core(y, num_particles, model, init_fn.owner.pack(kwargs), "APF", obs_times, resample_algorithm,
                                    resample_fn, threshold, return_particles, mv_owner=init_fn.owner, mv_params=kwargs, **ctl)
    if model == "rnet":
        if "r_seed" in kwargs or "r_stream" in kwargs:
            raise ValueError("r_seed / r_stream: the scalar Gaussian-observation models only (closures of the README's form)")
        return _rn_filter("APF", y, num_particles, init_fn.owner, kwargs, obs_times, resample_algorithm, resample_fn, threshold,
                          return_particles, ctl)
    theta = models.theta_from_kwargs((init_fn, transition_fn, log_likelihood_fn, aux_log_likelihood_fn), kwargs)
    return particle_filter_core(y, num_particles, model, theta, "APF", obs_times, resample_algorithm, resample_fn,
                                threshold, return_particles, **ctl)


def _rn_filter(algorithm, y, num_particles, owner, params, obs_times, resample_algorithm, resample_fn, threshold, return_particles, ctl):
    """bootstrap_filter / auxiliary_filter on a reaction network (models.reaction_network): every refusal is raised here, on the host"""
    if resample_fn == "multinomial":
        raise ValueError("reaction_network: stratified / systematic resampling only")
    draws = ctl.get("draws")
    if draws is not None and (draws.get("z_init") is not None or draws.get("z_trans") is not None):
        raise ValueError("reaction_network: the transition draws a data-dependent number of variates; injected z_* are not supported (u_res is)")
    theta = owner.pack(params)
    if obs_times is None or np.ndim(obs_times) == 1:               # (a rate schedule reaches the last observation time)
        owner.check_times(theta.size, int(np.shape(y)[0]), obs_times)
    return particle_filter_core(y, num_particles, "rnet", theta, algorithm, obs_times, resample_algorithm, resample_fn,
                                threshold, return_particles, rn_owner=owner, **ctl)


def _mv_no_r_stream(kwargs):
    if "r_seed" in kwargs or "r_stream" in kwargs:
        raise ValueError("r_seed / r_stream: the scalar Gaussian-observation models only (closures of the README's form)")


def resample_move_filter(y, num_particles, init_fn, transition_fn, log_likelihood_fn, move_fn, obs_times=None,
                         resample_fn=None, return_particles=True, **kwargs):
    """resample_move_filter (R/resample_move_filter.R:190-236): resample at every step (SISR), then move every
    particle.  `move_fn` must be the built-in random-walk Metropolis move (`model.rw_move_fn(sd)`), the move of the
    reference's own example; arbitrary R closures cannot run on the device."""
    resample_fn = _match_arg(resample_fn, _RESAMPLE_FNS, "resample_fn")
    kwargs.pop("resample_algorithm", None)                    # removed from ... by the reference too (:213-216)
    from .closures import is_closure_model, particle_filter_closures
    if is_closure_model(init_fn, transition_fn, log_likelihood_fn, move_fn):
        _refuse_smooth(kwargs, "closure mode")
        extra = {k: kwargs.pop(k) for k in ("ctx", "u_res") if k in kwargs}
        return particle_filter_closures(y, num_particles, init_fn, transition_fn, log_likelihood_fn, None, move_fn, obs_times,
                                        "RMPF", "SISR", resample_fn, None, return_particles, **extra, **kwargs)
    ctl = {k: kwargs.pop(k) for k in ("seed", "stream", "draws", "ctx", "return_ancestors", "smooth", "trajectories") if k in kwargs}
    if not isinstance(move_fn, models.MoveFn):
        raise TypeError("move_fn must be a built-in move descriptor (model.rw_move_fn(sd))")
    model = models.resolve(init_fn, transition_fn, log_likelihood_fn)
    if model == "rnet":
        raise ValueError("reaction_network: resample_move_filter (RMPF) is not available: a move on integer states is not defined")
    if move_fn.model != model or model == "sir":
        raise ValueError("move_fn belongs to a different model")
    if model == "lgmv":
        _mv_no_r_stream(kwargs)
        return particle_filter_core(y, num_particles, model, init_fn.owner.pack(kwargs), "RMPF", obs_times, "SISR", resample_fn, None,
                                    return_particles, move_sd=move_fn.sd, mv_owner=init_fn.owner, mv_params=kwargs, **ctl)
    theta = models.theta_from_kwargs((init_fn, transition_fn, log_likelihood_fn), kwargs)
    return particle_filter_core(y, num_particles, model, theta, "RMPF", obs_times, "SISR", resample_fn, None,
                                return_particles, move_sd=move_fn.sd, **ctl)


def dump_draws(algorithm, T, N, resample_fn, seed, stream, obs_times=None, ctx=None, dim=None):
    """The device generator's draws for one filter run, as arrays a CPU run can consume
    (same layout as the `draws` argument).  dim: the state dimension of the multivariate family
    (models.linear_gaussian_mv); its draws are component-major, z_init [d][N], z_trans [calls][d][N], z_move [T][d][N]."""
    if dim is not None:
        return _dump_draws_mv(algorithm, T, N, resample_fn, seed, stream, obs_times, ctx, int(dim))
    ctx = ctx or _lib.default_context(N)
    lib = _lib.load()
    max_trans, max_res = noise_shape(algorithm, T, obs_times)
    zi = np.empty(N)
    _lib.check(lib.bssm_dump_normals(ctx.handle, seed, stream, 1, 0, N, _ptr(zi)))
    zt = np.empty((max(max_trans, 1), N))
    for k in range(max_trans):
        _lib.check(lib.bssm_dump_normals(ctx.handle, seed, stream, 2, k, N, _ptr(zt[k])))
    nu = 1 if resample_fn == "systematic" else N
    ur = np.empty((max(max_res, 1), nu))
    for k in range(max_res):
        _lib.check(lib.bssm_dump_uniforms(ctx.handle, seed, stream, k, nu, _ptr(ur[k])))
    out = {"z_init": zi, "z_trans": zt, "u_res": ur.reshape(-1) if nu == 1 else ur}
    if algorithm == "RMPF":
        zm, um = np.empty((max(T, 1), N)), np.empty((max(T, 1), N))
        for i in range(T):
            _lib.check(lib.bssm_dump_move_draws(ctx.handle, seed, stream, i + 1, N, _ptr(zm[i]), _ptr(um[i])))
        out["z_move"], out["u_move"] = zm, um
    return out


def dump_rpois(lam, seed, stream, call=0, leap=0, r=0, ctx=None):
    """The Poisson draws of the tau-leap transition (bssm_dump_rpois): out[j] is what particle j draws for reaction r in leap `leap`
    of transition call `call` at the mean lam[j], under (seed, stream)."""
    lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1)
    if lam.size < 1:
        raise ValueError("dump_rpois: lam holds at least one mean")
    ctx = ctx or _lib.default_context(lam.size)
    out = np.empty(lam.size)
    _lib.check(_lib.load().bssm_dump_rpois(ctx.handle, int(seed), int(stream), int(call), int(leap), int(r), lam.size, _ptr(lam), _ptr(out)))
    return out


def dump_rbinom(n, q, seed, stream, call=0, leap=0, r=0, ctx=None):
    """The binomial draws of the Euler-multinomial transition (bssm_dump_rbinom): out[j] is what particle j draws for reaction r in leap
    `leap` of transition call `call` from n[j] trials at the probability q[j], under (seed, stream).  n and q broadcast against each other."""
    n, q = np.broadcast_arrays(np.asarray(n, dtype=np.float64), np.asarray(q, dtype=np.float64))
    n, q = np.ascontiguousarray(n).reshape(-1), np.ascontiguousarray(q).reshape(-1)
    if n.size < 1:
        raise ValueError("dump_rbinom: n and q hold at least one pair")
    ctx = ctx or _lib.default_context(n.size)
    out = np.empty(n.size)
    _lib.check(_lib.load().bssm_dump_rbinom(ctx.handle, int(seed), int(stream), int(call), int(leap), int(r), n.size, _ptr(n), _ptr(q), _ptr(out)))
    return out


def dump_rgamma(shape, seed, stream, call=0, leap=0, g=0, ctx=None):
    """The gamma draws of the reaction networks' gamma white noise (bssm_dump_rgamma): out[j] is what particle j draws for the noise group
    with leader g in leap `leap` of transition call `call` at the shape shape[j] (scale 1), under (seed, stream)."""
    shape = np.ascontiguousarray(shape, dtype=np.float64).reshape(-1)
    if shape.size < 1:
        raise ValueError("dump_rgamma: shape holds at least one value")
    ctx = ctx or _lib.default_context(shape.size)
    out = np.empty(shape.size)
    _lib.check(_lib.load().bssm_dump_rgamma(ctx.handle, int(seed), int(stream), int(call), int(leap), int(g), shape.size, _ptr(shape), _ptr(out)))
    return out


def _dump_draws_mv(algorithm, T, N, resample_fn, seed, stream, obs_times, ctx, d):
    ctx = ctx or _lib.default_context(N, dim=d)
    lib = _lib.load()
    max_trans, max_res = noise_shape(algorithm, T, obs_times)
    zi = np.empty((d, N))
    _lib.check(lib.bssm_dump_normals_mv(ctx.handle, seed, stream, 1, 0, N, d, _ptr(zi)))
    zt = np.empty((max(max_trans, 1), d, N))
    for k in range(max_trans):
        _lib.check(lib.bssm_dump_normals_mv(ctx.handle, seed, stream, 2, k, N, d, _ptr(zt[k])))
    nu = 1 if resample_fn == "systematic" else N
    ur = np.empty((max(max_res, 1), nu))
    for k in range(max_res):
        _lib.check(lib.bssm_dump_uniforms(ctx.handle, seed, stream, k, nu, _ptr(ur[k])))
    out = {"z_init": zi, "z_trans": zt, "u_res": ur.reshape(-1) if nu == 1 else ur}
    if algorithm == "RMPF":
        zm, um = np.empty((max(T, 1), d, N)), np.empty((max(T, 1), N))
        for i in range(T):
            _lib.check(lib.bssm_dump_move_draws_mv(ctx.handle, seed, stream, i + 1, N, d, _ptr(zm[i]), _ptr(um[i])))
        out["z_move"], out["u_move"] = zm, um
    return out
