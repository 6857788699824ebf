"""GPU tests of negative-binomial observations in the reaction-network family (models.reaction_network(obs="negbin", size=);
BSSM_MODEL_RNET_NB: rn_dnbinom_log and the OBS instantiations of rn_loglik, k_step_rn, step_emul_rn, k_pf_batch_rn; rn_block_check,
pf_run_rn, pf_run_batch_rn and its [F][T][p] tables).  The reference is the numpy restatement of the definition
(tests/rnet_nb_restated.py) at the bars of tests/test_gpu_rnet_limits.py; the batched = single identity, "obs='poisson' is no keyword",
pmmh and the refusals behind the ABI need no restatement."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_nb_restated as NB  # noqa: E402
from test_gpu_rnet import run, same  # noqa: E402
from test_gpu_rnet_limits import (FULL8_OBSERVE, FULL8_PAR, FULL8_REACTIONS, FULL8_SPECIES, FULL8_X0, OT, SIRS3_PAR, Y_FULL8, Y_SIRS3,  # noqa: E402
                                  compare_with_restatement, u_res_for)
from test_gpu_rnet_incidence import NETS as INC_NETS, OT as OT_INC, seir5  # noqa: E402
from test_gpu_rnet_tv import pattern  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 15, 8)
    yield c
    c.close()


# --- the networks of test_gpu_rnet_limits / test_gpu_rnet_tv, with the observation family as a keyword ------------------------------------
def sirs3(B, **kw):
    return B.models.reaction_network(("S", "I", "R"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"R": 1}, {"S": 1}, "rho")],
                                     x0=(40, 6, 4), observe=[{"I": 0.3}, {"S": 0.05, "R": 0.2}], **kw)


def full8(B, **kw):
    return B.models.reaction_network(FULL8_SPECIES, FULL8_REACTIONS, x0=[FULL8_X0[s] for s in FULL8_SPECIES], observe=FULL8_OBSERVE, **kw)


# sirs3: mu_0 = 0.3 I is a few units, above size_0 = 0.8 (lr by log(r / s)); mu_1 = 0.05 S + 0.2 R is about 3, below size_1 = 25 (lr by
# log1p).  gamma = 0.9 lets the infection die out in some particles: I = 0 under y_0 > 0 is the -inf case.  9 in the tight component
# surprises the filter (SISAR resamples there and not everywhere); both components see a 0.
SIRS3_SIZE = (0.8, 25.0)
SIRS3_NB_PAR = dict(SIRS3_PAR, gamma=0.9)
Y_SIRS3_NB = np.array([[2, 3], [7, 0], [0, 9], [8, 1], [3, 3]], dtype=np.float64)
# full8: the typical mu_k is 0.3 .. 0.6 for k < 7 and 0 .. 2 for H: eight different sizes on both sides of it.  k6 = 4 makes the Euler
# mean of H negative wherever H >= 1 (H - 4 H + 0.06 F G with F G about 30): the look-ahead's clamp acts, under y_7 = 0 too, where the
# unclamped density would give -inf for 0.0.  Three larger counts in the tight components (sizes 5, 8, 12) make SISAR resample.
FULL8_SIZE = (0.1, 5.0, 0.2, 8.0, 0.3, 12.0, 0.25, 0.5)
FULL8_NB_PAR = dict(FULL8_PAR, k6=4.0)
Y_FULL8_NB = Y_FULL8.copy()
Y_FULL8_NB[2, 1], Y_FULL8_NB[3, 5], Y_FULL8_NB[1, 3] = 4, 3, 4
Y_SIRS3_MISS = Y_SIRS3_NB.copy()
Y_SIRS3_MISS[1, 1], Y_SIRS3_MISS[3, 0] = np.nan, np.nan

# name: (constructor keywords -> descriptor, parameters, y)
REST = {"sirs3": (lambda B: sirs3(B, obs="negbin", size=SIRS3_SIZE), SIRS3_NB_PAR, Y_SIRS3_NB),
        "full8": (lambda B: full8(B, obs="negbin", size=FULL8_SIZE), FULL8_NB_PAR, Y_FULL8_NB),
        "sirs3_missing": (lambda B: sirs3(B, obs="negbin", size=SIRS3_SIZE, missing="skip"), SIRS3_NB_PAR, Y_SIRS3_MISS)}


def restated(oracle, m, par, y, N, algorithm, seed=23, stream=4):
    """the restatement's run on OT under SISAR + stratified, its counts and the u_res it used, with what the inputs were chosen for
    asserted on the restatement itself: both branches of lr, a y == 0 component, between 1 and N - 1 particles at -inf at some
    observation, a filter that resamples at some observations and not at all"""
    u = u_res_for(algorithm, len(y), N, "stratified")
    counts = {}
    t0 = time.perf_counter()
    ref = NB.pf_run_rn(oracle, m.pack(par), y, N, u, seed=seed, stream=stream, algorithm=algorithm, counts=counts, resample_algorithm="SISAR",
                       resample_fn="stratified", obs_times=OT, return_particles=True)
    print("restatement: %.2f s" % (time.perf_counter() - t0), {k: counts[k] for k in NB.KEYS}, "n_inf", counts["n_inf"], "resampled", ref["resampled"])
    assert np.isfinite(ref["loglike"]) and ref["early_return_step"] == 0
    assert counts["lr_log"] > 0 and counts["lr_log1p"] > 0 and counts["y0"] > 0 and counts["mu0_inf"] > 0
    assert any(1 <= n <= N - 1 for n in counts["n_inf"]), counts["n_inf"]
    assert all(counts["fired"].get(r, 0) > 0 for r in range(m.R)), counts["fired"]
    assert ref["resampled"].any() and not ref["resampled"].all()
    return ref, counts, u


# --- 1. against the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [385, 2561])
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("name", ["sirs3", "full8"])
def test_against_the_restatement(B, ctx, oracle, name, algorithm, N):
    """p = 2 with sizes (0.8, 25) and p = 8 with eight different sizes against the numpy restatement, one and two blocks, on
    OT = 1, 2, 2, 4, 5 (a repeated time, a gap), SISAR + stratified with injected u_res, at test_gpu_rnet_limits' bars: log-likelihood
    and history 1e-6 relative, `resampled` equal, at most 1 ancestor in 1000 different, and where none differs ESS and state
    estimates at 1e-9 and the integer states exactly.  (Catches: size read at the wrong offset or as size[c] for G[k][c]'s c; the table
    c(t, k) not uploaded, so that lgamma(y + 1) stands in its place; the look-ahead's mu unclamped.)"""
    make, par, y = REST[name]
    m = make(B)
    ref, counts, u = restated(oracle, m, par, y, N, algorithm)
    if name == "full8" and algorithm == "APF":
        assert counts["clamped"] > 0                             # (the clamp acted: an unclamped look-ahead gives other first-stage weights)
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=23, stream=4, draws={"u_res": u})
    compare_with_restatement(got, ref)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_missing_components_against_the_restatement(B, ctx, oracle, algorithm):
    """missing="skip" with a NaN in either component: the density and the look-ahead sum over the observed components only, and the
    table entry of a NaN is never read"""
    make, par, y = REST["sirs3_missing"]
    m = make(B)
    ref, _, u = restated(oracle, m, par, y, 385, algorithm)
    got = run(B, m, algorithm, y, 385, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=23, stream=4, draws={"u_res": u})
    compare_with_restatement(got, ref)
    full = run(B, make(B), algorithm, np.nan_to_num(y, nan=1.0), 385, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT,
               seed=23, stream=4, draws={"u_res": u})
    assert full["loglike"] != got["loglike"]                     # (the components that were skipped carry weight when observed)


# --- 2. batched = single ------------------------------------------------------------------------------------------------------------------
def _batched_equals_single(B, ctx, m, y, pars, ot, N):
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    F = len(pars)
    seeds, streams = [11 + f for f in range(F)], [3 + f for f in range(F)]
    lls = set()
    for ra, rf in (("SISAR", "stratified"), ("SISR", "systematic"), ("SIS", "stratified")):
        bat = B.bootstrap_filter_batch(y, N, *fns, pars, seeds, streams, obs_times=ot, resample_algorithm=ra, resample_fn=rf, ctx=ctx)
        assert np.all(bat["status"] == 0)
        for f in range(F):
            one = B.bootstrap_filter(y, N, *fns, obs_times=ot, resample_algorithm=ra, resample_fn=rf, ctx=ctx, return_particles=False,
                                     seed=seeds[f], stream=streams[f], **pars[f])
            np.testing.assert_array_equal(bat["loglike"][f], one["loglike"])
            np.testing.assert_array_equal(bat["loglike_history"][f], one["loglike_history"])
            np.testing.assert_array_equal(bat["ess"][f], one["ess"])
            np.testing.assert_array_equal(bat["state_est"][f].reshape(one["state_est"].shape), one["state_est"])
            np.testing.assert_array_equal(bat["n_res_calls"][f], one["_extras"]["n_res_calls"])
            np.testing.assert_array_equal(bat["early_return_step"][f], one["_extras"]["early_return_step"])
            if N >= 385:
                assert np.isfinite(one["loglike"]), (N, ra, f)
        if ra == "SISAR":
            lls = {float(v) for v in bat["loglike"]}
    return lls


@pytest.mark.parametrize("N", [7, 1000])
def test_batched_equals_single(B, ctx, N):
    """k_pf_batch_rn<DM, RN_OBS_NB> = pf_run_rn bit for bit: three filters with three different size vectors and different rates, every
    output.  With the sizes exchanged between the filters the batched log-likelihoods change: the filters' tables differ.  (Catches:
    one table c(t, k) shared by the filters, or a table stride other than T p.)"""
    m = sirs3(B, obs="negbin", size=("r0", "r1"))
    pars = [dict(SIRS3_NB_PAR, r0=0.8, r1=25.0), dict(SIRS3_NB_PAR, beta=0.025, r0=3.0, r1=0.6), dict(SIRS3_NB_PAR, rho=0.4, r0=40.0, r1=6.0)]
    lls = _batched_equals_single(B, ctx, m, Y_SIRS3_NB, pars, OT, N)
    if N == 1000:
        assert len(lls) == 3
        swapped = [dict(q, r0=pars[(f + 1) % 3]["r0"], r1=pars[(f + 1) % 3]["r1"]) for f, q in enumerate(pars)]
        fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
        a = B.bootstrap_filter_batch(Y_SIRS3_NB, N, *fns, pars, [11, 12, 13], [3, 4, 5], obs_times=OT, ctx=ctx)
        b = B.bootstrap_filter_batch(Y_SIRS3_NB, N, *fns, swapped, [11, 12, 13], [3, 4, 5], obs_times=OT, ctx=ctx)
        assert np.all(a["loglike"] != b["loglike"])


@pytest.mark.parametrize("N", [7, 1000])
def test_batched_equals_single_with_everything(B, ctx, N):
    """the same with a counter, a rate schedule, missing="skip" and obs_times together (d = 5 under DM = 8, p = 2): size[p] sits between
    G and the two tails, and every offset behind it moves by p"""
    _, par, y, *_ = INC_NETS["seir5"]
    y = np.array(y, dtype=np.float64)
    assert np.isnan(y).any() and np.isnan(y).all(axis=1).any()       # a missing component and a row with nothing observed
    m = seir5(B, rate_schedule=pattern(OT_INC[-1], 3), missing="skip", obs="negbin", size=("r0", "r1"))
    assert m.counters == ("C",) and m.pack(dict(par, r0=1.0, r1=2.0)).size == m.n_theta()
    pars = [dict(par, r0=0.7, r1=30.0), dict(par, beta=0.002, r0=5.0, r1=0.9), dict(par, sigma=0.3, r0=60.0, r1=3.0)]
    lls = _batched_equals_single(B, ctx, m, y, pars, OT_INC, N)
    if N == 1000:
        assert len(lls) == 3


# --- 3. Poisson untouched -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, 2561])
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_poisson_keyword_changes_no_bit(B, ctx, algorithm, N):
    """obs="poisson" is the descriptor without the keyword: every output of bootstrap_filter / auxiliary_filter bit for bit"""
    for make, par, y in ((sirs3, SIRS3_PAR, Y_SIRS3), (full8, FULL8_PAR, Y_FULL8)):
        kw = dict(resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=19, stream=7)
        a, b = run(B, make(B), algorithm, y, N, ctx, par, **kw), run(B, make(B, obs="poisson"), algorithm, y, N, ctx, par, **kw)
        assert a["_extras"]["early_return_step"] == 0 and np.isfinite(a["loglike"])
        same(a, b)


@pytest.mark.parametrize("N", [7, 1000])
def test_poisson_keyword_changes_no_bit_batched(B, ctx, N):
    for make, par, y in ((sirs3, SIRS3_PAR, Y_SIRS3), (full8, FULL8_PAR, Y_FULL8)):
        outs = [B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, [par] * 2, 5, [1, 2], obs_times=OT, ctx=ctx)
                for m in (make(B), make(B, obs="poisson"))]
        assert np.all(outs[0]["status"] == 0) and np.all(np.isfinite(outs[0]["loglike"]))
        for key in ("loglike", "loglike_history", "ess", "state_est", "n_res_calls", "early_return_step"):
            np.testing.assert_array_equal(outs[0][key], outs[1][key], err_msg=key)


# --- 4. pmmh --------------------------------------------------------------------------------------------------------------------------
def test_pmmh_learns_size_on_the_lockstep_path(B, monkeypatch):
    """a short pmmh on the SEIR with the onsets counted learns the dispersion r next to beta: the lock-step batched path (every draw
    carries its own size in its block, every filter its own table), and every log-likelihood that path handed to the accept / reject
    step equals bootstrap_filter's for the same draw, seed and stream"""
    import bayesssm_amd.filters as filters
    m = B.models.reaction_network(("S", "E", "I", "R", "C"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1, "C": 1}, 0.5),
                                                             ({"I": 1}, {"R": 1}, 0.3)], x0=(180, 8, 12, 0, 0), observe={"C": 0.6}, counters=("C",),
                                  obs="negbin", size="r")
    assert m.param_order == ("beta", "r")
    y = np.array([2, 3, 1, 9, 4, 2, 12, 5, 6, 3], dtype=np.float64)             # (overdispersed: 9 and 12 among counts of 1 .. 6)
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    seen = []
    real = filters.bootstrap_filter_batch

    def recording(y_, n, i_, t_, l_, thetas, seeds, streams, **kw):
        out = real(y_, n, i_, t_, l_, thetas, seeds, streams, **kw)
        seen.append((int(n), np.array(thetas), list(seeds), list(streams), dict(kw), np.array(out["loglike"])))
        return out

    monkeypatch.setattr(filters, "bootstrap_filter_batch", recording)
    priors = {"beta": B.prior_exponential(100.0), "r": B.prior_exponential(0.2)}
    init = [dict(beta=0.004, r=3.0), dict(beta=0.0045, r=6.0)]
    tc = B.default_tune_control(pilot_m=20, pilot_burn_in=5, pilot_n=100, pilot_reps=3, pilot_proposal_sd=0.05)
    res = B.pmmh(B.bootstrap_filter, y, 25, *fns, priors, init, 5, num_chains=2, param_transform={k: "log" for k in priors}, tune_control=tc,
                 seed=7, print_result=False)
    assert res["_extras"]["batched"] is True and res["_extras"]["batched_launches"] > 0 and res["_extras"]["batched_launches"] == len(seen)
    r_chain = np.asarray(res["theta_chain"]["r"]).reshape(-1)
    assert len(set(r_chain)) > 2 and np.all(np.isfinite(r_chain)) and np.all(r_chain > 0)     # (r moved: the draws' sizes differed)
    o_k, o_size = 3 + m.dim, m.n_theta() - m.dim - m.p
    checked = 0
    for n, thetas, seeds, streams, kw, ll in seen[:2] + seen[-3:]:             # the pilot's first launches and the chains' last ones
        assert thetas.shape[1] == m.n_theta()
        for f in range(thetas.shape[0]):
            extra = {k: v for k, v in kw.items() if k in ("resample_algorithm", "resample_fn") and v is not None}
            one = B.bootstrap_filter(y, n, *fns, obs_times=kw.get("obs_times"), return_particles=False, seed=seeds[f], stream=streams[f],
                                     beta=float(thetas[f, o_k]), r=float(thetas[f, o_size]), **extra)
            np.testing.assert_array_equal(ll[f], one["loglike"])
            checked += 1
    assert checked >= 5 and len({float(t[o_size]) for _, th, *_ in seen for t in th}) > 3


# --- 5. behind the ABI ------------------------------------------------------------------------------------------------------------------
def test_refusals_behind_the_abi(B, ctx):
    """rn_block_check, pf_run_rn and pf_run_batch_rn under model id 7 through ctypes: the Poisson block's length, a size of 0, -1 and NaN,
    RMPF, multinomial resampling and a batched N above bssm_pf_batch_max_particles_rn(d) are refused before any kernel is launched"""
    from bayesssm_amd import _lib
    lib = _lib.load()
    p_ = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    T, d = len(OT), 3
    y = np.ascontiguousarray(Y_SIRS3_NB)
    ot = np.ascontiguousarray(OT, dtype=np.int32)
    good = sirs3(B, obs="negbin", size=SIRS3_SIZE).pack(SIRS3_NB_PAR)
    pois = sirs3(B).pack(SIRS3_NB_PAR)
    o_size = good.size - 2
    assert good.size == pois.size + 2 and np.array_equal(good[o_size:], SIRS3_SIZE)

    def single(theta, model=7, algorithm="BPF", rf="stratified", N=64):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        se, ess, llh, ll = np.zeros((T + 1, d)), np.zeros(T + 1), np.zeros(T), np.zeros(1)
        cfg = _lib.PfConfig(model, _lib.ALGORITHM[algorithm], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN[rf], N, T,
                            float("nan"), p_(theta), int(theta.size), p_(y), p_(ot), 1, 0, None, None, None, 0, 0, 0.1, None, None)
        res = _lib.PfResult(p_(se), p_(ess), p_(llh), p_(ll), None, None, None, None, None, None, None, None)
        rc = lib.bssm_pf_run(ctx.handle, C.byref(cfg), C.byref(res))
        return rc, lib.bssm_last_error().decode(), float(ll[0])

    def batched(thetas, model=7, rf="stratified", N=64):
        thetas = np.ascontiguousarray(thetas, dtype=np.float64)
        F = thetas.shape[0]
        ll, status = np.zeros(F), np.zeros(F, dtype=np.int32)
        seeds, streams = np.arange(F, dtype=np.uint64) + 1, np.arange(F, dtype=np.uint64)
        cfg = _lib.PfConfig(model, _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN[rf], N, T,
                            float("nan"), None, int(thetas.shape[1]), p_(y), p_(ot), 0, 0, None, None, None, 0, 0, 0.0, None, None)
        res = _lib.PfBatchResult(p_(ll), None, None, None, None, None, p_(status), None)
        rc = lib.bssm_pf_run_batch(ctx.handle, C.byref(cfg), F, p_(thetas), p_(seeds), p_(streams), C.byref(res))
        return rc, lib.bssm_last_error().decode(), ll

    def good_runs():
        rc, _, ll = single(good)
        assert rc == _lib.OK and np.isfinite(ll)
        rc, _, lls = batched(np.stack([good, good]))
        assert rc == _lib.OK and np.all(np.isfinite(lls))
        return {k: v["launches"] for k, v in ctx.get_profile().items()}

    assert _lib.RN_OBS_MODEL["negbin"] == 7
    ctx.set_profile(True)
    try:
        rc, msg, _ = single(pois)                                             # the Poisson block under id 7 ...
        assert rc == _lib.ERR_ARG and "wrong length" in msg, msg
        rc, msg, _ = batched(np.stack([pois, pois]))
        assert rc == _lib.ERR_ARG and "wrong length" in msg, msg
        rc, msg, _ = single(good, model=6)                                    # ... and the negative-binomial block under id 6
        assert rc == _lib.ERR_ARG and "wrong length" in msg, msg
        for bad in (0.0, -1.0, np.nan, np.inf):
            for k in (0, 1):
                blk = good.copy(); blk[o_size + k] = bad
                rc, msg, _ = single(blk)
                assert rc == _lib.ERR_ARG and "sizes size[p] must be finite and > 0" in msg, msg
                rc, msg, _ = batched(np.stack([good, blk]))
                assert rc == _lib.ERR_ARG and "sizes size[p] must be finite and > 0" in msg, msg
        rc, msg, _ = single(good, algorithm="RMPF")
        assert rc == _lib.ERR_ARG and "no move step" in msg, msg
        rc, msg, _ = single(good, rf="multinomial")
        assert rc == _lib.ERR_ARG and "stratified / systematic" in msg, msg
        rc, msg, _ = batched(np.stack([good, good]), rf="multinomial")
        assert rc == _lib.ERR_ARG and "stratified / systematic" in msg, msg
        cap = lib.bssm_pf_batch_max_particles_rn(d)
        assert 1000 <= cap <= 2048
        rc, msg, _ = batched(np.stack([good, good]), N=cap + 1)
        assert rc == _lib.ERR_CAPACITY and "bssm_pf_batch_max_particles_rn" in msg, msg
        # no refused call launched a kernel: nothing is in the profile, and nothing was left pending either -- the profile of the runs
        # that follow is that of the same runs alone
        assert ctx.get_profile() == {}
        after = good_runs()
        ctx.set_profile(True)
        alone = good_runs()
        assert after == alone and sum(alone.values()) > 0
        assert batched(np.stack([good, good]), N=cap)[0] == _lib.OK
    finally:
        ctx.set_profile(False)
