"""The lock-step multi-filter path (bssm_pf_run_multi, bssm_pmmh_chains_multi, multi.hip.h) where the filters of one launch DIVERGE.

Up to four large filters share every launch (blockIdx.y = filter); what stays per filter is the run state (DevState: dead,
do_resample, res_calls, total_bits), the gmax slot, the block records and the X0 / X1 swap the host performs for every filter
whether or not it resampled.  tests/test_gpu_multi.py covers launches whose filters behave alike; here one filter takes the
degenerate early return (R/particle_filter_core.R:189-202) while its neighbours go on, the filters of a launch take different
resample decisions, a PMMH iteration sends only a subset of the chains, the grid has one block / a ragged last block / 512
blocks, and the test aids (record_window, force_fallback, stage_expansion) are set on the multi kernels.

Reference of every filter: bootstrap_filter(..., seed = seeds[k], stream = streams[k], return_particles = False) on a context of
its own with default options -- the path the other GPU modules hold to the oracle.  Bar: BIT IDENTITY of loglike,
loglike_history, ess, state_est, early_return_step and n_res_calls (-inf == -inf counts as equal).  Every call states through
Context.multi_stats() whether it took the lock-step kernels or ran one filter after the other."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = (1 << 20) + 1               # the contexts also hold the first size past the lock-step kernels' reach
PHI, SX = 0.8, 1.0
OT = [1, 1, 2, 5, 5, 6, 9]        # a repeated time at the very start, gaps of 3, a repeated time after a gap


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def refctx(B):
    cx = B.Context(0, CAP, 1)     # default options, never changed: the single path
    yield cx
    cx.close()


@pytest.fixture(scope="module")
def ctxs(B):
    cs = [B.Context(0, CAP, 1) for _ in range(4)]
    yield cs
    for cx in cs:
        cx.close()


def _model(B, name):
    return B.models.linear_gaussian() if name == "lg" else B.models.ar1_sin()


def _simulate(rng, T, sin=False):
    x, ys = rng.standard_normal(), []
    for _ in range(T):
        x = PHI * x + (np.sin(x) if sin else 0.0) + SX * rng.standard_normal(); ys.append(x + rng.standard_normal())
    return np.array(ys)


def _thetas(sigma_ys):
    return np.array([[PHI, SX, sy] for sy in sigma_ys])


def _single(B, refctx, model, ys, N, theta, seed, stream, **kw):
    m = _model(B, model)
    return B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, return_particles=False, seed=int(seed), stream=int(stream),
                              ctx=refctx, phi=theta[0], sigma_x=theta[1], sigma_y=theta[2], **kw)


def _multi(B, cs, model, ys, N, thetas, seeds, streams, path, **kw):
    """one bssm_pf_run_multi call on the contexts cs; `path` = the path it must take, counted on cs[0] and on no other context"""
    m = _model(B, model)
    before = [cx.multi_stats() for cx in cs]
    out = B.bootstrap_filter_multi(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, thetas, seeds, streams, ctxs=cs, **kw)
    after = [cx.multi_stats() for cx in cs]
    other = "sequential" if path == "lockstep" else "lockstep"
    assert after[0][path] == before[0][path] + 1 and after[0][other] == before[0][other], (path, before[0], after[0])
    assert after[1:] == before[1:]
    assert (out["status"] == 0).all()
    return out


def _same(out, k, ref, msg):
    """row k of a multi result against a single-path result: bit identity"""
    assert out["loglike"][k] == ref["loglike"], (msg, k, out["loglike"][k], ref["loglike"])       # (-inf == -inf holds)
    for key in ("loglike_history", "ess", "state_est"):
        np.testing.assert_array_equal(out[key][k], ref[key], err_msg="%s filter %d %s" % (msg, k, key))
    assert out["early_return_step"][k] == ref["_extras"]["early_return_step"], (msg, k)
    assert out["n_res_calls"][k] == ref["_extras"]["n_res_calls"], (msg, k)


# ---- a. deaths at different observations ------------------------------------------------------------------------------------

DEATH_SY = (0.5, 1e3, 1e6, 1e7)
DEATH_STEPS = [3, 6, 0, 0]


def _death_series(model):
    """simulated at sigma_y = 1, then y[2] = 1e6 and y[5] = 1e9: every log-weight is below -1e8 when y^2 / (2 sigma_y^2) > 1e8, so
    sigma_y = 0.5 returns at observation 3 (2e12), sigma_y = 1e3 passes it (5e5) and returns at 6 (5e11), 1e6 and 1e7 pass both
    (5e5, 5e3) -- margins of two orders of magnitude or more, whatever the draws are"""
    ys = _simulate(np.random.default_rng(31), 8, sin=(model == "ar1sin"))
    ys[2], ys[5] = 1e6, 1e9
    return ys


@pytest.mark.parametrize("model", ["lg", "ar1sin"])
@pytest.mark.parametrize("ra,rf", [("SISR", "systematic"), ("SISAR", "stratified")])
@pytest.mark.parametrize("N", [7, 2049, 50001])
def test_deaths_at_different_observations(B, refctx, ctxs, model, ra, rf, N):
    ys = _death_series(model)
    T = len(ys)
    thetas = _thetas(DEATH_SY)
    seeds, streams = [21, 22, 23, 24], [5, 6, 7, 8]
    kw = dict(resample_algorithm=ra, resample_fn=rf)
    refs = [_single(B, refctx, model, ys, N, thetas[k], seeds[k], streams[k], **kw) for k in range(4)]
    # the input condition, taken from the single-path runs
    assert [r["_extras"]["early_return_step"] for r in refs] == DEATH_STEPS
    assert refs[0]["loglike"] == -np.inf and refs[1]["loglike"] == -np.inf
    assert np.isfinite(refs[2]["loglike"]) and np.isfinite(refs[3]["loglike"])
    for k, dead in enumerate(DEATH_STEPS):
        if dead:
            assert (refs[k]["ess"][dead:] == 0).all() and (refs[k]["state_est"][dead:] == 0).all() and (refs[k]["loglike_history"][dead:] == 0).all()
            assert refs[k]["loglike_history"][dead - 1] == -np.inf and np.isfinite(refs[k]["loglike_history"][:dead - 1]).all()
    # the dying filters first (blockIdx.y = 0, 1; ctxs[0] dies), then reversed (blockIdx.y = 3 dies first, ctxs[0] survives)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
        out = _multi(B, ctxs, model, ys, N, thetas[order], [seeds[k] for k in order], [streams[k] for k in order], "lockstep", **kw)
        assert out["early_return_step"].tolist() == [DEATH_STEPS[k] for k in order]
        for row, k in enumerate(order):
            _same(out, row, refs[k], "%s N=%d %s %s order %s" % (model, N, ra, rf, order))
            assert np.isfinite(out["loglike"][row]) == (DEATH_STEPS[k] == 0)
            assert out["ess"].shape == (4, T + 1) and out["loglike_history"].shape == (4, T)


# ---- b. resample decisions that differ within a launch --------------------------------------------------------------------

DIV_SY = (0.05, 1.0, 1e3)
DIV_SEEDS, DIV_STREAMS = [31, 32, 33], [1, 2, 3]


def _divergent_series(model, ot):
    """sigma_y = 0.05: a few particles carry each observation (ESS far below N / 2); sigma_y = 1e3: the weights stay uniform to
    1e-5 (ESS above 0.9 N throughout); sigma_y = 1 in between.  The series (generator seeds 41 / 47) are chosen so that the
    oracle's filter takes these decisions on numpy draws of a dozen seeds at every N below; the tests assert them on the runs
    themselves.  With OT the series is one on which the repeated times resample as well."""
    return _simulate(np.random.default_rng(47 if ot else 41), len(OT) if ot else 10, sin=(model == "ar1sin"))


def _divergent_refs(B, refctx, model, ys, N, rf, ot, thr):
    """the single path with return_ancestors (for `resampled`), and the input conditions on the decisions"""
    thetas = _thetas(DIV_SY)
    kw = dict(resample_algorithm="SISAR", resample_fn=rf, obs_times=ot, threshold=thr)
    refs = [_single(B, refctx, model, ys, N, thetas[k], DIV_SEEDS[k], DIV_STREAMS[k], **kw) for k in range(3)]
    anc = [_single(B, refctx, model, ys, N, thetas[k], DIV_SEEDS[k], DIV_STREAMS[k], return_ancestors=True, **kw) for k in range(3)]
    for r, a in zip(refs, anc):
        assert r["loglike"] == a["loglike"] and (r["_extras"]["resampled"] == a["_extras"]["resampled"]).all()
    dec = np.array([a["_extras"]["resampled"] for a in anc]).astype(bool)
    assert dec[0].all(), ("filter 0 must resample at every observation", dec[0])
    assert not dec[2].any(), ("filter 2 must never resample", dec[2])
    assert (dec.any(axis=0) & ~dec.all(axis=0)).any()                   # an observation at which the three decisions are not all equal
    nres = [r["_extras"]["n_res_calls"] for r in refs]
    assert nres[0] == len(ys) and nres[2] == 0 and nres[0] != nres[2]
    assert nres == dec.sum(axis=1).tolist()
    return thetas, kw, refs


DIV_CASES = [(7, None), (4097, None), (50001, None), (4097, OT)]


@pytest.mark.parametrize("model", ["lg", "ar1sin"])
@pytest.mark.parametrize("rf", ["stratified", "systematic"])
@pytest.mark.parametrize("N,ot", DIV_CASES, ids=["7", "4097", "50001", "4097-obs_times"])
def test_resample_decisions_differ_within_a_launch(B, refctx, ctxs, model, rf, N, ot):
    ys = _divergent_series(model, ot)
    for thr in (None, 0.9 * N):
        thetas, kw, refs = _divergent_refs(B, refctx, model, ys, N, rf, ot, thr)
        out = _multi(B, ctxs[:3], model, ys, N, thetas, DIV_SEEDS, DIV_STREAMS, "lockstep", **kw)
        for k in range(3):
            _same(out, k, refs[k], "%s N=%d %s thr=%s" % (model, N, rf, thr))
        assert len(set(out["n_res_calls"].tolist())) > 1


# ---- c. edges -------------------------------------------------------------------------------------------------------------------

BIG_SEEDS, BIG_STREAMS = [2 ** 40 + 5, 12, 2 ** 40 + 5], [2 ** 33 + 3, 7, 2 ** 33 + 3]       # filters 0 and 2: the same (theta, seed, stream)
EDGE_THETAS = np.array([[0.8, 1.0, 0.7], [0.5, 1.3, 1.1], [0.8, 1.0, 0.7]])


def _edge_case(B, refctx, cs, model, ys, N, ra, rf, path, F=3):
    kw = dict(resample_algorithm=ra, resample_fn=rf)
    out = _multi(B, cs[:F], model, ys, N, EDGE_THETAS[:F], BIG_SEEDS[:F], BIG_STREAMS[:F], path, **kw)
    for k in range(min(F, 2)):
        ref = _single(B, refctx, model, ys, N, EDGE_THETAS[k], BIG_SEEDS[k], BIG_STREAMS[k], **kw)
        _same(out, k, ref, "%s N=%d %s %s" % (model, N, ra, rf))
        if k == 0 and F == 3:
            _same(out, 2, ref, "twin of filter 0")
    if F == 3:
        assert out["loglike"][0] == out["loglike"][2] and out["loglike"][0] != out["loglike"][1]
    assert np.isfinite(out["loglike"]).all()
    return out


@pytest.mark.parametrize("ra,rf", [("SISR", "stratified"), ("SISAR", "systematic")])
@pytest.mark.parametrize("N", [1, 2, 7, 2048, 2049, 4097, (1 << 20) - 777, 1 << 20])
def test_grid_edges_take_the_lockstep_kernels(B, refctx, ctxs, ra, rf, N):
    """one block (1, 2, 7, 2048), two (2049), three (4097), a ragged last block at 512 blocks, 512 full blocks; seeds and streams at or
    above 2^32; two filters of the launch with the same (theta, seed, stream)"""
    T = 5 if N < (1 << 19) else 3
    for model in ("lg", "ar1sin"):
        ys = _simulate(np.random.default_rng(N % 1000 + 1), T, sin=(model == "ar1sin"))
        _edge_case(B, refctx, ctxs, model, ys, N, ra, rf, "lockstep")


@pytest.mark.parametrize("ra,rf", [("SISR", "stratified"), ("SISAR", "systematic")])
def test_past_the_grid_limit_and_one_filter_run_sequentially(B, refctx, ctxs, ra, rf):
    """N = 2^20 + 1 is 513 blocks (the in-kernel resolve holds two records per thread: 512) and F = 1 has nothing to share a launch
    with: both run through bssm_pf_run, are counted as sequential and still equal the single path"""
    ys = _simulate(np.random.default_rng(77), 3)
    _edge_case(B, refctx, ctxs, "lg", ys, (1 << 20) + 1, ra, rf, "sequential")
    ys = _simulate(np.random.default_rng(78), 6, sin=True)
    for N in (7, 4097):
        _edge_case(B, refctx, ctxs, "ar1sin", ys, N, ra, rf, "sequential", F=1)


@pytest.mark.parametrize("ra,rf", [("SISR", "stratified"), ("SISAR", "systematic")])
def test_single_observation(B, refctx, ctxs, ra, rf):
    for N in (1, 7, 2049, 50001):
        for model in ("lg", "ar1sin"):
            out = _edge_case(B, refctx, ctxs, model, np.array([0.4]), N, ra, rf, "lockstep")
            assert out["loglike_history"].shape == (3, 1) and (out["loglike_history"][:, 0] == out["loglike"]).all()


# ---- d. against the oracle directly ---------------------------------------------------------------------------------------------

def _oracle_rows(B, oracle, refctx, model, ys, N, thetas, seeds, streams, rf, **kw):
    T = len(ys)
    rows = []
    for k in range(len(thetas)):
        d = B.dump_draws("BPF", T, N, rf, seeds[k], streams[k], obs_times=kw.get("obs_times"), ctx=refctx)       # filter k's own generator stream
        rows.append(oracle.pf_run(model, thetas[k], ys, N, d["z_init"], d["z_trans"], d["u_res"], resample_fn=rf, **kw))
    return rows


def _near(out, k, ref, msg):
    """the project's bar against the oracle (tests/test_gpu_filter.py): log-likelihood 1e-6 relative"""
    assert out["early_return_step"][k] == ref["early_return_step"], msg
    assert out["n_res_calls"][k] == ref["n_res_calls"], msg
    if np.isfinite(ref["loglike"]):
        assert abs(out["loglike"][k] - ref["loglike"]) <= 1e-6 * abs(ref["loglike"]), (msg, out["loglike"][k], ref["loglike"])
    else:
        assert out["loglike"][k] == ref["loglike"], msg
    np.testing.assert_allclose(out["loglike_history"][k], ref["loglike_history"], rtol=1e-6, atol=1e-12, err_msg=msg)
    np.testing.assert_allclose(out["ess"][k], ref["ess"], rtol=1e-6, err_msg=msg)
    np.testing.assert_allclose(out["state_est"][k], ref["state_est"], rtol=1e-6, atol=1e-8, err_msg=msg)


@pytest.mark.parametrize("model", ["lg", "ar1sin"])
def test_deaths_against_the_oracle(B, oracle, refctx, ctxs, model):
    N, ra, rf = 4097, "SISAR", "stratified"
    ys = _death_series(model)
    thetas, seeds, streams = _thetas(DEATH_SY), [21, 22, 23, 24], [5, 6, 7, 8]
    refs = _oracle_rows(B, oracle, refctx, model, ys, N, thetas, seeds, streams, rf, resample_algorithm=ra)
    assert [r["early_return_step"] for r in refs] == DEATH_STEPS               # the oracle alone: the input condition
    out = _multi(B, ctxs, model, ys, N, thetas, seeds, streams, "lockstep", resample_algorithm=ra, resample_fn=rf)
    for k in range(4):
        _near(out, k, refs[k], "%s filter %d" % (model, k))
    assert np.isfinite(out["loglike"][2:]).all()
    for k in range(4):       # `resampled` is not among the multi call's outputs: the single path (bit-identical above) carries it
        one = _single(B, refctx, model, ys, N, thetas[k], seeds[k], streams[k], resample_algorithm=ra, resample_fn=rf, return_ancestors=True)
        assert (one["_extras"]["resampled"] == refs[k]["resampled"]).all()
        _same(out, k, one, "single path")


@pytest.mark.parametrize("model,ot", [("lg", None), ("ar1sin", OT)], ids=["lg", "ar1sin-obs_times"])
def test_divergent_decisions_against_the_oracle(B, oracle, refctx, ctxs, model, ot):
    N, rf = 4097, "systematic"
    ys = _divergent_series(model, ot)
    for thr in (None, 0.9 * N):
        thetas, kw, ones = _divergent_refs(B, refctx, model, ys, N, rf, ot, thr)
        okw = {k: v for k, v in kw.items() if k != "resample_fn"}
        refs = _oracle_rows(B, oracle, refctx, model, ys, N, thetas, DIV_SEEDS, DIV_STREAMS, rf, **okw)
        dec = np.array([r["resampled"] for r in refs]).astype(bool)
        assert dec[0].all() and not dec[2].any()                                   # the oracle alone: the input condition
        out = _multi(B, ctxs[:3], model, ys, N, thetas, DIV_SEEDS, DIV_STREAMS, "lockstep", **kw)
        for k in range(3):
            _near(out, k, refs[k], "%s filter %d thr=%s" % (model, k, thr))
            assert (ones[k]["_extras"]["resampled"] == refs[k]["resampled"]).all()
            _same(out, k, ones[k], "single path")


# ---- e. test aids on the multi kernels ----------------------------------------------------------------------------------------

AIDS = [("record_window", 1, 0), ("force_fallback", 1, 0), ("force_fallback", 2, 0), ("force_fallback", 5, 0), ("stage_expansion", 0, 1)]


@pytest.mark.parametrize("name,value,default", AIDS, ids=["%s=%d" % (n, v) for n, v, _ in AIDS])
@pytest.mark.parametrize("N", [2049, 50001])
def test_test_aids_on_the_multi_kernels(B, refctx, name, value, default, N):
    """the same value on every context keeps the lock-step kernels (which read it); the results are the default single path's"""
    cs = [B.Context(0, N, 1) for _ in range(3)]
    try:
        for model, rf in (("lg", "stratified"), ("ar1sin", "systematic")):
            ys = _divergent_series(model, None)
            thetas, kw, refs = _divergent_refs(B, refctx, model, ys, N, rf, None, None)
            for cx in cs:
                cx.set_option(name, value)
            out = _multi(B, cs, model, ys, N, thetas, DIV_SEEDS, DIV_STREAMS, "lockstep", **kw)
            for k in range(3):
                _same(out, k, refs[k], "%s = %d on all, %s N=%d" % (name, value, model, N))
    finally:
        for cx in cs:
            try:
                cx.set_option(name, default)
            finally:
                cx.close()


@pytest.mark.parametrize("name,value,default", [("stage_expansion", 0, 1), ("record_window", 1, 0)], ids=["stage_expansion", "record_window"])
@pytest.mark.parametrize("N", [2049, 50001])
def test_test_aids_that_differ_between_contexts_run_sequentially(B, refctx, name, value, default, N):
    cs = [B.Context(0, N, 1) for _ in range(3)]
    try:
        ys = _divergent_series("lg", None)
        thetas, kw, refs = _divergent_refs(B, refctx, "lg", ys, N, "stratified", None, None)
        for odd in (1, 0):                               # the odd one out is a later context, then ctxs[0] itself
            for j, cx in enumerate(cs):
                cx.set_option(name, value if j == odd else default)
            out = _multi(B, cs, "lg", ys, N, thetas, DIV_SEEDS, DIV_STREAMS, "sequential", **kw)
            for k in range(3):
                _same(out, k, refs[k], "%s differs on context %d, N=%d" % (name, odd, N))
    finally:
        for cx in cs:
            try:
                cx.set_option(name, default)
            finally:
                cx.close()


# ---- f. PMMH iterations that send a subset of the chains ---------------------------------------------------------------------

def _prior(B, kind, a, b):
    return {"normal": lambda: B.prior_normal(a, b), "uniform": lambda: B.prior_uniform(a, b), "exponential": lambda: B.prior_exponential(a),
            "flat": lambda: B.prior_flat()}[kind]()


def _pmmh_case(B, oracle, refctx, ys, N, m_it, inits, covs, tr, kinds, seeds, ra, rf):
    """K chains through bssm_pmmh_chains_multi; per chain the oracle's loop over the DEVICE filter (it records the iterations that
    ran one) on the chain's own draws, and run_chain_device.  Returns the multi results and, per iteration, how many chains ran a filter."""
    from bayesssm_amd.pmmh import run_chain_device, run_chains_multi_device, chain_draws
    K, T = len(inits), len(ys)
    priors = [_prior(B, *k) for k in kinds]
    m = B.models.linear_gaussian()
    cs = [B.Context(0, N, 1) for _ in range(K)]
    try:
        outs = run_chains_multi_device(ys, m_it, "lg", 3, inits, covs, tr, priors, N, seeds, list(range(K)), cs, None, ra, rf, True)
        stats = [cx.multi_stats() for cx in cs]
    finally:
        for cx in cs:
            cx.close()
    ran = np.zeros(m_it, dtype=int)
    for k in range(K):
        its = []

        def pf(th, it, k=k, its=its):
            its.append(it)
            r = B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, return_particles=False, seed=seeds[k], stream=(k << 32) | it,
                                   resample_algorithm=ra, resample_fn=rf, ctx=refctx, phi=th[0], sigma_x=th[1], sigma_y=th[2])
            return r["loglike"], r["state_est"]

        d = chain_draws(seeds[k], k, m_it, 3)
        ref = oracle.pmmh_chain(pf, m_it, inits[k], covs[k], tr, kinds, d["z_prop"], d["u_accept"], se_len=T + 1)
        assert len(set(its)) == len(its) == ref["pf_calls"]
        ran[its] += 1
        one = run_chain_device(pf_wrapper=B.bootstrap_filter, y=ys, m=m_it, model="lg", n_params=3, init_theta=inits[k], proposal_cov=covs[k],
                               transform=tr, priors=priors, num_particles=N, seed=seeds[k], chain_index=k, resample_algorithm=ra, resample_fn=rf,
                               return_latent_state_est=True, ctx=refctx)
        for r, what in ((one, "run_chain_device"), (ref, "oracle loop")):
            for key in ("theta_chain", "loglike_chain", "state_est_chain"):
                np.testing.assert_array_equal(outs[k][key], r[key], err_msg="chain %d %s vs %s" % (k, key, what))
            assert outs[k]["accepted"] == r["accepted"], (k, what)
    # which path each iteration took: counted on the first context SENT, so summed over the contexts
    assert sum(s["lockstep"] for s in stats) == int((ran >= 2).sum())
    assert sum(s["sequential"] for s in stats) == int((ran == 1).sum())
    return outs, ran


def test_pmmh_iterations_send_subsets_of_the_chains(B, oracle, refctx):
    """phi has a narrow uniform prior (identity transform): a proposal outside it is rejected before any filter runs (R/pmmh.R
    :435-442), so an iteration sends 0, 1, 2 or 3 of the chains.  With proposal sd 0.2 against a support of width 0.3 about half
    of the proposals stay inside whatever the chain did before, and seeds 301 .. 303 give every subset size several times under
    stand-in filters on the CPU; the run itself is held to it below."""
    ys = _simulate(np.random.default_rng(9), 12)
    kinds = [("uniform", 0.6, 0.9), ("exponential", 1.0, 0.0), ("exponential", 1.0, 0.0)]
    inits = [[0.7, 1.0, 1.0], [0.75, 0.8, 1.2], [0.8, 1.2, 0.9]]
    m_it = 40
    outs, ran = _pmmh_case(B, oracle, refctx, ys, 4097, m_it, inits, [np.diag([0.04, 0.02, 0.02])] * 3, ["identity", "log", "log"], kinds,
                           [301, 302, 303], "SISAR", "stratified")
    assert ran[0] == 3
    assert {0, 1, 2, 3} <= set(ran[1:].tolist()), np.bincount(ran[1:], minlength=4)        # the input condition
    for o in outs:
        assert ((o["theta_chain"][:, 0] >= 0.6) & (o["theta_chain"][:, 0] <= 0.9)).all() and 0 < o["accepted"] < m_it - 1


def test_pmmh_one_chain_whose_filters_all_die(B, oracle, refctx):
    """y[4] = 1e9: chain 1 (sigma_y about 0.5) loses every filter at observation 5, so its acceptance ratio is (-Inf) - (-Inf) = NaN at
    every iteration and the NA guard (R/pmmh.R:488-490) keeps it in place; chains 0 and 2 (sigma_y about 1e6: 1e18 / 2e12 = 5e5) move"""
    ys = _simulate(np.random.default_rng(10), 8)
    ys[4] = 1e9
    kinds = [("normal", 0.0, 1.0), ("exponential", 1.0, 0.0), ("flat", 0.0, 0.0)]
    inits = [[0.7, 1.0, 1e6], [0.7, 1.0, 0.5], [0.6, 1.2, 2e6]]
    m_it = 12
    outs, ran = _pmmh_case(B, oracle, refctx, ys, 4097, m_it, inits, [np.diag([0.01, 0.01, 0.01])] * 3, ["identity", "log", "log"], kinds,
                           [11, 12, 13], "SISR", "systematic")
    assert (ran == 3).all()
    assert outs[1]["accepted"] == 0 and (outs[1]["loglike_chain"] == -np.inf).all() and (outs[1]["theta_chain"] == np.array(inits[1])).all()
    for k in (0, 2):
        assert outs[k]["accepted"] > 0 and np.isfinite(outs[k]["loglike_chain"]).all()
