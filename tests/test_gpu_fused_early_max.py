"""Fused launch, option `fused_early_max`: the global max M of the log-weights is broadcast ahead of (M, S, status) and the
workers take exp(lw - M) in the wait for S (bayesssm_amd/csrc/fused.hip.h, duty 1 in two steps).

No arithmetic changes -- the same exp_nonpos on the same arguments, the same quotient, every sum in its old association order -- so
`fused = 2` with `fused_early_max = 1` must be BIT-EQUAL to `fused = 2` with `fused_early_max = 0` and to `fused = 0` (the
multi-launch path, which the other GPU modules hold to the oracle): loglike, loglike_history, ess, state_est, ancestors.
fused_stats must show that the fused launches ran, with no time-out.

The shapes are the smallest at which the two-step exchange can go wrong: one block with a partial lane (the resolver is the only
worker and waits on its own M line), a second block that is nearly empty (its out-of-range lanes stay 0.0), L = 1 with the
8-byte gather form, more than 256 blocks (the pair form, two records per resolver thread), observations that do not resample
(the carry-over branch reads v[] after the division), a degenerate observation (M < -1e8: the M line is written on the DEAD
exit) and the tag wrap with the new line in the workspace.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("loglike_history", "ess", "state_est")


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def cx(B):
    c = B.Context(0, (1 << 19) + 2048, 1)
    yield c
    c.close()


def _simulate(rng, T, sin=False):
    x, ys = rng.standard_normal(), []
    for _ in range(T):
        x = 0.8 * x + (np.sin(x) if sin else 0.0) + rng.standard_normal()
        ys.append(x + rng.standard_normal())
    return np.array(ys)


def _three(cx, run):
    """(early_max = 1, early_max = 0, multi-launch) and how many fused launches / time-outs the two fused runs made"""
    outs, launches = [], []
    for fused, early in ((2, 1), (2, 0), (0, 0)):
        cx.set_option("fused", fused)
        cx.set_option("fused_early_max", early)
        before = cx.fused_stats()
        outs.append(run())
        after = cx.fused_stats()
        launches.append(after["launches"] - before["launches"])
        assert after["timeouts"] == before["timeouts"], (fused, early, after)
    assert launches[0] > 0 and launches[0] == launches[1] and launches[2] == 0, launches
    return outs


def _equal(a, b2, msg):
    assert (a["loglike"] == b2["loglike"]) or (np.isinf(a["loglike"]) and np.isinf(b2["loglike"])), (msg, a["loglike"], b2["loglike"])
    for key in KEYS:
        np.testing.assert_array_equal(a[key], b2[key], err_msg="%s %s" % (msg, key))
    np.testing.assert_array_equal(a["_extras"]["ancestors"], b2["_extras"]["ancestors"], err_msg="%s ancestors" % msg)
    assert a["_extras"]["early_return_step"] == b2["_extras"]["early_return_step"], msg
    assert (a["_extras"]["resampled"] == b2["_extras"]["resampled"]).all(), msg


def _check(cx, run, msg):
    e1, e0, ml = _three(cx, run)
    _equal(e1, e0, msg + " early_max 1 vs 0")
    _equal(e1, ml, msg + " early_max 1 vs multi-launch")
    return e1


SHAPES = [
    # N, T, obs_times
    (50, 8, None),
    (2049, 8, None),
    (3 * 2048 + 7, 7, [1, 2, 4, 4, 7, 8, 11]),        # gaps > 1 and a repeated time
    (1 << 16, 6, None),
    ((1 << 19) + 2048, 3, None),
]


@pytest.mark.parametrize("rf", ["systematic", "stratified"])
@pytest.mark.parametrize("model", ["lg", "ar1sin"])
def test_early_max_bit_equal(B, cx, model, rf):
    rng = np.random.default_rng(1700 + (model == "lg") + 2 * (rf == "systematic"))
    m = B.models.linear_gaussian() if model == "lg" else B.models.ar1_sin()
    for N, T, ot in SHAPES:
        ys = _simulate(rng, T, sin=(model == "ar1sin"))
        kw = dict(resample_algorithm="SISR", resample_fn=rf, return_particles=False, return_ancestors=True, obs_times=ot, seed=17, stream=N % 1000,
                  ctx=cx, phi=0.8, sigma_x=1.0, sigma_y=0.7)
        r = _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "%s %s N=%d" % (model, rf, N))
        assert r["_extras"]["resampled"].all() and np.isfinite(r["loglike"])


@pytest.mark.parametrize("rf", ["systematic", "stratified"])
@pytest.mark.parametrize("model", ["lg", "ar1sin"])
def test_early_max_carry_over_branch(B, cx, model, rf):
    """An ESS threshold of N / 2 with flat weights (sigma_y = 2) and two outlying observations: some observations resample, the others
    carry their particles over -- the branch that reads v[] after the division by S."""
    rng = np.random.default_rng(1710)
    m = B.models.linear_gaussian() if model == "lg" else B.models.ar1_sin()
    for N in (2049, 3 * 2048 + 7):
        ys = _simulate(rng, 8, sin=(model == "ar1sin"))
        ys[2] += 9.0; ys[5] -= 9.0
        kw = dict(resample_algorithm="SISAR", threshold=0.5 * N, resample_fn=rf, return_particles=False, return_ancestors=True, seed=18, stream=3,
                  ctx=cx, phi=0.8, sigma_x=1.0, sigma_y=2.0)
        r = _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "%s %s SISAR N=%d" % (model, rf, N))
        rs = r["_extras"]["resampled"]
        assert rs.any() and not rs.all(), rs


def test_early_max_resample_move(B, cx):
    rng = np.random.default_rng(1720)
    m = B.models.linear_gaussian()
    ys = _simulate(rng, 6)
    kw = dict(resample_fn="systematic", return_ancestors=True, seed=19, stream=4, ctx=cx, phi=0.8, sigma_x=1.0, sigma_y=0.6)
    _check(cx, lambda: B.resample_move_filter(ys, 3 * 2048 + 7, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.rw_move_fn(0.3), **kw), "rmpf")


@pytest.mark.parametrize("N", [50, 2049])
def test_early_max_degenerate_observation(B, cx, N):
    """One observation 1e5 sigma_y away: every log-weight is about -5e9 < -1e8, the filter returns early at that observation.  The resolver
    writes the M line on that exit too: no time-out, same early return on every path."""
    rng = np.random.default_rng(1730)
    m = B.models.linear_gaussian()
    ys = _simulate(rng, 7)
    ys[3] = 1e5
    kw = dict(resample_algorithm="SISR", resample_fn="systematic", return_particles=False, return_ancestors=True, seed=20, stream=5, ctx=cx,
              phi=0.8, sigma_x=1.0, sigma_y=1.0)
    r = _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "degenerate N=%d" % N)
    assert r["_extras"]["early_return_step"] == 4 and r["loglike"] == -np.inf


def test_early_max_tag_wrap(B, cx):
    """fused_tag = -3: the launch counter wraps at the third launch and the workspace -- the M line included -- is zeroed in the stream."""
    rng = np.random.default_rng(1740)
    m = B.models.linear_gaussian()
    ys = _simulate(rng, 8)
    N = 3 * 2048 + 7
    kw = dict(resample_algorithm="SISR", resample_fn="stratified", return_particles=False, return_ancestors=True, seed=21, stream=6, ctx=cx,
              phi=0.8, sigma_x=1.0, sigma_y=0.7)

    def run():
        cx.set_option("fused_tag", -3)
        return B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw)
    _check(cx, run, "tag wrap")
