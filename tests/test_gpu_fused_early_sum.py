"""Fused launch, first exchange: S on a line of its own ahead of (M, S, status), the head block without its prefix wait, the
resolver's own answers from LDS and its bookkeeping behind its W record (bayesssm_amd/csrc/fused.hip.h, the `early_max != 0` path).

Nothing of this changes an operation or an operand -- only when values cross workgroups and which values a workgroup reads from
its own chip -- so every case runs three ways, `fused = 2` with `fused_early_max = 1`, `fused = 2` with `fused_early_max = 0`
(the path that stays as it was) and `fused = 0` (the multi-launch path, which the other GPU modules hold to the oracle), and every
returned array must be equal BIT FOR BIT.

The shapes are the smallest at which each new path can go wrong (2048 particles a block, the resolver is block 5B/16):
  N = 50, 2048      B = 1    the resolver IS block 0: no a1 wait and the LDS hand-over in the same workgroup
  N = 2049          B = 2    resolver is block 0, ragged last block
  N = 4*2048 + 5    B = 5    resolver is block 1: block 0 and the resolver are distinct, the resolver's prefix is in thread 1, not 0
  N = 17*2048       B = 17   resolver is block 5; several lanes hold records
  N = 2^16 + 3      B = 33   the gather takes the paired form across waves
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("state_est", "ess", "loglike_history")
SHAPES = [50, 2048, 2049, 4 * 2048 + 5, 17 * 2048, (1 << 16) + 3]
OBS_TIMES = [1, 2, 2, 4, 5, 7, 8, 8]          # a repeated time (no transition) and gaps of 2


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def cx(B):
    c = B.Context(0, 1 << 17, 1)
    yield c
    c.close()


def _simulate(rng, T, sin=False):
    x, ys = rng.standard_normal(), []
    for _ in range(T):
        x = 0.8 * x + (np.sin(x) if sin else 0.0) + rng.standard_normal()
        ys.append(x + rng.standard_normal())
    return np.array(ys)


def _model(B, model):
    return B.models.linear_gaussian() if model == "lg" else B.models.ar1_sin()


def _three(cx, run):
    """(early_max = 1, early_max = 0, multi-launch) results and the fused_stats difference of each of the three runs"""
    outs, deltas = [], []
    try:
        for fused, early in ((2, 1), (2, 0), (0, 0)):
            cx.set_option("fused", fused)
            cx.set_option("fused_early_max", early)
            before = cx.fused_stats()
            outs.append(run())
            after = cx.fused_stats()
            deltas.append({k: after[k] - before[k] for k in after})
            assert deltas[-1]["timeouts"] == 0, (fused, early, after)
    finally:
        cx.set_option("fused", 1)
        cx.set_option("fused_early_max", 1)
    assert deltas[0]["launches"] > 0 and deltas[0]["launches"] == deltas[1]["launches"] and deltas[2]["launches"] == 0, deltas
    return outs, deltas


def _equal(a, b2, msg, histories=False):
    assert np.float64(a["loglike"]).tobytes() == np.float64(b2["loglike"]).tobytes(), (msg, a["loglike"], b2["loglike"])
    for key in KEYS + (("particles_history", "weights_history") if histories else ()):
        assert a[key].shape == b2[key].shape and a[key].tobytes() == b2[key].tobytes(), (msg, key)
    for key in ("resampled", "ancestors"):
        assert np.array_equal(a["_extras"][key], b2["_extras"][key]), (msg, key)
    assert a["_extras"]["early_return_step"] == b2["_extras"]["early_return_step"], msg


def _check(cx, run, msg, histories=False, stand_down=False):
    (e1, e0, ml), deltas = _three(cx, run)
    _equal(e1, e0, msg + ": early_max 1 vs 0", histories)
    _equal(e1, ml, msg + ": early_max 1 vs multi-launch", histories)
    if stand_down:
        assert deltas[0]["stand_downs"] == 1 and deltas[1]["stand_downs"] == 1, (msg, "the run did not stand down", deltas)
    else:
        assert deltas[0]["stand_downs"] == 0 and deltas[1]["stand_downs"] == 0, (msg, deltas)
    return e1


@pytest.mark.parametrize("rf", ["systematic", "stratified"])
@pytest.mark.parametrize("model", ["lg", "ar1sin"])
def test_early_sum_sisr(B, cx, model, rf):
    rng = np.random.default_rng(1900 + (model == "lg") + 2 * (rf == "systematic"))
    m = _model(B, model)
    for N in SHAPES:
        ys = _simulate(rng, 10, sin=(model == "ar1sin"))
        kw = dict(resample_algorithm="SISR", resample_fn=rf, return_particles=False, return_ancestors=True, seed=19, stream=N % 1000, ctx=cx,
                  phi=0.8, sigma_x=1.0, sigma_y=0.7)
        r = _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "%s %s SISR N=%d" % (model, rf, N))
        assert r["_extras"]["resampled"].all() and np.isfinite(r["loglike"])


@pytest.mark.parametrize("rf", ["systematic", "stratified"])
@pytest.mark.parametrize("model", ["lg", "ar1sin"])
def test_early_sum_sisar_mixed(B, cx, model, rf):
    """ESS threshold N / 2, flat weights (sigma_y = 2) and two outlying observations: some observations resample, the others leave on
    the carry-over exit, where the resolver's bookkeeping runs in front of the return instead of behind duty 1."""
    rng = np.random.default_rng(1910)
    m = _model(B, model)
    for N in SHAPES:
        ys = _simulate(rng, 8, sin=(model == "ar1sin"))
        ys[2] += 9.0; ys[5] -= 9.0
        kw = dict(resample_algorithm="SISAR", threshold=0.5 * N, resample_fn=rf, return_particles=False, return_ancestors=True, seed=20, stream=3,
                  ctx=cx, phi=0.8, sigma_x=1.0, sigma_y=2.0)
        r = _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "%s %s SISAR N=%d" % (model, rf, N))
        rs = np.asarray(r["_extras"]["resampled"])
        assert rs.any() and not rs.all(), (N, rs)


@pytest.mark.parametrize("rf", ["systematic", "stratified"])
@pytest.mark.parametrize("model", ["lg", "ar1sin"])
def test_early_sum_sis(B, cx, model, rf):
    rng = np.random.default_rng(1920)
    m = _model(B, model)
    for N in SHAPES:
        ys = _simulate(rng, 6, sin=(model == "ar1sin"))
        kw = dict(resample_algorithm="SIS", resample_fn=rf, return_particles=False, return_ancestors=True, seed=21, stream=4, ctx=cx,
                  phi=0.8, sigma_x=1.0, sigma_y=1.5)
        r = _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "%s %s SIS N=%d" % (model, rf, N))
        assert not np.asarray(r["_extras"]["resampled"]).any()


@pytest.mark.parametrize("rf", ["systematic", "stratified"])
@pytest.mark.parametrize("model", ["lg", "ar1sin"])
def test_early_sum_obs_times(B, cx, model, rf):
    rng = np.random.default_rng(1930)
    m = _model(B, model)
    for N in SHAPES:
        ys = _simulate(rng, len(OBS_TIMES), sin=(model == "ar1sin"))
        kw = dict(resample_algorithm="SISR", resample_fn=rf, return_particles=False, return_ancestors=True, obs_times=OBS_TIMES, seed=22, stream=5,
                  ctx=cx, phi=0.8, sigma_x=1.0, sigma_y=0.7)
        _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "%s %s obs_times N=%d" % (model, rf, N))


@pytest.mark.parametrize("ra", ["SISR", "SISAR"])
def test_early_sum_histories_and_ancestors(B, cx, ra):
    """B = 5: particles, weights (w_out is written behind the status test, from the quotients taken in the wait) and ancestors."""
    rng = np.random.default_rng(1940)
    m = _model(B, "lg")
    N = 4 * 2048 + 5
    ys = _simulate(rng, 9)
    ys[4] += 9.0
    kw = dict(resample_algorithm=ra, threshold=0.5 * N, resample_fn="stratified", return_particles=True, return_ancestors=True, seed=23, stream=6,
              ctx=cx, phi=0.8, sigma_x=1.0, sigma_y=2.0)
    r = _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "histories " + ra, histories=True)
    assert r["particles_history"].size >= N * len(ys) and r["weights_history"].size >= N * len(ys)


@pytest.mark.parametrize("N", [50, 2049, 4 * 2048 + 5, 17 * 2048])
def test_early_sum_degenerate_observation(B, cx, N):
    """One observation 1e5 sigma_y away: every log-weight is about -5e9 < -1e8 and the filter returns early there.  The resolver writes the
    M line, the S line (S = 0) and c1 on that exit too: no time-out, the same early return on every path."""
    rng = np.random.default_rng(1950)
    m = _model(B, "lg")
    ys = _simulate(rng, 7)
    ys[3] = 1e5
    kw = dict(resample_algorithm="SISR", resample_fn="systematic", return_particles=False, return_ancestors=True, seed=24, stream=7, ctx=cx,
              phi=0.8, sigma_x=1.0, sigma_y=1.0)
    r = _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "degenerate N=%d" % N)
    assert r["_extras"]["early_return_step"] == 4 and r["loglike"] == -np.inf


@pytest.mark.parametrize("force", [1, 2])
@pytest.mark.parametrize("N", [4 * 2048 + 5, 17 * 2048])
def test_early_sum_force_fallback(B, cx, N, force):
    """The resolve's exact fallbacks forced (1: serial walk, 2: general routine): a fused launch that reaches the last block's side entry
    that way voids itself and the run is repeated on the multi-launch path -- the same result either way."""
    rng = np.random.default_rng(1960 + force)
    m = _model(B, "ar1sin")
    ys = _simulate(rng, 6, sin=True)
    kw = dict(resample_algorithm="SISR", resample_fn="systematic", return_particles=False, return_ancestors=True, seed=25, stream=8, ctx=cx,
              phi=0.8, sigma_x=1.0, sigma_y=0.7)

    def run():
        cx.set_option("force_fallback", force)
        try:
            return B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw)
        finally:
            cx.set_option("force_fallback", 0)
    (e1, e0, ml), deltas = _three(cx, run)
    _equal(e1, e0, "force_fallback %d: early_max 1 vs 0" % force)
    _equal(e1, ml, "force_fallback %d: early_max 1 vs multi-launch" % force)
    assert deltas[0]["stand_downs"] == deltas[1]["stand_downs"], deltas


def test_early_sum_stand_down_small_sigma_y(B, cx):
    """sigma_y = 0.05 at B = 17: the weights span hundreds of binades, a block's record needs more than the in-launch records carry, the run
    stands down (bssm_ctx_fused_stats) and is repeated unfused -- with the unfused result."""
    rng = np.random.default_rng(8)
    m = _model(B, "lg")
    N = 17 * 2048
    ys = _simulate(rng, 8)
    kw = dict(resample_algorithm="SISR", resample_fn="systematic", return_particles=False, return_ancestors=True, seed=13, stream=N, ctx=cx,
              phi=0.8, sigma_x=1.0, sigma_y=0.05)
    _check(cx, lambda: B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw), "stand-down", stand_down=True)
