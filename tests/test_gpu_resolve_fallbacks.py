"""The exact-scan resolver's fallbacks, forced, against the oracle and against the same run without forcing.

The resolver (kernels.hip.h resolve_in_block / k_resolve, and the fused launch's resolver duty) turns the per-block records
into the exact sequential state entering every block.  Where the records do not cover a state it has two exact fallbacks:
the serial walk (one lane steps every block with block_out_exact) and the general routine for one link (a block whose side
entry fast path misses).  Ordinary runs almost never take them, so the option `force_fallback` takes them on purpose:
  1  every resolve takes the serial walk          2  every block with a side entry takes the general routine
  4  (with 1 or 2) only in the sum(w) pass
Both are exact, so a forced run must return BIT FOR BIT what the unforced run returns -- ancestors and weight histories
included: a wrong sum(w) shows first in the ancestors -- and equal the oracle (R/particle_filter_core.R:33-266,
src/resampling.cpp:16-66 restated in oracle/bssm_oracle.c).

A fused launch (fused.hip.h) fetches the last block's single side entry into the walk's LDS slot only; both fallbacks read
it from the resolver's private list, which that launch never wrote.  A fallback that reaches that block therefore voids the
launch (LIT_FROM_W): the run stands down and is repeated on the multi-launch path, with the same result.

Last: the fused path's launch counter (the tag every granule on the wire carries) wrapping past 2^32 - 1.
"""
import zlib

import numpy as np
import pytest

from test_gpu_resample import _weights

pytestmark = pytest.mark.gpu

FF_WALK, FF_GENERAL, FF_SUM_ONLY = 1, 2, 4


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


# ---------------------------------------------------------------------------------------------------------------------
# resampler level (multi-launch kernels)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rctx(B):
    cx = B.Context(0, 1 << 22, 1)
    yield cx
    cx.close()


#   B = 1, 1, 1, 1, 2, 3, 512, 513, 2048 blocks of 2048 weights: the in-kernel resolve (B <= 512), k_resolve_all
#   (512 < B <= 2048) and, with inkernel_resolve = 0, k_resolve
SIZES = [1, 2, 2047, 2048, 2049, 4097, 1 << 20, (1 << 20) + 1, 1 << 22]
KINDS = ["uniformish", "skewed", "sparse", "range", "ties"]


@pytest.mark.parametrize("inkernel", [1, 0])
@pytest.mark.parametrize("force", [FF_WALK, FF_GENERAL])
@pytest.mark.parametrize("n", SIZES)
def test_resampler_forced_fallback_vs_oracle(B, rctx, oracle, n, force, inkernel):
    rng = np.random.default_rng(n + 10 * force + inkernel)
    rctx.set_option("inkernel_resolve", inkernel)
    rctx.set_option("force_fallback", force)
    try:
        for kind in KINDS:
            w = _weights(rng, n, kind)
            U = rng.random()
            got, cum, stats = B.resample_systematic_cpp(n, w, U=U, ctx=rctx, return_cum=True, return_stats=True)
            want, wcum = oracle.resample_systematic(n, w, U, return_cum=True)
            assert cum.tobytes() == wcum.tobytes(), (kind, "systematic cum_sum")
            assert (got == want).all(), (kind, "systematic ancestors")
            if force & FF_WALK:
                assert int(stats[1]) > 0, (kind, "the serial walk did not run", stats)
            Us = rng.random(n)
            got, cum, stats = B.resample_stratified_cpp(n, w, U=Us, ctx=rctx, return_cum=True, return_stats=True)
            want, wcum = oracle.resample_stratified(n, w, Us, return_cum=True)
            assert cum.tobytes() == wcum.tobytes(), (kind, "stratified cum_sum")
            assert (got == want).all(), (kind, "stratified ancestors")
            if force & FF_WALK:
                assert int(stats[1]) > 0, (kind, "the serial walk did not run", stats)
    finally:
        rctx.set_option("force_fallback", 0)
        rctx.set_option("inkernel_resolve", 1)


def test_force_fallback_option_range(B, rctx):
    for bad in (-1, 8):
        with pytest.raises(B.BssmError):
            rctx.set_option("force_fallback", bad)


# ---------------------------------------------------------------------------------------------------------------------
# filter level: injected draws, histories and ancestors
# ---------------------------------------------------------------------------------------------------------------------
FILTER_N = [2049, 50001, (1 << 20) - 777, 1 << 20]
T_FILTER = 6
THETA = (0.8, 1.0, 0.5)          # sigma_y = 0.5: SISAR resamples at most observations as well
_CASES = {}


@pytest.fixture(scope="module")
def fctx(B):
    cx = B.Context(0, 1 << 20, 1)
    yield cx
    cx.close()


def _simulate(rng, T, sin):
    phi, sx, sy = THETA
    x, ys = rng.standard_normal(), []
    for _ in range(T):
        x = phi * x + (np.sin(x) if sin else 0.0) + sx * rng.standard_normal()
        ys.append(x + sy * rng.standard_normal())
    return np.array(ys)


def _run(B, cx, case, fused, force):
    model, ra, rf, N, ys, d = case["key"] + (case["ys"], case["draws"])
    m = B.models.linear_gaussian() if model == "lg" else B.models.ar1_sin()
    cx.set_option("fused", fused)
    cx.set_option("force_fallback", force)
    try:
        return B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm=ra, resample_fn=rf,
                                  return_particles=True, return_ancestors=True, draws=d, ctx=cx,
                                  phi=THETA[0], sigma_x=THETA[1], sigma_y=THETA[2])
    finally:
        cx.set_option("force_fallback", 0)
        cx.set_option("fused", 1)


def _case(B, cx, oracle, model, ra, rf, N):
    """(series, draws, oracle result, unforced multi-launch result), computed once per configuration"""
    key = (model, ra, rf, N)
    if key not in _CASES:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        ys = _simulate(rng, T_FILTER, model == "ar1sin")
        mt, mr = oracle.noise_shape("BPF", T_FILTER, None)
        d = {"z_init": rng.standard_normal(N), "z_trans": rng.standard_normal((mt, N)),
             "u_res": rng.random((mr, 1 if rf == "systematic" else N))}
        ref = oracle.pf_run(model, THETA, ys, N, d["z_init"], d["z_trans"], d["u_res"], resample_algorithm=ra, resample_fn=rf,
                            return_ancestors=True, return_particles=True)
        assert ref["n_res_calls"] >= 1, "the case must resample at least once"
        case = {"key": key, "ys": ys, "draws": d, "ref": ref}
        case["base"] = _run(B, cx, case, 0, 0)
        _CASES.clear()                 # (one configuration at a time: the draws and histories of 2^20 particles are large)
        _CASES[key] = case
    return _CASES[key]


def _bitwise(a, b2, msg):
    assert a["loglike"] == b2["loglike"], (msg, a["loglike"], b2["loglike"])
    for k in ("loglike_history", "ess", "state_est", "particles_history", "weights_history"):
        assert a[k].tobytes() == b2[k].tobytes(), (msg, k)
    for k in ("resampled", "ancestors"):
        assert np.array_equal(a["_extras"][k], b2["_extras"][k]), (msg, k)
    assert a["_extras"]["n_res_calls"] == b2["_extras"]["n_res_calls"] and a["_extras"]["early_return_step"] == 0, msg


def _vs_oracle(res, ref, msg):
    nres = ref["n_res_calls"]
    assert res["_extras"]["n_res_calls"] == nres and (res["_extras"]["resampled"] == ref["resampled"]).all(), msg
    assert np.array_equal(res["_extras"]["ancestors"], ref["ancestors"][:nres]), (msg, "ancestors differ from the oracle")
    assert abs(res["loglike"] - ref["loglike"]) <= 1e-6 * abs(ref["loglike"]), (msg, res["loglike"], ref["loglike"])
    np.testing.assert_allclose(res["loglike_history"], ref["loglike_history"], rtol=1e-6, atol=1e-9, err_msg=msg)
    np.testing.assert_allclose(res["ess"], ref["ess"], rtol=1e-6, err_msg=msg)
    np.testing.assert_allclose(res["state_est"], ref["state_est"], rtol=1e-6, atol=1e-8, err_msg=msg)
    np.testing.assert_allclose(res["weights_history"], ref["weights_history"], rtol=1e-9, atol=1e-300, err_msg=msg)


FILTER_CASES = [(model, ra, rf, N) for model in ("lg", "ar1sin") for ra in ("SISR", "SISAR") for rf in ("systematic", "stratified")
                for N in FILTER_N]


@pytest.mark.parametrize("model,ra,rf,N", FILTER_CASES)
def test_filter_forced_fallback_multi_launch(B, fctx, oracle, model, ra, rf, N):
    case = _case(B, fctx, oracle, model, ra, rf, N)
    _vs_oracle(case["base"], case["ref"], "unforced")
    before = fctx.fused_stats()
    for force in (FF_WALK, FF_GENERAL, FF_WALK | FF_SUM_ONLY):
        res = _run(B, fctx, case, 0, force)
        msg = "force_fallback=%d" % force
        _bitwise(res, case["base"], msg)
        _vs_oracle(res, case["ref"], msg)
        if force & FF_WALK:
            assert int(res["_extras"]["scan_stats"][1]) > 0, (msg, "the serial walk did not run", res["_extras"]["scan_stats"])
    assert fctx.fused_stats()["launches"] == before["launches"], "fused = 0 must not launch the fused kernel"


@pytest.mark.parametrize("model,ra,rf,N", FILTER_CASES)
def test_filter_forced_fallback_fused(B, fctx, oracle, model, ra, rf, N):
    """fused = 2 with the fallbacks forced: the last block's single side entry (nearly every resampling launch has one: the
    lanes next to cum == 1 are never PURE) is reached by the fallback, so the launch voids itself and the run is repeated on
    the multi-launch path -- bit for bit the unforced multi-launch run, and the oracle's."""
    case = _case(B, fctx, oracle, model, ra, rf, N)
    for force in (FF_WALK, FF_GENERAL, FF_WALK | FF_SUM_ONLY, FF_GENERAL | FF_SUM_ONLY):
        msg = "fused=2 force_fallback=%d" % force
        before = fctx.fused_stats()
        res = _run(B, fctx, case, 2, force)
        after = fctx.fused_stats()
        _bitwise(res, case["base"], msg)
        _vs_oracle(res, case["ref"], msg)
        assert after["runs"] == before["runs"] + 1 and after["launches"] == before["launches"] + T_FILTER, (msg, before, after)
        assert after["timeouts"] == before["timeouts"], (msg, before, after)
        assert after["stand_downs"] == before["stand_downs"] + 1, (msg, "the forced fallback did not stand the launch down", before, after,
                                                                   res["_extras"]["scan_stats"])
    # and unforced, the same configuration stays fused
    before = fctx.fused_stats()
    res = _run(B, fctx, case, 2, 0)
    after = fctx.fused_stats()
    _bitwise(res, case["base"], "fused=2 unforced")
    assert after["launches"] == before["launches"] + T_FILTER and after["timeouts"] == before["timeouts"], (before, after)


# ---------------------------------------------------------------------------------------------------------------------
# the fused launch counter past 2^32 - 1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1 << 20, 50001])
def test_fused_tag_wrap(B, N):
    """The granules on the wire carry the launch number as their tag, and a never-written granule carries 0: a launch with
    tag 0 would take zeros for published records.  The counter starts 3 launches before the wrap; the run (T = 8) crosses it,
    the next one continues from the restarted count.  Both stay fused and equal the multi-launch run bit for bit."""
    T = 8
    cx = B.Context(0, 1 << 20, 1)
    rng = np.random.default_rng(N)
    phi, sx, sy = 0.8, 1.0, 1.0
    x, ys = rng.standard_normal(), []
    for _ in range(T):
        x = phi * x + sx * rng.standard_normal()
        ys.append(x + sy * rng.standard_normal())
    m = B.models.linear_gaussian()
    kw = dict(resample_algorithm="SISR", resample_fn="systematic", return_particles=True, return_ancestors=True, seed=7, stream=N,
              ctx=cx, phi=phi, sigma_x=sx, sigma_y=sy)
    cx.set_option("fused", 0)
    base = B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw)
    cx.set_option("fused", 2)
    cx.set_option("fused_tag", -3)
    for run in ("across the wrap", "after the wrap"):
        before = cx.fused_stats()
        res = B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, **kw)
        after = cx.fused_stats()
        _bitwise(res, base, run)
        assert after["launches"] == before["launches"] + T, (run, before, after)
        assert after["stand_downs"] == before["stand_downs"] and after["timeouts"] == before["timeouts"], (run, before, after)
    cx.close()
