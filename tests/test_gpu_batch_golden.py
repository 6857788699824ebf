"""The three batch runners behind bssm_pf_run_batch / bssm_pf_run_batch_tv (scalar models, multivariate family, reaction networks)
and the two lock-step PMMH entry points (bssm_pmmh_chains_batch, bssm_pmmh_chains_multi) against fixtures recorded from the build
BEFORE their staging, common fill, launch bracket, read-back and chain loop were put into shared host code
(tools/record_batch_golden.py, on the GPU).  loglike, state_est, ess, loglike_history, early_return_step, n_res_calls and status of
every filter, and theta_chain, loglike_chain and accepted of every chain, must be equal byte for byte (NaN rows by bit pattern);
every refusal the five entry points give before they touch the device must keep its status and its text, calls that break two rules
at once included (the order of the checks).  The cases are the recorder's, every one of them: F = 3 different filters, N = 777,
T = 6 at the times 1, 1, 3, 4, 4, 7; LG with BPF / APF / RMPF and with multinomial resampling, AR(1)+sin, SIR, T = 0; the
multivariate family's observation families, a missing y, shared time-varying arrays, two array sets through bssm_pf_run_batch_tv,
d = 1; the reaction networks' transition methods, gamma noise, negative-binomial counts with a size per filter, a rate schedule; and
per family a call in which filter 1 alone returns early at step 2."""
import json

import numpy as np
import pytest

import tools.record_batch_golden as rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import bayesssm_amd as B
    cx = rec.context(B)
    yield B, cx
    cx.close()


def _assert_bytes_equal(name, got, want):
    assert set(got) == set(want)
    for k in sorted(got):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape, got[k].dtype, want[k].dtype)
        g, w = np.ascontiguousarray(got[k]).view(np.uint8).ravel(), np.ascontiguousarray(want[k]).view(np.uint8).ravel()
        if not np.array_equal(g, w):
            item = got[k].dtype.itemsize
            bad = np.unique(np.flatnonzero(g != w) // item)
            raise AssertionError("%s %s: %d of %d differ, first at %d: %r, recorded %r" % (
                name, k, bad.size, got[k].size, bad[0], got[k].ravel()[bad[0]], want[k].ravel()[bad[0]]))


def _recorded(name):
    with np.load(rec.golden_path(name)) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(rec.CASES))
def test_filters_bit_equal_to_parent_build(ctx, name):
    B, cx = ctx
    want = _recorded(name)
    assert set(want) == set(rec.KEYS)
    _assert_bytes_equal(name, rec.run_case(B, cx, name), want)
    # what the case is there for has happened, in the fixture and (being equal) in this run
    early = want["early_return_step"].tolist()
    assert early == ([0, 2, 0] if name.startswith("dead_") else [0, 0, 0]), early
    assert np.all(want["status"] == 0) and len(set(want["loglike"].tolist())) == (1 if name == "lg_T0" else rec.F)
    if name.startswith("dead_"):
        late = want["state_est"][1, 2:]
        assert np.all(np.isnan(late)) if want["state_est"].shape[-1] > 1 and want["state_est"].ndim == 3 else np.all(late == 0.0), late
        assert np.all(want["ess"][1, 2:] == 0.0) and np.all(want["loglike_history"][1, 2:] == 0.0) and want["loglike"][1] == -np.inf
        assert np.all(np.isfinite(want["state_est"][[0, 2]])) and np.all(want["ess"][[0, 2]] > 0.0) and np.all(np.isfinite(want["loglike"][[0, 2]]))


@pytest.mark.parametrize("name", rec.CHAIN_CASES)
def test_lockstep_chains_bit_equal_to_parent_build(ctx, name):
    B, cx = ctx
    want = _recorded(name)
    assert set(want) == set(rec.CHAIN_KEYS)
    _assert_bytes_equal(name, rec.run_case(B, cx, name), want)
    assert rec.chains_compacted(want["theta_chain"])          # some iteration ran a part of the chains only


def test_both_lockstep_entry_points_recorded_the_same_chains():
    a, b = (_recorded(name) for name in rec.CHAIN_CASES)
    _assert_bytes_equal("chains", a, b)


def test_refusals_keep_status_and_text(ctx):
    B, cx = ctx
    with open(rec.refusals_path()) as fh:
        want = json.load(fh)
    assert set(want) == set(rec.REFUSALS)
    got = {}
    for name in rec.REFUSALS:
        st, msg = rec.refusal(B, cx, name)
        got[name] = {"status": st, "message": msg}
    assert got == want
