"""The single-filter runners behind bssm_pf_run (scalar models, multivariate family, reaction networks) against fixtures recorded
from the build BEFORE their set-up, read-back and observation loop were put into shared host code (tools/record_runner_golden.py,
on the GPU): loglike, loglike_history, ess, state_est, resampled, the early-return step and, where the case asks for them,
ancestors, particles_history and weights_history must be equal byte for byte (NaN rows by bit pattern).  The cases are the
recorder's, every one of them: N = 4096 + 777, T = 6 at the times 1, 1, 3, 4, 4, 7; BPF / APF / RMPF x SIS / SISR / SISAR x
stratified / systematic on the scalar LG model, its fused and multi-launch paths, histories with ancestors, injected draws, SIR;
the multivariate family's algorithms, observation families, time-varying pieces and histories; the reaction networks' algorithms x
transition methods, negative-binomial counts and a rate schedule; and per family a run whose second observation is impossible."""
import numpy as np
import pytest

import tools.record_runner_golden as rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import bayesssm_amd as B
    cx = rec.context(B)
    yield B, cx
    cx.close()


@pytest.mark.parametrize("name", list(rec.CASES))
def test_outputs_bit_equal_to_parent_build(ctx, name):
    B, cx = ctx
    with np.load(rec.golden_path(name)) as z:
        want = {k: z[k] for k in z.files}
    before = cx.fused_stats()
    got = rec.run_case(B, cx, name)
    after = cx.fused_stats()
    assert (after["runs"] - before["runs"] == 1) == (name == "lg_fused2"), (before, after)      # the path asked for is the one that ran
    assert set(got) == set(want)
    for k in sorted(got):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape, got[k].dtype, want[k].dtype)
        g, w = np.ascontiguousarray(got[k]).view(np.uint8).ravel(), np.ascontiguousarray(want[k]).view(np.uint8).ravel()
        if not np.array_equal(g, w):
            item = got[k].dtype.itemsize
            bad = np.unique(np.flatnonzero(g != w) // item)
            raise AssertionError("%s %s: %d of %d differ, first at %d: %r, recorded %r" % (
                name, k, bad.size, got[k].size, bad[0], got[k].ravel()[bad[0]], want[k].ravel()[bad[0]]))
    # what the dead_* cases are there for has happened, in the fixture and (being equal) in this run
    early, dim = int(want["early_return_step"][0]), want["state_est"].ndim
    assert early == (2 if name.startswith("dead_") else 0), early
    if early:
        late = want["state_est"][early:]
        assert np.all(np.isnan(late)) if dim > 1 else np.all(late == 0.0), late       # matrix(NA) rows for d > 1, numeric() zeros for a scalar state
        assert np.all(want["ess"][early:] == 0.0) and np.all(want["loglike_history"][early:] == 0.0) and want["loglike"][0] == -np.inf
        assert want["particles_history"].shape[0] == early and want["weights_history"].shape[0] == early      # histories end where the run did
