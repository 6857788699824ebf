"""Whole filter runs with the range-specialised device functions (bayesssm_amd/csrc/fastmath.hip.h) against fixtures recorded
from the build BEFORE they went in (tools/record_fastmath_golden.py, on the GPU): loglike, loglike_history, ess and state_est
must be bit-equal.  N = 4096 + 777, T = 12, device generator, multi-launch (fused = 0) and fused (2):
  * LG and AR(1)+sin under SISR (ess is N at every step: the figure after resampling);
  * LG under SISAR, whose ess is the one computed from sum e and sum e^2 of the exp(lw - max) wherever it does not resample;
  * LG with the first observation 40 sigma_y away, under SISAR that never resamples: the weights of that step are compared too,
    and must show that exp was taken through its subnormal results and into exact zeros on the kernels' own path."""
import numpy as np
import pytest

import tools.record_fastmath_golden as rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import bayesssm_amd as B
    cx = B.Context(0, 1 << 20, 1)
    yield B, cx
    cx.close()


@pytest.mark.parametrize("case", rec.CASES, ids=[c[0] for c in rec.CASES])
def test_outputs_bit_equal_to_parent_build(ctx, case):
    B, cx = ctx
    name, model, fused, sigma_y, far, ra, threshold = case
    with np.load(rec.golden_path(name)) as z:
        want = {k: z[k] for k in z.files}
    np.testing.assert_array_equal(want["ys"], rec.observations(model, sigma_y, far))       # the fixture is of this series
    before = cx.fused_stats()
    got = rec.run_case(B, cx, model, fused, sigma_y, want["ys"], far, ra, threshold)
    after = cx.fused_stats()
    assert (after["runs"] - before["runs"] == 1) == (fused == 2), (before, after)          # the path asked for is the one that ran
    assert set(got) == set(want) - {"ys"}
    for k in got:
        assert got[k].shape == want[k].shape, k
        diff = np.flatnonzero(got[k].view(np.uint64) != want[k].view(np.uint64))
        assert diff.size == 0, "%s %s: %d of %d differ, first at %d: %r, recorded %r" % (
            name, k, diff.size, got[k].size, diff[0], got[k][diff[0]], want[k][diff[0]])
    # what each case is there for has happened, in the fixture and (being bit-equal) in this run
    ess = want["ess"][1:]
    if ra == "SISAR" and far is None:
        assert np.sum((ess > 1.0) & (ess < rec.N)) >= 2, ess          # an ESS computed from the weights, not the N of a resampled step
    if far is not None:
        assert np.all(ess < rec.N), ess                                # never resampled: the weights of the far step are exp(lw - max) / S
        sub, zero, normal = rec.underflow_reach(got["w_far"])
        print("%s: %d weights from a subnormal exp, %d exactly 0, %d normal; ess of that step %.17g" % (name, sub, zero, normal, ess[far]))
        assert sub > 0 and zero > 0 and normal > 0, (sub, zero, normal)
        assert np.isfinite(got["loglike"][0]) and np.all(np.isfinite(got["loglike_history"]))      # and the run went on
