"""Dev/bench tool: what missing-data support (models.linear_gaussian_mv(..., missing="skip"); the context option mv_y_missing) costs
the multivariate family's batched kernel, at tools/bench_mv_obs.py's shape: 512 filters x N = 1000, T = 1000, (d, p) = (3, 2),
Gaussian, SISAR + stratified, one launch of k_pf_batch_mv (bootstrap_filter_batch).
  full      a NaN-free y through the default descriptor -- the leg an older build of the library (BAYESSSM_AMD_LIB) can run too:
            the uniform branch around every component must not show here
  skip      the same y through missing="skip" (the option set, nothing missing): the same kernel, the same numbers
  third     a third of the entries missing (whole rows and single components)
Device times are the HIP-event times the library reports, one line per run and the range over the repeats.  The checksum line
compares two builds on the same inputs.

    python tools/bench_mv_missing.py [repeats] [--full-only]
(--full-only: for a build of the library that predates the option, selected with BAYESSSM_AMD_LIB)
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import bayesssm_amd as b  # noqa: E402
from bench_mv_obs import F, N, T, data, model_pieces  # noqa: E402
from bench_mv_tv import D, P, stats  # noqa: E402


def punch(y, seed=8):
    """about a third of the entries missing: every seventh row whole, the rest entry by entry"""
    rng = np.random.default_rng(seed)
    y = y.copy()
    gone = rng.random(y.shape) < 0.22
    gone[::7] = True
    y[gone] = np.nan
    return y, float(gone.mean())


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    print("library: %s" % b._lib.LIB_PATH)
    q = model_pieces()
    y = data(q, "gaussian", T)
    y3, share = punch(y)
    legs = [("full", "refuse", y)]
    if "--full-only" not in sys.argv:
        legs += [("skip", "skip", y), ("third", "skip", y3)]
    ctx = b.Context(0, 2048, 8)
    for leg, missing, yy in legs:
        m = b.models.linear_gaussian_mv(D, P, **({"missing": missing} if missing != "refuse" else {}), **q)
        thetas = np.array([m.pack({})] * F)

        def run():
            return b.bootstrap_filter_batch(yy, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, thetas, 1, resample_algorithm="SISAR",
                                            resample_fn="stratified", ctx=ctx)
        run()                                                         # warm-up
        outs = [run() for _ in range(repeats)]
        ms = [o["device_ms"] for o in outs]
        print("%-5s %d filters x N = %d, T = %d%s: device %s; runs %s" % (
            leg, F, N, T, " (%.0f%% of the entries missing)" % (100 * share) if leg == "third" else "", stats(ms),
            " ".join("%.3f" % v for v in ms)), flush=True)
        print("%-5s loglike sha256 %s (filter 0: %.12f; early returns: %d)" % (
            leg, hashlib.sha256(outs[-1]["loglike"].tobytes()).hexdigest()[:16], outs[-1]["loglike"][0], int(np.count_nonzero(outs[-1]["early_return_step"]))))
    ctx.close()
