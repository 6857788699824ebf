"""Dev/bench tool: what per-filter SETS of the time-varying b / h0 of the multivariate linear-Gaussian family cost in the batched
kernel (k_pf_batch_mv).  The shape of tools/bench_mv_tv.py's batch leg: 512 filters x N = 1000, T = 1000 at (d, p) = (3, 2),
SISAR + stratified, twice:
  shared   b and h0 as ONE array each, the descriptor's, through bssm_pf_run_batch (what the parent commit runs too)
  sets     b and h0 as 512 sets (b_k = g_k b, h0_k = a_k h0) through bssm_pf_run_batch_tv
Device times are the HIP-event times the library reports; medians with the range over the repeats.  The last line of a leg
is a checksum of the log-likelihoods, to compare two builds of the library on the same inputs.

    python tools/bench_mv_tv_sets.py [repeats] [--no-sets]
(--no-sets: the shared leg only -- for a build of the library that predates the sets, selected with BAYESSSM_AMD_LIB)
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import bayesssm_amd as b  # noqa: E402
from bench_mv_tv import D, P, arrays, data, pieces, stats  # noqa: E402

F, N, T = 512, 1000, 1000

if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 7
    print("library: %s" % b._lib.LIB_PATH)
    q = pieces()
    tv = arrays(q, T)
    tv.pop("H")
    y = data(q, dict(tv, H=np.broadcast_to(q["H"], (T, P, D))), T)
    m = b.models.linear_gaussian_mv(D, P, time_varying=tv, **q)
    thetas = np.array([m.pack({})] * F)
    ctx = b.Context(0, 2048, 8)
    gains = 1.0 + 0.001 * np.arange(F)
    legs = {"shared": {}}
    if "--no-sets" not in sys.argv:
        legs["sets"] = {"time_varying": {"b": gains[:, None, None] * tv["b"], "h0": gains[::-1, None, None] * tv["h0"]}}
    for name, kw in legs.items():
        def run():
            return b.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, thetas, 1, resample_algorithm="SISAR",
                                            resample_fn="stratified", ctx=ctx, **kw)
        run()                                                         # warm-up
        outs = [run() for _ in range(repeats)]
        print("%-6s %d filters x N = %d, T = %d: device %s" % (name, F, N, T, stats([o["device_ms"] for o in outs])), flush=True)
        print("%-6s loglike sha256 %s (filter 0: %.12f)" % (name, hashlib.sha256(outs[-1]["loglike"].tobytes()).hexdigest()[:16], outs[-1]["loglike"][0]))
    ctx.close()
