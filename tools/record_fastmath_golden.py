"""Dev tool: record the filter outputs that tests/test_gpu_fastmath_filter.py holds the range-specialised device functions
(bayesssm_amd/csrc/fastmath.hip.h) to, bit for bit.  Run it on a GPU with the build whose results are the reference -- the
commit BEFORE the specialised functions went in (BAYESSSM_AMD_LIB selects another build of the library):
    python tools/record_fastmath_golden.py [OUT_DIR, default tests/golden]
One small .npz per case: the observations, loglike / loglike_history / ess / state_est of the run and, for the cases with a far
observation, the weights of that step."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, T = 4096 + 777, 12            # three scan workgroups, the last one partly filled
OUTPUTS = ("loglike", "loglike_history", "ess", "state_est")
FAR_THRESHOLD = 0.5              # an ESS is >= 1: SISAR with this threshold never resamples
# name, model, fused option, sigma_y, index of the observation moved 40 sigma_y away (or None), resample_algorithm, threshold
CASES = [("%s_fused%d" % (model, fused), model, fused, 0.7, None, "SISR", None) for model in ("lg", "ar1sin") for fused in (0, 2)]
# SISR records ess = N at every step (the figure after resampling); SISAR at its default threshold N / 2 records the ESS
# itself -- (sum e)^2 / sum e^2 of the exp(lw - max) -- at every step that it does not resample
CASES += [("lg_sisar_fused%d" % fused, "lg", fused, 0.7, None, "SISAR", None) for fused in (0, 2)]
# the deep-underflow end of exp.  The FIRST observation lies 40 sigma_y away, sigma_y = 0.15: the particles there are 0.8 N(0, 1) +
# N(0, 1), sd 1.28 = 8.5 sigma_y, and the outermost of 4873 lie about 3.7 sd = 31 sigma_y to either side, so lw - max runs from 0 down
# to about -((40 + 31)^2 - (40 - 31)^2) / 2 = -2500: through the subnormal results (-708.4 .. -745.1) and far into the exact zeros.
# SISAR that never resamples keeps the evidence: the weights of that step (w_far; underflow_reach() below) and its ESS; the steps
# after it carry log(0) = -inf log-weights through exp as well.
CASES += [("lg_far_fused%d" % fused, "lg", fused, 0.15, 0, "SISAR", FAR_THRESHOLD) for fused in (0, 2)]


def observations(model, sigma_y, far):
    rng = np.random.default_rng(1405)
    x, ys = rng.standard_normal(), []
    for _ in range(T):
        x = 0.8 * x + (np.sin(x) if model == "ar1sin" else 0.0) + rng.standard_normal()
        ys.append(x + sigma_y * rng.standard_normal())
    ys = np.array(ys)
    if far is not None:
        ys[far] += 40.0 * sigma_y
    return ys


def golden_path(name, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), "fastmath_%s.npz" % name)


def run_case(B, cx, model, fused, sigma_y, ys, far=None, resample_algorithm="SISR", threshold=None):
    m = B.models.linear_gaussian() if model == "lg" else B.models.ar1_sin()
    cx.set_option("fused", fused)
    try:
        res = B.bootstrap_filter(ys, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm=resample_algorithm,
                                 resample_fn="systematic", threshold=threshold, return_particles=far is not None, seed=1405,
                                 stream=3, ctx=cx, phi=0.8, sigma_x=1.0, sigma_y=sigma_y)
    finally:
        cx.set_option("fused", 1)
    out = {k: np.atleast_1d(np.asarray(res[k], dtype=np.float64)) for k in OUTPUTS}
    if far is not None:
        out["w_far"] = np.array(res["weights_history"][far + 1], dtype=np.float64)      # the normalised weights exp(lw - max) / S
    return out


def underflow_reach(w):
    """(subnormal, zero, normal) counts among normalised weights w = exp(lw - max) / S.  S is a sum of at most N < 2^13 terms <= 1
    of which one is 1, so 1 <= S < 2^13 and a weight in (0, 2^-1035) is the quotient of an exp() result below 2^-1022: a subnormal one."""
    return int(np.sum((w > 0) & (w < 2.0 ** -1035))), int(np.sum(w == 0)), int(np.sum(w >= 2.0 ** -1022))


def main():
    import bayesssm_amd as B
    out_dir = sys.argv[1] if len(sys.argv) > 1 else None
    cx = B.Context(0, 1 << 20, 1)
    for name, model, fused, sigma_y, far, ra, threshold in CASES:
        ys = observations(model, sigma_y, far)
        out = run_case(B, cx, model, fused, sigma_y, ys, far, ra, threshold)
        print("%-18s loglike %.17g  min ess %.6g  steps with ess < N: %d" % (name, out["loglike"][0], out["ess"].min(), np.sum(out["ess"] < N)))
        if far is not None:
            sub, zero, normal = underflow_reach(out["w_far"])
            print("%-18s weights of the far step: %d from a subnormal exp, %d exactly 0, %d normal" % ("", sub, zero, normal))
            assert sub > 0 and zero > 0 and normal > 0, "the far observation does not reach the underflow end of exp"
        np.savez_compressed(golden_path(name, out_dir), ys=ys, **out)
    cx.close()


if __name__ == "__main__":
    main()
