"""Dev tool: gamma white noise on the rates (models.reaction_network(method="euler_multinomial", leaps=K, noise={"beta": sigma})) against
plain Euler-multinomial leaps at the same K, on tools/bench_rnet_leap.py's SEIR (d = 4, R = 3, p = 1, x0 scaled to a population n, beta
scaled by 1 / n) and with its timing loop, as tools/bench_rnet_em.py:
  single    one bootstrap filter, N = 2^16, T = 50, SISAR / stratified: device time per observation
  batched   512 filters x N = 1000, T = 50 in k_pf_batch_rn: device time per observation
  python tools/bench_rnet_gwn.py --mode single|batched [--pops 1e6] [--methods em:16,gwn:16:0.1] [--reps 5] [--warmup 1]
A method is em:K or gwn:K:sigma (noise on beta: one gamma draw per leap next to the SEIR's three binomials).  Plain Euler-multinomial leaps
are measured against the parent commit's library with the same command and --methods em:16 (BAYESSSM_AMD_LIB), which uses nothing this
feature added.  Prints one JSON line per case."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_rnet_em as E  # noqa: E402
import bench_rnet_leap as L  # noqa: E402

_em_seir = E.seir


def seir(B, n, method):
    if not method.startswith("gwn:"):
        return _em_seir(B, n, method)
    _, K, sigma = method.split(":")
    return B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                            ({"I": 1}, {"R": 1}, "gamma")], x0=(round(0.86 * n), 0, round(0.14 * n), 0), observe={"I": L.RHO},
                                     method="euler_multinomial", leaps=int(K), noise={"beta": float(sigma)})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("single", "batched"), required=True)
    ap.add_argument("--pops", default="1e6")
    ap.add_argument("--methods", default="em:16,gwn:16:0.1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    pops = [int(float(v)) for v in a.pops.split(",")]
    import bayesssm_amd as B
    E.seir = seir                                          # (single and batched build their descriptors through the module's seir)
    (E.single if a.mode == "single" else E.batched)(B, pops, a.methods.split(","), a.reps, a.warmup)
