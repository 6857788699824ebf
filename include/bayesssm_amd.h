/*
 * bayesssm_amd.h -- C ABI of the MI355X particle-filter engine.
 *
 * This is the drop-in boundary for bayesSSM's hot path.  Every entry point is
 * `extern "C"`, takes plain pointers/sizes and returns an int status
 * (BSSM_OK == 0); `bssm_last_error()` gives the message of the last failure on
 * the calling thread.  Nothing here throws, and no torch/R types appear.
 *
 * What each group replaces in the reference (paths relative to the bayesSSM
 * checkout):
 *
 *   bssm_resample_*        SEXP _bayesSSM_resample_{multinomial,stratified,systematic}_cpp
 *                          (SEXP nSEXP, SEXP weightsSEXP)      src/RcppExports.cpp:15,27,39
 *                          = resample_*_cpp(n, weights)        src/resampling.cpp:5,16,43
 *                          called from .resample_*             R/resampling.R:19,39,59
 *   bssm_pf_run            .particle_filter_core               R/particle_filter_core.R:19-267
 *                          via bootstrap_filter / auxiliary_filter
 *                                                              R/bootstrap_filter.R:129-171
 *                                                              R/auxiliary_filter.R:163-216
 *                          (also resample_move_filter, R/resample_move_filter.R:190-236, with the built-in move)
 *   bssm_pf_run_batch      the same filters, many at once: the pilot's repeated runs (R/pmmh_tuning.R:29-64) and
 *                          PMMH's small filters (N <= 1000, R/pmmh_tuning.R:55-57); one workgroup per filter
 *   bssm_pmmh_chain        the per-chain loop of pmmh()        R/pmmh.R:403-415,422-500
 *                          (+ R/utils.R:102-152 transforms)
 *   bssm_pmmh_chains_batch the chain fan-out of pmmh()         R/pmmh.R:511-531, chains in lock-step over the batch
 *
 * Random draws.  The reference takes them from R's global RNG
 * (Rcpp::RNGScope, src/RcppExports.cpp:18,30,42).  Here they are either
 * INPUTS (the R glue / the parity tests draw them and pass them in) or, when
 * the pointers are NULL, generated on the device by a counter-based generator
 * keyed by (seed, stream) -- see csrc/rng.h.
 *
 * Indices returned to the caller are 1-based int32, as the reference's
 * IntegerVector is (src/resampling.cpp:36,62).
 */
#ifndef BAYESSSM_AMD_H
#define BAYESSSM_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
#define BSSM_OK 0
#define BSSM_ERR_NEGATIVE_WEIGHT 1   /* "Weights must be non-negative"          src/resampling.cpp:6,18,45 */
#define BSSM_ERR_ZERO_SUM 2          /* "Sum of weights must be greater than 0" src/resampling.cpp:8,22,49 */
#define BSSM_ERR_LENGTH 3            /* "Number of particles must match the length of weights" R/resampling.R:17 */
#define BSSM_ERR_ARG 4               /* invalid argument (message says which)   */
#define BSSM_ERR_HIP 5               /* HIP runtime failure                     */
#define BSSM_ERR_CAPACITY 6          /* problem larger than the context was created for */

/* ---- enums (values match the oracle's) ---------------------------------- */
#define BSSM_MODEL_LG 0       /* x' = phi x + N(0,sx);            y ~ N(x, sy)   tests/testthat/test-pmmh_tuning.R:163-173 */
#define BSSM_MODEL_AR1SIN 1   /* x' = phi x + sin x + N(0,sx);    y ~ N(x, sy)   README.md:137-146 */
#define BSSM_MODEL_SIR 2      /* stochastic SIR, state (s, i), Gillespie day, y ~ Poisson(i);
                                 theta = (lambda, gamma, n_total, s0, i0)          vignettes/articles/stochastic-sir-model.Rmd:143-176,285-310 */
#define BSSM_MODEL_LGMV 3     /* multivariate linear-Gaussian family, state dimension d <= 8, observation dimension p <= 8 (BPF, APF, RMPF;
                               * stratified / systematic resampling):
                               *   x0 = m0 + L0 z;  x' = A x + b + L z;  log g = c0 (p == 0) or sum_k dnorm(y_k, h0_k + (H x)_k, sd_k, log = TRUE)
                               *   APF aux log g: log g at the transition mean A x + b (p == 0: c0)
                               *   RMPF move: prop = x + sd z, z ~ N(0, I_d), accepted when log(u) < log g(prop) - log g(x) (p == 0: always);
                               *   move draw of component c of particle i at observation t: Philox counter (i, t, DRAW_MOVE | (c << 8), stream)
                               * theta = the packed block  d, p, m0[d], L0[d d], A[d d], b[d], L[d d], c0, H[p d], h0[p], sd[p]  (row-major matrices),
                               * y = [T][p] row-major, state_est = [T+1][d]; injected draws z_init [d][N], z_trans [calls][d][N], z_move [T][d][N],
                               * u_move [T][N].  Covers the reference's multi-dimensional cases (tests/testthat/test-bootstrap_filter.R:211-230,
                               * test-pmmh.R:619-668) without the host closures.  bssm_pf_run_batch / bssm_pf_run_batch_tv run its bootstrap filter only.
                               * Time-varying b, h0, H (known inputs, seasonal offsets, dynamic regression): bssm_pf_config.mv_tv, see bssm_mv_tv;
                               * A, L, sd, m0, L0, c0 are constant. */
/* BSSM_MODEL_LGMV with another observation density over the same linear predictor  eta_k = h0_k + sum_c H_kc x_c  (accumulated in
 * the order the Gaussian mean is, from the same constant or time-varying rows).  Both ids take BSSM_MODEL_LGMV's packed block in
 * BSSM_MODEL_LGMV's layout (sd keeps its slot and is not read), the same y / state_est / draw layouts, bssm_mv_tv and
 * bssm_mv_tv_batch, and run through the same entry points (bssm_pf_run with BPF / APF / RMPF; bssm_pf_run_batch and
 * bssm_pf_run_batch_tv with the bootstrap filter).  log g = the sum over k = 0 .. p-1 of the component log-densities, from 0.0;
 * the APF's aux log g is the same density at the transition mean, the RMPF move uses it in its acceptance ratio.  p >= 1
 * (BSSM_ERR_ARG otherwise: a model without observation components has no observation family). */
#define BSSM_MODEL_LGMV_POIS 4   /* counts through a log link, dpois(y_k, exp(eta_k), log = TRUE):
                                  *   lambda = exp(eta_k);  -inf unless lambda < +inf;  y_k == 0: -lambda;  else (y_k eta_k - lambda) - lgamma(y_k + 1)
                                  * lgamma(y + 1) is taken on the host per (t, k) and uploaded next to y, as for BSSM_MODEL_SIR.
                                  * Every y must be finite, >= 0 and integral (BSSM_ERR_ARG otherwise). */
#define BSSM_MODEL_LGMV_LOGVAR 5 /* y_k ~ N(0, exp(eta_k)), the stochastic-volatility observation (canonical SV: d = p = 1, H = 1, A = phi, b = mu (1 - phi)):
                                  *   (-0.5 log(2 pi) - 0.5 eta_k) - (0.5 y_k^2) exp(-eta_k);  the last term is 0 when 0.5 y_k^2 == 0;  -inf for a non-finite eta_k */
#define BSSM_MODEL_RNET 6     /* mass-action reaction network (SEIR, SIRS, Lotka-Volterra, birth-death, ...): d <= 8 species held as integer-valued
                               * doubles, 1 <= R <= 8 reactions, 1 <= p <= 8 Poisson observation components (BPF and APF; SIS / SISR / SISAR;
                               * stratified / systematic).  theta is a packed block of doubles (n_theta = its length):
                               *   d, R, p, x0[d], k[R], s1[R], s2[R], nu[R][d] row-major, G[p][d] row-major
                               * init: every particle starts at x0 (no draws).  Propensity of reaction r: k_r (s1 = s2 = -1), k_r x[s1] (s2 = -1) or
                               * (k_r x[s1]) x[s2]; one that is not > 0 counts as 0.0; s1 == s2 (dimerisation) is refused.  k_r arrives already
                               * scaled (SIR: lambda / n_total).  One transition = one unit of time of Gillespie's direct method, as BSSM_MODEL_SIR
                               * runs it: total = a_0 + a_1 + ... (left to right), one Philox block per event keyed (particle, call,
                               * DRAW_TRANS | event << 8, stream), dt = -log(u) / total, the first r in 0..R-2 with u' < (a_0 + .. + a_r) / total
                               * fires (else R-1), x += nu[r]; at most 2^20 events.  Log-likelihood: lambda_k = 0.0 + sum_c G_kc x_c,
                               * 0.0 + sum_k dpois(y_k, lambda_k, log = TRUE) with lgamma(y + 1) taken on the host per (t, k); y [T][p] must be finite,
                               * >= 0 and integral.  APF look-ahead: the same density at m_c = x_c + sum_r nu[r][c] a_r, lambda_k clamped at 0.0.
                               * With d = 2, R = 2, p = 1, k = (lambda / n_total, gamma), s1 = (0, 1), s2 = (1, -1), nu = ((-1, 1), (0, -1)),
                               * G = (0, 1) every output equals BSSM_MODEL_SIR's bit for bit.  Injected z_* are refused (data-dependent number of
                               * draws), as are RMPF and multinomial resampling.
                               * Counter species (incidence): the block may end in an optional tail reset[d] of 0.0 / 1.0 after G, so n_theta is
                               * 3 + d + 3 R + R d + p d or that + d; without the tail every output is what it was.  A species c with reset[c] = 1
                               * is set to 0.0 before the Gillespie loop of the first transition of each observation's gap loop (t == prev_t + 1):
                               * over an obs_times gap it accumulates over the whole gap, at a repeated observation time nothing is reset, and the
                               * APF's second-stage transition never resets.  Tail entries other than 0 and 1, and a flagged species that appears in
                               * s1 or s2, are refused (BSSM_ERR_ARG).  In bssm_pf_run_batch every block of one call has the same length.
                               * Rate schedule (time-varying rates): after reset[d] (then always present, all 0.0 without counters) the block may
                               * carry a second tail  n_times, M[n_times][R] row-major  of finite multipliers >= 0, so the third length is
                               * 3 + d + 3 R + R d + p d + d + 1 + n_times R.  The transition TO absolute time tau uses row tau - 1: the propensity of
                               * reaction r starts from k_r * M[tau-1][r] (then times x[s1], times x[s2], as above; a schedule of ones changes no
                               * bit).  tau = prev_t + step in the gap loop; the observation's time for the APF's second-stage transition and for the
                               * propensities of its look-ahead; at a repeated observation time the bootstrap filter reads no row.  n_times must be an
                               * integer >= 1 that agrees with n_theta and reaches the last observation time (T without obs_times); a negative or
                               * non-finite multiplier is refused (all BSSM_ERR_ARG).  In bssm_pf_run_batch every block carries its own schedule.
                               * A piecewise-constant rate with learnable levels needs no parameter-dependent schedule: write the reaction twice
                               * (rates beta1, beta2) with 0 / 1 indicator columns; a zero multiplier gives the propensity 0.0 exactly.
                               * With BSSM_OPT_MV_Y_MISSING a NaN y_k is a component that was not observed: the log-likelihood and the look-ahead sum
                               * over the observed k only (a row with nothing observed gives 0.0); +-inf is refused either way. */
#define BSSM_MODEL_RNET_NB 7  /* BSSM_MODEL_RNET with negative-binomial (overdispersed) observations: y_k ~ NegBin(mean = mu_k, size = r_k), variance
                               * mu + mu^2 / r.  The block is BSSM_MODEL_RNET's with size[p] (finite, > 0, else BSSM_ERR_ARG) inserted directly
                               * after G[p][d]; the optional tails reset[d] and n_times, M[n_times][R] follow as before, so the three lengths are
                               * BSSM_MODEL_RNET's + p.  mu_k = lambda_k exactly as BSSM_MODEL_RNET forms it (for the look-ahead at the Euler mean,
                               * clamped at 0.0), r = size_k, and the density is, in this order, fp64 without contraction:
                               *   if (!(mu > 0.0)) return (y == 0.0 && mu == 0.0) ? 0.0 : -inf;
                               *   s = r + mu;  lr = (r < mu) ? log(r / s) : log1p(-(mu / s));
                               *   if (y == 0.0) return r * lr;
                               *   return (c + r * lr) + y * log(mu / s);
                               * c(t, k) = (lgamma(y + r) - lgamma(r)) - lgamma(y + 1) is taken on the host per (t, k) with C's lgamma (0.0 for a NaN
                               * y_k, never read) and uploaded where BSSM_MODEL_RNET uploads lgamma(y + 1); in bssm_pf_run_batch per filter, from that
                               * filter's own size.  This is dnbinom(y, size = r, mu = mu, log = TRUE).  Everything else -- transition, draw keys,
                               * counters, rate schedule, BSSM_OPT_MV_Y_MISSING, the checks of y as counts, the refusals (RMPF, multinomial, injected
                               * z_*), bssm_pf_batch_max_particles_rn -- is BSSM_MODEL_RNET's. */

#define BSSM_BPF 0            /* bootstrap_filter  */
#define BSSM_APF 1            /* auxiliary_filter  */
#define BSSM_RMPF 2           /* resample_move_filter with the built-in random-walk Metropolis move (R/resample_move_filter.R:166-176) */

#define BSSM_SIS 0
#define BSSM_SISR 1
#define BSSM_SISAR 2

#define BSSM_STRATIFIED 0
#define BSSM_SYSTEMATIC 1
#define BSSM_MULTINOMIAL 2    /* inverse CDF on the exact cum_sum: the reference's law, not Rcpp::sample's stream (throughput mode) */
#define BSSM_MULTINOMIAL_R 3  /* Rcpp::sample(n, n, true, prob) as published (Walker alias / sorted inversion), U = its unif_rand()
                                 stream: the reference's own draws for R's seed (parity mode; sequential set-up, one workgroup) */

#define BSSM_TR_IDENTITY 0
#define BSSM_TR_LOG 1
#define BSSM_TR_LOGIT 2

#define BSSM_PRIOR_NORMAL 0   /* dnorm(x, a, b, log=TRUE)  */
#define BSSM_PRIOR_EXP 1      /* dexp(x, rate=a, log=TRUE) */
#define BSSM_PRIOR_UNIFORM 2  /* dunif(x, a, b, log=TRUE)  */
#define BSSM_PRIOR_FLAT 3     /* 0                          */
#define BSSM_PRIOR_HALFNORMAL 4 /* extraDistr::dhnorm(x, sigma = a, log=TRUE)  (stochastic-sir-model.Rmd:267-274) */

typedef struct bssm_ctx bssm_ctx;

/* ---- context ------------------------------------------------------------ */
/* One context per GPU (and per host thread that drives it).  Owns all device
 * memory for filters of up to `max_particles` particles of dimension
 * `max_dim`, and one HIP stream. */
int bssm_ctx_create(int device, long long max_particles, int max_dim, bssm_ctx** out);
void bssm_ctx_destroy(bssm_ctx* ctx);
const char* bssm_last_error(void);
const char* bssm_status_string(int status);   /* the reference's error text for a status */
int bssm_device_count(void);
int bssm_ctx_synchronize(bssm_ctx* ctx);
/* The HIP stream (hipStream_t) all of this context's kernels are launched on. */
void* bssm_ctx_stream(bssm_ctx* ctx);

/* Per-context options: test aids and A/B switches (the library keeps no process-global mutable state besides the
 * per-thread last-error string).  Defaults in brackets. */
#define BSSM_OPT_RECORD_WINDOW 1       /* [0 = automatic] validity window of the exact-scan records in ulps; a tiny window forces the literal fallbacks (tests) */
#define BSSM_OPT_BATCH_LITERAL_MAX 2   /* [384] largest N whose exact sums the batched kernel takes by the in-order pass */
#define BSSM_OPT_STAGE_EXPANSION 3     /* [1] stage the resampled particles in LDS and store them coalesced */
#define BSSM_OPT_INKERNEL_RESOLVE 4    /* [1] grids of <= 512 blocks: the consuming kernels resolve the pass before them; 0 = k_resolve launches */
#define BSSM_OPT_DEBUG_STOP 5          /* [0] DEV builds (make DEV=1): stage stamps */
#define BSSM_OPT_RENORMALIZE 7         /* [1] filters: the resampler's prob = weights / sum(weights) on the already normalised weights (src/resampling.cpp:24,51); 0 folds it away */
#define BSSM_OPT_RECOMPUTE_LW 8        /* [1] bootstrap filters, Gaussian-observation models: k_step does not store the log-weights, k_weights re-evaluates them */
#define BSSM_OPT_FUSED 9               /* [1] bootstrap / resample-move filters, scalar Gaussian-observation models, 256 < blocks <= 512 (2^19 < N <= 2^20): ONE launch per observation (workgroups keep their particles on chip; block records cross workgroups as tagged granules); 0 = the multi-launch path; 2 = fused at every N <= 2^20 (tests) */
#define BSSM_OPT_FUSED_PREFETCH 10     /* [0] fused path: the next observation's transition normals are drawn in the time the workgroups wait for the resolver (measured slower: +2 us per observation) */
#define BSSM_OPT_FORCE_FALLBACK 11     /* [0] test aid: the exact-scan resolvers take their exact fallbacks although the records cover the states -- bit 1: every resolve walks all blocks in order (serial walk), bit 2: every block with a side entry / literal tail takes the general per-block routine, bit 4: only in the sum(w) pass.  Results must not change */
#define BSSM_OPT_FUSED_TAG 12          /* test aid: the fused path's launch counter (uint32; the next launch carries value + 1) -- -3 reaches the wrap at the third launch; zeroes the fused workspace */
#define BSSM_OPT_FUSED_EARLY_MAX 0      /* [1] fused path: every block publishes its max(log-weights) ahead of its two sums; the resolver broadcasts the global max M on a line of its own, ahead of (M, sum, status), and the workers take exp(lw - M) while they wait for the sum -- only the division by it stays behind the answer.  Same arithmetic, same results; 0 = one gather, one answer (measured in 5a) */
#define BSSM_OPT_FUSE_STEP 6          /* [0] SISR bootstrap filters: the next observation's transition + weight inside the expansion kernel */
#define BSSM_OPT_MV_Y_MISSING 13      /* [0] multivariate family (BSSM_MODEL_LGMV, _POIS, _LOGVAR) in bssm_pf_run / bssm_pf_run_batch / bssm_pf_run_batch_tv, and BSSM_MODEL_RNET in bssm_pf_run / bssm_pf_run_batch: 1 = a NaN in y[i][k] means that component k of observation i was not observed -- the log-likelihood (and the aux log-likelihood, and both terms of the move's ratio) is the sum over the observed k only, 0.0 for a row with nothing observed; +-inf stays refused, the Poisson checks and the lgamma(y + 1) table cover observed entries only.  0 = NaN is refused (as every other model and entry point always does) */
#define BSSM_OPT_RN_LEAPS 14           /* [0] reaction networks (BSSM_MODEL_RNET, BSSM_MODEL_RNET_NB; ignored by every other model): 0 = the transition is
                                        * Gillespie's direct method; K in 1 .. 1024 = tau-leaping with K leaps per unit of time (a value outside 0 .. 1024 is
                                        * refused, BSSM_ERR_ARG).  Read by bssm_pf_run and bssm_pf_run_batch at the call; the blocks and bssm_pf_config are
                                        * the same.  fp64, no contraction, in the order written.  One transition (to absolute time tau, one particle j, after
                                        * the counters' reset, which is unchanged and only on the first call of a gap loop): for leap l = 0 .. K-1
                                        *   a[0 .. R) = the propensities at the current x, as under Gillespie (the rates of the moment -- a schedule applies
                                        *   as before --, a value not > 0 counts as 0.0);  for r = 0 .. R-1 in order:
                                        *     lam = a[r] / (double)K;  n = rpois(lam);
                                        *     cap = the minimum of x[c] over the species c with nu[r][c] < 0 (none: no cap);  n = min(n, cap);
                                        *     x[c] = x[c] + nu[r][c] * n for every c.
                                        * The propensities are not recomputed inside a leap; the cap sees the x that the earlier reactions of the leap left, so
                                        * no species goes below 0.0 from a state without a negative component.
                                        * rpois(lam) for reaction r in leap l of transition call `call`: attempt a uses the Philox block q at
                                        *   (j, call, DRAW_TRANS | (((l * 8 + r) << 6 | a) << 8), stream),  u1 = u01(q.x, q.y), u2 = u01(q.z, q.w)
                                        * (the stride 8 is the most reactions, not R: appending a zero-rate reaction moves no key).
                                        *   !(lam > 0.0): 0.0.
                                        *   lam < 10.0: inversion by sequential search on u1 of attempt 0:  p = exp(-lam); F = p; k = 0.0;
                                        *     while (u1 > F && k < 128.0) { k = k + 1.0; p = p * lam / k; F = F + p; }  return k;
                                        *   lam >= 10.0: Hoermann's transformed rejection with squeeze (PTRS, 1993):
                                        *     slam = sqrt(lam); loglam = log(lam); b = 0.931 + 2.53 * slam; a_ = -0.059 + 0.02483 * b;
                                        *     invalpha = 1.1239 + 1.1328 / (b - 3.4); vr = 0.9277 - 3.6224 / (b - 2.0);
                                        *     attempts a = 0 .. 63:  U = u1 - 0.5; V = u2; us = 0.5 - fabs(U); k = floor((2.0 * a_ / us + b) * U + lam + 0.43);
                                        *       accept k if us >= 0.07 && V <= vr;  reject if k < 0.0 || (us < 0.013 && V > us);  otherwise accept k if
                                        *       log(V) + log(invalpha) - log(a_ / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0)   (the device's lgamma);
                                        *     after 64 rejections floor(lam) (not reachable in practice: the loop is bounded).
                                        * Log-likelihood, APF look-ahead (the Euler mean of the particles as they stand), counters, BSSM_OPT_MV_Y_MISSING, tau of
                                        * the schedule, resampling and the outputs are as under Gillespie; the APF's second-stage transition is a tau-leap
                                        * transition that never resets.  bssm_dump_rpois returns the sampler's draws. */
#define BSSM_OPT_RN_METHOD (BSSM_OPT_RN_LEAPS + 1)   /* = 15: it qualifies BSSM_OPT_RN_LEAPS.  [0] reaction networks (BSSM_MODEL_RNET, BSSM_MODEL_RNET_NB; ignored by every other model): 0 = BSSM_OPT_RN_LEAPS decides as
                                        * above (0 Gillespie's direct method, K tau-leaping); 1 = Euler-multinomial leaps, BSSM_OPT_RN_LEAPS = K in 1 .. 1024 of them per
                                        * unit of time.  A value outside {0, 1} is refused here (BSSM_ERR_ARG); 1 with BSSM_OPT_RN_LEAPS = 0 is refused by bssm_pf_run and
                                        * bssm_pf_run_batch at the call (the two options are set one after the other), as is a block with a reaction that has neither
                                        * a source nor is sourceless (below), before any launch.  The blocks and bssm_pf_config are the same.  fp64, no contraction,
                                        * in the order written.
                                        * Classification of a reaction (static, from the block alone):
                                        *   source(r) = the one reactant c in {s1[r], s2[r]} with nu[r][c] == -1, provided the other reactant (if any) has nu[r][.] >= 0
                                        *               (a catalyst: I in S + I -> E + I) and no species that is not a reactant has nu[r][.] < 0;  o(r) = the other
                                        *               reactant, if any.
                                        *   sourceless: no species has nu[r][.] < 0 (order 0: immigration; catalytic production X -> 2X).
                                        *   refused:    everything else -- both reactants consumed (A + B -> C), a reactant with nu < -1, a species that is no
                                        *               reactant with nu < 0.
                                        * One transition (one unit of time, to absolute time tau, particle j, transition call `call`).  After the counters' reset
                                        * (unchanged, only on the first call of a gap loop), for leap l = 0 .. K-1, with x the state at the start of the leap, held for
                                        * the whole leap, and xn = x:
                                        *   1. for each species c = 0 .. d-1 in order, over the reactions r_1 < r_2 < ... with source(r) == c:
                                        *        h_r = kr[r], times x[o(r)] if the reaction has another reactant; a value that is not > 0 counts as 0.0  (kr: the rates
                                        *              of the moment, as for the propensities -- a rate schedule applies unchanged)
                                        *        H = 0.0 + h_{r_1} + h_{r_2} + ...  (left to right);  if !(H > 0.0) every count of the group is 0.0, nothing is drawn;  else
                                        *        pe = -expm1(-H / (double)K);  rem = x[c];  prem = 1.0;  for each i in order:
                                        *          p_i = (h_{r_i} / H) * pe;  q = p_i / prem;  if (!(q > 0.0)) q = 0.0;  if (q > 1.0) q = 1.0;
                                        *          n_i = rbinom(rem, q);  rem = rem - n_i;  prem = prem - p_i;  xn[c'] = xn[c'] + nu[r_i][c'] * n_i for every c'
                                        *   2. for each sourceless reaction r in order:  a_r = the propensity at x;  n = rpois(a_r / (double)K) (BSSM_OPT_RN_LEAPS's
                                        *      sampler, not capped);  xn[c'] = xn[c'] + nu[r][c'] * n for every c'
                                        *   3. x = xn
                                        * A compartment loses at most what it held; what arrives during a leap cannot leave in it; the order of the groups and of the
                                        * reactions inside a group changes no distribution.
                                        * Draw keys: reaction r in leap l, attempt a, reads the Philox block w at
                                        *   (j, call, DRAW_TRANS | (((l * 8 + r) << 6 | a) << 8), stream),  u1 = u01(w.x, w.y), u2 = u01(w.z, w.w)   (rpois's layout).
                                        * rbinom(n, q), n an integer-valued double:
                                        *   !(n > 0.0) or !(q > 0.0): 0.0.   q >= 1.0: n.   flip = q > 0.5;  qq = flip ? 1.0 - q : q;  the result is flip ? n - k : k with
                                        *   n * qq < 10.0: inversion by sequential search on u1 of attempt 0:
                                        *     pr = exp(n * log1p(-qq)); F = pr; k = 0.0; odds = qq / (1.0 - qq);
                                        *     while (u1 > F && k < n && k < 128.0) { k = k + 1.0; pr = pr * ((n - k + 1.0) / k) * odds; F = F + pr; }
                                        *   otherwise Hoermann's transformed rejection with squeeze (BTRS, 1993), at most 64 attempts:
                                        *     spq = sqrt((n * qq) * (1.0 - qq)); b = 1.15 + 2.53 * spq; a_ = (-0.0873 + 0.0248 * b) + 0.01 * qq; cc = n * qq + 0.5;
                                        *     vr = 0.92 - 4.2 / b;
                                        *     attempts a = 0 .. 63:  U = u1 - 0.5; V = u2; us = 0.5 - fabs(U); k = floor((2.0 * a_ / us + b) * U + cc);
                                        *       accept k if us >= 0.07 && V <= vr;  reject if k < 0.0 || k > n;  otherwise accept k if, with
                                        *       alpha = (2.83 + 5.1 / b) * spq; m = floor((n + 1.0) * qq); lr = log(qq / (1.0 - qq)),
                                        *       log(V * alpha / (a_ / (us * us) + b)) <=
                                        *         (((lgamma(m + 1.0) + lgamma(n - m + 1.0)) - lgamma(k + 1.0)) - lgamma(n - k + 1.0)) + (k - m) * lr   (the device's lgamma);
                                        *     after 64 rejections k = floor(n * qq) (not reachable in practice: the loop is bounded).
                                        * Log-likelihoods, BSSM_OPT_MV_Y_MISSING, the APF look-ahead (the Euler mean of the particles as they stand), counters, tau of
                                        * the schedule, resampling and the outputs are as under Gillespie; the APF's second-stage transition is an Euler-multinomial
                                        * transition that never resets.  bssm_dump_rbinom returns the sampler's draws. */
#define BSSM_OPT_RN_NOISE (BSSM_OPT_RN_LEAPS + 2)    /* = 16: it qualifies BSSM_OPT_RN_METHOD = 1.  [0] reaction networks (ignored by every other model): 1 = gamma white noise on the
                                        * rates (extra-demographic stochasticity; He, Ionides and King 2010).  A value outside {0, 1} is refused here; 1 with
                                        * BSSM_OPT_RN_METHOD != 1 or BSSM_OPT_RN_LEAPS = 0 is refused by bssm_pf_run and bssm_pf_run_batch (BSSM_ERR_ARG, before any launch).
                                        * The packed block then carries lead[R], sigma[R] directly after G[p][d] (BSSM_MODEL_RNET_NB: after size[p]), in front of
                                        * the optional tails; every length is the one without noise + 2 R.  lead[r] = -1 for a reaction without noise, otherwise
                                        * the lowest reaction index g of r's noise group (lead[g] == g, lead[r] <= r, else BSSM_ERR_ARG); sigma[r] = the group's
                                        * sigma, finite and > 0 and one value per group (else BSSM_ERR_ARG); a block without any group is refused.
                                        * The Euler-multinomial transition above changes in one place: the integrated per-capita hazard of reaction r over leap l
                                        * is h_r * w_r instead of h_r / K, with
                                        *   r in group g:   s2 = sigma_g * sigma_g;  sh = 1.0 / ((double)K * s2);  w_r = s2 * rgamma(sh)   (one draw per particle,
                                        *                   call, leap and group: mean 1 / K, variance sigma^2 / K);      r in no group:  w_r = 1.0 / (double)K;
                                        *   step 1: hw_r = h_r * w_r;  H = 0.0 + hw_{r_1} + hw_{r_2} + ...;  nothing is drawn if !(H > 0.0);  pe = -expm1(-H);
                                        *           p_i = (hw_{r_i} / H) * pe;  the clamp, rbinom, rem and prem as above;     step 2: n = rpois(a_r * w_r).
                                        * rgamma(sh): Marsaglia and Tsang (2000), the normal by inversion (AS 241).  Attempt a of leader g in leap l reads the Philox
                                        * block w at (j, call, DRAW_TRANS | (1u << 27) | (((l * 8 + g) << 6 | a) << 8), stream) (bit 27: the other keys end at bit 26);
                                        * u1 = u01(w.x, w.y), u2 = u01(w.z, w.w).
                                        *   boost = sh < 1.0;  al = boost ? sh + 1.0 : sh;  dd = al - 1.0 / 3.0;  cc = 1.0 / sqrt(9.0 * dd);
                                        *   attempts a = 0 .. 62:  x = qnorm(u1);  v = 1.0 + cc * x;  reject if !(v > 0.0);  v = v * v * v;  x2 = x * x;
                                        *     accept if u2 < 1.0 - 0.0331 * (x2 * x2);  otherwise accept if log(u2) < 0.5 * x2 + dd * ((1.0 - v) + log(v));
                                        *     the result is dd * v;   after 63 rejections dd (not reachable in practice: the loop is bounded);
                                        *   if boost: result = result * exp(log(ub) / sh), ub the u1 of the block at a = 63.
                                        * A w that underflows to 0.0 is a leap without hazard.  Densities, the APF look-ahead (the noise has mean 1 / K: the Euler mean
                                        * stands), counters and tau of the schedule are unchanged.  bssm_dump_rgamma returns the sampler's draws. */
int bssm_ctx_set_option(bssm_ctx* ctx, int option, int value);
int bssm_ctx_get_stamps(bssm_ctx* ctx, long long* out /* [4][16] */);
/* Fused path bookkeeping: out[0] runs started fused, out[1] fused launches, out[2] runs repeated on the multi-launch path because a
 * record needed another block's terms, out[3] runs repeated after a time-out (workgroups not all resident: the GPU was shared). */
int bssm_ctx_fused_stats(bssm_ctx* ctx, long long* out /* [4] */);
/* bssm_pf_run_multi bookkeeping, kept on the call's ctxs[0]: out[0] calls that took the lock-step kernels (one launch carries every
 * filter), out[1] calls that ran one filter after the other through bssm_pf_run.  Plain host counters, no device work. */
int bssm_ctx_multi_stats(bssm_ctx* ctx, long long* out /* [2] */);
int bssm_ctx_fused_stamps(bssm_ctx* ctx, long long* out /* [2][24]: DEV builds, clock64() stage stamps of the last fused launch */);

/* ---- resamplers: host-pointer form (what the R glue binds) --------------- */
/* n outputs over nw weights (the reference always passes n == nw).
 * U: the uniform draw(s) the reference takes from R's RNG --
 *   systematic : one double  (R::runif(0,1),   src/resampling.cpp:55)
 *   stratified : n doubles   (Rcpp::runif(n),  src/resampling.cpp:28)
 *   multinomial: n doubles   (inverse-CDF draws; distributional parity only,
 *                             the reference uses Rcpp::sample)
 * indices_out: n int32, 1-based. */
int bssm_resample_systematic(bssm_ctx* ctx, int n, const double* weights, int nw, double U, int* indices_out);
int bssm_resample_stratified(bssm_ctx* ctx, int n, const double* weights, int nw, const double* U, int* indices_out);
int bssm_resample_multinomial(bssm_ctx* ctx, int n, const double* weights, int nw, const double* U, int* indices_out);
/* Rcpp::sample(n, n, true, prob) as published (what src/resampling.cpp:11 draws): U = its n unif_rand() values in order;
 * n must equal nw ("probs.size() != n!").  This is the form the R glue binds for _bayesSSM_resample_multinomial_cpp. */
int bssm_resample_multinomial_r(bssm_ctx* ctx, int n, const double* weights, int nw, const double* U, int* indices_out);

/* Device-pointer form: weights / U / indices already in HBM; runs on the
 * context's stream and does not synchronise.  kind = BSSM_STRATIFIED/... ;
 * d_U may be NULL for systematic (then U_scalar is used).  cum_out (optional,
 * device, nw doubles) receives the exact sequential cumulative sum. */
int bssm_resample_device(bssm_ctx* ctx, int kind, int n, const double* d_weights, int nw,
                         double U_scalar, const double* d_U, int* d_indices_out, double* d_cum_out);
/* Status of the last device-form call (synchronises the stream). */
int bssm_resample_device_status(bssm_ctx* ctx);

/* Host-pointer form with diagnostics: cum_out (optional, nw doubles) receives
 * the exact sequential cum_sum of prob = weights/sum(weights)
 * (src/resampling.cpp:24-25,51-52); stats (optional, 4 long long):
 * {blocks with a literal tail, serial block walks, literal terms, scan blocks}.
 * kind = BSSM_STRATIFIED / BSSM_SYSTEMATIC / BSSM_MULTINOMIAL; U as above
 * (systematic reads U[0]). */
int bssm_resample_ex(bssm_ctx* ctx, int kind, int n, const double* weights, int nw, const double* U,
                     int* indices_out, double* cum_out, long long* stats);

/* ---- particle filter ---------------------------------------------------- */
/* BSSM_MODEL_LGMV: pieces that change with time in a known way, given as DATA next to y (host pointers; any may be NULL = the
 * packed block's constant piece).  The reference hands every closure the time index (R/bootstrap_filter.R:142-148); here
 *   b_t  [n_times][d]   the transition TO absolute time tau is x' = A x + b_t[tau - 1] + L z, tau = prev_t + step in the gap loop
 *                       (R/particle_filter_core.R:125-136); the APF's second transition (:159) and its aux transition mean use
 *                       tau = the observation's time.  n_times >= the last observation time (T without obs_times).
 *   h0_t [T][p], H_t [T][p][d]   indexed by OBSERVATION ROW i, as y is: the likelihood, the aux likelihood and the move's two
 *                       likelihoods at observation i use row i.  Must be NULL when p == 0.
 * All values must be finite.  bssm_pf_run_batch shares the arrays among the filters of a call, as it shares y;
 * bssm_pf_run_batch_tv takes one array set per filter (or per group of filters), see bssm_mv_tv_batch. */
typedef struct {
    int n_times;
    const double* b_t;
    const double* h0_t;
    const double* H_t;
} bssm_mv_tv;

typedef struct {
    int model;               /* BSSM_MODEL_*                                   */
    int algorithm;           /* BSSM_BPF / BSSM_APF                            */
    int resample_algorithm;  /* BSSM_SIS / SISR / SISAR                        */
    int resample_fn;         /* BSSM_STRATIFIED / SYSTEMATIC / MULTINOMIAL     */
    long long num_particles;
    int T;                   /* number of observations                         */
    double threshold;        /* NaN: NULL => auto (R/particle_filter_core.R:44-50); any other value is used as given */
    const double* theta;     /* model parameters (host), n_theta doubles       */
    int n_theta;
    const double* y;         /* observations (host), T doubles                 */
    const int* obs_times;    /* host, T ints, or NULL => 1..T                  */
    unsigned long long seed;     /* device generator key (throughput mode)     */
    unsigned long long stream;   /* e.g. chain index / iteration               */
    /* parity mode: injected draws (host pointers); NULL => device generator  */
    const double* z_init;    /* N standard normals                             */
    const double* z_trans;   /* [n_trans_calls][N]                             */
    const double* u_res;     /* systematic [n_res_calls]; else [n_res_calls][N] */
    int return_particles;    /* fill particles_history / weights_history       */
    int return_ancestors;    /* fill ancestors                                 */
    /* BSSM_RMPF only: proposal sd of the move, and (parity mode) its injected draws [T][N] each
     * (BSSM_MODEL_LGMV: z_move [T][d][N], u_move [T][N]) */
    double move_sd;
    const double* z_move;
    const double* u_move;
    /* BSSM_MODEL_LGMV only (ignored for the other models): time-varying b / h0 / H, or NULL => the block's constants */
    const bssm_mv_tv* mv_tv;
} bssm_pf_config;

typedef struct {
    double* state_est;        /* (T+1) x d, row-major (d = 1; 2 for the SIR model) */
    double* ess;              /* T+1                                           */
    double* loglike_history;  /* T, cumulative (R/particle_filter_core.R:209)  */
    double* loglike;          /* 1                                             */
    int* early_return_step;   /* 1: 0 = ran to the end, i = degenerate at obs i (:189-202) */
    int* n_res_calls;         /* 1                                             */
    int* resampled;           /* T or NULL: weight-triggered resample ran at obs i */
    int* ancestors;           /* [max_res_calls][N] 1-based, or NULL           */
    double* particles_history;/* (T+1) x (N d) row-major rows = as.numeric(N x d), or NULL */
    double* weights_history;  /* (T+1) x N, or NULL                            */
    double* device_ms;        /* 1 or NULL: HIP-event time of the run on the stream */
    long long* scan_stats;    /* 3 or NULL: {blocks with a literal tail, serial walks, literal terms} summed over the run */
} bssm_pf_result;

int bssm_pf_run(bssm_ctx* ctx, const bssm_pf_config* cfg, bssm_pf_result* res);

/* ---- genealogy (ancestor-tracing) smoother ------------------------------------------------------------------------
 * bssm_pf_run_smooth runs the filter bssm_pf_run would run for cfg with return_particles = return_ancestors = 1 (the launch
 * path those two select), keeps the histories and the ancestor rows on the device -- they come to the host only where cfg
 * itself asks for them -- and traces every final particle back through its ancestors there:
 *   b_T(j) = j,  b_{i-1}(j) = a_i(b_i(j)),  a_i = the ancestor rows of observation i composed in launch order (none: identity;
 *   the auxiliary filter's two: first[second[j]]);
 *   smoothed[i][c] = sum_j W[j] P[i][c][b_i(j)]  with W = weights_history[T], P[i] = particles_history[i];
 *   n_lineages[i]  = the number of distinct b_i(j)  (n_lineages[T] == N);
 *   trajectories[k][i][c] = P[i][c][b_i(j_k)],  j_k = the first j with cum[j] >= u_k, cum the multinomial resampler's exact
 *   cum_sum of W (cumsum(W / sum(W)), both sequential in fp64), N where u_k lies beyond cum[N-1];  u_k from the generator
 *   under (cfg->seed, cfg->stream) with a purpose tag of its own.
 * Every filter output in res is what bssm_pf_run writes for the same cfg, bit for bit.  A run that returns early on degenerate
 * weights (early_return_step != 0) is not traced: smooth_ms = 0 and the smoother's arrays are left as they were.
 * BSSM_ERR_ARG for a NULL struct or array or n_trajectories outside 0 .. 4096; BSSM_ERR_CAPACITY, with the bytes needed in
 * bssm_last_error(), when the histories do not fit the device's free memory. */
typedef struct {
    int n_trajectories;       /* K: 0 .. 4096 */
} bssm_smooth_config;

typedef struct {
    double* smoothed;         /* (T+1) x d, row-major, as state_est               */
    int* n_lineages;          /* T+1                                              */
    double* trajectories;     /* K x (T+1) x d, or NULL when K == 0               */
    double* trajectory_u;     /* K uniforms of the terminal draw, or NULL when K == 0 */
    int* trajectory_index;    /* K terminal particles j_k, 1-based, or NULL when K == 0 */
    int* call_obs;            /* [max_res_calls] the observation index (1 .. T) of every ancestor row, n_res_calls of them written; or NULL */
    double* smooth_ms;        /* 1 or NULL: HIP-event time of the trace alone     */
} bssm_smooth_result;

int bssm_pf_run_smooth(bssm_ctx* ctx, const bssm_pf_config* cfg, bssm_pf_result* res, const bssm_smooth_config* scfg,
                       bssm_smooth_result* sres);

/* ---- closure mode: the device half of one observation for ARBITRARY models -------------------------------------
 * The reference's models are user closures (init_fn / transition_fn / log_likelihood_fn, R/particle_filter-doc.R:7-35);
 * closures cannot run on the GPU, so for models that are not built in the host evaluates them (any state dimension,
 * y a T x p matrix, t-dependent) and hands the device the N log-weights of the observation; the device does what
 * .particle_filter_core does with them (R/particle_filter_core.R:189-224):
 *   all(lw < -1e8) guard; max / exp / sum normalisation -> weights; log-likelihood increment max + log(sum) - log(N);
 *   ESS = 1 / sum(w^2); resample decision (SIS / SISR / SISAR vs threshold; `always` = the APF's first stage and the
 *   resample-move filter); resample_*_cpp -> 1-based ancestor indices (the host gathers particles[indices, ], as
 *   R/resampling.R:20,40,60 does).
 * lw: N host doubles.  U: the resampler's draws (1 for systematic, N otherwise) or NULL => generator (seed, stream, call).
 * weights_out (N, optional), ancestors_out (N, required when a resample can happen), scalars[4] = {log-likelihood
 * increment, ESS, max, sum}; flags_out[2] = {resampled, degenerate (all log-weights < -1e8: the caller returns -Inf)}. */
int bssm_pf_weigh_resample(bssm_ctx* ctx, long long n, const double* log_weights, int always, int resample_algorithm,
                           double threshold, int resample_fn, const double* U, unsigned long long seed,
                           unsigned long long stream, int call, double* weights_out, int* ancestors_out,
                           double* scalars_out, int* flags_out);

/* ---- one filter, particle blocks sharded over ranks (prototype) ----
 * Rank r of `world` holds the particles [r N / world, (r + 1) N / world) = a contiguous run of scan blocks of the GLOBAL
 * block numbering and runs the same kernels on them; per observation the ranks exchange
 *   (1) the per-block log-sum-exp partials         (all_gather, 24 B a block)       R/particle_filter_core.R:204-207
 *   (2) the block records of sum(w)                (all_gather)                      src/resampling.cpp:20
 *   (3) the block records of cumsum(w / total)     (all_gather)                      src/resampling.cpp:24-25
 *   (4) the resampled particles                    (all-to-all: every rank's outputs are one contiguous range) R/resampling.R:40
 * and every rank resolves the exact sums redundantly, so the result is bit-identical to bssm_pf_run on one GPU.
 * The collectives are the caller's (host-staged callbacks: torch.distributed / RCCL / MPI); they return 0 on success.
 * Limits of the prototype: bootstrap filter, scalar-state Gaussian models, stratified / systematic resampling,
 * N a multiple of world x 2048 and at most 2^22 IN ALL (the block-record workspace of this build: every rank resolves the records
 * of all blocks -- inside the consuming kernels up to 2^20, by one 1024-thread workgroup per rank above), no histories.  Every rank
 * returns the full result.  A rank whose run state carries an error is noticed by all ranks at exchange (4) of that observation (its
 * status rides along) and all leave together; a callback that fails returns at once on that rank -- the collective layer's own
 * time-out is what ends the other ranks' wait then. */
typedef struct {
    int rank, world;
    int (*all_gather)(void* user, const void* send, void* recv, long long bytes_per_rank);       /* recv holds world x bytes_per_rank */
    int (*exchange)(void* user, const double* send, const long long* send_counts /* [world] */,
                    double* recv, const long long* recv_counts /* [world] */);                    /* all-to-all of doubles, pieces in rank order */
    void* user;
    /* 0: the callbacks receive HOST pointers (the library stages device data through host memory: gloo, MPI, the one-GPU tests).
     * 1: they receive DEVICE pointers of the context's GPU (RCCL: ncclAllGather / grouped ncclSend + ncclRecv, no host copies).  The
     *    library has synchronised the context's stream before a call; the callback either completes before it returns or enqueues
     *    its work on bssm_ctx_stream(ctx), which the library synchronises again after the call.  all_gather may be called IN PLACE
     *    (send == recv + rank x bytes_per_rank), as ncclAllGather allows. */
    int device_buffers;
} bssm_shard;
int bssm_pf_run_sharded(bssm_ctx* ctx, const bssm_pf_config* cfg, const bssm_shard* shard, bssm_pf_result* res);

/* ---- many small filters per launch ----------------------------------------
 * The reference runs its filters at N <= 1000 inside PMMH (R/pmmh.R:403-415,445-457) and 100 of them at N = 100 in the
 * pilot (R/pmmh_tuning.R:111-151): launch-bound one at a time.  bssm_pf_run_batch runs n_filters independent bootstrap
 * filters -- same data and settings (cfg), one theta / seed / stream each -- in ONE kernel launch, one workgroup per
 * filter with the whole T loop on chip (cfg->algorithm: BPF, APF or RMPF; every built-in model and resampler).  Each
 * filter's outputs are bit-identical to bssm_pf_run with that theta, seed and stream.  Limits: num_particles <=
 * bssm_pf_batch_max_particles() (2048), device generator only (cfg->theta, seed, stream, z_*, u_res, return_* are not used).
 * BSSM_MODEL_LGMV (bootstrap filter, stratified / systematic resampling): thetas holds n_filters packed blocks in the layout
 * bssm_pf_run takes (cfg->n_theta doubles each, without log(sd)), all of the same (d, p); cfg->y is [T][p]; state_est is
 * [n_filters][T+1][d]; num_particles <= bssm_pf_batch_max_particles_mv(d) (2048 for d <= 4, at least 1000 for d <= 8). */
typedef struct {
    double* loglike;          /* [n_filters]                                                    */
    double* state_est;        /* [n_filters][T+1][d] or NULL  (d = 2 for the SIR model, the block's d for LGMV) */
    double* ess;              /* [n_filters][T+1] or NULL                                       */
    double* loglike_history;  /* [n_filters][T]   or NULL                                       */
    int* early_return_step;   /* [n_filters] or NULL                                            */
    int* n_res_calls;         /* [n_filters] or NULL                                            */
    int* status;              /* [n_filters] or NULL: per-filter BSSM_* status; when NULL the first failure is returned */
    double* device_ms;        /* 1 or NULL                                                      */
} bssm_pf_batch_result;

int bssm_pf_batch_max_particles(void);
int bssm_pf_batch_max_particles_mv(int d);      /* BSSM_MODEL_LGMV with d state components; 0 for d outside 1..8 */
/* BSSM_MODEL_RNET and BSSM_MODEL_RNET_NB in bssm_pf_run_batch (bootstrap filter only; thetas: n_filters packed blocks of one (d, R, p); cfg->y [T][p];
 * state_est [n_filters][T+1][d]): the largest num_particles with d species, at least 1000 for every d; 0 for d outside 1..8 */
int bssm_pf_batch_max_particles_rn(int d);
/* BSSM_MODEL_RNET_NB: the tables c(t, k) of n_filters filters on one y [T][p] as bssm_pf_run_batch fills them on the host:
 * out [n_filters][T][p], filter f with the sizes at sizes + f * size_stride (for packed blocks: thetas + the offset of size[p],
 * size_stride = n_theta).  No device work; exported so that a benchmark can time the host's share of a batched call. */
int bssm_rn_nb_tables(const double* y, int T, int p, int n_filters, const double* sizes, long long size_stride, double* out);
int bssm_pf_run_batch(bssm_ctx* ctx, const bssm_pf_config* cfg, int n_filters, const double* thetas /* [n_filters][cfg->n_theta] */,
                      const unsigned long long* seeds, const unsigned long long* streams, bssm_pf_batch_result* res);

/* BSSM_MODEL_LGMV: time-varying b / h0 / H that differ between the filters of one batched call -- arrays that depend on the
 * sampled parameters (an input gain b_t = g u_t, a seasonal amplitude h0_t = a sin(w t)), one SET per parameter draw.  The sets
 * of a piece lie one after the other (host memory); filter f reads set set_of[f], so the filters that share a draw (the
 * pilot's repeated runs, R/pmmh_tuning.R:111-151) share one set and the upload grows with the draws, not with the filters.
 * A piece is indexed within its set exactly as in bssm_mv_tv.  A stride is the full size of one set in doubles
 * (n_times d, T p, T p d), or 0: one array shared by every filter.  A NULL pointer = the packed block's constant piece.
 * Every set is validated (and uploaded), referenced by a filter or not. */
typedef struct {
    int n_times;              /* rows of b_t per set */
    int n_sets;               /* G >= 1 array sets */
    const int* set_of;        /* [n_filters] set index of each filter; NULL: filter f uses set f (then n_sets == n_filters) or the one set */
    const double* b_t;  long long b_stride;    /* [G][n_times][d]; stride in doubles between sets, 0 = one array shared by all */
    const double* h0_t; long long h0_stride;   /* [G][T][p]    */
    const double* H_t;  long long H_stride;    /* [G][T][p][d] */
} bssm_mv_tv_batch;

/* bssm_pf_run_batch for BSSM_MODEL_LGMV with the array sets of `tv` (cfg->mv_tv must be NULL).  Filter f returns bit for bit
 * what bssm_pf_run returns for thetas[f], seeds[f], streams[f] and a bssm_mv_tv of its set.  BSSM_ERR_ARG with a message
 * "bssm_pf_run_batch_tv: mv_tv: ..." for arrays bssm_pf_run would refuse, a stride that is neither 0 nor a set's size, or a set
 * index outside [0, n_sets); BSSM_ERR_CAPACITY when the sets do not fit the staging buffers. */
int bssm_pf_run_batch_tv(bssm_ctx* ctx, const bssm_pf_config* cfg, int n_filters, const double* thetas,
                         const unsigned long long* seeds, const unsigned long long* streams,
                         const bssm_mv_tv_batch* tv, bssm_pf_batch_result* res);

/* ---- genealogy smoother of a batched call --------------------------------------------------------------------------
 * bssm_pf_run_batch_smooth runs the filters bssm_pf_run_batch (tv == NULL) or bssm_pf_run_batch_tv would run, with the kernel
 * form that also leaves every filter's histories on the device, and traces all of them in one more launch (one workgroup per
 * filter).  Filter f's smoothed / n_lineages / trajectories / trajectory_u / trajectory_index are bit for bit what
 * bssm_pf_run_smooth returns for thetas[f], seeds[f], streams[f] (and the filter's set of tv); the filter outputs in res are
 * bssm_pf_run_batch's, bit for bit.  The K paths of a filter are drawn under that filter's own (seed, stream).
 * A filter that returned early on degenerate weights, or whose status is not BSSM_OK, is not traced: traced[f] = 0, its rows of
 * the double arrays are NaN and those of the int arrays 0; the other filters are unaffected.
 * Covers the bootstrap filter of BSSM_MODEL_LGMV* and BSSM_MODEL_RNET / _NB with stratified / systematic resampling
 * (BSSM_ERR_ARG names this for anything else).  The histories take n_filters ((T+1) d N 8 + max(T,1) (N + 1) 4 + N 8) bytes
 * of device memory, checked against what is free before anything is launched: BSSM_ERR_CAPACITY with the bytes in
 * bssm_last_error() when they do not fit (the call is not split). */
typedef struct {
    double* smoothed;         /* [n_filters][T+1][d]                                     */
    int* n_lineages;          /* [n_filters][T+1]                                        */
    double* trajectories;     /* [n_filters][K][T+1][d], or NULL when K == 0             */
    double* trajectory_u;     /* [n_filters][K], or NULL when K == 0                     */
    int* trajectory_index;    /* [n_filters][K] 1-based, or NULL when K == 0             */
    int* traced;              /* [n_filters]: 1 traced, 0 not                            */
    double* smooth_ms;        /* 1 or NULL: HIP-event time of the trace launch alone     */
} bssm_smooth_batch_result;

int bssm_pf_run_batch_smooth(bssm_ctx* ctx, const bssm_pf_config* cfg, int n_filters, const double* thetas,
                             const unsigned long long* seeds, const unsigned long long* streams,
                             const bssm_mv_tv_batch* tv /* may be NULL */, bssm_pf_batch_result* res,
                             const bssm_smooth_config* scfg, bssm_smooth_batch_result* sres);

/* K (<= 4) independent LARGE filters in lock-step on one stream: the kernels of bssm_pf_run with one argument set per filter
 * (blockIdx.y), so that independent PMMH chains (R/pmmh.R:511-531) share the launches of their filter runs (R/pmmh.R:445-457)
 * instead of each walking its own chain of latency-bound launches.  ctxs[k] owns filter k's buffers (same device); cfg holds the
 * shared data and settings (theta / seed / stream / injected draws / histories unused), thetas [n_filters][cfg->n_theta].  Each
 * filter's outputs are bit-identical to bssm_pf_run with that theta, seed and stream.  Configurations the lock-step kernels do
 * not cover (APF / RMPF, SIR, multinomial, N > 2^20) run one after the other through bssm_pf_run. */
int bssm_pf_run_multi(bssm_ctx* const* ctxs, int n_filters, const bssm_pf_config* cfg, const double* thetas,
                      const unsigned long long* seeds, const unsigned long long* streams, bssm_pf_batch_result* res);

/* Number of transition_fn / resample calls the filter makes at most (sizes of
 * the injected-draw arrays and of `ancestors`). */
int bssm_pf_noise_shape(int algorithm, int T, const int* obs_times, int* max_trans, int* max_res);

/* Dump the device generator's draws so a CPU run can consume the same ones
 * (host output pointers). */
int bssm_dump_normals(bssm_ctx* ctx, unsigned long long seed, unsigned long long stream,
                      int purpose /* 1 init, 2 transition */, int call, long long n, double* out);
int bssm_dump_normals_mv(bssm_ctx* ctx, unsigned long long seed, unsigned long long stream, int purpose, int call, long long N, int d, double* out /* [d][N] */);
int bssm_dump_uniforms(bssm_ctx* ctx, unsigned long long seed, unsigned long long stream,
                       int call, long long n, double* out);
int bssm_dump_move_draws(bssm_ctx* ctx, unsigned long long seed, unsigned long long stream,
                         int call, long long n, double* z_out, double* u_out);
/* BSSM_MODEL_LGMV's move draws of observation `call` (1..T): z_out [d][N] normals, u_out [N] acceptance uniforms; at d = 1 the
 * same numbers as bssm_dump_move_draws */
int bssm_dump_move_draws_mv(bssm_ctx* ctx, unsigned long long seed, unsigned long long stream, int call, long long N, int d,
                            double* z_out /* [d][N] */, double* u_out /* [N] */);
/* The Poisson draws of the reaction networks' tau-leap transition (BSSM_OPT_RN_LEAPS): out[j] is what particle j draws for reaction r
 * (0 .. 7) in leap `leap` (0 .. 1023) of transition call `call` at the mean lam[j], j = 0 .. n-1 (host pointers). */
int bssm_dump_rpois(bssm_ctx* ctx, unsigned long long seed, unsigned long long stream, int call, int leap, int r, long long n,
                    const double* lam /* [n] */, double* out /* [n] */);
/* The binomial draws of the reaction networks' Euler-multinomial transition (BSSM_OPT_RN_METHOD): out[j] is what particle j draws for
 * reaction r (0 .. 7) in leap `leap` (0 .. 1023) of transition call `call` from n[j] trials at the probability q[j], j = 0 .. n_draws-1
 * (host pointers). */
int bssm_dump_rbinom(bssm_ctx* ctx, unsigned long long seed, unsigned long long stream, int call, int leap, int r, long long n_draws,
                     const double* n /* [n_draws] */, const double* q /* [n_draws] */, double* out /* [n_draws] */);
/* The gamma draws of the reaction networks' gamma white noise (BSSM_OPT_RN_NOISE): out[j] is what particle j draws for the noise group with
 * leader g (0 .. 7) in leap `leap` (0 .. 1023) of transition call `call` at the shape shape[j] (finite, > 0; scale 1), j = 0 .. n-1 (host
 * pointers). */
int bssm_dump_rgamma(bssm_ctx* ctx, unsigned long long seed, unsigned long long stream, int call, int leap, int g, long long n,
                     const double* shape /* [n] */, double* out /* [n] */);

/* Per-kernel-class device time of the last bssm_pf_run with profiling enabled
 * (bssm_ctx_set_profile(ctx, 1) inserts HIP events around every launch; slower,
 * so never inside a timed throughput region).  names: array of const char*. */
int bssm_ctx_set_profile(bssm_ctx* ctx, int enable);
int bssm_ctx_get_profile(bssm_ctx* ctx, int max_entries, const char** names, double* total_ms, long long* launches);

/* ---- PMMH: one chain ---------------------------------------------------- */
typedef struct {
    bssm_pf_config pf;         /* filter settings; theta/seed/stream are overwritten per iteration */
    int m;                     /* iterations (rows of theta_chain)                */
    int n_params;              /* == pf.n_theta                                   */
    const double* init_theta;  /* starting point (the reference uses the pilot mean, R/pmmh.R:373) */
    const double* proposal_cov;/* n_params x n_params, on the ORIGINAL scale (pilot covariance, :374) */
    const int* transform;      /* BSSM_TR_* per parameter                         */
    const int* prior_kind;     /* BSSM_PRIOR_* per parameter                      */
    const double* prior_a;     /* per parameter                                   */
    const double* prior_b;
    unsigned long long seed;   /* chain seed (R/pmmh.R:346,511)                   */
    int chain_index;
    int return_latent_state_est;
    /* parity mode: the chain-level draws as INPUTS (host pointers); NULL => the generator keyed by (seed, chain_index).
     * z_prop[i][0..n_params) = the rnorm(n_params) MASS::mvrnorm takes at iteration i (R/pmmh.R:425), u_accept[i] = the
     * runif(1) of the acceptance test (:492); row / entry 0 are not used (the loop starts at i = 2 in R). */
    const double* z_prop;      /* [m][n_params] or NULL */
    const double* u_accept;    /* [m] or NULL */
} bssm_pmmh_config;

typedef struct {
    double* theta_chain;       /* m x n_params, row-major                         */
    double* loglike_chain;     /* m                                               */
    double* state_est_chain;   /* m x (T+1) x d, or NULL                          */
    int* accepted;             /* 1: number of accepted proposals                 */
    double* device_ms;         /* 1 or NULL: summed filter device time            */
} bssm_pmmh_result;

int bssm_pmmh_chain(bssm_ctx* ctx, const bssm_pmmh_config* cfg, bssm_pmmh_result* res);
/* The chain-level draws the generator gives chain (seed, chain_index): what a CPU run of the same loop consumes
 * (z_prop_out [m][n_params], u_accept_out [m]; host pointers, no GPU needed). */
int bssm_pmmh_chain_draws(unsigned long long seed, int chain_index, int m, int n_params, double* z_prop_out, double* u_accept_out);

/* n_chains chains advancing in lock-step over bssm_pf_run_batch: iteration i of every chain is ONE kernel launch (one
 * workgroup per chain).  The chains must share data, filter settings and m, and meet bssm_pf_run_batch's limits
 * (N <= 2048).  ress[k] is exactly what bssm_pmmh_chain returns for
 * cfgs[k]; device_ms reports the total device time divided by n_chains. */
int bssm_pmmh_chains_batch(bssm_ctx* ctx, int n_chains, const bssm_pmmh_config* cfgs, bssm_pmmh_result* ress);
/* The lock-step loop over bssm_pf_run_multi for filters above the batched kernel's size: one context per chain, at most 4 chains. */
int bssm_pmmh_chains_multi(bssm_ctx* const* ctxs, int n_chains, const bssm_pmmh_config* cfgs, bssm_pmmh_result* results);

#ifdef __cplusplus
}
#endif
#endif /* BAYESSSM_AMD_H */
