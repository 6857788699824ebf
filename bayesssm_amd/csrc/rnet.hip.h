// rnet.hip.h -- mass-action reaction networks (SEIR, SIRS, Lotka-Volterra, birth-death, ...) on the device: d <= 8 species held as
// integer-valued doubles, R <= 8 reactions of order 0, 1 or 2, p <= 8 Poisson observation components.
//
// The reference's flagship vignette (vignettes/articles/stochastic-sir-model.Rmd:152-176, 285-310) is one instance; struct Sir
// (kernels.hip.h) hard-wires it.  This family states the same closures for any such network:
//   init_fn          every particle starts at x0                                       (no draws)
//   transition_fn    one unit of time of Gillespie's direct method, Sir::transition step for step:
//                      a_r = k_r | k_r x[s1] | (k_r x[s1]) x[s2]   (order 0 | 1 | 2);  a propensity that is not > 0 counts as 0.0
//                      total = a_0 + a_1 + ...                    (left to right);  stop when total <= 0
//                      one Philox block per event at (particle, call, DRAW_TRANS | ev << 8, stream):
//                      dt = -log(u01(r.x, r.y)) / total;  stop when t + dt > 1;  u = u01(r.z, r.w)
//                      the first r in 0 .. R-2 with u < (a_0 + ... + a_r) / total fires, otherwise reaction R-1;  x += nu[r]
//   log_likelihood   lambda_k = 0.0 + G_k0 x_0 + G_k1 x_1 + ...;   0.0 + sum_k Sir::dpois_log(y_k, lambda_k, lgamma(y_k + 1))
//                    over the observed k only: a NaN y_k (let through by the host under the context option mv_y_missing alone) is a
//                    component that was not observed -- mv_observed's test, a wave-uniform branch around lambda_k and the density;
//                    a row with nothing observed gives 0.0.  The look-ahead skips the same components.
//   aux (APF)        the same density at the one-unit Euler mean  m_c = x_c + nu[0][c] a_0 + nu[1][c] a_1 + ...,  lambda_k clamped at 0.0
// With d = 2, R = 2, p = 1, k = (lambda / n_total, gamma), s1 = (0, 1), s2 = (1, -1), nu = ((-1, +1), (0, -1)), G = (0, 1) every
// expression reduces bit for bit to struct Sir's, draw keys included (tests/test_gpu_rnet.py pins it).
// Counter species (incidence: the firings of a reaction since the previous report).  The block may end in a tail reset[d] of
// 0.0 / 1.0 after G; species c with reset[c] = 1.0 is a counter:
//   transition_fn(particles, t) sets every counter component to 0.0 before its Gillespie loop if and only if it is the first call
//   of the gap loop of R/particle_filter_core.R:125-136 (step == 1, that is t == prev_t + 1).
//   With obs_times gaps a counter therefore accumulates over the whole gap (weekly incidence from daily steps).  At a repeated
//   observation time (gap <= 0) nothing moves and nothing is reset.  The auxiliary filter's second-stage transition (:159, called
//   with t = prev_t) never resets, so under the reference's APF a counter spans gap + 1 units: the reference's own double
//   transition.  The APF look-ahead is unchanged (the Euler mean of the particles as they stand), as are the draw keys, the event
//   numbering and the arithmetic of everything else.  The state estimate and the histories report a counter like any species
//   (row 0 is x0).  A counter is no reactant of any reaction (the reset would change the dynamics): the host refuses such a block.
// Rate schedule (time-varying rates: seasons, interventions).  After reset[d] the block may carry a second tail  n_times,
// M[n_times][R]  of finite multipliers >= 0 (reset[d] is then always present, all 0.0 without counters).  The transition TO
// absolute time tau uses row tau - 1:  a_r = (k_r M[tau-1][r]) | (k_r M[tau-1][r]) x[s1] | ((k_r M[tau-1][r]) x[s1]) x[s2] -- one
// multiplication in front of today's, so a schedule of ones changes no bit (k * 1.0 is exact).  tau follows the multivariate
// family's b_t: prev_t + step in the gap loop (:125-136); the observation's time for the APF's second-stage transition (:159) and
// for the propensities of the APF look-ahead's Euler mean.  At a repeated observation time the bootstrap filter reads no row.
// The one new multiplication is taken on the host, in fp64 as the device would take it: the DEVICE copy of the block holds the
// products k_r M[tau-1][r] in the schedule's place (pf_run_rn, pf_run_batch_rn: rn_sched_products), so a row is the rate vector of
// its moment.  The kernels get "the rates of the moment" as a wave-uniform pointer (RnPar::rates_row: that row, or k itself
// without a schedule) and read it through the scalar cache, as the block, so the event loop holds no more live values than it
// did.  "No schedule" is a template parameter of k_step_rn (SCHED = false: the rates at rp.P + o_k(), the code as it was) and an
// offset into the block for k_pf_batch_rn's step; there is no runtime branch on it.  Draw keys, event numbering, the selection walk, the reset and everything else are as
// without a schedule.
// Negative-binomial (overdispersed) observations (BSSM_MODEL_RNET_NB; OBS = RN_OBS_NB below).  Component k is
//   y_k ~ NegBin(mean = mu_k, size = r_k):  variance mu + mu^2 / r,
// mu_k = lambda_k exactly as above (the same accumulation; for the look-ahead at the Euler mean, clamped at 0.0), r_k = size_k > 0 from
// the block: size[p] directly after G[p][d], in front of the optional tails (RnPar::nsz = p, so size() and every offset behind it
// move by p).  The density, in this order (rn_dnbinom_log):
//   if (!(mu > 0.0)) return (y == 0.0 && mu == 0.0) ? 0.0 : -inf;          as Sir::dpois_log treats lambda <= 0
//   s = r + mu;  lr = (r < mu) ? log(r / s) : log1p(-(mu / s));            as R's dnbinom_mu takes log(size / (size + mu))
//   if (y == 0.0) return r * lr;
//   return (c + r * lr) + y * log(mu / s);
// with the table entry  c(t, k) = (lgamma(y + r) - lgamma(r)) - lgamma(y + 1)  taken on the host with C's lgamma per (t, k) (0.0 where
// y is NaN, never read) and uploaded in the slot that holds lgamma(y + 1) for the Poisson family (lgyrow).  In the batched path c
// depends on the filter's own size: the table is [F][T][p] (BatchArgs::lgy_stride = T p; 0 = the one shared Poisson table).
// The family is a template parameter of rn_loglik, k_step_rn (the instantiations that take weights; the transition-only ones are
// shared), step_emul_rn and k_pf_batch_rn, Poisson by default: no runtime branch on it, and the Poisson instantiations fix
// rp.nsz = 0 at compile time, so they are the code they were.  y == 0 and the mv_observed test are wave-uniform; mu > 0 and r < mu
// are per lane.
// Tau-leaping (large populations; context option BSSM_OPT_RN_LEAPS = K in 1 .. 1024, 0 = Gillespie's method above; METH = RN_TAU_LEAP
// below).  The transition covers one unit of time, to absolute time tau, for one particle j.  After the counters' reset (unchanged, and
// only on `first`), for leap l = 0 .. K-1:
//   a[0 .. R) = the propensities at the current x, exactly as rn_propensities forms them (the rates of the moment; a value that is not
//   > 0 counts as 0.0; a rate schedule applies as above).  For r = 0 .. R-1 in order:
//     lam = a[r] / (double)K;   n = rpois(lam);
//     cap = the minimum of x[c] over the species c with nu[r][c] < 0 (no cap if the reaction consumes nothing);   n = min(n, cap);
//     x[c] = x[c] + nu[r][c] * n  for every c.
//   The propensities are not recomputed inside a leap.  The cap sees the x that the earlier reactions of the same leap have changed, so
//   no species goes below 0.0 from a state with no negative component.
// rpois(lam) for reaction r in leap l of call `call` (rn_rpois):
//   attempt a uses the Philox block q at (j, call, DRAW_TRANS | (((l * RNR + r) << 6 | a) << 8), stream);  u1 = u01(q.x, q.y),
//   u2 = u01(q.z, q.w).  The stride is RNR = 8, not R, so appending a zero-rate reaction moves no key.
//   !(lam > 0.0): 0.0.
//   lam < 10.0: inversion by sequential search on u1 of attempt 0:
//     p = exp(-lam); F = p; k = 0.0;   while (u1 > F && k < 128.0) { k = k + 1.0; p = p * lam / k; F = F + p; }   return k;
//     (the bound ends the walk for a u1 that rounding leaves above the summed mass)
//   lam >= 10.0: Hoermann's transformed rejection with squeeze (PTRS, 1993):
//     slam = sqrt(lam); loglam = log(lam);   b = 0.931 + 2.53 * slam; a_ = -0.059 + 0.02483 * b;
//     invalpha = 1.1239 + 1.1328 / (b - 3.4); vr = 0.9277 - 3.6224 / (b - 2.0);
//     for attempts a = 0 .. 63:   U = u1 - 0.5; V = u2; us = 0.5 - fabs(U);   k = floor((2.0 * a_ / us + b) * U + lam + 0.43);
//       accept if us >= 0.07 && V <= vr;   reject if k < 0.0 || (us < 0.013 && V > us);
//       otherwise accept if log(V) + log(invalpha) - log(a_ / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0)   (the device's lgamma)
//     after 64 rejections floor(lam) (not reachable in practice; it is there so that the loop is bounded).
// Unchanged: the log-likelihood, the APF look-ahead (the Euler mean of the particles as they stand), the counter semantics, missing
// observations, tau for the schedule, gather, carry, state estimate and histories.  The APF's second-stage transition is a tau-leap
// transition that never resets.  K is a wave-uniform kernel argument and the method a template parameter of the kernels with a transition
// (Gillespie by default: those instantiations are the code they were); there is no runtime branch on it.
// Euler-multinomial leaps (context option BSSM_OPT_RN_METHOD = 1 with BSSM_OPT_RN_LEAPS = K in 1 .. 1024; METH = RN_EULER_MULTINOM below): the
// discretisation of compartmental models that pomp's reulermultinom made the field's default.  Every individual of a compartment leaves
// during a leap with probability 1 - exp(-H / K), H the sum of the per-capita hazards of the compartment's exits, and the leavers are split
// over the exits multinomially: nothing goes negative, nothing is cut, and competing exits are treated alike whatever their order.
// Classification of a reaction (static, from the block alone; the host derives and checks it, the device derives it wave-uniformly):
//   source(r) = the one reactant c in {s1[r], s2[r]} with nu[r][c] == -1, provided the other reactant (if any) has nu[r][.] >= 0 (a catalyst:
//               I in S + I -> E + I) and no species that is not a reactant has nu[r][.] < 0;  o(r) = the other reactant, if any.
//   sourceless: no reactant has nu < 0 and no other species either (order 0: immigration; catalytic production X -> 2X): nu[r][.] >= 0.
//   refused under this method, with BSSM_ERR_ARG before any launch: everything else -- both reactants consumed (A + B -> C), a reactant
//               with nu < -1, a species that is no reactant with nu < 0.
// One transition (one unit of time, to absolute time tau, particle j, transition call `call`).  After the counters' reset (unchanged, and
// only on `first`), for leap l = 0 .. K-1 with x the state at the start of the leap, held for the whole leap, and xn = x:
//   1. for each species c = 0 .. d-1 in order, over the reactions r_1 < r_2 < ... with source(r) == c:
//        h_r = kr[r], times x[o(r)] if the reaction has another reactant; a value that is not > 0 counts as 0.0  (kr: the rates of the moment,
//              as rn_propensities receives them -- a rate schedule applies unchanged; h_r is recomputed, not stored)
//        H = 0.0 + h_{r_1} + h_{r_2} + ...  (left to right);   if !(H > 0.0) every count of the group is 0.0 and nothing is drawn;  otherwise
//        pe = -expm1(-H / (double)K);  rem = x[c];  prem = 1.0;   for each i in order:
//          p_i = (h_{r_i} / H) * pe;   q = p_i / prem;  if (!(q > 0.0)) q = 0.0;  if (q > 1.0) q = 1.0;     (the clamp to [0, 1]; a NaN gives 0.0)
//          n_i = rbinom(rem, q);   rem = rem - n_i;   prem = prem - p_i;   xn[c'] = xn[c'] + nu[r_i][c'] * n_i  for every c'
//   2. for each sourceless reaction r in order:  a_r = the propensity at x as rn_propensities forms it;  n = rpois(a_r / (double)K) (rn_rpois
//      above, not capped);   xn[c'] = xn[c'] + nu[r][c'] * n  for every c'
//   3. x = xn
// All counts are drawn from the state at the start of the leap: a compartment loses at most what it held, what arrives during a leap cannot
// leave in the same leap, and the result does not depend on the order in which the groups are processed.
// Draw keys: the draw for reaction r in leap l, attempt a, reads the Philox block at (j, call, DRAW_TRANS | (((l * RNR + r) << 6 | a) << 8),
// stream) -- rn_rpois's layout (reused as it is for the sourceless reactions), stride RNR = 8: appending a zero-rate reaction moves no key.
// rbinom(n, q) (rn_rbinom; n an integer-valued double; u1 = u01(w.x, w.y), u2 = u01(w.z, w.w) of the attempt's block w):
//   !(n > 0.0) or !(q > 0.0): 0.0.   q >= 1.0: n.   (neither draws)     flip = q > 0.5;  qq = flip ? 1.0 - q : q;  the result is flip ? n - k : k with
//   n * qq < 10.0: inversion by sequential search on u1 of attempt 0:
//     pr = exp(n * log1p(-qq)); F = pr; k = 0.0; odds = qq / (1.0 - qq);
//     while (u1 > F && k < n && k < 128.0) { k = k + 1.0; pr = pr * ((n - k + 1.0) / k) * odds; F = F + pr; }
//   otherwise Hoermann's BTRS (transformed rejection with squeeze, 1993; the sibling of PTRS), at most 64 attempts:
//     spq = sqrt((n * qq) * (1.0 - qq)); b = 1.15 + 2.53 * spq; a_ = (-0.0873 + 0.0248 * b) + 0.01 * qq; cc = n * qq + 0.5; vr = 0.92 - 4.2 / b;
//     attempts a = 0 .. 63:  U = u1 - 0.5; V = u2; us = 0.5 - fabs(U); k = floor((2.0 * a_ / us + b) * U + cc);
//       accept k if us >= 0.07 && V <= vr;   reject if k < 0.0 || k > n;   otherwise accept k if   (rn_btrs_full_test; the device's log, lgamma)
//         alpha = (2.83 + 5.1 / b) * spq; m = floor((n + 1.0) * qq); lr = log(qq / (1.0 - qq));
//         log(V * alpha / (a_ / (us * us) + b)) <= (((lgamma(m + 1.0) + lgamma(n - m + 1.0)) - lgamma(k + 1.0)) - lgamma(n - k + 1.0)) + (k - m) * lr
//     after 64 rejections k = floor(n * qq) (not reachable in practice; it is there so that the loop is bounded).
//   The constants are those of the published algorithm (tests/test_rnet_em_cpu.py holds the sampler against the exact pmf).
// Unchanged: the log-likelihoods, missing observations, the APF look-ahead (the Euler mean of the particles as they stand), the counter
// semantics, tau for the schedule, gather, carry, state estimate and histories.  The APF's second-stage transition is an Euler-multinomial
// transition that never resets.  The method is a third value of the kernels' METH; the Gillespie and tau-leap instantiations are the code
// they were.  The classification travels through the kernel as two packed words of 4 bits a reaction (rn_classify), so the rolled loops over
// c and r test it with scalar shifts and compares.
// Gamma white noise on the rates (extra-demographic stochasticity: He, Ionides and King 2010; pomp's rgammawn next to reulermultinom; context
// options BSSM_OPT_RN_METHOD = 1 and BSSM_OPT_RN_NOISE = 1 with BSSM_OPT_RN_LEAPS = K; METH = RN_EULER_MULTINOM_GWN below).  The block carries, directly after size[nsz] and in
// front of the optional tails, lead[R] and sigma[R] (RnPar::nnz = 2 R; 0 under every other method, so a block without noise is byte for byte
// what it was): lead[r] = -1.0 for a reaction without noise, otherwise the lowest reaction index g of the noise group that r belongs to
// (lead[g] == g), and sigma[r] = the group's sigma, finite and > 0 (the same value for every member; 0.0 where lead[r] = -1).
// The transition is the Euler-multinomial transition above with one change: the integrated per-capita hazard of reaction r over leap l is
// h_r * w_r instead of h_r / K:
//   reaction in noise group g:  s2 = sigma_g * sigma_g;  sh = 1.0 / ((double)K * s2);  w_r = s2 * rgamma(sh)     one draw per (particle, call,
//                               leap, group), shared by the group's reactions: mean 1 / K, variance sigma^2 / K
//   reaction in no group:       w_r = 1.0 / (double)K
//   step 1:  hw_r = h_r * w_r;  H = 0.0 + hw_{r_1} + hw_{r_2} + ...;  nothing is drawn if !(H > 0.0);  pe = -expm1(-H);  p_i = (hw_{r_i} / H) * pe;
//            the clamp, rbinom, rem and prem as above
//   step 2 (sourceless reactions):  n = rpois(a_r * w_r)
// Unchanged: the counters' reset, tau and the schedule's rows, the densities, and the APF look-ahead (the noise has mean 1 / K, so the Euler
// mean stands).  The APF's second-stage transition draws noise like any transition.
// rgamma(sh) (rn_rgamma): Marsaglia and Tsang (2000) with the normal taken by inversion (qnorm_as241), so that one Philox block serves one
// attempt.  Attempt a of group leader g in leap l reads the block w at
//   (j, call, DRAW_TRANS | (1u << 27) | (((l * RNR + g) << 6 | a) << 8), stream);   u1 = u01(w.x, w.y), u2 = u01(w.z, w.w).
// Bit 27 is free: the binomial and Poisson keys end at bit 26 (l = 1023, r = 7, a = 63).  No existing key moves.
//   boost = sh < 1.0;  al = boost ? sh + 1.0 : sh;  dd = al - 1.0 / 3.0;  cc = 1.0 / sqrt(9.0 * dd);
//   attempts a = 0 .. 62:  x = qnorm_as241(u1);  v = 1.0 + cc * x;  reject if !(v > 0.0);  v = v * v * v;  x2 = x * x;
//     accept if u2 < 1.0 - 0.0331 * (x2 * x2);   otherwise accept if log(u2) < 0.5 * x2 + dd * ((1.0 - v) + log(v));   the result is dd * v
//   after 63 rejections the result is dd (not reachable in practice: the loop is bounded)
//   if boost:  result = result * exp(log(ub) / sh),  ub the u1 of the block at a = 63
// A result that underflows to 0.0 is a leap without hazard.  The draw is a pure function of its key: the transition holds the last group's w
// and draws again when another group's is asked for, which changes no value.
// Particles are SoA [d][N], as the multivariate family's: k_carry_mv, k_reduce_state_est and k_record_history are reused.
// Arithmetic: fp64, contraction off, the order of operations above.
#pragma once
#include "mv.hip.h"

namespace bssm {

constexpr int RNR = 8;            // most reactions
constexpr int RN_OBS_POIS = 0;    // y_k ~ Poisson(lambda_k)                          BSSM_MODEL_RNET
constexpr int RN_OBS_NB = 1;      // y_k ~ NegBin(mean = lambda_k, size = size_k)     BSSM_MODEL_RNET_NB
constexpr int RN_GILLESPIE = 0;   // transition: Gillespie's direct method            BSSM_OPT_RN_LEAPS = 0
constexpr int RN_TAU_LEAP = 1;    // transition: K tau-leaps per unit of time         BSSM_OPT_RN_LEAPS = K
constexpr int RN_EULER_MULTINOM = 2;   // transition: K Euler-multinomial leaps           BSSM_OPT_RN_METHOD = 1, BSSM_OPT_RN_LEAPS = K
constexpr int RN_EULER_MULTINOM_GWN = 3;   // the same with gamma white noise on the rates  BSSM_OPT_RN_METHOD = 1, BSSM_OPT_RN_NOISE = 1, BSSM_OPT_RN_LEAPS = K
constexpr int RN_MAX_LEAPS = 1024;
constexpr uint32_t RN_GWN_KEY = 1u << 27;  // the gamma draws' bit of the counter word: the binomial and Poisson keys end at bit 26
// rn_classify's code of a reaction, 4 bits: 0 .. 7 = source(r) (in the word of the other reactants: o(r)), 8 = sourceless, 15 = none
constexpr uint32_t RN_EM_SOURCELESS = 8u, RN_EM_NONE = 15u;
// packed parameter block (doubles): d, R, p, x0[d], k[R], s1[R], s2[R], nu[R][d], G[p][d], then size[p] (nsz = p: the negative-binomial
// family only; nsz = 0 otherwise), then lead[R], sigma[R] (nnz = 2 R: RN_EULER_MULTINOM_GWN only; nnz = 0 otherwise), then optionally
// reset[d] (tail != 0), then optionally n_times, M[n_times][R] (n_times != 0; only after reset[d])
struct RnPar {
    const double* P; int d, R, p, tail, n_times, nsz, nnz;
    __host__ __device__ int o_x0() const { return 3; }
    __host__ __device__ int o_k() const { return 3 + d; }
    __host__ __device__ int o_s1() const { return o_k() + R; }
    __host__ __device__ int o_s2() const { return o_s1() + R; }
    __host__ __device__ int o_nu() const { return o_s2() + R; }
    __host__ __device__ int o_G() const { return o_nu() + R * d; }
    __host__ __device__ int o_size() const { return o_G() + p * d; }           // (nsz != 0 only)
    __host__ __device__ int o_lead() const { return o_size() + nsz; }          // (nnz != 0 only)
    __host__ __device__ int o_sigma() const { return o_lead() + R; }
    __host__ __device__ int size() const { return o_size() + nsz + nnz; }
    __host__ __device__ int o_reset() const { return size(); }                 // (tail != 0 only)
    __host__ __device__ int size_tail() const { return size() + d; }
    // (n_times != 0 only; the entry before it is n_times.)  In the DEVICE copy of the block this section does not hold M as the
    // header documents it for the caller's block but the products k_r * M[tau][r], taken on the host (rn_sched_products)
    __host__ __device__ int o_sched() const { return size_tail() + 1; }
    __host__ __device__ int size_sched() const { return o_sched() + n_times * R; }
    // the rates of the transition TO absolute time tau >= 1: the schedule's row tau - 1 of the device copy (products), or k
    __host__ __device__ const double* rates_row(int tau) const { return P + (n_times ? o_sched() + (long long)(tau - 1) * R : (long long)o_k()); }
};

// x[s] for a wave-uniform species index s (a block entry): compares against constants, so x[] stays in registers
template <int DM>
__device__ __forceinline__ double rn_pick(const double (&x)[DM], int s)
{
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < DM; c++) if (s == c) v = x[c];
    return v;
}

// the propensities a[0 .. R) of one particle (0.0 beyond R); kr: the rates of the moment (wave-uniform, RnPar::rates_row)
template <int DM>
__device__ __forceinline__ void rn_propensities(const RnPar& rp, const double* __restrict__ kr, const double (&x)[DM], double (&a)[RNR])
{
#pragma unroll
    for (int r = 0; r < RNR; r++) {
        a[r] = 0.0;
        if (r < rp.R) {
            const int s1 = (int)rp.P[rp.o_s1() + r], s2 = (int)rp.P[rp.o_s2() + r];
            double v = kr[r];
            if (s1 >= 0) v = v * rn_pick<DM>(x, s1);
            if (s2 >= 0) v = v * rn_pick<DM>(x, s2);
            a[r] = v > 0.0 ? v : 0.0;
        }
    }
}

// one unit of time for ONE particle.  nu: the stoichiometry [R][d] in LDS -- the reaction that fires differs from lane to lane, and a
// register array indexed by it would live in scratch; x[] is indexed statically throughout.
template <int DM>
__device__ __forceinline__ void rn_transition(double (&x)[DM], const RnPar& rp, const double* __restrict__ kr, const double* nu, PhiloxKey key, uint32_t call, uint32_t particle)
{
    const int d = rp.d, R = rp.R;
    double t = 0.0;
    uint32_t ev = 0;
    while (t < 1.0 && ev < (1u << 20)) {
        double a[RNR];
        rn_propensities<DM>(rp, kr, x, a);
        double total = a[0];
#pragma unroll
        for (int r = 1; r < RNR; r++) if (r < R) total = total + a[r];
        if (total <= 0.0) break;
        u32x4 c; c.x = particle; c.y = call; c.z = DRAW_TRANS | (ev << 8); c.w = key.stream;
        const u32x4 q = philox4x32_10(c, key.k0, key.k1);
        const double dt = -log(u01_from_bits(q.x, q.y)) / total;
        if (t + dt > 1.0) break;
        t = t + dt;
        const double u = u01_from_bits(q.z, q.w);
        // The walk over r = 0 .. R-2 needs no guard on R: a[r] is 0.0 from R on, so at r = R-1 the running sum IS total (the same
        // additions in the same order), the quotient is 1.0 and every lane still looking takes reaction R-1 there -- what the
        // "otherwise" of the definition gives it.  Lanes that have chosen skip the division; past R-1 that is the whole wave.
        int rsel = R - 1;
        bool found = false;
        double cum = a[0];
#pragma unroll
        for (int r = 0; r < RNR - 1; r++) {
            if (r > 0) cum = cum + a[r];
            if (!found) { if (u < cum / total) { rsel = r; found = true; } }
        }
#pragma unroll
        for (int k = 0; k < DM; k++) if (k < d) x[k] = x[k] + nu[rsel * d + k];
        ev++;
    }
}

// the full acceptance test of PTRS, reached by roughly every second attempt at lam = 10 and by 1 in 5 to 10 from lam = 1e4 on
// (tests/test_rnet_leap_cpu.py prints the counts).  A function of its own: inlined, the constants of lgamma and the two logs were hoisted
// out of the attempt, reaction and leap loops and took every kernel with a tau-leap transition to the VGPR limit with scratch spills
// (DESIGN.md 1d).  static: the header may be included by more than one translation unit.
static __device__ __attribute__((noinline)) bool rn_ptrs_full_test(double V, double linva, double a_, double us, double b, double lam, double k, double loglam)
{
    return log(V) + linva - log(a_ / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0);
}

// rpois(lam) of the tau-leap transition (the head of this file): the draw of `particle` for reaction r in leap l of transition call
// `call`, lr = l * RNR + r.  Attempt a reads the Philox block at (particle, call, DRAW_TRANS | ((lr << 6 | a) << 8), stream); the block
// of attempt 0 serves the inversion and the first PTRS attempt alike, so it is drawn in front of the per-lane branch on lam.
// What depends on lam alone (slam, b, a_, invalpha and its log, vr, loglam) is taken once, outside the attempt loop; the accept test
// and with it the loop's trip count are per lane (the squeeze accepts about half of the draws at lam = 10 and 9 in 10 from lam = 1e4 on;
// about 1 attempt in 4 is rejected at lam = 10, 1 in 9 from 1e4 on).
__device__ __forceinline__ double rn_rpois(double lam, PhiloxKey key, uint32_t call, uint32_t particle, uint32_t lr)
{
    if (!(lam > 0.0)) return 0.0;
    u32x4 c; c.x = particle; c.y = call; c.z = DRAW_TRANS | ((lr << 6) << 8); c.w = key.stream;
    u32x4 q = philox4x32_10(c, key.k0, key.k1);
    if (lam < 10.0) {                                     // inversion by sequential search; k < 128: a u1 that rounding leaves above the summed mass
        const double u1 = u01_from_bits(q.x, q.y);
        double p = exp(-lam), F = p, k = 0.0;
        while (u1 > F && k < 128.0) { k = k + 1.0; p = p * lam / k; F = F + p; }
        return k;
    }
    // Hoermann's transformed rejection with squeeze (PTRS, 1993)
    const double slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam, a_ = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    const double linva = log(invalpha);
    double res = floor(lam);                              // after 64 rejections (not reachable in practice: the loop is bounded)
#pragma unroll 1
    for (uint32_t a = 0; a < 64u; a++) {
        if (a > 0) { c.z = DRAW_TRANS | (((lr << 6) | a) << 8); q = philox4x32_10(c, key.k0, key.k1); }
        const double U = u01_from_bits(q.x, q.y) - 0.5, V = u01_from_bits(q.z, q.w), us = 0.5 - fabs(U);
        const double k = floor((2.0 * a_ / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) { res = k; break; }
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        if (rn_ptrs_full_test(V, linva, a_, us, b, lam, k, loglam)) { res = k; break; }
    }
    return res;
}

// one unit of time for ONE particle by K tau-leaps (the head of this file).  The reaction index is wave-uniform, so nu[r][c] comes off the
// block through the scalar cache under the r < R and c < d guards (no LDS staging on this path) and x[] stays statically indexed.
template <int DM>
__device__ __forceinline__ void rn_transition_leap(double (&x)[DM], const RnPar& rp, const double* __restrict__ kr, int K, PhiloxKey key, uint32_t call, uint32_t particle)
{
    const int d = rp.d, R = rp.R;
    const double dK = (double)K;
#pragma unroll 1
    for (int l = 0; l < K; l++) {
        double a[RNR];
        rn_propensities<DM>(rp, kr, x, a);                // (held for the whole leap)
        // r is a rolled, wave-uniform loop counter: with the loop unrolled the eight inlined samplers took every instantiation to
        // the 128-VGPR limit with 170 .. 230 VGPR spills; a[r] is picked by compares against constants, as rn_pick does
#pragma unroll 1
        for (int r = 0; r < R; r++) {
            double ar = 0.0;
#pragma unroll
            for (int q = 0; q < RNR; q++) if (r == q) ar = a[q];
            double n = rn_rpois(ar / dK, key, call, particle, (uint32_t)(l * RNR + r));
            double cap = INFINITY;                        // the smallest count among the species the reaction consumes, as they stand
#pragma unroll
            for (int c = 0; c < DM; c++) if (c < d) { if (rp.P[rp.o_nu() + r * d + c] < 0.0) cap = x[c] < cap ? x[c] : cap; }
            n = cap < n ? cap : n;
#pragma unroll
            for (int c = 0; c < DM; c++) if (c < d) x[c] = x[c] + rp.P[rp.o_nu() + r * d + c] * n;
        }
    }
}

// the classification of the head of this file for the Euler-multinomial transition, from a block that the host has checked (pf_run_rn,
// pf_run_batch_rn: rn_em_check): 4 bits a reaction, srcs = source(r) | RN_EM_SOURCELESS | RN_EM_NONE (r >= R), oths = o(r) | RN_EM_NONE.
// Everything here is wave-uniform (block entries through the scalar cache), so the two words live in SGPRs.
__device__ __forceinline__ void rn_classify(const RnPar& rp, uint32_t& srcs, uint32_t& oths)
{
    srcs = 0u; oths = 0u;
#pragma unroll
    for (int r = 0; r < RNR; r++) {
        uint32_t s = RN_EM_NONE, o = RN_EM_NONE;
        if (r < rp.R) {
            const int s1 = (int)rp.P[rp.o_s1() + r], s2 = (int)rp.P[rp.o_s2() + r];
            const double n1 = s1 >= 0 ? rp.P[rp.o_nu() + r * rp.d + s1] : 0.0, n2 = s2 >= 0 ? rp.P[rp.o_nu() + r * rp.d + s2] : 0.0;
            if (n1 < 0.0) { s = (uint32_t)s1; if (s2 >= 0) o = (uint32_t)s2; }
            else if (n2 < 0.0) { s = (uint32_t)s2; o = (uint32_t)s1; }
            else s = RN_EM_SOURCELESS;
        }
        srcs |= s << (4 * r); oths |= o << (4 * r);
    }
}

// the full acceptance test of BTRS (four lgamma and two logs), a function of its own as rn_ptrs_full_test is and for its reason.  What
// depends on (n, qq, spq) alone and is needed only here (alpha, m, lr) is taken here, not held across the attempt loop.
static __device__ __attribute__((noinline)) bool rn_btrs_full_test(double V, double a_, double us, double b, double spq, double n, double qq, double k)
{
    const double alpha = (2.83 + 5.1 / b) * spq, m = floor((n + 1.0) * qq), lr = log(qq / (1.0 - qq));
    return log(V * alpha / (a_ / (us * us) + b)) <= (((lgamma(m + 1.0) + lgamma(n - m + 1.0)) - lgamma(k + 1.0)) - lgamma(n - k + 1.0)) + (k - m) * lr;
}

// rbinom(n, q) of the Euler-multinomial transition (the head of this file): the draw of `particle` for reaction r in leap l of transition
// call `call`, lr = l * RNR + r; rn_rpois's keys.  The block of attempt 0 serves the inversion and the first BTRS attempt alike.
// A function of its own, not inlined: the transition holds x[] and xn[] of its particle and x[] of the pair's other one across the draw, and
// with the sampler inlined next to them k_step_rn spilled 79 (DM = 2) to 359 (DM = 8) VGPRs; as a call, 7 to 134.
static __device__ __attribute__((noinline)) double rn_rbinom(double n, double q, PhiloxKey key, uint32_t call, uint32_t particle, uint32_t lr)
{
    if (!(n > 0.0) || !(q > 0.0)) return 0.0;
    if (q >= 1.0) return n;
    const bool flip = q > 0.5;
    const double qq = flip ? 1.0 - q : q;
    u32x4 c; c.x = particle; c.y = call; c.z = DRAW_TRANS | ((lr << 6) << 8); c.w = key.stream;
    u32x4 w = philox4x32_10(c, key.k0, key.k1);
    double k;
    if (n * qq < 10.0) {                                  // inversion by sequential search; k < 128 cannot bind at a mean below 10: the loop is bounded
        const double u1 = u01_from_bits(w.x, w.y);
        double pr = exp(n * log1p(-qq)), F = pr;
        const double odds = qq / (1.0 - qq);
        k = 0.0;
        while (u1 > F && k < n && k < 128.0) { k = k + 1.0; pr = pr * ((n - k + 1.0) / k) * odds; F = F + pr; }
    } else {                                              // Hoermann's transformed rejection with squeeze (BTRS, 1993)
        const double spq = sqrt((n * qq) * (1.0 - qq));
        const double b = 1.15 + 2.53 * spq, a_ = (-0.0873 + 0.0248 * b) + 0.01 * qq, cc = n * qq + 0.5, vr = 0.92 - 4.2 / b;
        k = floor(n * qq);                                // after 64 rejections (not reachable in practice: the loop is bounded)
#pragma unroll 1
        for (uint32_t a = 0; a < 64u; a++) {
            if (a > 0) { c.z = DRAW_TRANS | (((lr << 6) | a) << 8); w = philox4x32_10(c, key.k0, key.k1); }
            const double U = u01_from_bits(w.x, w.y) - 0.5, V = u01_from_bits(w.z, w.w), us = 0.5 - fabs(U);
            const double kk = floor((2.0 * a_ / us + b) * U + cc);
            if (us >= 0.07 && V <= vr) { k = kk; break; }
            if (kk < 0.0 || kk > n) continue;
            if (rn_btrs_full_test(V, a_, us, b, spq, n, qq, kk)) { k = kk; break; }
        }
    }
    return flip ? n - k : k;
}

// the per-capita hazard h_r of a reaction with a source: kr[r], times x[o(r)] if there is another reactant; not > 0 counts as 0.0
template <int DM>
__device__ __forceinline__ double rn_hazard(const double (&x)[DM], const double* __restrict__ kr, uint32_t oths, int r)
{
    const uint32_t o = (oths >> (4 * r)) & 15u;
    double h = kr[r];
    if (o < (uint32_t)DM) h = h * rn_pick<DM>(x, (int)o);
    return h > 0.0 ? h : 0.0;
}

// rn_rpois for the sourceless reactions of the Euler-multinomial transition, as a call for rn_rbinom's reason (rn_rpois itself stays inlined
// into the tau-leap transition: those instantiations are the code they were)
static __device__ __attribute__((noinline)) double rn_rpois_call(double lam, PhiloxKey key, uint32_t call, uint32_t particle, uint32_t lr)
{
    return rn_rpois(lam, key, call, particle, lr);
}

// rgamma(sh) of the gamma white noise (the head of this file): the draw of `particle` for the noise group with leader g in leap l of
// transition call `call`, lg = l * RNR + g.  A function of its own, not inlined, for rn_rbinom's reason: the transition holds x[], xn[] and
// the pair's other particle across the draw, and qnorm_as241's three pairs of polynomials inlined next to them would be hoisted and spilled.
// qnorm_as241 as a call: inlined into rn_rgamma's attempt loop, the 48 coefficients of its three branches were hoisted out of the loop and
// took the sampler itself to 127 VGPRs with 192 B of scratch (k_dump_rgamma, which holds nothing else, showed it)
static __device__ __attribute__((noinline)) double rn_qnorm(double p) { return qnorm_as241(p); }

static __device__ __attribute__((noinline)) double rn_rgamma(double sh, PhiloxKey key, uint32_t call, uint32_t particle, uint32_t lg)
{
    const bool boost = sh < 1.0;
    const double al = boost ? sh + 1.0 : sh;
    const double dd = al - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * dd);
    u32x4 c; c.x = particle; c.y = call; c.w = key.stream;
    double res = dd;                                      // after 63 rejections (not reachable in practice: the loop is bounded)
#pragma unroll 1
    for (uint32_t a = 0; a < 63u; a++) {
        c.z = DRAW_TRANS | RN_GWN_KEY | (((lg << 6) | a) << 8);
        const u32x4 w = philox4x32_10(c, key.k0, key.k1);
        const double x = rn_qnorm(u01_from_bits(w.x, w.y)), u2 = u01_from_bits(w.z, w.w);
        double v = 1.0 + cc * x;
        if (!(v > 0.0)) continue;
        v = v * v * v;
        const double x2 = x * x;
        if (u2 < 1.0 - 0.0331 * (x2 * x2)) { res = dd * v; break; }
        if (log(u2) < 0.5 * x2 + dd * ((1.0 - v) + log(v))) { res = dd * v; break; }
    }
    if (boost) {                                          // Gamma(sh) = Gamma(sh + 1) U^(1 / sh)
        c.z = DRAW_TRANS | RN_GWN_KEY | (((lg << 6) | 63u) << 8);
        const u32x4 w = philox4x32_10(c, key.k0, key.k1);
        res = res * exp(log(u01_from_bits(w.x, w.y)) / sh);
    }
    return res;
}

// the noise weight w_r of reaction r in leap l (the head of this file): 1 / K without a group; otherwise sigma^2 rgamma(1 / (K sigma^2)) of
// the group's leader.  held / wheld: the leader whose draw this particle holds for this leap (-1: none) and its w -- the draw is a pure
// function of its key, so holding it changes no value; a net with one group (the usual case) draws once per leap.  lead and sigma are
// block entries at wave-uniform addresses (the scalar cache).
__device__ __forceinline__ double rn_noise_w(const RnPar& rp, int r, int l, double dK, int& held, double& wheld, PhiloxKey key, uint32_t call, uint32_t particle)
{
    const int g = (int)rp.P[rp.o_lead() + r];
    if (g < 0) return 1.0 / dK;
    if (g != held) {
        const double sg = rp.P[rp.o_sigma() + r];
        const double s2 = sg * sg, sh = 1.0 / (dK * s2);
        wheld = s2 * rn_rgamma(sh, key, call, particle, (uint32_t)(l * RNR + g));
        held = g;
    }
    return wheld;
}

// one unit of time for ONE particle by K Euler-multinomial leaps (the head of this file).  c and r are rolled, wave-uniform loop counters and
// the classification is tested on the packed words with scalar shifts; x[], xn[] are picked by compares against constants and nu[r][c]
// comes off the block through the scalar cache, so the register arrays stay statically indexed (no LDS staging on this path).
// GWN: gamma white noise on the rates (RN_EULER_MULTINOM_GWN): the hazards are weighted by rn_noise_w instead of divided by K.  A template
// parameter: without it the code is what it was.
template <int DM, bool GWN = false>
__device__ __forceinline__ void rn_transition_em(double (&x)[DM], const RnPar& rp, const double* __restrict__ kr, int K, uint32_t srcs, uint32_t oths,
                                                 PhiloxKey key, uint32_t call, uint32_t particle)
{
    const int d = rp.d, R = rp.R;
    const double dK = (double)K;
#pragma unroll 1
    for (int l = 0; l < K; l++) {
        double xn[DM];
        int held = -1;                                    // (GWN only)
        double wheld = 0.0;
#pragma unroll
        for (int c = 0; c < DM; c++) xn[c] = x[c];
#pragma unroll 1
        for (int c = 0; c < d; c++) {                     // 1. the compartments with exits
            double H = 0.0;
#pragma unroll 1
            for (int r = 0; r < R; r++) if (((srcs >> (4 * r)) & 15u) == (uint32_t)c) {
                if (GWN) H = H + rn_hazard<DM>(x, kr, oths, r) * rn_noise_w(rp, r, l, dK, held, wheld, key, call, particle);
                else H = H + rn_hazard<DM>(x, kr, oths, r);
            }
            if (H > 0.0) {                                // (per lane; a compartment without exits leaves the whole wave at 0.0)
                const double pe = GWN ? -expm1(-H) : -expm1(-H / dK);
                double rem = rn_pick<DM>(x, c), prem = 1.0;
#pragma unroll 1
                for (int r = 0; r < R; r++) {
                    if (((srcs >> (4 * r)) & 15u) != (uint32_t)c) continue;
                    double hw = rn_hazard<DM>(x, kr, oths, r);
                    if (GWN) hw = hw * rn_noise_w(rp, r, l, dK, held, wheld, key, call, particle);
                    const double p = (hw / H) * pe;
                    double q = p / prem;
                    if (!(q > 0.0)) q = 0.0;
                    if (q > 1.0) q = 1.0;
                    const double n = rn_rbinom(rem, q, key, call, particle, (uint32_t)(l * RNR + r));
                    rem = rem - n; prem = prem - p;
#pragma unroll
                    for (int c2 = 0; c2 < DM; c2++) if (c2 < d) xn[c2] = xn[c2] + rp.P[rp.o_nu() + r * d + c2] * n;
                }
            }
        }
#pragma unroll 1
        for (int r = 0; r < R; r++) {                     // 2. the sourceless reactions: Poisson counts, nothing to cap
            if (((srcs >> (4 * r)) & 15u) != RN_EM_SOURCELESS) continue;
            const int s1 = (int)rp.P[rp.o_s1() + r], s2 = (int)rp.P[rp.o_s2() + r];
            double v = kr[r];                             // (rn_propensities' a[r])
            if (s1 >= 0) v = v * rn_pick<DM>(x, s1);
            if (s2 >= 0) v = v * rn_pick<DM>(x, s2);
            v = v > 0.0 ? v : 0.0;
            const double lam = GWN ? v * rn_noise_w(rp, r, l, dK, held, wheld, key, call, particle) : v / dK;
            const double n = rn_rpois_call(lam, key, call, particle, (uint32_t)(l * RNR + r));
#pragma unroll
            for (int c2 = 0; c2 < DM; c2++) if (c2 < d) xn[c2] = xn[c2] + rp.P[rp.o_nu() + r * d + c2] * n;
        }
#pragma unroll
        for (int c = 0; c < DM; c++) x[c] = xn[c];        // 3.
    }
}

// the counters' reset of the first transition of a gap loop, for a pair of particles: the flags come off the scalar cache and are
// compared under the c < d unroll, so x[] stays statically indexed
template <int DM>
__device__ __forceinline__ void rn_reset_counters(const RnPar& rp, double (&x0)[DM], double (&x1)[DM])
{
#pragma unroll
    for (int c = 0; c < DM; c++) if (c < rp.d) { if (rp.P[rp.o_reset() + c] != 0.0) { x0[c] = 0.0; x1[c] = 0.0; } }
}

// dnbinom(y, size = r, mu = mu, log = TRUE) = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + r log(r / (r + mu)) + y log(mu / (r + mu)),
// c = the first three terms (the host's table entry, see the head of this file).  R's dnbinom_mu evaluates the same quantity
// through dbinom_raw (stirlerr / bd0); how closely the two agree has not been measured.
__device__ __forceinline__ double rn_dnbinom_log(double y, double mu, double r, double c)
{
    if (!(mu > 0.0)) return (y == 0.0 && mu == 0.0) ? 0.0 : -INFINITY;
    const double s = r + mu;
    const double lr = (r < mu) ? log(r / s) : log1p(-(mu / s));
    if (y == 0.0) return r * lr;
    return (c + r * lr) + y * log(mu / s);
}

// log_likelihood_fn (AUX: at the Euler mean, its propensities with the rates kr of the moment) of one particle; OBS: the observation
// family (RN_OBS_NB: lgyrow holds the table c(t, k), and size_k comes off the block at a wave-uniform address, as G does)
template <int DM, bool AUX, int OBS = RN_OBS_POIS>
__device__ __forceinline__ double rn_loglik(const RnPar& rp, const double* __restrict__ kr, const double (&xin)[DM], const double* __restrict__ yrow, const double* __restrict__ lgyrow)
{
    const int d = rp.d, R = rp.R, p = rp.p;
    double x[DM];
#pragma unroll
    for (int c = 0; c < DM; c++) x[c] = xin[c];
    if (AUX) {
        double a[RNR];
        rn_propensities<DM>(rp, kr, xin, a);
#pragma unroll
        for (int c = 0; c < DM; c++) {
            if (c < d) {
                double m = xin[c];
#pragma unroll
                for (int r = 0; r < RNR; r++) if (r < R) m = m + rp.P[rp.o_nu() + r * d + c] * a[r];
                x[c] = m;
            }
        }
    }
    double l = 0.0;
#pragma unroll
    for (int k = 0; k < MVD; k++) {
        if (k < p) {
            MvObsK ok; ok.y = yrow[k]; ok.sd = 0.0; ok.lsd = 0.0; ok.lgy = lgyrow[k];
            if (mv_observed(ok)) {
                double lam = 0.0;
#pragma unroll
                for (int c = 0; c < DM; c++) if (c < d) lam = lam + rp.P[rp.o_G() + k * d + c] * x[c];
                if (AUX) lam = lam > 0.0 ? lam : 0.0;
                if (OBS == RN_OBS_NB) l = l + rn_dnbinom_log(ok.y, lam, rp.P[rp.o_size() + k], ok.lgy);
                else l = l + Sir::dpois_log(ok.y, lam, ok.lgy);
            }
        }
    }
    return l;
}

// init_fn + the t = 0 state estimate partials; init_block's particle mapping (a pair per thread and round), so that the partial
// sums associate as the built-in SIR's do
__global__ __launch_bounds__(NT) void k_init_rn(double* __restrict__ x, long long N, RnPar rp, double* __restrict__ se_part /* [B][d] */)
{
    __shared__ double sh4[NWV];
    const int d = rp.d;
    const long long base = (long long)blockIdx.x * EB;
    const double invN = 1.0 / (double)N;
    double acc[MVD];
#pragma unroll
    for (int c = 0; c < MVD; c++) acc[c] = 0.0;
#pragma unroll 1
    for (int r = 0; r < EL / 2; r++) {
        const long long j = base + 2 * (threadIdx.x + NT * r);
        if (j < N) {
#pragma unroll
            for (int c = 0; c < MVD; c++) {
                if (c < d) {
                    const double v = rp.P[rp.o_x0() + c];
                    x[(long long)c * N + j] = v; acc[c] += v * invN;
                    if (j + 1 < N) { x[(long long)c * N + j + 1] = v; acc[c] += v * invN; }
                }
            }
        }
    }
    for (int c = 0; c < d; c++) { const double s = block_sum(acc[c], sh4); if (threadIdx.x == 0) se_part[(long long)blockIdx.x * d + c] = s; }
}

// transition_fn and / or weight_fn with the block partials of the log-sum-exp: k_step_sir for the family.
//   WEIGHT 1: lw = log_likelihood(y, x');  WEIGHT 2: the aux log-likelihood at the CURRENT particles, no transition;  SUBAUX: lw -= auxg[j]
// DM >= d: the size of the register arrays.  first (wave-uniform): this is the first transition of a gap loop -- with a tail in
// the block the counters are set to 0.0 after the load and before the transition.
// SCHED: the block carries a rate schedule and krow (wave-uniform, the last argument) points to the rates of this launch
// (RnPar::rates_row); without it (the default) krow is not read and the rates are k at rp.P + o_k(), the code of the family before
// schedules existed: with one pointer for both cases the no-schedule filters measured 0.4-0.6 % slower than before.
// OBS: the observation family of the instantiations that take weights (the transition-only ones are shared: they read rp.nsz, a
// wave-uniform kernel argument, where they need the offset of reset[d]).  The Poisson instantiations fix rp.nsz = 0 at compile time.
// METH: the transition method of the instantiations with TRANS (the weight-only and look-ahead ones are shared), Gillespie's direct
// method by default: no runtime branch on it.  RN_TAU_LEAP, RN_EULER_MULTINOM and RN_EULER_MULTINOM_GWN run `leaps` (wave-uniform, the last argument; not read
// otherwise) leaps per unit of time and stage no stoichiometry in LDS.
template <int DM, bool TRANS, int WEIGHT, bool SUBAUX, bool SCHED = false, int OBS = RN_OBS_POIS, int METH = RN_GILLESPIE>
__global__ __launch_bounds__(NTS) void k_step_rn(double* __restrict__ x, double* __restrict__ lw, const double* __restrict__ auxg, long long N, RnPar rp,
                                                 const double* __restrict__ yrow /* [p] */, const double* __restrict__ lgyrow /* [p] */, PhiloxKey key, uint32_t call, int first,
                                                 double* __restrict__ pm, double* __restrict__ ps, double* __restrict__ pq, unsigned long long* __restrict__ gmax,
                                                 const double* __restrict__ krow_arg /* [R], SCHED only */, int leaps /* RN_TAU_LEAP, RN_EULER_MULTINOM only */)
{
    static_assert(OBS == RN_OBS_POIS || WEIGHT != 0, "the transition-only kernels are shared by the observation families");
    static_assert(METH == RN_GILLESPIE || TRANS, "the kernels without a transition are shared by the transition methods");
    if (WEIGHT != 0 && OBS == RN_OBS_POIS) rp.nsz = 0;
    if (METH != RN_EULER_MULTINOM_GWN) rp.nnz = 0;       // (the kernels without a transition read nothing behind size[nsz] through rp's offsets)
    const double* __restrict__ krow = SCHED ? krow_arg : rp.P + rp.o_k();
    static_assert(WEIGHT != 2 || !TRANS, "the auxiliary weights are taken on the particles before the transition");
    static_assert(!SUBAUX || WEIGHT == 1, "SUBAUX corrects the second-stage weights");
    __shared__ double sh[2 * (NTS / 64)];
    __shared__ double snu[RNR * MVD];
    const int d = rp.d;
    if (TRANS && METH == RN_GILLESPIE) {
        if ((int)threadIdx.x < rp.R * d) snu[threadIdx.x] = rp.P[rp.o_nu() + threadIdx.x];
        __syncthreads();
    }
    const long long j = (long long)blockIdx.x * EB + 2 * (long long)threadIdx.x;
    double l0 = -INFINITY, l1 = -INFINITY;
    if (j < N) {
        const bool two = (j + 1 < N);
        double x0[DM], x1[DM];
#pragma unroll
        for (int c = 0; c < DM; c++) { x0[c] = 0.0; x1[c] = 0.0; if (c < d) { x0[c] = x[(long long)c * N + j]; if (two) x1[c] = x[(long long)c * N + j + 1]; } }
        if (TRANS) {
            if (first && rp.tail) rn_reset_counters<DM>(rp, x0, x1);
            if (METH == RN_EULER_MULTINOM || METH == RN_EULER_MULTINOM_GWN) {
                uint32_t srcs, oths;
                rn_classify(rp, srcs, oths);
                rn_transition_em<DM, METH == RN_EULER_MULTINOM_GWN>(x0, rp, krow, leaps, srcs, oths, key, call, (uint32_t)j);
                if (two) rn_transition_em<DM, METH == RN_EULER_MULTINOM_GWN>(x1, rp, krow, leaps, srcs, oths, key, call, (uint32_t)(j + 1));
            } else if (METH == RN_TAU_LEAP) {
                rn_transition_leap<DM>(x0, rp, krow, leaps, key, call, (uint32_t)j);
                if (two) rn_transition_leap<DM>(x1, rp, krow, leaps, key, call, (uint32_t)(j + 1));
            } else {
                rn_transition<DM>(x0, rp, krow, snu, key, call, (uint32_t)j);
                if (two) rn_transition<DM>(x1, rp, krow, snu, key, call, (uint32_t)(j + 1));
            }
#pragma unroll
            for (int c = 0; c < DM; c++) if (c < d) { x[(long long)c * N + j] = x0[c]; if (two) x[(long long)c * N + j + 1] = x1[c]; }
        }
        if (WEIGHT) {
            l0 = rn_loglik<DM, WEIGHT == 2, OBS>(rp, krow, x0, yrow, lgyrow);
            l1 = rn_loglik<DM, WEIGHT == 2, OBS>(rp, krow, x1, yrow, lgyrow);
            if (SUBAUX) { l0 = l0 - auxg[j]; if (two) l1 = l1 - auxg[j + 1]; }
            lw[j] = l0;
            if (two) lw[j + 1] = l1; else l1 = -INFINITY;
        }
    }
    if (WEIGHT) {
        const double bm = block_max_n<NTS / 64>(fmax(l0, l1), sh);
        double s = 0.0, q = 0.0;
        if (bm > -INFINITY) {
            // exp_nonpos: bm is the block's fmax over l0, l1, so l - bm <= 0
            if (l0 > -INFINITY) { const double e = exp_nonpos(l0 - bm); s += e; q += e * e; }
            if (l1 > -INFINITY) { const double e = exp_nonpos(l1 - bm); s += e; q += e * e; }
        }
        block_sum2_n<NTS / 64>(s, q, sh);
        if (threadIdx.x == 0) { pm[blockIdx.x] = bm; ps[blockIdx.x] = s; pq[blockIdx.x] = q; if (gmax) atomicMax(gmax + (blockIdx.x % GM_SLOTS) * GM_STRIDE, f64_key(bm)); }
    }
}

// particles[indices, ] for the ancestors k_apply emitted, d component rows, with the state estimate partials -- k_gather_mv, but
// workgroup b takes the outputs that the elements of block b OWN (the ancestors are sorted: [first i with anc[i] > b EB, first
// i with anc[i] > (b + 1) EB)), strided over its threads.  That is how the expansion kernel groups the built-in SIR's state
// estimate (apply_block: Tb .. Te), so the partials -- and their sum -- associate as the built-in model's do for any number of blocks.
__global__ __launch_bounds__(NT) void k_gather_rn(const int* __restrict__ anc_base, long long anc_stride, long long N, int d,
                                                  const double* __restrict__ xsrc, double* __restrict__ xdst, double* __restrict__ se_part, DevState* st,
                                                  const double* __restrict__ auxsrc, double* __restrict__ auxdst)
{
    __shared__ double sh4[NWV];
    if (st->dead || !st->do_resample || st->flags) return;
    const int* anc = anc_base + (long long)st->cur_call * anc_stride;
    const double invN = 1.0 / (double)N;
    long long lim[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const long long owner_end = ((long long)blockIdx.x + e) * EB;      // outputs owned by the elements below owner_end come first
        long long lo = 0, hi = N;
        while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((long long)anc[mid] > owner_end) hi = mid; else lo = mid + 1; }
        lim[e] = lo;
    }
    double acc[MVD];
#pragma unroll
    for (int c = 0; c < MVD; c++) acc[c] = 0.0;
    for (long long i = lim[0] + threadIdx.x; i < lim[1]; i += NT) {
        const long long src = anc[i] - 1;
#pragma unroll
        for (int c = 0; c < MVD; c++) if (c < d) { const double v = xsrc[(long long)c * N + src]; xdst[(long long)c * N + i] = v; acc[c] += v * invN; }
        if (auxdst) auxdst[i] = auxsrc[src];
    }
    if (!se_part) return;
    for (int c = 0; c < d; c++) { const double s = block_sum(acc[c], sh4); if (threadIdx.x == 0) se_part[(long long)blockIdx.x * d + c] = s; }
}

// ---------------------------------------------------------------------------
// k_pf_batch_rn: many small bootstrap filters of this family per launch, one workgroup = one whole filter with the T loop on
// chip.  It re-enacts pf_run_rn's launches call for call, with the functions k_pf_batch_mv re-enacts pf_run_mv's with (see there;
// only k_init_rn and step_emul_rn are its own): a batched filter returns bit for bit what bssm_pf_run returns for the same block,
// seed and stream.  With one block, k_gather_rn's range is every output, strided over the threads: the EL rounds below.
// LDS: MvBatchSmem and the stoichiometry (static), then the state [d][N] and the ancestors int[N].
// ---------------------------------------------------------------------------
__host__ __device__ constexpr int rn_batch_max_particles(int d)
{
    return (d < 1 || d > MVD) ? 0
         : ((MV_BATCH_LDS - (int)sizeof(MvBatchSmem) - 256 - RNR * MVD * 8) / (8 * d + 4) < EB ? (MV_BATCH_LDS - (int)sizeof(MvBatchSmem) - 256 - RNR * MVD * 8) / (8 * d + 4) : EB);
}

// k_step_rn<DM, TRANS, WEIGHT> for one block of N <= EB particles by NT threads (the partials land in S.pm1, S.ps1, S.pq1);
// first: as k_step_rn's; ko: the offset in the block of the rates of the moment (k_step_rn's krow is rp.P + ko; an offset, not a
// pointer, because a second pointer live across the T loop cost this kernel another 32 B of scratch)
// METH, leaps: as k_step_rn's (only the per-particle transition call differs)
template <int DM, bool TRANS, bool WEIGHT, int OBS = RN_OBS_POIS, int METH = RN_GILLESPIE>
__device__ __forceinline__ void step_emul_rn(MvBatchSmem& S, const double* snu, double* __restrict__ X, long long N, const RnPar& rp, const double* __restrict__ yrow,
                                             const double* __restrict__ lgyrow, PhiloxKey key, uint32_t call, int first, int ko, int leaps)
{
    const double* __restrict__ krow = rp.P + ko;
    constexpr int R = NTS / NT;
    const int t = threadIdx.x;
    const int d = rp.d;
#pragma unroll 1
    for (int r = 0; r < R; r++) {
        const long long j = 2 * (long long)(t + NT * r);
        if (j >= N) continue;
        const bool two = (j + 1 < N);
        double x0[DM], x1[DM];
#pragma unroll
        for (int c = 0; c < DM; c++) { x0[c] = 0.0; x1[c] = 0.0; if (c < d) { x0[c] = X[(long long)c * N + j]; if (two) x1[c] = X[(long long)c * N + j + 1]; } }
        if (TRANS) {
            if (first && rp.tail) rn_reset_counters<DM>(rp, x0, x1);
            if (METH == RN_EULER_MULTINOM || METH == RN_EULER_MULTINOM_GWN) {
                uint32_t srcs, oths;
                rn_classify(rp, srcs, oths);
                rn_transition_em<DM, METH == RN_EULER_MULTINOM_GWN>(x0, rp, krow, leaps, srcs, oths, key, call, (uint32_t)j);
                if (two) rn_transition_em<DM, METH == RN_EULER_MULTINOM_GWN>(x1, rp, krow, leaps, srcs, oths, key, call, (uint32_t)(j + 1));
            } else if (METH == RN_TAU_LEAP) {
                rn_transition_leap<DM>(x0, rp, krow, leaps, key, call, (uint32_t)j);
                if (two) rn_transition_leap<DM>(x1, rp, krow, leaps, key, call, (uint32_t)(j + 1));
            } else {
                rn_transition<DM>(x0, rp, krow, snu, key, call, (uint32_t)j);
                if (two) rn_transition<DM>(x1, rp, krow, snu, key, call, (uint32_t)(j + 1));
            }
#pragma unroll
            for (int c = 0; c < DM; c++) if (c < d) { X[(long long)c * N + j] = x0[c]; if (two) X[(long long)c * N + j + 1] = x1[c]; }
        }
        if (WEIGHT) {
            const double l0 = rn_loglik<DM, false, OBS>(rp, krow, x0, yrow, lgyrow);
            const double l1 = rn_loglik<DM, false, OBS>(rp, krow, x1, yrow, lgyrow);
            S.LW[j] = l0; if (two) S.LW[j + 1] = l1;
        }
    }
    if (WEIGHT) batch_lse_partials(S, N);
}

// g.theta: [F][g.theta_stride] packed blocks; g.y, g.lgy: [T][p]; g.state_est: [F][T+1][d]
// OBS = RN_OBS_NB: the blocks carry size[p] after G, and g.lgy is the filters' own tables c(t, k), [F][T][p] (g.lgy_stride = T p);
// the Poisson instantiation reads no stride (one shared table)
// METH: the transition method (k_step_rn's), leaps its wave-uniform count of leaps (RN_TAU_LEAP, RN_EULER_MULTINOM only; not read otherwise)
// REC: BatchNoRec, or BatchRec: the launch also leaves its histories for the smoother (batch_record, mv.hip.h)
template <int DM, int OBS = RN_OBS_POIS, int METH = RN_GILLESPIE, class REC = BatchNoRec>
__global__ __launch_bounds__(NT) void k_pf_batch_rn(BatchArgs g, int d, int nreact, int p, int leaps, REC rec)
{
    __shared__ MvBatchSmem S;
    __shared__ double snu[RNR * MVD];
    extern __shared__ __attribute__((aligned(16))) double XD[];        // [d][N] state, then int[N] ancestors (1-based)
    const int fi = blockIdx.x, t = threadIdx.x;
    const long long N = g.N;
    const int T = g.T;
    double* X = XD;
    int* ANC = reinterpret_cast<int*>(XD + (long long)d * N);
    RnPar rp; rp.P = g.theta + (long long)fi * g.theta_stride; rp.d = d; rp.R = nreact; rp.p = p;
    rp.nsz = OBS == RN_OBS_NB ? p : 0;
    rp.nnz = METH == RN_EULER_MULTINOM_GWN ? 2 * nreact : 0;
    // (the host checked: size(), size() + d, or size() + d + 1 + n_times R with the block's own n_times entry agreeing)
    rp.tail = g.theta_stride != rp.size() ? 1 : 0;
    rp.n_times = g.theta_stride > rp.size_tail() ? (g.theta_stride - rp.size_tail() - 1) / nreact : 0;
    const PhiloxKey key = g.keys[fi];
    const bool lit = g.N <= g.lit_max;
    const double invN = 1.0 / (double)N;
    double* se_out = g.state_est + (long long)fi * (T + 1) * d;
    if (METH == RN_GILLESPIE) { if (t < nreact * d) snu[t] = rp.P[rp.o_nu() + t]; }
    batch_reset_state(S.st);
    {   // k_init_rn
        double acc[DM];
#pragma unroll
        for (int c = 0; c < DM; c++) acc[c] = 0.0;
#pragma unroll 1
        for (int r = 0; r < EL / 2; r++) {
            const long long j = 2 * (t + NT * r);
            if (j < N) {
#pragma unroll
                for (int c = 0; c < DM; c++) {
                    if (c < d) {
                        const double v = rp.P[rp.o_x0() + c];
                        X[(long long)c * N + j] = v; acc[c] += v * invN;
                        if (j + 1 < N) { X[(long long)c * N + j + 1] = v; acc[c] += v * invN; }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < DM; c++) if (c < d) { const double s = block_sum(acc[c], S.sm.sh4); if (t == 0) se_out[c] = 0.0 + s; }
    }
    __syncthreads();
    batch_record(rec, S, g, fi, d, 0, X, ANC);
    int ktrans = 0, ot = 0;
    for (int i = 1; i <= T; i++) {                                                        // R/particle_filter_core.R:123
        const int gap = batch_next_obs(g, i, ot);                                         // :124
        const double* yrow = g.y + (long long)(i - 1) * p;
        const double* lgyrow = g.lgy + (OBS == RN_OBS_NB ? (long long)fi * g.lgy_stride : 0LL) + (long long)(i - 1) * p;
        for (int step = 1; step <= gap; step++) {                                         // :125-136, the last one with weight_fn (:177-183)
            const int krow = rp.n_times ? rp.o_sched() + (ot - gap + step - 1) * nreact : rp.o_k();     // rates_row(prev_t + step), as an offset
            if (step == gap) step_emul_rn<DM, true, true, OBS, METH>(S, snu, X, N, rp, yrow, lgyrow, key, (uint32_t)ktrans, step == 1, krow, leaps);
            else step_emul_rn<DM, true, false, RN_OBS_POIS, METH>(S, snu, X, N, rp, yrow, lgyrow, key, (uint32_t)ktrans, step == 1, krow, leaps);
            ktrans++;
            __syncthreads();
        }
        if (gap <= 0) { step_emul_rn<DM, false, true, OBS>(S, snu, X, N, rp, yrow, lgyrow, key, 0u, 0, rp.o_k(), 0); __syncthreads(); }
        batch_weigh_resample(S, g, key, fi, i, lit, ANC);                                 // :204-224: ancestors only
        double acc[DM];
#pragma unroll
        for (int c = 0; c < DM; c++) acc[c] = 0.0;
        const bool gather = !S.st.dead && S.st.do_resample && !S.st.flags;               // k_gather_rn's guard
        const bool carry = g.resample_algorithm != 1 && !S.st.dead && !S.st.do_resample; // k_carry_mv's (launched for SIS / SISAR)
        if (gather) {                                                                     // particles[indices, ], a component at a time
#pragma unroll
            for (int c = 0; c < DM; c++) {
                if (c < d) {
                    double v[EL];
#pragma unroll
                    for (int r = 0; r < EL; r++) {
                        const long long k = t + NT * r;
                        v[r] = (k < N) ? X[(long long)c * N + ANC[k] - 1] : 0.0;
                        if (k < N) acc[c] += v[r] * invN;
                    }
                    __syncthreads();
#pragma unroll
                    for (int r = 0; r < EL; r++) { const long long k = t + NT * r; if (k < N) X[(long long)c * N + k] = v[r]; }
                }
            }
        } else if (carry) {                                                               // state estimate = colSums(particles * weights) (:238)
#pragma unroll 1
            for (int r = 0; r < EL; r++) {
                const long long j = t + NT * r;
                if (j < N) {
                    const double wj = S.LW[j];
#pragma unroll
                    for (int c = 0; c < DM; c++) if (c < d) acc[c] += X[(long long)c * N + j] * wj;
                }
            }
        }
        if (gather || carry) {
#pragma unroll
            for (int c = 0; c < DM; c++) if (c < d) { const double s = block_sum(acc[c], S.sm.sh4); if (t == 0) se_out[(long long)i * d + c] = 0.0 + s; }
        } else if (t == 0) {
            for (int c = 0; c < d; c++) se_out[(long long)i * d + c] = 0.0;              // (no partial written: the zeroed slot)
        }
        if (S.st.dead) break;                            // degenerate weights: the reference returns at once (:189-202)
        batch_record(rec, S, g, fi, d, i, X, ANC);
        __syncthreads();
    }
    batch_publish_state(g, fi, S.st);
}

// bssm_dump_rpois: out[j] = the draw of particle j for reaction r in leap `leap` of transition call `call` at the mean lam[j]
__global__ void k_dump_rpois(PhiloxKey key, uint32_t call, uint32_t lr, long long n, const double* __restrict__ lam, double* __restrict__ out)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = rn_rpois(lam[j], key, call, (uint32_t)j, lr);
}

// bssm_dump_rgamma: out[j] = the draw of particle j for the noise group with leader g in leap `leap` of transition call `call` at the shape sh[j]
__global__ void k_dump_rgamma(PhiloxKey key, uint32_t call, uint32_t lg, long long n, const double* __restrict__ sh, double* __restrict__ out)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = rn_rgamma(sh[j], key, call, (uint32_t)j, lg);
}

// bssm_dump_rbinom: out[j] = the draw of particle j for reaction r in leap `leap` of transition call `call` at (nn[j], q[j])
__global__ void k_dump_rbinom(PhiloxKey key, uint32_t call, uint32_t lr, long long n, const double* __restrict__ nn, const double* __restrict__ q, double* __restrict__ out)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = rn_rbinom(nn[j], q[j], key, call, (uint32_t)j, lr);
}

}  // namespace bssm
