// mv.hip.h -- multivariate linear-Gaussian family (state dimension d <= 8, observation dimension p <= 8) on the device.
//
// The reference's models are R closures over an N x d particle matrix (R/particle_filter_core.R:76-88; its own multi-dimensional
// cases: tests/testthat/test-bootstrap_filter.R:211-230, tests/testthat/test-pmmh.R:619-668 -- a 2-d random walk with a constant
// log-likelihood).  This family covers those and the general linear-Gaussian state-space model:
//   init_fn          x0 = m0 + L0 z                      z ~ N(0, I_d)          (matrix(rnorm(N d), ncol = d), shifted and scaled)
//   transition_fn    x' = A x + b + L z                  L lower triangular (a Cholesky factor of Q)
//   log_likelihood   p == 0: the constant c0             (the reference tests' rep(1, nrow(particles)))
//                    p >  0: sum_k dnorm(y_k, h0_k + (H x)_k, sd_k, log = TRUE)      (independent observation components)
//                    or, over the same linear predictor eta_k = h0_k + (H x)_k (the OBS template parameter, mv_obs_log):
//                      Poisson counts through a log link     sum_k dpois(y_k, exp(eta_k), log = TRUE)
//                      log-variance (stochastic volatility)  sum_k dnorm(y_k, 0, exp(eta_k / 2), log = TRUE)
//   aux (APF)        the log-likelihood at the transition mean A x + b              (k_step_mv<false, 2>)
//   move (RMPF)      random-walk Metropolis, d independent normals per particle     (k_move_mv)
// Only the model evaluation is new: normalisation, log-likelihood, ESS, the resample decision and the exact resampling run in the
// same kernels as every other filter (k_local / k_apply, which here emit ANCESTORS); particles[indices, ] is then a gather of d
// coalesced component rows (k_gather_mv).  Particles are SoA [d][N].
// Arithmetic (fp64, contraction off), in one fixed order of operations (the parity tests restate it on the CPU operation for operation):
//   x'_c = ((b_c + A_c0 x_0) + A_c1 x_1 + ... ) + L_c0 z_0 + ... + L_cc z_c        (left to right)
// Time-varying pieces (data next to y, not part of the block): b_t [n_times][d], h0_t [T][p], H_t [T][p][d] replace the block's
// b / h0 / H where given.  The transition TO absolute time tau reads b_t[tau - 1] (tau = prev_t + step in the gap loop; the
// APF's second transition and its aux transition mean: tau = the observation's time); everything evaluated at observation
// row i (likelihood, aux likelihood, the move's two likelihoods) reads h0_t[i - 1], H_t[i - 1].  Only where a coefficient is
// loaded from changes, never the order of operations.
#pragma once
#include "kernels.hip.h"

namespace bssm {

constexpr int MVD = 8;            // largest state / observation dimension
// packed parameter block (doubles): d, p, m0[d], L0[d d], A[d d], b[d], L[d d], c0, H[p d], h0[p], sd[p], log(sd)[p]
struct MvPar {
    const double* P; int d, p;
    __host__ __device__ int o_m0() const { return 2; }
    __host__ __device__ int o_L0() const { return 2 + d; }
    __host__ __device__ int o_A() const { return o_L0() + d * d; }
    __host__ __device__ int o_b() const { return o_A() + d * d; }
    __host__ __device__ int o_L() const { return o_b() + d; }
    __host__ __device__ int o_c0() const { return o_L() + d * d; }
    __host__ __device__ int o_H() const { return o_c0() + 1; }
    __host__ __device__ int o_h0() const { return o_H() + p * d; }
    __host__ __device__ int o_sd() const { return o_h0() + p; }
    __host__ __device__ int o_lsd() const { return o_sd() + p; }
    __host__ __device__ int size() const { return o_lsd() + p; }
};

// the time-varying rows of ONE launch: b [d], h0 [p], H [p][d]; a null pointer = the block's constant piece.  Wave-uniform, as the
// block is: the loads stay on the scalar cache.
struct MvTv {
    const double* b; const double* h0; const double* H;
    __device__ const double* b_of(const MvPar& mp) const { return b ? b : mp.P + mp.o_b(); }
    __device__ const double* h0_of(const MvPar& mp) const { return h0 ? h0 : mp.P + mp.o_h0(); }
    __device__ const double* H_of(const MvPar& mp) const { return H ? H : mp.P + mp.o_H(); }
};
// the whole arrays, for the batched kernel; b_t holds n_times rows.  One array per piece shared by all filters of the launch, as
// y is (stride 0), or one SET per parameter draw: filter f reads set set_of[f] (nullptr: set 0), sb / sh0 / sH doubles apart.
// The set index comes from blockIdx.x alone, so the offset pointers stay workgroup-uniform and the loads on the scalar cache.
struct MvTvBatch {
    const double* b; const double* h0; const double* H; int n_times;
    const int* set_of; long long sb, sh0, sH;
};

struct MvNoise { const double* arr; PhiloxKey key; uint32_t purpose, call; };      // arr: [d][N] injected draws of this call, or nullptr

// Observation families over the linear predictor eta_k = h0_k + (H x)_k (accumulated as the Gaussian mean always was).
constexpr int MV_OBS_GAUSS = 0;     // dnorm(y_k, eta_k, sd_k, log = TRUE)              BSSM_MODEL_LGMV
constexpr int MV_OBS_POIS = 1;      // dpois(y_k, exp(eta_k), log = TRUE)                BSSM_MODEL_LGMV_POIS
constexpr int MV_OBS_LOGVAR = 2;    // dnorm(y_k, 0, exp(eta_k / 2), log = TRUE)         BSSM_MODEL_LGMV_LOGVAR
// what component k's density reads besides eta: sd / log(sd) from the block (Gaussian), lgamma(y_k + 1) from the host's table
// (Poisson; lgyrow: row i - 1 of [T][p], as yrow).  Wave-uniform loads.  A family does not load what it does not read.
struct MvObsK { double y, sd, lsd, lgy; };
template <int OBS>
__device__ __forceinline__ MvObsK mv_obs_k(const MvPar& mp, const double* __restrict__ yrow, const double* __restrict__ lgyrow, int k)
{
    MvObsK o; o.y = yrow[k]; o.sd = 0.0; o.lsd = 0.0; o.lgy = 0.0;
    if (OBS == MV_OBS_GAUSS) { o.sd = mp.P[mp.o_sd() + k]; o.lsd = mp.P[mp.o_lsd() + k]; }
    if (OBS == MV_OBS_POIS) o.lgy = lgyrow[k];
    return o;
}
// Missing observations (the context option mv_y_missing; otherwise the host refuses them): a NaN in y_k means that component k of
// this observation was not seen, and the log-likelihood is the sum over the observed k only (in increasing k from 0.0; a row
// with nothing observed gives every particle 0.0, what a reference closure returning zeros gives).  y_k depends on (row, k)
// alone and comes off the scalar cache, so this is a wave-uniform branch around component k's eta accumulation and density:
// no lane diverges, no particle loads anything more, and a missing y_k reaches no arithmetic.  With every y_k observed the
// operations and their order are what they were.
__device__ __forceinline__ bool mv_observed(const MvObsK& o) { return o.y == o.y; }
// log-density of observation component k at the linear predictor eta, in one fixed order of operations:
//   Gaussian      r_dnorm_log(y, eta, sd, log(sd))
//   Poisson       lambda = exp(eta);  -inf unless lambda < +inf;  y == 0: -lambda;  else (y eta - lambda) - lgamma(y + 1).
//                 This is Sir::dpois_log (kernels.hip.h, with its note on R's dpois_raw) with log(lambda) = eta taken exactly.
//   log-variance  (-log(sqrt(2 pi)) - 0.5 eta) - (0.5 (y y)) exp(-eta);  the last term is 0 when 0.5 (y y) == 0.0 (no 0 * inf);
//                 -inf for a non-finite eta
template <int OBS>
__device__ __forceinline__ double mv_obs_log(const MvObsK& o, double eta)
{
    if (OBS == MV_OBS_POIS) {
        const double lambda = exp(eta);
        if (!(lambda < INFINITY)) return -INFINITY;
        if (o.y == 0.0) return -lambda;
        return (o.y * eta - lambda) - o.lgy;
    }
    if (OBS == MV_OBS_LOGVAR) {
        if (!isfinite(eta)) return -INFINITY;
        const double hq = 0.5 * (o.y * o.y);
        const double t = (hq == 0.0) ? 0.0 : hq * exp(-eta);
        return (-BSSM_LN_SQRT_2PI - 0.5 * eta) - t;
    }
    return r_dnorm_log(o.y, eta, o.sd, o.lsd);
}

// init_fn (R/particle_filter_core.R:76-88) + the t = 0 state estimate partials (:109-112)
__global__ __launch_bounds__(NT) void k_init_mv(double* __restrict__ x, long long N, MvPar mp, MvNoise ns, double* __restrict__ se_part /* [B][d] */)
{
    __shared__ double sh4[NWV];
    const int d = mp.d;
    const long long base = (long long)blockIdx.x * EB;
    const double invN = 1.0 / (double)N;
    double acc[MVD];
#pragma unroll
    for (int c = 0; c < MVD; c++) acc[c] = 0.0;
#pragma unroll 1
    for (int r = 0; r < EL; r++) {
        const long long j = base + threadIdx.x + NT * r;
        if (j < N) {
            double z[MVD];
#pragma unroll
            for (int c = 0; c < MVD; c++) {
                z[c] = 0.0;
                if (c < d) {
                    if (ns.arr) z[c] = ns.arr[(long long)c * N + j];
                    else { double z0, z1; normal_pair(ns.key, ns.purpose, ns.call, (uint32_t)c, (uint32_t)(j >> 1), z0, z1); z[c] = (j & 1) ? z1 : z0; }
                }
            }
#pragma unroll
            for (int c = 0; c < MVD; c++) {
                if (c < d) {
                    double v = mp.P[mp.o_m0() + c];
#pragma unroll
                    for (int k = 0; k < MVD; k++) if (k <= c) v = v + mp.P[mp.o_L0() + c * d + k] * z[k];
                    x[(long long)c * N + j] = v;
                    acc[c] += v * invN;
                }
            }
        }
    }
    for (int c = 0; c < d; c++) { const double s = block_sum(acc[c], sh4); if (threadIdx.x == 0) se_part[(long long)blockIdx.x * d + c] = s; }
}

// transition_fn and / or weight_fn (R/particle_filter_core.R:127,177-183) with the block partials of the log-sum-exp, as k_step
//   WEIGHT 1: lw = log_likelihood(y, x')
//   WEIGHT 2: lw = the auxiliary log-likelihood at the CURRENT particles, no transition (:142-147): the log-likelihood at the
//             transition mean  m = A x + b,  m_c = (b_c + A_c0 x_0) + A_c1 x_1 + ...  (p == 0: the constant c0)
//   SUBAUX  : lw -= auxg[j], the first stage's aux log-weight of the ancestor, already gathered (:175)
//   OBS     : the observation family (mv_obs_log); lgyrow [p]: this observation's row of lgamma(y + 1), read by the Poisson family only
template <bool TRANS, int WEIGHT, bool SUBAUX = false, int OBS = MV_OBS_GAUSS>
__global__ __launch_bounds__(NTS) void k_step_mv(double* __restrict__ x, double* __restrict__ lw, const double* __restrict__ auxg, long long N, MvPar mp, MvTv tv,
                                                 const double* __restrict__ yrow /* [p] */, const double* __restrict__ lgyrow, MvNoise ns, double* __restrict__ pm,
                                                 double* __restrict__ ps, double* __restrict__ pq, unsigned long long* __restrict__ gmax)
{
    static_assert(WEIGHT != 2 || !TRANS, "the auxiliary weights are taken on the particles before the transition");
    static_assert(!SUBAUX || WEIGHT == 1, "SUBAUX corrects the second-stage weights");
    __shared__ double sh[2 * (NTS / 64)];
    const int d = mp.d, p = mp.p;
    const double* __restrict__ Pb = tv.b_of(mp);
    const double* __restrict__ Ph0 = tv.h0_of(mp);
    const double* __restrict__ PH = tv.H_of(mp);
    const long long j = (long long)blockIdx.x * EB + 2 * (long long)threadIdx.x;
    double l0 = -INFINITY, l1 = -INFINITY;
    if (j < N) {
        const bool two = (j + 1 < N);
        double x0[MVD], x1[MVD];
#pragma unroll
        for (int c = 0; c < MVD; c++) { x0[c] = 0.0; x1[c] = 0.0; if (c < d) { x0[c] = x[(long long)c * N + j]; if (two) x1[c] = x[(long long)c * N + j + 1]; } }
        if (TRANS) {
            double z0[MVD], z1[MVD];
#pragma unroll
            for (int c = 0; c < MVD; c++) {
                z0[c] = 0.0; z1[c] = 0.0;
                if (c < d) {
                    if (ns.arr) { z0[c] = ns.arr[(long long)c * N + j]; if (two) z1[c] = ns.arr[(long long)c * N + j + 1]; }
                    else normal_pair(ns.key, ns.purpose, ns.call, (uint32_t)c, (uint32_t)(j >> 1), z0[c], z1[c]);
                }
            }
            double n0[MVD], n1[MVD];
#pragma unroll
            for (int c = 0; c < MVD; c++) {
                n0[c] = 0.0; n1[c] = 0.0;
                if (c < d) {
                    double a0 = Pb[c], a1 = a0;
#pragma unroll
                    for (int k = 0; k < MVD; k++) if (k < d) { const double A = mp.P[mp.o_A() + c * d + k]; a0 = a0 + A * x0[k]; a1 = a1 + A * x1[k]; }
#pragma unroll
                    for (int k = 0; k < MVD; k++) if (k <= c) { const double L = mp.P[mp.o_L() + c * d + k]; a0 = a0 + L * z0[k]; a1 = a1 + L * z1[k]; }
                    n0[c] = a0; n1[c] = a1;
                }
            }
#pragma unroll
            for (int c = 0; c < MVD; c++) if (c < d) { x0[c] = n0[c]; x1[c] = n1[c]; x[(long long)c * N + j] = n0[c]; if (two) x[(long long)c * N + j + 1] = n1[c]; }
        }
        if (WEIGHT == 2 && p > 0) {          // the transition mean replaces the particles (nothing is stored: TRANS is off)
            double m0[MVD], m1[MVD];
#pragma unroll
            for (int c = 0; c < MVD; c++) {
                m0[c] = 0.0; m1[c] = 0.0;
                if (c < d) {
                    double a0 = Pb[c], a1 = a0;
#pragma unroll
                    for (int k = 0; k < MVD; k++) if (k < d) { const double A = mp.P[mp.o_A() + c * d + k]; a0 = a0 + A * x0[k]; a1 = a1 + A * x1[k]; }
                    m0[c] = a0; m1[c] = a1;
                }
            }
#pragma unroll
            for (int c = 0; c < MVD; c++) { x0[c] = m0[c]; x1[c] = m1[c]; }
        }
        if (WEIGHT) {
            if (p == 0) { l0 = mp.P[mp.o_c0()]; l1 = l0; }
            else {
                l0 = 0.0; l1 = 0.0;
#pragma unroll
                for (int k = 0; k < MVD; k++) {
                    if (k < p) {
                        const MvObsK ok = mv_obs_k<OBS>(mp, yrow, lgyrow, k);
                        if (mv_observed(ok)) {
                            double m0 = Ph0[k], m1 = m0;
#pragma unroll
                            for (int c = 0; c < MVD; c++) if (c < d) { const double H = PH[k * d + c]; m0 = m0 + H * x0[c]; m1 = m1 + H * x1[c]; }
                            l0 = l0 + mv_obs_log<OBS>(ok, m0);
                            l1 = l1 + mv_obs_log<OBS>(ok, m1);
                        }
                    }
                }
            }
            if (SUBAUX) { l0 = l0 - auxg[j]; if (two) l1 = l1 - auxg[j + 1]; }
            if (!two) l1 = -INFINITY;
            lw[j] = l0; if (two) lw[j + 1] = l1;
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

// particles[indices, ] (R/resampling.R:40,60) for the ancestors k_apply emitted, d component rows; state estimate partials (:237-241).
// The auxiliary filter's first stage (:155-157) also carries aux_log_weights[indices] (auxsrc -> auxdst) and takes no state
// estimate (se_part == nullptr).
__global__ __launch_bounds__(NT) void k_gather_mv(const int* __restrict__ anc_base, long long anc_stride, long long N, int d,
                                                  const double* __restrict__ xsrc, double* __restrict__ xdst, double* __restrict__ se_part, DevState* st,
                                                  const double* __restrict__ auxsrc, double* __restrict__ auxdst)
{
    __shared__ double sh4[NWV];
    if (st->dead || !st->do_resample || st->flags) return;
    const int* anc = anc_base + (long long)st->cur_call * anc_stride;
    const double invN = 1.0 / (double)N;
    double acc[MVD];
#pragma unroll
    for (int c = 0; c < MVD; c++) acc[c] = 0.0;
#pragma unroll 1
    for (int r = 0; r < EL; r++) {
        const long long i = (long long)blockIdx.x * EB + threadIdx.x + NT * r;
        if (i < N) {
            const long long src = anc[i] - 1;
#pragma unroll
            for (int c = 0; c < MVD; c++) if (c < d) { const double v = xsrc[(long long)c * N + src]; xdst[(long long)c * N + i] = v; acc[c] += v * invN; }
            if (auxdst) auxdst[i] = auxsrc[src];
        }
    }
    if (!se_part) return;
    for (int c = 0; c < d; c++) { const double s = block_sum(acc[c], sh4); if (threadIdx.x == 0) se_part[(long long)blockIdx.x * d + c] = s; }
}

// no resampling at this observation: carry over, state estimate = colSums(particles * weights) (:238)
__global__ __launch_bounds__(NT) void k_carry_mv(const double* __restrict__ xsrc, double* __restrict__ xdst, const double* __restrict__ w, long long N, int d,
                                                 double* __restrict__ se_part, const DevState* __restrict__ st)
{
    __shared__ double sh4[NWV];
    if (st->dead || st->do_resample) return;
    double acc[MVD];
#pragma unroll
    for (int c = 0; c < MVD; c++) acc[c] = 0.0;
#pragma unroll 1
    for (int r = 0; r < EL; r++) {
        const long long j = (long long)blockIdx.x * EB + threadIdx.x + NT * r;
        if (j < N) {
            const double wj = w[j];
#pragma unroll
            for (int c = 0; c < MVD; c++) if (c < d) { const double v = xsrc[(long long)c * N + j]; xdst[(long long)c * N + j] = v; acc[c] += v * wj; }
        }
    }
    for (int c = 0; c < d; c++) { const double s = block_sum(acc[c], sh4); if (threadIdx.x == 0) se_part[(long long)blockIdx.x * d + c] = s; }
}

// One (normal, uniform) draw set of the resample-move step: component c of particle i at observation `call` is keyed by the
// Philox counter (i, call, DRAW_MOVE | (c << 8), stream); z_c = qnorm(u01(r.x, r.y)), the acceptance uniform is u01(r.z, r.w) of
// component 0.  At d = 1 this is move_draws (rng.h) exactly.
__device__ __forceinline__ void move_draw_mv(PhiloxKey key, uint32_t call, uint32_t i, uint32_t c, double& z, double& u)
{
    u32x4 ctr; ctr.x = i; ctr.y = call; ctr.z = DRAW_MOVE | (c << 8); ctr.w = key.stream;
    const u32x4 r = philox4x32_10(ctr, key.k0, key.k1);
    z = qnorm_as241(u01_from_bits(r.x, r.y));
    u = u01_from_bits(r.z, r.w);
}

// resample_move_filter's move step (R/particle_filter_core.R:226-234) for the family: the d-dimensional form of the reference
// example's random-walk Metropolis move (R/resample_move_filter.R:166-176) -- d independent normals per particle,
//   prop_c = x_c + (0.0 + sd z_c);  accept when log(u) < loglik(prop) - loglik(x)   (p == 0: always)
// One particle per lane; then the state-estimate partials, which the core takes AFTER the move (:237-241), as move_block.
// zmv: [d][N] injected normals of this observation, umv: [N] (or both nullptr: the generator).
// The proposals are built a component at a time (a loop the compiler keeps rolled: a generator draw is long) and parked in
// this lane's own LDS column; the likelihoods then run fully unrolled on register arrays, as in k_step_mv.
template <int OBS = MV_OBS_GAUSS>
__global__ __launch_bounds__(NT) void k_move_mv(double* __restrict__ x, long long N, MvPar mp, MvTv tv, const double* __restrict__ yrow, const double* __restrict__ lgyrow, double move_sd,
                                                const double* __restrict__ zmv, const double* __restrict__ umv, PhiloxKey key, uint32_t call,
                                                double* __restrict__ se_part, const DevState* __restrict__ st)
{
    __shared__ double sh4[NWV];
    __shared__ double sprop[MVD][NT];
    if (st->dead) return;
    const int d = mp.d, p = mp.p;
    const double* __restrict__ Ph0 = tv.h0_of(mp);
    const double* __restrict__ PH = tv.H_of(mp);
    const double invN = 1.0 / (double)N;
    double acc[MVD];
#pragma unroll
    for (int c = 0; c < MVD; c++) acc[c] = 0.0;
#pragma unroll 1
    for (int r = 0; r < EL; r++) {
        const long long j = (long long)blockIdx.x * EB + threadIdx.x + NT * r;
        if (j < N) {
            double u = 0.0;
#pragma unroll 1
            for (int c = 0; c < d; c++) {
                double z, uc;
                if (zmv) { z = zmv[(long long)c * N + j]; uc = umv[j]; }
                else move_draw_mv(key, call, (uint32_t)j, (uint32_t)c, z, uc);
                if (c == 0) u = uc;
                sprop[c][threadIdx.x] = x[(long long)c * N + j] + r_rnorm(0.0, move_sd, z);
            }
            double cur[MVD], prop[MVD];
#pragma unroll
            for (int c = 0; c < MVD; c++) {
                cur[c] = 0.0; prop[c] = 0.0;
                if (c < d) { cur[c] = x[(long long)c * N + j]; prop[c] = sprop[c][threadIdx.x]; }
            }
            // log-likelihoods of the particle and of the proposal, in k_step_mv's order of operations
            double lc = mp.P[mp.o_c0()], lp = lc;
            if (p > 0) {
                lc = 0.0; lp = 0.0;
#pragma unroll
                for (int k = 0; k < MVD; k++) {
                    if (k < p) {
                        const MvObsK ok = mv_obs_k<OBS>(mp, yrow, lgyrow, k);
                        if (mv_observed(ok)) {
                            double mc = Ph0[k], mq = mc;
#pragma unroll
                            for (int c = 0; c < MVD; c++) if (c < d) { const double H = PH[k * d + c]; mc = mc + H * cur[c]; mq = mq + H * prop[c]; }
                            lc = lc + mv_obs_log<OBS>(ok, mc);
                            lp = lp + mv_obs_log<OBS>(ok, mq);
                        }
                    }
                }
            }
            // (two branches, not a select of prop[c] / cur[c]: the compiler turns that into a select of the two arrays' addresses,
            //  which puts both arrays in scratch)
            if ((p == 0) || (log(u) < (lp - lc))) {
#pragma unroll
                for (int c = 0; c < MVD; c++) if (c < d) { x[(long long)c * N + j] = prop[c]; acc[c] += prop[c] * invN; }
            } else {
#pragma unroll
                for (int c = 0; c < MVD; c++) if (c < d) acc[c] += cur[c] * invN;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < MVD; c++) if (c < d) { const double s = block_sum(acc[c], sh4); if (threadIdx.x == 0) se_part[(long long)blockIdx.x * d + c] = s; }
}

// ---------------------------------------------------------------------------
// k_pf_batch_mv: many small filters of this family per launch, ONE workgroup = ONE whole bootstrap filter with the T loop on
// chip -- k_pf_batch (kernels.hip.h) for d <= 8 state components.  It re-enacts pf_run_mv's launches call for call, so a
// batched filter returns bit for bit what bssm_pf_run returns for the same packed block, seed and stream:
//   k_init_mv                  the same thread mapping (NT threads, EL rounds), normals keyed by (component, j >> 1)
//   k_step_mv<TRANS, WEIGHT>   step_emul_mv: thread t plays the threads t + NT r of the NTS-thread kernel (step_emul's mapping);
//                              its reductions: batch_lse_partials
//   k_local / resolve / k_apply   batch_weigh_resample, ancestors only (as k_apply emits them here)
//   k_gather_mv / k_carry_mv   per-thread partials over the EL rounds, block_sum, then what k_reduce_state_est does with
//                              one block: 0.0 + the partial.  The gather runs a component at a time (every thread loads its EL
//                              values X[c][anc[i] - 1], barrier, stores them).  k_pf_batch_rn holds a copy of this tail: as one
//                              shared function it added 45 - 445 spilled SGPRs to every k_pf_batch_rn instantiation and took
//                              k_pf_batch_rn<2, Poisson, gamma noise> from two waves per SIMD to one (profiles r22_a, r22_c)
// The run state, its publishing and the observation clock: batch_reset_state, batch_publish_state, batch_next_obs.
// LDS: the static part (MvBatchSmem) plus, sized by the launch, ONE state buffer [d][N] and the ancestors int[N].
// ---------------------------------------------------------------------------
struct MvBatchSmem {
    SegSmem sm;
    uint64_t tin[NT + 1];
    int Tl[EB];
    alignas(16) double LW[EB];        // log-weights, then (in place) the normalised weights
    alignas(16) double SCR[EB];       // the in-order pass publishes its prob terms in apply_block's destination buffer
    double es[NT];
    double shm[NTS / 64], shs[NTS / 64], shq[NTS / 64];
    DevState st;
    BlockRec br;
    double pm1, ps1, pq1, ainw1, ainp1;
    uint64_t cin1;
    int Tbegin;
};
constexpr int MV_BATCH_LDS = 160 * 1024;     // LDS of one CU: the whole budget of one workgroup
// largest N of a batched filter with d state components: static LDS + d N doubles + N ancestors (0 for d outside 1..8)
__host__ __device__ constexpr int mv_batch_max_particles(int d)
{
    return (d < 1 || d > MVD) ? 0
         : ((MV_BATCH_LDS - (int)sizeof(MvBatchSmem) - 256) / (8 * d + 4) < EB ? (MV_BATCH_LDS - (int)sizeof(MvBatchSmem) - 256) / (8 * d + 4) : EB);
}
__host__ __device__ constexpr size_t mv_batch_dyn_lds(int d, long long N) { return (size_t)N * (8 * d + 4); }

// ---- the steps of an on-chip filter that are not model arithmetic, written once for k_pf_batch_mv and k_pf_batch_rn (rnet.hip.h).
// k_pf_batch (kernels.hip.h) keeps its own text: it is the kernel the small-N PMMH runs on, and as a caller of these its time per
// observation moved (profiles r22_b)

// the run state at the start of a filter (thread 0; k_reset_state's fields and force_fallback, which no *_block body reads
// without a resolver of its own)
__device__ __forceinline__ void batch_reset_state(DevState& st)
{
    if (threadIdx.x != 0) return;
    st.loglike = 0.0; st.lse_max = 0.0; st.lse_sum = 0.0; st.ess = 0.0; st.total_bits = 0;
    st.do_resample = 0; st.dead = 0; st.flags = 0; st.res_calls = 0; st.cur_call = 0; st.debug_stop = 0;
    st.out_lo = 0; st.out_hi = 0; st.force_fallback = 0;
    st.stat_hard_blocks = 0; st.stat_serial_walks = 0; st.stat_literal_terms = 0;
}
// ... and what the host reads of it at the end
__device__ __forceinline__ void batch_publish_state(const BatchArgs& g, int fi, const DevState& st)
{
    if (threadIdx.x == 0) { g.loglike[fi] = st.loglike; g.dead[fi] = st.dead; g.flags[fi] = st.flags; g.res_calls[fi] = st.res_calls; }
}

// the observation clock (R/particle_filter_core.R:123-124): ot moves from the time of observation i - 1 (0 before the first)
// to observation i's; returns the gap between the two, the number of transitions to run
__device__ __forceinline__ int batch_next_obs(const BatchArgs& g, int i, int& ot)
{
    const int prev_t = ot;
    ot = g.obs_times ? g.obs_times[i - 1] : i;
    return ot - prev_t;
}

// The log-sum-exp partials (S.pm1, S.ps1, S.pq1) of the log-weights in S.LW: block_max_n<NTS/64> then block_sum2_n<NTS/64> of the
// NTS-thread step kernels (k_step_mv, k_step_rn).  Wave w + 4 r there is wave w of round r here (the same 64 lanes); its per-wave
// values are combined in wave order.  The log-weights come back from LDS exactly as they were stored.
__device__ __forceinline__ void batch_lse_partials(MvBatchSmem& S, long long N)
{
    constexpr int R = NTS / NT;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __syncthreads();
    double l0[R], l1[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const long long j = 2 * (long long)(t + NT * r);
        l0[r] = -INFINITY; l1[r] = -INFINITY;
        if (j < N) { l0[r] = S.LW[j]; if (j + 1 < N) l1[r] = S.LW[j + 1]; }
        const double v = wave_max(fmax(l0[r], l1[r]));
        if (lane == 0) S.shm[wave + (NT / 64) * r] = v;
    }
    __syncthreads();
    double bm = S.shm[0];
#pragma unroll
    for (int i = 1; i < NTS / 64; i++) bm = fmax(bm, S.shm[i]);
#pragma unroll
    for (int r = 0; r < R; r++) {
        double s_ = 0.0, q_ = 0.0;
        if (bm > -INFINITY) {
            // exp_nonpos: bm is the block's maximum over every l0[], l1[], so l - bm <= 0
            if (l0[r] > -INFINITY) { const double e = exp_nonpos(l0[r] - bm); s_ += e; q_ += e * e; }
            if (l1[r] > -INFINITY) { const double e = exp_nonpos(l1[r] - bm); s_ += e; q_ += e * e; }
        }
        s_ = wave_sum(s_); q_ = wave_sum(q_);
        if (lane == 0) { S.shs[wave + (NT / 64) * r] = s_; S.shq[wave + (NT / 64) * r] = q_; }
    }
    __syncthreads();
    double sum = 0.0, sq = 0.0;
#pragma unroll
    for (int i = 0; i < NTS / 64; i++) { sum += S.shs[i]; sq += S.shq[i]; }
    if (t == 0) { S.pm1 = bm; S.ps1 = sum; S.pq1 = sq; }
}

// k_local<W, from log-weights>, the resolve launches and k_apply for a filter of one block, ancestors only (as k_apply emits them for
// this family and the reaction networks): normalise + loglik / ESS / decision + the exact sum(weights) of the block (:204-218,
// src/resampling.cpp:20-24), then the 1-based ancestors into ANC [N].  Ends on a barrier.  k_pf_batch (kernels.hip.h) keeps its own
// two copies of these steps, with particles, the auxiliary pair and the multinomial leg: as a caller of one function its auxiliary
// instantiation for AR(1)+sin took 96 B of scratch a lane for its 32 (profiles r22_a, r22_c).
__device__ __forceinline__ void batch_weigh_resample(MvBatchSmem& S, const BatchArgs& g, const PhiloxKey& key, const int fi, const int obs_i,
                                                     const bool lit, int* ANC)
{
    const long long N = g.N;
    FromLw fl;
    fl.lw = S.LW; fl.xw = nullptr; fl.w_out = S.LW; fl.pm = &S.pm1; fl.ps = &S.ps1; fl.pq = &S.pq1; fl.nb = 1; fl.gmax = nullptr; fl.fold = g.fold; fl.lead = 0; fl.pub = 0; fl.ain_out = &S.ainw1;
    fl.plan = PLAN_PF; fl.N = N; fl.obs_i = obs_i; fl.resample_algorithm = g.resample_algorithm; fl.threshold = g.threshold;
    fl.ess_out = g.ess + (long long)fi * (g.T + 1); fl.llh_out = g.llh + (long long)fi * g.T; fl.resampled_out = nullptr;
    if (lit) local_block<MODE_W, true, NT, true>(S.sm, S.tin, S.es, 0, 1, S.LW, N, nullptr, g.lim, &S.br, nullptr, &S.st, fl, NoResolve(), nullptr, 1);
    else local_block<MODE_W, true, NT, false>(S.sm, S.tin, S.es, 0, 1, S.LW, N, nullptr, g.lim, &S.br, nullptr, &S.st, fl, NoResolve(), nullptr, 1);
    __syncthreads();
    if (threadIdx.x == 0 && !S.st.dead && !S.st.flags && S.st.do_resample) {      // what the resolve launches come to for one block
        const uint64_t fs = g.fold ? d2b(1.0) : S.br.prefix.o[0];
        const double tot = b2d(fs);
        S.st.total_bits = fs;
        if (tot == 0.0) S.st.flags |= FLAG_ZERO_SUM;
        if (!isfinite(tot)) S.st.flags |= FLAG_NONFINITE;
        S.ainp1 = S.ainw1 / tot; S.cin1 = 0;
    }
    __syncthreads();
    ApplyArgs a;
    a.w = S.LW; a.nw = N; a.ain_p = &S.ainp1; a.cin = &S.cin1; a.lim = g.lim; a.n = (int)N;
    a.u_base = nullptr; a.u_stride = 0; a.key = key; a.anc_out = ANC; a.anc_stride = 0; a.cum_out = nullptr;
    // (the in-order pass needs a destination buffer for its terms: the weights "gathered" into the scratch, otherwise unused)
    a.xsrc = lit ? S.LW : nullptr; a.xdst = lit ? S.SCR : nullptr; a.dim = 1; a.xstride = 0;
    a.auxsrc = nullptr; a.auxdst = nullptr; a.se_part = nullptr; a.nstage = 0; a.lead = 0; a.last = 0; a.step_model = -1; a.step_lw = nullptr;
    if (g.resample_fn == 1) {                                                         // systematic
        if (lit) apply_block<1, true>(S.sm, S.tin, S.Tl, S.Tbegin, 0, 1, a, &S.st); else apply_block<1, false>(S.sm, S.tin, S.Tl, S.Tbegin, 0, 1, a, &S.st);
    } else {                                                                          // stratified
        if (lit) apply_block<0, true>(S.sm, S.tin, S.Tl, S.Tbegin, 0, 1, a, &S.st); else apply_block<0, false>(S.sm, S.tin, S.Tl, S.Tbegin, 0, 1, a, &S.st);
    }
    __syncthreads();
}

// What a batched filter leaves behind for the genealogy smoother (k_trace_batch, smooth.hip.h): per filter exactly what a
// single-filter smoothing run leaves on the device --
//   hist [F][T+1][d][N]   row i: the particle set after observation i's gather or carry (row 0: after the init), k_record_history's ph row
//   anc [F][cap][N]       1-based, one row per resample call in call order (cap = max(T, 1): the bootstrap filter makes at most one a row)
//   call_obs [F][cap]     the observation of every row (k_note_calls)
//   W [F][N]              weights_history[T]: 1 / N when observation T resampled (and for T = 0), its normalised weights when it carried
// The number of rows is the filter's res_calls.  A filter that returns early records nothing from that observation on.
// REC is a template parameter of the two kernels: with BatchNoRec (the plain launch) every call below is empty.
struct BatchNoRec { static constexpr bool on = false; };
struct BatchRec {
    static constexpr bool on = true;
    double* hist; double* W; int* anc; int* call_obs; int cap;
};
// Observation i (0: the initial set) of filter fi is complete in X (LDS, [d][N]) and every thread is past the barrier behind its last
// store; S.st, S.LW and ANC are observation i's.  Each lane streams 16 contiguous bytes (a wave: 1 KiB) where the rows are 16-byte
// aligned (d N even; the pool's buffers are), 8 otherwise.  Nothing here writes LDS.
template <class REC>
__device__ __forceinline__ void batch_record(const REC& rec, const MvBatchSmem& S, const BatchArgs& g, const int fi, const int d, const int i,
                                             const double* __restrict__ X, const int* __restrict__ ANC)
{
    if constexpr (REC::on) {
        const int t = threadIdx.x, N = g.N;
        const long long n = (long long)d * N;
        double* __restrict__ dst = rec.hist + ((long long)fi * (g.T + 1) + i) * n;
        if ((n & 1) == 0) { for (long long k = 2 * t; k < n; k += 2 * NT) bulk_store16<0>(dst + k, X[k], X[k + 1]); }
        else for (long long k = t; k < n; k += NT) dst[k] = X[k];
        const bool resampled = i > 0 && S.st.do_resample && !S.st.flags;                  // the gather's guard (the caller left on dead)
        const int row = S.st.cur_call;
        if (resampled && row >= 0 && row < rec.cap) {
            int* __restrict__ arow = rec.anc + ((long long)fi * rec.cap + row) * N;
            for (int k = t; k < N; k += NT) arow[k] = ANC[k];
            if (t == 0) rec.call_obs[(long long)fi * rec.cap + row] = i;
        }
        if (i == g.T) {
            double* __restrict__ w = rec.W + (long long)fi * N;
            const bool flat = i == 0 || S.st.do_resample;                                 // k_record_history's rule; row 0 is rep(1 / N, N)
            const double invN = 1.0 / (double)N;
            for (int k = t; k < N; k += NT) w[k] = flat ? invN : S.LW[k];
        }
    }
}

// k_step_mv<TRANS, WEIGHT> for one block of N <= EB particles by NT threads (the partials land in S.pm1, S.ps1, S.pq1)
template <int DM, bool TRANS, bool WEIGHT, int OBS>
__device__ __forceinline__ void step_emul_mv(MvBatchSmem& S, double* __restrict__ X, long long N, const MvPar& mp, const MvTv& tv, const double* __restrict__ yrow,
                                             const double* __restrict__ lgyrow, PhiloxKey key, uint32_t call)
{
    constexpr int R = NTS / NT;
    const int t = threadIdx.x;
    const int d = mp.d, p = mp.p;
    const double* __restrict__ Pb = tv.b_of(mp);
    const double* __restrict__ Ph0 = tv.h0_of(mp);
    const double* __restrict__ PH = tv.H_of(mp);
#pragma unroll 1
    for (int r = 0; r < R; r++) {
        const long long j = 2 * (long long)(t + NT * r);
        if (j >= N) continue;
        const bool two = (j + 1 < N);
        double x0[DM], x1[DM];
#pragma unroll
        for (int c = 0; c < DM; c++) { x0[c] = 0.0; x1[c] = 0.0; if (c < d) { x0[c] = X[(long long)c * N + j]; if (two) x1[c] = X[(long long)c * N + j + 1]; } }
        if (TRANS) {
            double z0[DM], z1[DM];
#pragma unroll
            for (int c = 0; c < DM; c++) {
                z0[c] = 0.0; z1[c] = 0.0;
                if (c < d) normal_pair(key, DRAW_TRANS, call, (uint32_t)c, (uint32_t)(j >> 1), z0[c], z1[c]);
            }
            double n0[DM], n1[DM];
#pragma unroll
            for (int c = 0; c < DM; c++) {
                n0[c] = 0.0; n1[c] = 0.0;
                if (c < d) {
                    double a0 = Pb[c], a1 = a0;
#pragma unroll
                    for (int k = 0; k < DM; k++) if (k < d) { const double A = mp.P[mp.o_A() + c * d + k]; a0 = a0 + A * x0[k]; a1 = a1 + A * x1[k]; }
#pragma unroll
                    for (int k = 0; k < DM; k++) if (k <= c) { const double L = mp.P[mp.o_L() + c * d + k]; a0 = a0 + L * z0[k]; a1 = a1 + L * z1[k]; }
                    n0[c] = a0; n1[c] = a1;
                }
            }
#pragma unroll
            for (int c = 0; c < DM; c++) if (c < d) { x0[c] = n0[c]; x1[c] = n1[c]; X[(long long)c * N + j] = n0[c]; if (two) X[(long long)c * N + j + 1] = n1[c]; }
        }
        if (WEIGHT) {
            double l0, l1;
            if (p == 0) { l0 = mp.P[mp.o_c0()]; l1 = l0; }
            else {
                l0 = 0.0; l1 = 0.0;
#pragma unroll
                for (int k = 0; k < MVD; k++) {
                    if (k < p) {
                        const MvObsK ok = mv_obs_k<OBS>(mp, yrow, lgyrow, k);
                        if (mv_observed(ok)) {
                            double m0 = Ph0[k], m1 = m0;
#pragma unroll
                            for (int c = 0; c < DM; c++) if (c < d) { const double H = PH[k * d + c]; m0 = m0 + H * x0[c]; m1 = m1 + H * x1[c]; }
                            l0 = l0 + mv_obs_log<OBS>(ok, m0);
                            l1 = l1 + mv_obs_log<OBS>(ok, m1);
                        }
                    }
                }
            }
            S.LW[j] = l0; if (two) S.LW[j + 1] = l1;
        }
    }
    if (WEIGHT) batch_lse_partials(S, N);
}

// g.theta: [F][g.theta_stride] packed blocks WITH log(sd) (taken on the host, as pf_run_mv does); g.y: [T][p];
// g.state_est: [F][T+1][d].  DM >= d: the register arrays' size.  gt: the time-varying arrays (null pointers: the blocks' pieces),
// shared or one set per parameter draw (MvTvBatch).
// OBS: the observation family; g.lgy: [T][p] lgamma(y + 1) for the Poisson family (nullptr otherwise), as bssm_pf_run uploads it.
// REC: BatchNoRec, or BatchRec: the launch also leaves its histories for the smoother (batch_record).
template <int DM, int OBS = MV_OBS_GAUSS, class REC = BatchNoRec>
__global__ __launch_bounds__(NT) void k_pf_batch_mv(BatchArgs g, int d, int p, MvTvBatch gt, REC rec)
{
    __shared__ MvBatchSmem S;
    extern __shared__ __attribute__((aligned(16))) double XD[];        // [d][N] state, then int[N] ancestors (1-based)
    const int fi = blockIdx.x, t = threadIdx.x;
    const long long N = g.N;
    const int T = g.T;
    double* X = XD;
    int* ANC = reinterpret_cast<int*>(XD + (long long)d * N);
    MvPar mp; mp.P = g.theta + (long long)fi * g.theta_stride; mp.d = d; mp.p = p;
    const PhiloxKey key = g.keys[fi];
    const bool lit = g.N <= g.lit_max;
    const double invN = 1.0 / (double)N;
    double* se_out = g.state_est + (long long)fi * (T + 1) * d;
    {   // this filter's set of the time-varying arrays (uniform: blockIdx.x only; strides of 0 leave the shared arrays)
        const long long si = gt.set_of ? gt.set_of[blockIdx.x] : 0;
        if (gt.b) gt.b += si * gt.sb;
        if (gt.h0) gt.h0 += si * gt.sh0;
        if (gt.H) gt.H += si * gt.sH;
    }
    batch_reset_state(S.st);
    {   // k_init_mv: x0 = m0 + L0 z  and the t = 0 state estimate
        double acc[DM];
#pragma unroll
        for (int c = 0; c < DM; c++) acc[c] = 0.0;
#pragma unroll 1
        for (int r = 0; r < EL; r++) {
            const long long j = t + NT * r;
            if (j < N) {
                double z[DM];
#pragma unroll
                for (int c = 0; c < DM; c++) {
                    z[c] = 0.0;
                    if (c < d) { double z0, z1; normal_pair(key, DRAW_INIT, 0, (uint32_t)c, (uint32_t)(j >> 1), z0, z1); z[c] = (j & 1) ? z1 : z0; }
                }
#pragma unroll
                for (int c = 0; c < DM; c++) {
                    if (c < d) {
                        double v = mp.P[mp.o_m0() + c];
#pragma unroll
                        for (int k = 0; k < DM; k++) if (k <= c) v = v + mp.P[mp.o_L0() + c * d + k] * z[k];
                        X[(long long)c * N + j] = v;
                        acc[c] += v * invN;
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
        const double* yrow = p > 0 ? g.y + (long long)(i - 1) * p : nullptr;
        const double* lgyrow = OBS == MV_OBS_POIS ? g.lgy + (long long)(i - 1) * p : nullptr;
        MvTv tv;                                                                          // observation row i - 1; b: the row of the time reached
        tv.b = nullptr;
        tv.h0 = gt.h0 ? gt.h0 + (long long)(i - 1) * p : nullptr;
        tv.H = gt.H ? gt.H + (long long)(i - 1) * p * d : nullptr;
        for (int step = 1; step <= gap; step++) {                                         // :125-136, the last one with weight_fn (:177-183)
            const int tau = min(ot - gap + step, gt.n_times);                             // (the host checked n_times >= the last time)
            if (gt.b) tv.b = gt.b + (long long)(tau - 1) * d;
            if (step == gap) step_emul_mv<DM, true, true, OBS>(S, X, N, mp, tv, yrow, lgyrow, key, (uint32_t)ktrans);
            else step_emul_mv<DM, true, false, OBS>(S, X, N, mp, tv, yrow, lgyrow, key, (uint32_t)ktrans);
            ktrans++;
            __syncthreads();
        }
        if (gap <= 0) { step_emul_mv<DM, false, true, OBS>(S, X, N, mp, tv, yrow, lgyrow, key, 0u); __syncthreads(); }
        batch_weigh_resample(S, g, key, fi, i, lit, ANC);                                 // :204-224: ancestors only
        double acc[DM];
#pragma unroll
        for (int c = 0; c < DM; c++) acc[c] = 0.0;
        const bool gather = !S.st.dead && S.st.do_resample && !S.st.flags;               // k_gather_mv's guard
        const bool carry = g.resample_algorithm != 1 && !S.st.dead && !S.st.do_resample; // k_carry_mv's (launched for SIS / SISAR)
        if (gather) {                                                                     // particles[indices, ] (R/resampling.R:40,60)
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

__global__ void k_dump_normals_mv(PhiloxKey key, uint32_t purpose, uint32_t call, long long N, int d, double* __restrict__ out /* [d][N] */)
{
    const long long pair = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long j = 2 * pair;
    if (j >= N) return;
    for (int c = 0; c < d; c++) {
        double z0, z1;
        normal_pair(key, purpose, call, (uint32_t)c, (uint32_t)pair, z0, z1);
        out[(long long)c * N + j] = z0;
        if (j + 1 < N) out[(long long)c * N + j + 1] = z1;
    }
}

__global__ void k_dump_move_draws_mv(PhiloxKey key, uint32_t call, long long N, int d, double* __restrict__ zout /* [d][N] */, double* __restrict__ uout /* [N] */)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    for (int c = 0; c < d; c++) {
        double z, u;
        move_draw_mv(key, call, (uint32_t)i, (uint32_t)c, z, u);
        zout[(long long)c * N + i] = z;
        if (c == 0) uout[i] = u;
    }
}

}  // namespace bssm
