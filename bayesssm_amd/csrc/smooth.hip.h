// smooth.hip.h -- the genealogy (ancestor-tracing) smoother on the histories a single-filter run leaves on the device.
//
//   b_T(j) = j,   b_{i-1}(j) = a_i(b_i(j)),   a_i = the ancestor rows observation i produced, composed in launch order
//   smoothed[i][c]  = sum_j W[j] P[i][c][b_i(j)]          W = weights_history[T], P[i] = particles_history[i] ([d][N])
//   n_lineages[i]   = #{ b_i(j) : j }
//   trajectories[k] = ( P[i][.][b_i(j_k)] )_i             j_k by inverse CDF on the multinomial leg's exact cum_sum of W
//
//   k_note_calls     the observation index of every ancestor row, written as the rows are produced (call_obs)
//   k_trace          one thread per final particle, one launch for i = T .. 0: per-block partials of smoothed, lineage counts
//   k_trace_paths    one thread per trajectory
//   k_traj_uniforms  the uniforms of the terminal draw (purpose DRAW_SMOOTH: no other draw of the run moves)
// The block partials [T+1][B][d] are added by k_reduce_state_est (kernels.hip.h), as the filter's own state estimates are.
//
//   k_trace_batch    the same outputs for every filter of a batched launch that recorded its histories (batch_record, mv.hip.h):
//                    one workgroup per filter, in step, one launch
#pragma once
#include "kernels.hip.h"
#include "mv.hip.h"

namespace bssm {

constexpr uint32_t DRAW_SMOOTH = 8;      // (rng.h: 1 .. 7 are the filter's and the sampler's)

// After the launches of observation obs_i: every resample call made since the last note belongs to it.  noted: calls already labelled.
// (cap: the rows the ancestor buffer holds; res_calls never exceeds it)
__global__ void k_note_calls(const DevState* __restrict__ st, int* __restrict__ call_obs, int* __restrict__ noted, int obs_i, int cap)
{
    const int upto = st->res_calls < cap ? st->res_calls : cap;
    for (int k = *noted; k < upto; k++) call_obs[k] = obs_i;
    if (*noted < upto) *noted = upto;
}

// Uniform (0,1) number k of the terminal draw: resample_uniform's construction under the smoother's own purpose tag
__global__ void k_traj_uniforms(PhiloxKey key, int K, double* __restrict__ u)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= K) return;
    u32x4 c; c.x = (uint32_t)k >> 1; c.y = 0; c.z = DRAW_SMOOTH; c.w = key.stream;
    const u32x4 r = philox4x32_10(c, key.k0, key.k1);
    u[k] = (k & 1) ? u01_from_bits(r.z, r.w) : u01_from_bits(r.x, r.y);
}

// One step back along the genealogy: b (0-based, a particle of observation i) becomes a_i(b).  kc: the last ancestor row not yet
// consumed; the rows of observation i are applied last-launched first (a_i(j) = first[second[j]]).  (An entry outside 1 .. N is
// never written by the resamplers; it would leave b where it is and not become an address.)
__device__ __forceinline__ int trace_back(int b, int i, int& kc, const int* __restrict__ anc, long long N, const int* __restrict__ call_obs)
{
    while (kc >= 0 && call_obs[kc] == i) {
        const int a = anc[(long long)kc * N + b] - 1;
        b = (a >= 0 && a < N) ? a : b;
        kc--;
    }
    return b;
}

// ph [T+1][d][N], W [N], anc [n_calls][N] 1-based, call_obs [n_calls].  part [T+1][gridDim.x][d]; nlin [T+1] zeroed; seen: one bit
// per (i, particle), [T+1][words] zeroed, words = ceil(N / 32).
// Lineage count: the first thread to reach particle b of observation i sets its bit and counts.  A thread that finds the bit set has
// met a lineage it shares from here backwards with the thread that set it, and retires from counting: what reaches a node of
// observation i - 1 still counting is one thread per child node, so the atomics of a step number what the step after it counted, not N.
// A bitset per observation and not one stamp per particle: the blocks of a launch are not in step, and a stamp written for
// observation i - 1 would make a later thread of observation i count the particle a second time.
__global__ __launch_bounds__(NT) void k_trace(const double* __restrict__ ph, const double* __restrict__ W, const int* __restrict__ anc,
                                              const int* __restrict__ call_obs, int n_calls, long long N, int d, int T,
                                              double* __restrict__ part, int* __restrict__ nlin, unsigned int* __restrict__ seen, long long words)
{
    __shared__ double sh4[NWV];
    const long long j = (long long)blockIdx.x * NT + threadIdx.x;
    const bool live = j < N;
    const double wj = live ? W[j] : 0.0;
    int b = live ? (int)j : 0;
    bool counting = live;
    int kc = n_calls - 1;
    for (int i = T; i >= 0; i--) {
        const double* P = ph + (long long)i * d * N;
        for (int c = 0; c < d; c++) {
            const double s = block_sum(live ? wj * P[(long long)c * N + b] : 0.0, sh4);
            if (threadIdx.x == 0) part[((long long)i * gridDim.x + blockIdx.x) * d + c] = s;
        }
        int first = 0;
        if (counting) {
            const unsigned int bit = 1u << (b & 31);
            const unsigned int old = atomicOr(&seen[(long long)i * words + (b >> 5)], bit);
            first = (old & bit) ? 0 : 1;
            counting = first != 0;
        }
        const int cnt = __syncthreads_count(first);
        if (threadIdx.x == 0 && cnt) atomicAdd(&nlin[i], cnt);
        if (live && i > 0) b = trace_back(b, i, kc, anc, N, call_obs);
    }
}

// idx [K]: the terminal particles, 1-based (the multinomial leg's ancestors).  out [K][T+1][d]
__global__ void k_trace_paths(const double* __restrict__ ph, const int* __restrict__ anc, const int* __restrict__ call_obs, int n_calls,
                              long long N, int d, int T, const int* __restrict__ idx, int K, double* __restrict__ out)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= K) return;
    int b = idx[k] - 1;
    b = b < 0 ? 0 : (b >= N ? (int)(N - 1) : b);
    int kc = n_calls - 1;
    for (int i = T; i >= 0; i--) {
        const double* P = ph + (long long)i * d * N;
        for (int c = 0; c < d; c++) out[((long long)k * (T + 1) + i) * d + c] = P[(long long)c * N + b];
        if (i > 0) b = trace_back(b, i, kc, anc, N, call_obs);
    }
}

// ---------------------------------------------------------------------------
// k_trace_batch: the trace of F small filters (N <= EB) in one launch, workgroup f = filter f, on what batch_record left:
// hist [F][T+1][d][N], W [F][N], anc [F][cap][N], call_obs [F][cap]; the rows of filter f number res_calls[f].
// Thread t holds the lineages of the final particles t + NT r, r < EL, in registers and walks i = T .. 0 with trace_back's rule.
//   smoothed   round r of the workgroup is block r of k_trace (the same threads, the same block_sum: wave_sum, then tree_sum of the
//              per-wave values); the ceil(N / NT) partials are then added as k_reduce_state_est adds them -- lane b of the first
//              wave holds 0.0 + partial b, wave_sum, tree_sum over the waves (the others hold 0.0).  Bit for bit k_trace's value.
//   n_lineages the workgroup is in step, so one bitset in LDS serves every i: atomicOr, barrier, popcount, clear.
//   paths      the terminal particles j_k by the rule of 1e on cum = cumsum(W / sum(W)), both sums in order by one lane (what the
//              resampler's exact sums are defined to equal), the uniforms k_traj_uniforms' under the filter's own key; the search is
//              multinomial_block's.  At every i the lineages are published in LDS and thread k copies P[i][.][b_i(j_k)]: no thread
//              walks a path alone.
// A filter that returned early or carries a flag is not traced: traced[f] = 0, NaN in its float outputs, 0 in its int outputs.
// Two barriers per i.  Static LDS: 42.5 KiB.
// ---------------------------------------------------------------------------
constexpr int TRACE_MAX_K = 4096;
struct TraceBatchArgs {
    const double* hist; const double* W; const int* anc; const int* call_obs; int cap;
    const int* res_calls; const int* dead; const uint32_t* flags; const PhiloxKey* keys;      // [F], the filters' own outputs and keys
    int N, T, d, K;
    double* smoothed; int* nlin; double* traj; double* u; int* idx; int* traced;               // [F][T+1][d], [F][T+1], [F][K][T+1][d], [F][K], [F][K], [F]
};

__device__ __forceinline__ int wave_sum_i32(int x)
{
#define STEP(C, R) x = dpp_i32<C, R>(0, x) + x;
    BSSM_WAVE_SCAN_STEPS(STEP)
#undef STEP
    return __builtin_amdgcn_readlane(x, 63);
}

__global__ __launch_bounds__(NT) void k_trace_batch(TraceBatchArgs a)
{
    static_assert(EB / 32 == 64 && EL <= 64, "the lineage bitset is one word per lane of a wave; the partials of a step fit one wave");
    __shared__ double shp[MVD][EL][NWV];          // per-wave sums of (component, round)
    __shared__ unsigned int bits[EB / 32];
    __shared__ int BI[EB];                        // b_i(j) of the step, for the paths
    __shared__ int IDX[TRACE_MAX_K];              // terminal particles, 0-based
    __shared__ double CUM[EB];
    __shared__ double tot_s;
    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int N = a.N, T = a.T, d = a.d, K = a.K;
    const long long T1 = (long long)T + 1;
    double* __restrict__ sm = a.smoothed + (long long)f * T1 * d;
    int* __restrict__ nl = a.nlin + (long long)f * T1;
    double* __restrict__ tr = K > 0 ? a.traj + (long long)f * K * T1 * d : nullptr;
    if (a.dead[f] || a.flags[f]) {                // (uniform) not traced
        for (long long k = t; k < T1 * d; k += NT) sm[k] = NAN;
        for (long long k = t; k < T1; k += NT) nl[k] = 0;
        for (long long k = t; k < (long long)K * T1 * d; k += NT) tr[k] = NAN;
        for (int k = t; k < K; k += NT) { a.u[(long long)f * K + k] = NAN; a.idx[(long long)f * K + k] = 0; }
        if (t == 0) a.traced[f] = 0;
        return;
    }
    const double* __restrict__ H = a.hist + (long long)f * T1 * d * N;
    const double* __restrict__ W = a.W + (long long)f * N;
    const int* __restrict__ anc = a.anc + (long long)f * a.cap * N;
    const int* __restrict__ co = a.call_obs + (long long)f * a.cap;
    const int n_calls = a.res_calls[f] < a.cap ? a.res_calls[f] : a.cap;
    const int Bt = (N + NT - 1) / NT;
    double w[EL]; int b[EL];
#pragma unroll
    for (int r = 0; r < EL; r++) { const int j = t + NT * r; w[r] = j < N ? W[j] : 0.0; b[r] = j < N ? j : 0; }
    if (t < EB / 32) bits[t] = 0;
    if (K > 0) {
        const PhiloxKey key = a.keys[f];
        for (int j = t; j < N; j += NT) CUM[j] = W[j];
        __syncthreads();
        if (t == 0) { double tot = 0.0; for (int j = 0; j < N; j++) tot += CUM[j]; tot_s = tot; }                       // sum(W), in order
        __syncthreads();
        const double tot = tot_s;
        for (int j = t; j < N; j += NT) CUM[j] = CUM[j] / tot;                                                            // prob
        __syncthreads();
        if (t == 0) { double run = 0.0; for (int j = 0; j < N; j++) { run += CUM[j]; CUM[j] = run; } }                   // cumsum(prob), in order
        __syncthreads();
        for (int k = t; k < K; k += NT) {
            u32x4 c; c.x = (uint32_t)k >> 1; c.y = 0; c.z = DRAW_SMOOTH; c.w = key.stream;                               // k_traj_uniforms
            const u32x4 q = philox4x32_10(c, key.k0, key.k1);
            const double u = (k & 1) ? u01_from_bits(q.z, q.w) : u01_from_bits(q.x, q.y);
            int lo = 0, hi = N - 1;                                                                                       // multinomial_block's search
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (CUM[mid] < u) lo = mid + 1; else hi = mid; }
            IDX[k] = lo;
            a.u[(long long)f * K + k] = u; a.idx[(long long)f * K + k] = lo + 1;
        }
    }
    __syncthreads();
    int kc = n_calls - 1;
    for (int i = T; i >= 0; i--) {
        const double* __restrict__ P = H + (long long)i * d * N;
#pragma unroll
        for (int r = 0; r < EL; r++) {
            const int j = t + NT * r;
            if (j < N) { atomicOr(&bits[b[r] >> 5], 1u << (b[r] & 31)); if (K > 0) BI[j] = b[r]; }
        }
#pragma unroll 1
        for (int c = 0; c < d; c++) {
#pragma unroll
            for (int r = 0; r < EL; r++) {
                if (r < Bt) {                                                                                             // (uniform) block r of k_trace
                    const double v = wave_sum((t + NT * r < N) ? w[r] * P[(long long)c * N + b[r]] : 0.0);
                    if (lane == 0) shp[c][r][wave] = v;
                }
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll 1
            for (int c = 0; c < d; c++) {                                                                                 // k_reduce_state_est over Bt blocks
                double s = 0.0;
                if (lane < Bt) s += tree_sum<NWV>(shp[c][lane]);
                double q[NWV];
                q[0] = wave_sum(s);
#pragma unroll
                for (int k = 1; k < NWV; k++) q[k] = 0.0;
                const double v = tree_sum<NWV>(q);
                if (lane == 0) sm[(long long)i * d + c] = v;
            }
            const int cnt = wave_sum_i32((int)__popc(bits[lane]));
            bits[lane] = 0;
            if (lane == 0) nl[i] = cnt;
        }
        for (int k = t; k < K; k += NT) {
            const int bk = BI[IDX[k]];
            for (int c = 0; c < d; c++) tr[((long long)k * T1 + i) * d + c] = P[(long long)c * N + bk];
        }
        if (i > 0) {
            while (kc >= 0 && co[kc] == i) {                                                                              // trace_back, EL lineages
                const int* __restrict__ row = anc + (long long)kc * N;
#pragma unroll
                for (int r = 0; r < EL; r++) {
                    if (t + NT * r < N) { const int an = row[b[r]] - 1; b[r] = (an >= 0 && an < N) ? an : b[r]; }
                }
                kc--;
            }
        }
        __syncthreads();
    }
    if (t == 0) a.traced[f] = 1;
}

}  // namespace bssm
