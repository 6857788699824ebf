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
#pragma once
#include "kernels.hip.h"

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

}  // namespace bssm
