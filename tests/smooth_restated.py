"""numpy restatement of the genealogy (ancestor-tracing) smoother, from what a filter run returns with
return_particles=True, return_ancestors=True:

    particles_history [T+1, N d]   row i = the particle set P[i] recorded for observation i, component-major ([d][N])
    weights_history   [T+1, N]     W = weights_history[T]
    ancestors         [n_calls, N] 1-based rows in launch order
    call_obs          [n_calls]    the observation (1 .. T) every row belongs to

    b_T(j) = j,   b_{i-1}(j) = a_i(b_i(j)),   a_i = the rows of observation i composed in launch order (no row: the identity;
                                              two rows: first[second[j]])
    smoothed[i, c]  = sum_j W[j] P[i][c][b_i(j)]                 (math.fsum)
    n_lineages[i]   = the number of distinct b_i(j)              (np.unique)
    trajectories[k] = (P[i][.][b_i(j_k)])_i                      (pure indexing)
    j_k             = the first j with cum[j] >= u_k, N where u_k lies beyond cum[N-1];  cum = np.cumsum(W / np.cumsum(W)[-1]) --
                      the multinomial resampler's cum_sum: prob = W / sum(W), both sums sequential in fp64

Also here: the Rauch-Tung-Striebel pass for the 1-d linear-Gaussian model (the exact smoothed means) and a numpy SISR filter
that keeps its histories and ancestors, for the CPU test of the restatement."""
import math

import numpy as np


def lineages(ancestors, call_obs, T, N):
    """b [T+1, N], 0-based: b[i, j] = the particle of P[i] final particle j descends from"""
    ancestors = np.asarray(ancestors).reshape(-1, N)
    call_obs = np.asarray(call_obs, dtype=np.int64).reshape(-1)
    assert ancestors.shape[0] == call_obs.size
    b = np.empty((T + 1, N), dtype=np.int64)
    b[T] = np.arange(N)
    for i in range(T, 0, -1):
        cur = b[i]
        for k in np.flatnonzero(call_obs == i)[::-1]:          # a_i(j) = first[second[j]]: the last row launched is applied first
            cur = ancestors[k][cur] - 1
        b[i - 1] = cur
    return b


def smooth(particles_history, weights_history, ancestors, call_obs, d=1):
    """dict(smoothed [T+1, d], abs_sum [T+1, d] = sum_j |W[j] P[i][c][b_i(j)]|, n_lineages [T+1], b [T+1, N])"""
    wh = np.asarray(weights_history, dtype=np.float64)
    T, N = wh.shape[0] - 1, wh.shape[1]
    P = np.asarray(particles_history, dtype=np.float64).reshape(T + 1, d, N)
    b = lineages(ancestors, call_obs, T, N)
    W = wh[T]
    sm, ab = np.zeros((T + 1, d)), np.zeros((T + 1, d))
    for i in range(T + 1):
        for c in range(d):
            terms = W * P[i, c, b[i]]
            sm[i, c] = math.fsum(terms)
            ab[i, c] = math.fsum(np.abs(terms))
    nl = np.array([np.unique(b[i]).size for i in range(T + 1)], dtype=np.int64)
    return {"smoothed": sm, "abs_sum": ab, "n_lineages": nl, "b": b}


def terminal_indices(W, u):
    """j_k, 1-based, for the uniforms u"""
    W = np.asarray(W, dtype=np.float64)
    cum = np.cumsum(W / np.cumsum(W)[-1])
    idx = np.searchsorted(cum, np.asarray(u, dtype=np.float64), side="left")      # the first j with cum[j] >= u
    return np.minimum(idx, W.size - 1) + 1


def paths(particles_history, b, index, d=1):
    """trajectories [K, T+1, d] of the terminal particles index (1-based)"""
    T1, N = b.shape
    P = np.asarray(particles_history, dtype=np.float64).reshape(T1, d, N)
    j = np.asarray(index, dtype=np.int64) - 1
    return np.stack([P[i][:, b[i, j]].T for i in range(T1)], axis=1)


def rts_means_1d(y, A, b, L, m0, L0, h0=0.0, H=1.0, sd=1.0):
    """E[x_t | y_1:T], t = 0 .. T, of  x_0 ~ N(m0, L0^2),  x_t = A x_{t-1} + b + L z,  y_t ~ N(h0 + H x_t, sd^2):
    the Kalman filter forward (as exact_hmm.kalman_1d), then the Rauch-Tung-Striebel pass backward"""
    y = np.asarray(y, dtype=np.float64)
    T = y.size
    mf, Pf, mp, Pp = np.zeros(T + 1), np.zeros(T + 1), np.zeros(T + 1), np.zeros(T + 1)
    mf[0], Pf[0] = m0, L0 * L0
    for t in range(1, T + 1):
        mp[t], Pp[t] = A * mf[t - 1] + b, A * A * Pf[t - 1] + L * L
        S = H * H * Pp[t] + sd * sd
        g = Pp[t] * H / S
        mf[t], Pf[t] = mp[t] + g * (y[t - 1] - h0 - H * mp[t]), (1 - g * H) * Pp[t]
    ms = mf.copy()
    for t in range(T - 1, -1, -1):
        ms[t] = mf[t] + Pf[t] * A / Pp[t + 1] * (ms[t + 1] - mp[t + 1])
    return ms


def sisr_histories_1d(y, N, rng, A, b, L, m0, L0, h0=0.0, H=1.0, sd=1.0):
    """One bootstrap filter on the model itself, stratified resampling at every observation (exact_hmm.sisr_filter_1d's steps),
    that keeps what the smoother reads: particles_history [T+1, N], weights_history [T+1, N], ancestors [T, N] 1-based, call_obs [T]"""
    y = np.asarray(y, dtype=np.float64)
    x = m0 + L0 * rng.standard_normal(N)
    ph, wh, anc = [x.copy()], [np.full(N, 1.0 / N)], []
    for yt in y:
        x = A * x + b + L * rng.standard_normal(N)
        lw = -0.5 * ((yt - h0 - H * x) / sd) ** 2
        w = np.exp(lw - lw.max())
        c = np.cumsum(w)
        c /= c[-1]
        u = (np.arange(N) + rng.random(N)) / N
        pick = np.minimum(np.searchsorted(c, u, side="right"), N - 1)
        x = x[pick]
        anc.append(pick + 1)
        ph.append(x.copy())
        wh.append(np.full(N, 1.0 / N))
    return {"particles_history": np.array(ph), "weights_history": np.array(wh), "ancestors": np.array(anc, dtype=np.int32),
            "call_obs": np.arange(1, y.size + 1, dtype=np.int32)}


# The exact-smoother check (CPU: the numpy filter above; GPU: the device filter on the built-in linear-Gaussian model, which is this
# model with A = phi, b = 0, L = sigma_x, m0 = 0, L0 = 1, sd = sigma_y): T, N, the 32 replicates and the data are fixed here.
EXACT = dict(phi=0.8, sigma_x=0.7, sigma_y=0.6)
EXACT_T, EXACT_N = 6, 4096
EXACT_SEEDS = [(2100 + k, k) for k in range(32)]            # (seed, stream) of the device runs; the numpy runs use default_rng(seed)
EXACT_Y = np.array([0.35, -0.42, 0.91, 1.37, 0.18, -0.66])


def exact_means():
    q = EXACT
    return rts_means_1d(EXACT_Y, q["phi"], 0.0, q["sigma_x"], 0.0, 1.0, sd=q["sigma_y"])


def within_5_se(smoothed, exact):
    """smoothed [R, T+1]: for every t the mean over the R replicates lies within 5 standard errors (from the replicates themselves)
    of the exact smoothed mean.  Returns (ok [T+1], z [T+1])"""
    smoothed = np.asarray(smoothed, dtype=np.float64)
    se = smoothed.std(axis=0, ddof=1) / math.sqrt(smoothed.shape[0])
    z = (smoothed.mean(axis=0) - exact) / se
    return np.abs(z) <= 5.0, z
