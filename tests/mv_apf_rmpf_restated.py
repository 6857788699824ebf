"""CPU restatement of .particle_filter_core (R/particle_filter_core.R:19-267) for the multivariate linear-Gaussian family with all
three algorithms (BPF, APF, RMPF) -- the reference the device's pf_run_mv is compared with.  It follows the oracle's orc_pf_run
(oracle/bssm_oracle.c) line by line, with the family's model functions in the kernels' order of operations (mv.hip.h):

  transition      x'_c = ((b_c + A_c0 x_0) + A_c1 x_1 + ...) + L_c0 z_0 + ... + L_cc z_c
  log-likelihood  p == 0: c0;  else  l = 0.0;  l = l + dnorm(y_k, (h0_k + H_k0 x_0) + H_k1 x_1 + ..., sd_k, log = TRUE)
  aux (APF)       the log-likelihood at the transition mean  m_c = (b_c + A_c0 x_0) + A_c1 x_1 + ...
  move (RMPF)     prop_c = x_c + (0.0 + sd z_c); accept when log(u) < ll(prop) - ll(x)  (p == 0: always)

Resampling runs through the oracle's restatement of src/resampling.cpp (exact ancestors); sum() is R's long-double sequential sum.
Vectorised over particles only: every particle sees the scalar operations in the scalar order."""
import numpy as np

LN_SQRT_2PI = 0.918938533204672741780329736406


def unpack(theta):
    theta = np.asarray(theta, dtype=np.float64)
    d, p = int(theta[0]), int(theta[1])
    o = 2
    m0 = theta[o:o + d]; o += d
    L0 = theta[o:o + d * d].reshape(d, d); o += d * d
    A = theta[o:o + d * d].reshape(d, d); o += d * d
    b = theta[o:o + d]; o += d
    L = theta[o:o + d * d].reshape(d, d); o += d * d
    c0 = float(theta[o]); o += 1
    H = theta[o:o + p * d].reshape(p, d); o += p * d
    h0 = theta[o:o + p]; o += p
    sd = theta[o:o + p]
    return dict(d=d, p=p, m0=m0, L0=L0, A=A, b=b, L=L, c0=c0, H=H, h0=h0, sd=sd)


def rsum(x):
    """R's sum(): a long-double accumulator, left to right, rounded once"""
    x = np.asarray(x, dtype=np.float64)
    return float(np.cumsum(x.astype(np.longdouble))[-1]) if x.size else 0.0


def dnorm_log(y, mu, sd, log_sd):
    z = (y - mu) / sd
    out = -(LN_SQRT_2PI + 0.5 * np.abs(z) * np.abs(z) + log_sd)
    return np.where(np.isfinite(z), out, -np.inf)


def transition(q, x, z):
    d = q["d"]
    xn = np.empty_like(x)
    for c in range(d):
        v = np.full(x.shape[1], q["b"][c])
        for j in range(d):
            v = v + q["A"][c, j] * x[j]
        for j in range(c + 1):
            v = v + q["L"][c, j] * z[j]
        xn[c] = v
    return xn


def mean_of_transition(q, x):
    d = q["d"]
    m = np.empty_like(x)
    for c in range(d):
        v = np.full(x.shape[1], q["b"][c])
        for j in range(d):
            v = v + q["A"][c, j] * x[j]
        m[c] = v
    return m


def loglik(q, y, x):
    if q["p"] == 0:
        return np.full(x.shape[1], q["c0"])
    l = np.zeros(x.shape[1])
    for k in range(q["p"]):
        m = np.full(x.shape[1], q["h0"][k])
        for c in range(q["d"]):
            m = m + q["H"][k, c] * x[c]
        l = l + dnorm_log(y[k], m, q["sd"][k], np.log(q["sd"][k]))
    return l


def aux_loglik(q, y, x):
    return loglik(q, y, mean_of_transition(q, x)) if q["p"] > 0 else np.full(x.shape[1], q["c0"])


def pf_run_mv(oracle, theta, y, N, z_init, z_trans, u_res, algorithm="BPF", resample_algorithm="SISAR", resample_fn="stratified",
              threshold=None, obs_times=None, move_sd=0.0, z_move=None, u_move=None, return_particles=False):
    """theta: the packed block (models.LinearGaussianMV.pack); y [T][p]; z_init [d][N]; z_trans [calls][d][N]; u_res as for
    oracle.pf_run; z_move [T][d][N], u_move [T][N].  Returns the oracle's result dict (state_est [T+1][d], [T+1] for d = 1)."""
    q = unpack(theta)
    d = q["d"]
    y = np.asarray(y, dtype=np.float64).reshape(-1, q["p"]) if q["p"] > 0 else np.zeros((len(y), 0))
    T, dN = y.shape[0], float(N)
    if threshold is None:
        threshold = np.inf if resample_algorithm == "SIS" else dN if resample_algorithm == "SISR" else dN / 2
    z_init = np.asarray(z_init, dtype=np.float64).reshape(d, N)
    z_trans = np.asarray(z_trans, dtype=np.float64).reshape(-1, d, N)
    u_res = np.asarray(u_res, dtype=np.float64)
    u_res = u_res.reshape(-1) if resample_fn == "systematic" else u_res.reshape(-1, N)
    if algorithm == "RMPF":
        z_move = np.asarray(z_move, dtype=np.float64).reshape(-1, d, N)
        u_move = np.asarray(u_move, dtype=np.float64).reshape(-1, N)

    def resample(w, k):
        if resample_fn == "systematic":
            return oracle.resample_systematic(N, w, float(u_res[k]))
        return oracle.resample_stratified(N, w, u_res[k])

    x = np.empty((d, N))
    for c in range(d):                                             # init_fn :76
        v = np.full(N, q["m0"][c])
        for j in range(c + 1):
            v = v + q["L0"][c, j] * z_init[j]
        x[c] = v
    state_est = np.full((T + 1, d), np.nan) if d > 1 else np.zeros((T + 1, 1))
    ess, llh, resampled = np.zeros(T + 1), np.zeros(T), np.zeros(T, dtype=np.int32)
    ancestors, ph, wh = [], [], []
    w = np.full(N, 1.0 / dN)
    ess[0] = 1.0 / rsum(w * w)                                     # :106-107
    for c in range(d):
        state_est[0, c] = rsum(x[c] * w)                           # :109-112
    if return_particles:
        ph.append(x.reshape(-1).copy()); wh.append(w.copy())
    loglike, prev_t, ktrans, kres, early = 0.0, 0, 0, 0, 0
    for i in range(1, T + 1):                                      # :123
        ot = int(obs_times[i - 1]) if obs_times is not None else i
        gap = ot - prev_t                                          # :124
        for _ in range(gap):                                       # :125-136
            x = transition(q, x, z_trans[ktrans]); ktrans += 1
        prev_t = ot
        yi = y[i - 1]
        if algorithm == "APF":                                     # :140-175
            aux = aux_loglik(q, yi, x)
            tmp = np.exp(aux - np.max(aux))                        # :153
            tmp = tmp / rsum(tmp)                                  # :154
            idx = resample(tmp, kres)                              # :155
            ancestors.append(idx.copy()); kres += 1
            x = x[:, idx - 1]                                      # :157
            x = transition(q, x, z_trans[ktrans]); ktrans += 1     # :159
            lw = loglik(q, yi, x) - aux[idx - 1]                   # :169-175
        else:
            lw = loglik(q, yi, x)                                  # :177-183
        if np.all(lw < -1e8):                                      # :189-202
            loglike = -np.inf; llh[i - 1] = -np.inf; early = i
            break
        mx = np.max(lw)                                            # :204
        tmp = np.exp(lw - mx)                                      # :205
        s = rsum(tmp)                                              # :206
        w = tmp / s                                                # :207
        loglike = loglike + (mx + np.log(s) - np.log(dN))          # :208
        llh[i - 1] = loglike                                       # :209
        ess[i] = 1.0 / rsum(w * w)                                 # :211
        should = 0 if resample_algorithm == "SIS" else 1 if resample_algorithm == "SISR" else int(ess[i] < threshold)
        if algorithm == "RMPF":
            should = 1                                             # :220
        resampled[i - 1] = should
        if should:                                                 # :220-224
            idx = resample(w, kres)
            ancestors.append(idx.copy()); kres += 1
            x = x[:, idx - 1]
            w = np.full(N, 1.0 / dN)
            ess[i] = dN                                            # :223
        if algorithm == "RMPF":                                    # :226-234
            prop = np.empty_like(x)
            for c in range(d):
                prop[c] = x[c] + (0.0 + move_sd * z_move[i - 1, c])
            if q["p"] == 0:
                acc = np.ones(N, dtype=bool)
            else:
                acc = np.log(u_move[i - 1]) < (loglik(q, yi, prop) - loglik(q, yi, x))
            x = np.where(acc[None, :], prop, x)
        for c in range(d):
            state_est[i, c] = rsum(x[c] * w)                       # :238-240
        if return_particles:
            ph.append(x.reshape(-1).copy()); wh.append(w.copy())
    if early:
        ess[early:] = 0.0                                          # (the device's zeroed rows after an early return)
    res = {"state_est": state_est if d > 1 else state_est[:, 0], "ess": ess, "loglike": float(loglike), "loglike_history": llh,
           "algorithm": algorithm, "n_trans_calls": ktrans, "n_res_calls": kres, "early_return_step": early, "resampled": resampled,
           "ancestors": np.array(ancestors, dtype=np.int32).reshape(-1, N)}
    if return_particles:
        res["particles_history"], res["weights_history"] = np.array(ph), np.array(wh)
    return res
