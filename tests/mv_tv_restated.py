"""CPU restatement of .particle_filter_core (R/particle_filter_core.R:19-267) for the multivariate linear-Gaussian family with
TIME-VARYING b, h0, H (BPF, APF, RMPF) -- the reference the device's pf_run_mv / k_pf_batch_mv are compared with when
bssm_pf_config.mv_tv is given.  It follows the oracle's orc_pf_run (oracle/bssm_oracle.c) line by line, as
tests/mv_apf_rmpf_restated.py does for the constant model, and evaluates the model functions with that file's routines (the
kernels' order of operations) on the rows of the moment:

  transition TO absolute time tau      b = b_t[tau - 1]      tau = prev_t + step in the gap loop (:125-136);
                                                            the APF's second transition (:159): tau = the observation's time
  aux log-likelihood (APF, :142-147)   the transition mean with b_t[obs_time - 1], then h0_t[i - 1], H_t[i - 1]
  log-likelihood, the move's two       h0 = h0_t[i - 1], H = H_t[i - 1]       (i = the observation ROW, as y[i - 1])

This is the reference's own convention: it hands transition_fn the time prev_t + step in the gap loop and the observation's time
everywhere else (closure mode: bayesssm_amd/closures.py).  A piece that is None is the packed block's constant one."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_apf_rmpf_restated as R  # noqa: E402


def pf_run_mv_tv(oracle, theta, y, N, z_init, z_trans, u_res, b_t=None, h0_t=None, H_t=None, algorithm="BPF",
                 resample_algorithm="SISAR", resample_fn="stratified", threshold=None, obs_times=None, move_sd=0.0, z_move=None,
                 u_move=None, return_particles=False):
    """theta: the packed block; b_t [n_times][d], h0_t [T][p], H_t [T][p][d] or None; the other arguments and the result as
    mv_apf_rmpf_restated.pf_run_mv."""
    q = R.unpack(theta)
    d, p = q["d"], q["p"]
    y = np.asarray(y, dtype=np.float64).reshape(-1, p) if p > 0 else np.zeros((len(y), 0))
    T, dN = y.shape[0], float(N)
    b_t = None if b_t is None else np.asarray(b_t, dtype=np.float64).reshape(-1, d)
    h0_t = None if h0_t is None else np.asarray(h0_t, dtype=np.float64).reshape(T, p)
    H_t = None if H_t is None else np.asarray(H_t, dtype=np.float64).reshape(T, p, d)
    last = (int(obs_times[-1]) if obs_times is not None else T) if T > 0 else 0
    assert b_t is None or b_t.shape[0] >= last, "b_t must reach the last observation time"
    if threshold is None:
        threshold = np.inf if resample_algorithm == "SIS" else dN if resample_algorithm == "SISR" else dN / 2
    z_init = np.asarray(z_init, dtype=np.float64).reshape(d, N)
    z_trans = np.asarray(z_trans, dtype=np.float64).reshape(-1, d, N)
    u_res = np.asarray(u_res, dtype=np.float64)
    u_res = u_res.reshape(-1) if resample_fn == "systematic" else u_res.reshape(-1, N)
    if algorithm == "RMPF":
        z_move = np.asarray(z_move, dtype=np.float64).reshape(-1, d, N)
        u_move = np.asarray(u_move, dtype=np.float64).reshape(-1, N)

    def at(tau, i):
        """the model at (absolute time tau, observation row i): the block with the rows of the moment in place"""
        qt = dict(q)
        if b_t is not None:
            qt["b"] = b_t[tau - 1]
        if h0_t is not None:
            qt["h0"] = h0_t[i - 1]
        if H_t is not None:
            qt["H"] = H_t[i - 1]
        return qt

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
    ess[0] = 1.0 / R.rsum(w * w)                                   # :106-107
    for c in range(d):
        state_est[0, c] = R.rsum(x[c] * w)                         # :109-112
    if return_particles:
        ph.append(x.reshape(-1).copy()); wh.append(w.copy())
    loglike, prev_t, ktrans, kres, early = 0.0, 0, 0, 0, 0
    for i in range(1, T + 1):                                      # :123
        ot = int(obs_times[i - 1]) if obs_times is not None else i
        gap = ot - prev_t                                          # :124
        for step in range(1, gap + 1):                             # :125-136: transition_fn(particles, t = prev_t + step)
            x = R.transition(at(prev_t + step, i), x, z_trans[ktrans]); ktrans += 1
        prev_t = ot
        qi = at(ot, i)                                             # everything below sees t = the observation's time
        yi = y[i - 1]
        if algorithm == "APF":                                     # :140-175
            aux = R.aux_loglik(qi, yi, x)
            tmp = np.exp(aux - np.max(aux))                        # :153
            tmp = tmp / R.rsum(tmp)                                # :154
            idx = resample(tmp, kres)                              # :155
            ancestors.append(idx.copy()); kres += 1
            x = x[:, idx - 1]                                      # :157
            x = R.transition(qi, x, z_trans[ktrans]); ktrans += 1  # :159
            lw = R.loglik(qi, yi, x) - aux[idx - 1]                # :169-175
        else:
            lw = R.loglik(qi, yi, x)                               # :177-183
        if np.all(lw < -1e8):                                      # :189-202
            loglike = -np.inf; llh[i - 1] = -np.inf; early = i
            break
        mx = np.max(lw)                                            # :204
        tmp = np.exp(lw - mx)                                      # :205
        s = R.rsum(tmp)                                            # :206
        w = tmp / s                                                # :207
        loglike = loglike + (mx + np.log(s) - np.log(dN))          # :208
        llh[i - 1] = loglike                                       # :209
        ess[i] = 1.0 / R.rsum(w * w)                               # :211
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
            if p == 0:
                acc = np.ones(N, dtype=bool)
            else:
                acc = np.log(u_move[i - 1]) < (R.loglik(qi, yi, prop) - R.loglik(qi, yi, x))
            x = np.where(acc[None, :], prop, x)
        for c in range(d):
            state_est[i, c] = R.rsum(x[c] * w)                     # :238-240
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


def kalman_tv(q, ys, b_t=None, h0_t=None, H_t=None, obs_times=None):
    """Exact Kalman filter of the time-varying model for the BOOTSTRAP filter's dynamics (one transition per unit of time):
    returns (log-likelihood, filtering means [T][d]).  q: the unpacked block (mv_apf_rmpf_restated.unpack)."""
    d = q["d"]
    m, P = q["m0"].astype(np.float64).copy(), q["L0"] @ q["L0"].T
    Q, Rm = q["L"] @ q["L"].T, np.diag(q["sd"] ** 2)
    ll, means, prev_t = 0.0, [], 0
    for i in range(1, len(ys) + 1):
        ot = int(obs_times[i - 1]) if obs_times is not None else i
        for tau in range(prev_t + 1, ot + 1):
            b = q["b"] if b_t is None else b_t[tau - 1]
            m, P = q["A"] @ m + b, q["A"] @ P @ q["A"].T + Q
        prev_t = ot
        H = q["H"] if H_t is None else np.asarray(H_t[i - 1]).reshape(q["p"], d)
        h0 = q["h0"] if h0_t is None else h0_t[i - 1]
        S = H @ P @ H.T + Rm
        e = np.atleast_1d(ys[i - 1]) - (h0 + H @ m)
        ll += -0.5 * (len(e) * np.log(2 * np.pi) + np.linalg.slogdet(S)[1] + e @ np.linalg.solve(S, e))
        K = P @ H.T @ np.linalg.inv(S)
        m, P = m + K @ e, (np.eye(d) - K @ H) @ P
        means.append(m.copy())
    return float(ll), np.array(means)
