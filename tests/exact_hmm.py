"""Exact likelihoods of small state-space models, as probability models (numpy and scipy only; nothing of the project is imported).

The references:

* `ExactNet`: a mass-action reaction network with small populations is a finite-state hidden Markov model.  Its states are enumerated,
  the transition of one unit of time is a stochastic matrix (`expm(Q)` for Gillespie's direct method, an enumerated kernel for the two
  leap schemes), and the likelihood of a series of counts is a product of vector-matrix products.  Written from README.md and
  DESIGN.md section 1d read as a description of a probability model: what is drawn from which distribution, not how.
* `grid_filter_1d`: a point-mass filter on a uniform grid for the multivariate family at d = p = 1 (Gaussian, Poisson through a log
  link, log-variance), refined until the log-likelihood stands still; `kalman_1d` is the closed form that checks it.

`sisr_filter` is a plain numpy bootstrap filter (resampling at every observation) that draws from the exact kernel: the estimator
whose expectation `exp(loglike)` equals the exact likelihood, run on the true model.

Gamma white noise on the rates (`noise=`) keeps the model a finite-state HMM: the draws w are independent per (leap, group) and are
integrated out, so one noisy leap is the single stochastic matrix E_w[P(w)], taken by generalised Gauss-Laguerre quadrature (the weight
w^(shape - 1) exp(-w) is the gamma density itself, also where it is singular at 0), and one unit of time is its K-th power.  With noise
`simulate` and `sisr_filter` draw from the model itself (`rng.gamma`, `rng.binomial`, `rng.multinomial`, `rng.poisson`), never from the
quadrature kernel, so that they check it.

* `kalman_nd`: the Kalman filter of the multivariate linear-Gaussian family at any d and p (time-varying b, h0, H; partly missing rows;
  observation times with gaps and repeats), and `sisr_filter_nd`, the numpy bootstrap filter on that model.
"""
import numpy as np
import scipy.linalg
import scipy.special
import scipy.stats as st

NOISE_MISREADINGS = ("noise_per_reaction", "noise_per_unit", "noise_var_unscaled", "noise_skips_sourceless")
MISREADINGS = ("gap_one_unit", "schedule_row_tau", "no_counter_reset", "swap_size_mu", "missing_as_zero", "uncut") + NOISE_MISREADINGS
QUAD_TOL = 1e-10


class ExactNet:
    """species: names; reactions: (reactants, products, rate) with dicts species -> count and a number or (name, number); x0: counts;
    observe: one dict species -> coefficient per observation component.  `rate_names`: one name or None per reaction, for rates given
    as numbers.  `noise`: method="euler_multinomial" only, a dict from a rate name (all reactions whose rate has that name form one
    group) or a reaction index (a group of one) to sigma: per leap and group one w ~ sigma^2 Gamma(shape = 1 / (K sigma^2)), mean 1 / K
    and variance sigma^2 / K; the integrated hazard of a reaction of the group over the leap is h_r w, a sourceless one fires
    Poisson(a_r w) times; a reaction in no group has w = 1 / K.  `quad_start`: nodes per group of the first quadrature; it is doubled
    until no entry of the kernel moves by more than QUAD_TOL, and `n_nodes` is the count reached.  `cap`: largest count of any species
    kept for an open network (one with a reaction that consumes nothing); the mass that leaves the kept states goes to one absorbing
    state that no observation supports, and `filter` reports it.  `misread`: one of MISREADINGS, a deliberately wrong reading of the definition (tests of the reference)."""

    def __init__(self, species, reactions, x0, observe, counters=(), missing="refuse", rate_schedule=None, obs="poisson", size=None,
                 method="gillespie", leaps=None, cap=None, misread=None, noise=None, rate_names=None, quad_start=8):
        assert misread is None or misread in MISREADINGS
        assert obs in ("poisson", "negbin") and method in ("gillespie", "tau_leap", "euler_multinomial") and missing in ("refuse", "skip")
        self.species, self.d, self.R = tuple(species), len(species), len(reactions)
        ix = {s: c for c, s in enumerate(self.species)}
        self.rate = np.array([float(k[1] if isinstance(k, tuple) else k) for _, _, k in reactions])
        self.rate_names = [k[0] if isinstance(k, tuple) else None if rate_names is None else rate_names[r] for r, (_, _, k) in enumerate(reactions)]
        self.reactants = [tuple(ix[s] for s, n in lhs.items() for _ in range(int(n))) for lhs, _, _ in reactions]
        assert all(len(a) <= 2 and len(set(a)) == len(a) for a in self.reactants)
        self.nu = np.zeros((self.R, self.d), dtype=np.int64)
        for r, (lhs, rhs, _) in enumerate(reactions):
            for s, n in lhs.items():
                self.nu[r, ix[s]] -= int(n)
            for s, n in rhs.items():
                self.nu[r, ix[s]] += int(n)
        self.x0 = np.array(x0, dtype=np.int64)
        observe = [observe] if isinstance(observe, dict) else list(observe)
        self.G = np.zeros((len(observe), self.d))
        for k, row in enumerate(observe):
            for s, g in row.items():
                self.G[k, ix[s]] = float(g)
        self.p = len(observe)
        self.is_counter = np.array([s in counters for s in self.species])
        self.missing, self.obs, self.method, self.misread = missing, obs, method, misread
        self.size = None if size is None else np.broadcast_to(np.asarray(size, dtype=np.float64), (self.p,))
        self.M = None if rate_schedule is None else np.asarray(rate_schedule, dtype=np.float64)
        self.K = int(leaps) if method != "gillespie" else None
        self.open = any(not np.any(self.nu[r] < 0) for r in range(self.R))
        assert (cap is not None) == self.open, "an open network needs a cap, a closed one takes none"
        self.cap = cap
        self._enumerate()
        self._kernels = {}
        self.groups, self.quad_start, self.n_nodes = [], int(quad_start), 0   # groups: (reaction indices, sigma)
        assert noise is not None or misread not in NOISE_MISREADINGS
        if noise is not None:
            assert method == "euler_multinomial" and len(noise) > 0
            for key, sigma in noise.items():
                members = [r for r in range(self.R) if self.rate_names[r] == key] if isinstance(key, str) else [int(key)]
                assert members and all(0 <= r < self.R for r in members) and float(sigma) > 0, "noise names no reaction: %r" % (key,)
                assert not any(r in g for g, _ in self.groups for r in members), "a reaction is named twice"
                if misread == "noise_per_reaction":
                    self.groups += [((r,), float(sigma)) for r in members]
                else:
                    self.groups.append((tuple(members), float(sigma)))
        self.sourceless = [not np.any(self.nu[r] < 0) for r in range(self.R)]

    # ---- gamma white noise ---------------------------------------------------------------------------------------------------------
    def gamma_law(self, sigma):
        """(shape, scale) of one leap's w: mean 1 / K, variance sigma^2 / K"""
        if self.misread == "noise_var_unscaled":                       # variance sigma^2 per leap, the mean kept
            return 1.0 / (self.K * self.K * sigma * sigma), self.K * sigma * sigma
        return 1.0 / (self.K * sigma * sigma), sigma * sigma

    def weights(self, draws):
        """w [R, ...] from one draw [...] per group: the group's draw for its members, 1 / K for every other reaction"""
        w = np.full((self.R,) + np.shape(draws[0]), 1.0 / self.K)
        for (members, _), g in zip(self.groups, draws):
            for r in members:
                if not (self.misread == "noise_skips_sourceless" and self.sourceless[r]):
                    w[r] = g
        return w

    def quadrature(self, n):
        """n generalised Gauss-Laguerre nodes per group, as a tensor product over the groups: W [n^G, R] and the probabilities q [n^G]"""
        W, q = np.zeros((1, 0)), np.ones(1)
        for _, sigma in self.groups:
            shape, scale = self.gamma_law(sigma)
            x, a = scipy.special.roots_genlaguerre(n, shape - 1.0)
            W = np.concatenate([np.repeat(W, n, axis=0), np.tile(scale * x, len(W))[:, None]], axis=1)
            q = np.repeat(q, n) * np.tile(a / a.sum(), len(q))
        return self.weights(list(W.T)).T, q

    # ---- states ------------------------------------------------------------------------------------------------------------------
    def _enumerate(self):
        def zeroed(x):
            return tuple(0 if self.is_counter[c] else v for c, v in enumerate(x))
        start = tuple(int(v) for v in self.x0)
        seen, todo = {start: 0}, [start]
        if zeroed(start) not in seen:
            seen[zeroed(start)] = 1
            todo.append(zeroed(start))
        while todo:
            x = todo.pop()
            nxt = [zeroed(x)]
            for r in range(self.R):
                if self.rate[r] > 0 or self.M is not None:
                    z = tuple(v + int(n) for v, n in zip(x, self.nu[r]))
                    if min(z) >= 0 and (self.cap is None or max(z) <= self.cap):
                        nxt.append(z)
            for z in nxt:
                if z not in seen:
                    seen[z] = len(seen)
                    todo.append(z)
        self.states = np.array(list(seen), dtype=np.int64)            # [S, d]; the absorbing state has index S
        self.S = len(self.states)
        self.hi = int(self.states.max())
        self.base = self.hi + 1
        self._pow = self.base ** np.arange(self.d)
        self._lookup = np.full(self.base ** self.d, -1, dtype=np.int64)
        self._lookup[self.states @ self._pow] = np.arange(self.S)
        self.reset_to = self._lookup[np.where(self.is_counter, 0, self.states) @ self._pow]
        assert np.all(self.reset_to >= 0)

    def index_of(self, z):
        """indices of the states z [..., d]; the absorbing state S for one that is not kept"""
        z = np.asarray(z)
        ok = np.all((z >= 0) & (z <= self.hi), axis=-1)
        j = self._lookup[np.where(ok[..., None], z, 0) @ self._pow]
        j = np.where(ok & (j >= 0), j, self.S)
        if not self.open and self.misread != "uncut":
            assert np.all(j < self.S), "a closed network left its enumerated states"
        return j

    # ---- propensities ------------------------------------------------------------------------------------------------------------
    def _rates(self, mult):
        return self.rate if mult is None else self.rate * np.asarray(mult)

    def propensity(self, x, k):
        """mass action: k_r times the counts of the reactants"""
        return np.array([k[r] * np.prod([x[c] for c in self.reactants[r]]) for r in range(self.R)], dtype=np.float64)

    # ---- one unit of time --------------------------------------------------------------------------------------------------------
    def generator(self, mult=None):
        k = self._rates(mult)
        Q = np.zeros((self.S + 1, self.S + 1))
        for s, x in enumerate(self.states):
            a = self.propensity(x, k)
            for r in np.flatnonzero(a > 0):
                Q[s, self.index_of(x + self.nu[r])] += a[r]
            Q[s, s] -= a.sum()
        return Q

    def one_leap(self, mult=None, W=None, q=None):
        """the kernel of one leap; under the Euler-multinomial scheme with the weights W [n, R] of n quadrature nodes: their average
        with the probabilities q [n], or without q one kernel per node [n, S + 1, S + 1]"""
        k = self._rates(mult)
        if W is not None and q is None:
            P = np.zeros((len(W), self.S + 1, self.S + 1))
            P[:, self.S, self.S] = 1.0
            for s, x in enumerate(self.states):
                j, pr = self._em_terms(x, k, W)
                np.add.at(P[:, s, :].T, j, pr.T)
                P[:, s, self.S] += np.maximum(1.0 - P[:, s, :].sum(axis=1), 0.0)
            return P
        P = np.zeros((self.S + 1, self.S + 1))
        P[self.S, self.S] = 1.0
        for s, x in enumerate(self.states):
            if self.method == "tau_leap":
                self._tau_row(P[s], x, k)
            else:
                self._em_row(P[s], x, k, W, q)
        return P

    def _tau_row(self, row, x, k):
        """independent Poisson firing counts from the propensities at the start of the leap, taken in the order of the reactions, each
        cut at the smallest count among the species it consumes as the earlier reactions of the leap left them"""
        lam = self.propensity(x, k) / self.K
        dist = {tuple(int(v) for v in x): 1.0}
        gone = 0.0
        for r in range(self.R):
            if not lam[r] > 0:
                continue
            consumed = np.flatnonzero(self.nu[r] < 0)
            new = {}
            for z, pz in dist.items():
                if len(consumed) and self.misread != "uncut":
                    top = min(z[c] for c in consumed)
                    pm = st.poisson.pmf(np.arange(top + 1), lam[r])
                    pm[top] = st.poisson.sf(top - 1, lam[r])             # the cut: everything from `top` on
                else:
                    top = int(lam[r] + 12 * np.sqrt(lam[r])) + 25          # (a tail below 1e-18)
                    pm = st.poisson.pmf(np.arange(top + 1), lam[r])
                kept = 0.0
                for n in range(top + 1):
                    w = tuple(v + n * int(m) for v, m in zip(z, self.nu[r]))
                    if min(w) < 0 or max(w) > self.hi or self._lookup[np.dot(w, self._pow)] < 0:
                        continue
                    new[w] = new.get(w, 0.0) + pz * pm[n]
                    kept += pm[n]
                gone += pz * (1.0 - kept)
            dist = new
        for z, pz in dist.items():
            row[self._lookup[np.dot(z, self._pow)]] += pz
        row[self.S] += max(gone, 0.0)

    def _em_row(self, row, x, k, W=None, q=None):
        """per compartment: the number that leaves is Binomial(x_c, 1 - exp(-H)), H the sum over its exits of the per-capita hazard
        times the leap's weight (1 / K without noise), and the leavers are split over the exits multinomially by weighted hazard;
        reactions that consume nothing fire Poisson(a_r w_r) times; everything is drawn from the state at the start of the leap.
        With nodes W [n, R] and probabilities q [n]: the average of that row over the nodes"""
        j, pr = self._em_terms(x, k, np.full((1, self.R), 1.0 / self.K) if W is None else W)
        np.add.at(row, j, pr[0] if q is None else q @ pr)
        row[self.S] += max(1.0 - row.sum(), 0.0)                        # (the Poisson tails beyond 1e-18)

    def _em_terms(self, x, k, W):
        """the states j [M] that a leap from x can reach (with repeats) and their probabilities [n, M] under each row of W [n, R]"""
        nn = len(W)
        deltas, probs = [np.zeros((1, self.d), dtype=np.int64)], [np.ones((nn, 1))]
        exits = {}
        for r in range(self.R):
            down = np.flatnonzero(self.nu[r] < 0)
            if len(down) == 0:
                a = self.propensity(x, k)[r] * W[:, r]
                if a.max() > 0:
                    top = int(a.max() + 12 * np.sqrt(a.max())) + 25       # (a tail below 1e-18)
                    if self.cap is not None:                              # (all beyond the cap is one absorbing state)
                        top = min(top, self.cap + 1)
                    n = np.arange(top + 1)
                    pm = st.poisson.pmf(n[None, :], a[:, None])
                    pm[:, top] = st.poisson.sf(top - 1, a)
                    deltas.append(n[:, None] * self.nu[r][None, :])
                    probs.append(pm)
                continue
            assert len(down) == 1 and self.nu[r, down[0]] == -1 and down[0] in self.reactants[r], "no Euler-multinomial reading"
            c = int(down[0])
            h = k[r] * np.prod([x[o] for o in self.reactants[r] if o != c])
            if h > 0:
                exits.setdefault(c, []).append((r, float(h)))
        for c, ex in exits.items():
            if x[c] == 0:
                continue
            rs = [r for r, _ in ex]
            hw = np.array([v for _, v in ex])[None, :] * W[:, rs]         # [n, exits]
            H = hw.sum(axis=1)
            leave = -np.expm1(-H)
            dl, pr = [], []
            for n in range(int(x[c]) + 1):
                split = np.array(_compositions(n, len(ex)), dtype=np.int64)
                dl.append(split @ self.nu[rs])
                pr.append(st.binom.pmf(n, int(x[c]), leave)[:, None] * st.multinomial.pmf(split[None, :, :], n, (hw / H[:, None])[:, None, :]))
            deltas.append(np.concatenate(dl))
            probs.append(np.concatenate(pr, axis=1))
        D, Pr = deltas[0], probs[0]
        for dl, pr in zip(deltas[1:], probs[1:]):
            D = (D[:, None, :] + dl[None, :, :]).reshape(-1, self.d)
            Pr = (Pr[:, :, None] * pr[:, None, :]).reshape(nn, -1)
        return self.index_of(x[None, :] + D), Pr

    def _noisy_unit(self, mult, n):
        W, q = self.quadrature(n)
        if self.misread == "noise_per_unit":                              # one draw for the K leaps of the unit
            return np.einsum("n,nij->ij", q, np.linalg.matrix_power(self.one_leap(mult, W), self.K))
        return self.one_leap(mult, W, q)

    def unit_kernel(self, mult=None):
        key = None if mult is None else tuple(float(v) for v in mult)
        if key not in self._kernels:
            if self.method == "gillespie":
                P = scipy.linalg.expm(self.generator(mult))
            elif self.groups:
                n, P = self.quad_start, self._noisy_unit(mult, self.quad_start)
                while True:
                    n, prev = 2 * n, P
                    P = self._noisy_unit(mult, n)
                    if np.max(np.abs(P - prev)) <= QUAD_TOL:
                        break
                    assert n < 512, "the quadrature did not settle to %g" % QUAD_TOL
                self.n_nodes = max(self.n_nodes, n)
                if self.misread != "noise_per_unit":
                    P = np.linalg.matrix_power(P, self.K)
            else:
                P = np.linalg.matrix_power(self.one_leap(mult), self.K)
            self._kernels[key] = P
        return self._kernels[key]

    def _row(self, tau):
        """the multipliers of the transition TO absolute time tau: row tau - 1 of the schedule"""
        if self.M is None:
            return None
        if self.misread == "schedule_row_tau":
            return self.M[min(tau, len(self.M) - 1)]
        return self.M[tau - 1]

    def steps(self, obs_times):
        """per observation the list of (reset, multipliers) of its unit transitions: none at a repeated time; the counters are set to
        zero in front of the first unit of the interval only"""
        prev, out = 0, []
        for t in obs_times:
            gap = int(t) - prev
            if self.misread == "gap_one_unit" and gap > 1:
                units = [(True, self._row(int(t)))]
            else:
                units = [(u == 1, self._row(prev + u)) for u in range(1, gap + 1)]
            if self.misread == "no_counter_reset":
                units = [(False, m) for _, m in units]
            out.append(units)
            prev = int(t)
        return out

    # ---- observations ------------------------------------------------------------------------------------------------------------
    def obs_logpmf(self, yrow):
        """log p(y | state) for every kept state [S]"""
        return self.obs_logpmf_at(self.states, yrow)

    def obs_logpmf_at(self, x, yrow):
        """log p(y | x) for the states x [..., d]"""
        lam = (np.asarray(x) @ self.G.T).reshape(-1, self.p)
        return self._obs_logpmf(lam, yrow).reshape(np.shape(x)[:-1])

    def _obs_logpmf(self, lam, yrow):
        out = np.zeros(len(lam))
        for k, y in enumerate(np.atleast_1d(yrow)):
            if np.isnan(y):
                assert self.missing == "skip"
                if self.misread != "missing_as_zero":
                    continue
                y = 0.0
            mu = lam[:, k]
            pos = mu > 0
            lp = np.where(y == 0, 0.0, -np.inf) * np.ones(len(lam))   # mu == 0: a point mass at 0
            if self.obs == "poisson":
                lp[pos] = st.poisson.logpmf(y, mu[pos])
            else:
                r = self.size[k]
                if self.misread == "swap_size_mu":
                    lp[pos] = st.nbinom.logpmf(y, n=mu[pos], p=mu[pos] / (mu[pos] + r))
                else:
                    lp[pos] = st.nbinom.logpmf(y, n=r, p=r / (r + mu[pos]))
            out += lp
        return out

    # ---- the exact filter --------------------------------------------------------------------------------------------------------
    def _times(self, y, obs_times):
        y = np.asarray(y, dtype=np.float64).reshape(len(y), -1)
        return y, (np.arange(1, len(y) + 1) if obs_times is None else np.asarray(obs_times))

    def filter(self, y, obs_times=None):
        """loglike_history [T] (cumulative), filtered means [T, d], the mass lost at the cap, the number of states"""
        y, ot = self._times(y, obs_times)
        alpha = np.zeros(self.S + 1)
        alpha[self.index_of(self.x0)] = 1.0
        ll, llh, means, lost = 0.0, [], [], 0.0
        for yrow, units in zip(y, self.steps(ot)):
            for reset, mult in units:
                if reset:
                    alpha = np.append(np.bincount(self.reset_to, alpha[:self.S], minlength=self.S), alpha[self.S])
                alpha = alpha @ self.unit_kernel(mult)
            lost += alpha[self.S]
            a = alpha[:self.S] * np.exp(self.obs_logpmf(yrow))
            ll += np.log(a.sum())
            alpha = np.append(a / a.sum(), 0.0)
            llh.append(ll)
            means.append(alpha[:self.S] @ self.states)
        if self.misread is None:
            assert lost <= 1e-12, "mass lost at the cap: %g" % lost
        return {"loglike_history": np.array(llh), "filtered_mean": np.array(means), "lost": lost, "n_states": self.S}

    # ---- drawing from the exact model ------------------------------------------------------------------------------------------------
    def _move(self, idx, units, rng):
        for reset, mult in units:
            if reset:
                idx = self.reset_to[idx]
            cdf = np.cumsum(self.unit_kernel(mult)[:self.S, :self.S], axis=1)
            cdf /= cdf[:, -1:]
            flat = (cdf + np.arange(self.S)[:, None]).ravel()
            u = rng.random(idx.shape)
            idx = np.minimum(np.searchsorted(flat, u + idx, side="right") - idx * self.S, self.S - 1)
        return idx

    def _move_model(self, x, units, rng):
        """the noisy Euler-multinomial units on the counts x [..., d], drawn from the model itself: per leap one gamma draw per group
        and element, binomial leavers per compartment split multinomially, Poisson firings of the sourceless reactions"""
        assert self.groups and self.misread not in NOISE_MISREADINGS
        shp = x.shape[:-1]
        for reset, mult in units:
            if reset:
                x = np.where(self.is_counter, 0, x)
            k = self._rates(mult)
            for _ in range(self.K):
                w = self.weights([self.gamma_law(sigma)[1] * rng.gamma(self.gamma_law(sigma)[0], size=shp) for _, sigma in self.groups])
                new = x.copy()
                for c in range(self.d):
                    ex = [r for r in range(self.R) if self.nu[r, c] < 0]
                    if not ex:
                        continue
                    hw = np.stack([k[r] * np.prod([x[..., o] for o in self.reactants[r] if o != c], axis=0) * w[r] for r in ex], axis=-1)
                    H = hw.sum(axis=-1)
                    leavers = rng.binomial(x[..., c], -np.expm1(-H))
                    split = rng.multinomial(leavers, np.where(H[..., None] > 0, hw / np.where(H > 0, H, 1.0)[..., None], 1.0 / len(ex)))
                    for i, r in enumerate(ex):
                        new = new + split[..., i, None] * self.nu[r]
                for r in range(self.R):
                    if self.sourceless[r]:
                        a = k[r] * np.prod([x[..., o] for o in self.reactants[r]] + [np.ones(shp)], axis=0)
                        new = new + rng.poisson(a * w[r])[..., None] * self.nu[r]
                x = new
        return x

    def simulate(self, T, rng, obs_times=None):
        ot = np.arange(1, T + 1) if obs_times is None else np.asarray(obs_times)
        if self.groups:
            x, ys = self.x0[None, :].copy(), []
            for units in self.steps(ot):
                x = self._move_model(x, units, rng)
                mu = self.G @ x[0]
                ys.append(rng.poisson(mu) if self.obs == "poisson" else
                          [rng.negative_binomial(r, r / (r + m)) if m > 0 else 0 for r, m in zip(self.size, mu)])
            return np.array(ys, dtype=np.float64)
        idx, ys = np.array([self.index_of(self.x0)]), []
        for units in self.steps(ot):
            idx = self._move(idx, units, rng)
            mu = self.G @ self.states[idx[0]]
            if self.obs == "poisson":
                ys.append(rng.poisson(mu))
            else:
                ys.append([rng.negative_binomial(r, r / (r + m)) if m > 0 else 0 for r, m in zip(self.size, mu)])
        return np.array(ys, dtype=np.float64)

    def sisr_filter(self, y, N, F, rng, obs_times=None):
        """F bootstrap filters of N particles that draw from the exact kernel (with gamma white noise: from the model itself, never
        from the quadrature kernel) and resample (stratified) at every observation: loglike_history [F, T] and state_est [F, T, d], the
        mean of the resampled particles"""
        y, ot = self._times(y, obs_times)
        idx = np.full((F, N), self.index_of(self.x0))
        if self.groups:                                               # (the particles are counts, not state indices)
            idx = np.tile(self.x0, (F, N, 1))
        ll, llh, est = np.zeros(F), [], []
        for yrow, units in zip(y, self.steps(ot)):
            if self.groups:
                idx = self._move_model(idx, units, rng)
                w = np.exp(self.obs_logpmf_at(idx, yrow))
            else:
                idx = self._move(idx, units, rng)
                w = np.exp(self.obs_logpmf(yrow))[idx]
            ll = ll + np.log(w.mean(axis=1))
            llh.append(ll)
            c = np.cumsum(w, axis=1)
            c /= c[:, -1:]
            u = (np.arange(N)[None, :] + rng.random((F, N))) / N
            pick = np.searchsorted((c + np.arange(F)[:, None]).ravel(), (u + np.arange(F)[:, None]).ravel(), side="right").reshape(F, N)
            pick = np.minimum(pick - np.arange(F)[:, None] * N, N - 1)
            if self.groups:
                idx = np.take_along_axis(idx, pick[:, :, None], axis=1)
                est.append(idx.mean(axis=1))
            else:
                idx = np.take_along_axis(idx, pick, axis=1)
                est.append(self.states[idx].mean(axis=1))
        return {"loglike_history": np.array(llh).T, "state_est": np.transpose(np.array(est), (1, 0, 2))}


def _compositions(n, parts):
    """all ways to write n as an ordered sum of `parts` non-negative integers"""
    if parts == 1:
        return [(n,)]
    return [(a,) + rest for a in range(n + 1) for rest in _compositions(n - a, parts - 1)]


def uniformised(Q, tail=1e-14):
    """exp(Q) by uniformisation: sum_n Poisson(n; q) (I + Q / q)^n with q the largest exit rate, until the Poisson tail is below `tail`"""
    q = max(float(np.max(-np.diag(Q))), 1e-300)
    B = np.eye(len(Q)) + Q / q
    term, out, n = np.eye(len(Q)), np.zeros_like(Q), 0
    while True:
        out += st.poisson.pmf(n, q) * term
        if st.poisson.sf(n, q) < tail:
            return out
        term, n = term @ B, n + 1


# ---- d = p = 1, continuous state ----------------------------------------------------------------------------------------------------
def _obs_logpdf_1d(obs, y, eta, sd):
    if obs == "gaussian":
        return st.norm.logpdf(y, eta, sd)
    if obs == "poisson":
        return st.poisson.logpmf(y, np.exp(eta))
    assert obs == "logvar"
    return st.norm.logpdf(y, 0.0, np.exp(eta / 2))


def _grid_pass(n, y, A, b, L, m0, L0, h0, H, sd, obs):
    mean, s = b / (1 - A), L / np.sqrt(1 - A * A)
    lo, hi = min(mean - 8 * s, m0 - 8 * L0), max(mean + 8 * s, m0 + 8 * L0)
    x = np.linspace(lo, hi, n)
    dx = x[1] - x[0]
    K = st.norm.pdf(x[None, :], A * x[:, None] + b, L) * dx
    p = st.norm.pdf(x, m0, L0) * dx
    ll, llh, means = 0.0, [], []
    for yt in y:
        p = p @ K
        if not np.isnan(yt):
            p = p * np.exp(_obs_logpdf_1d(obs, yt, h0 + H * x, sd))
        ll += np.log(p.sum())
        p = p / p.sum()
        llh.append(ll)
        means.append(p @ x)
    return np.array(llh), np.array(means)


def grid_filter_1d(y, A, b, L, m0, L0, h0=0.0, H=1.0, sd=1.0, obs="gaussian", tol=1e-8):
    """x_0 ~ N(m0, L0^2), x_t = A x_{t-1} + b + L z_t, y_t | x_t from `obs` over eta = h0 + H x_t (NaN: not observed), |A| < 1.
    Point masses on a uniform grid over the stationary distribution +- 8 sd (and the initial one), doubled until the log-likelihood
    of every prefix changes by less than `tol` between two successive doublings; that is asserted here."""
    y = np.asarray(y, dtype=np.float64)
    n, prev = 129, None
    while n <= 8193:
        cur = _grid_pass(n, y, A, b, L, m0, L0, h0, H, sd, obs)
        if prev is not None and np.max(np.abs(cur[0] - prev[0])) < tol:
            return {"loglike_history": cur[0], "filtered_mean": cur[1], "n_grid": n}
        prev, n = cur, 2 * (n - 1) + 1
    raise AssertionError("the grid filter did not settle to %g" % tol)


def kalman_1d(y, A, b, L, m0, L0, h0=0.0, H=1.0, sd=1.0):
    m, P, ll, llh, means = m0, L0 * L0, 0.0, [], []
    for yt in np.asarray(y, dtype=np.float64):
        m, P = A * m + b, A * A * P + L * L
        if not np.isnan(yt):
            S = H * H * P + sd * sd
            ll += st.norm.logpdf(yt, h0 + H * m, np.sqrt(S))
            g = P * H / S
            m, P = m + g * (yt - h0 - H * m), (1 - g * H) * P
        llh.append(ll)
        means.append(m)
    return {"loglike_history": np.array(llh), "filtered_mean": np.array(means)}


def simulate_1d(T, rng, A, b, L, m0, L0, h0=0.0, H=1.0, sd=1.0, obs="gaussian"):
    x, ys = m0 + L0 * rng.standard_normal(), []
    for _ in range(T):
        x = A * x + b + L * rng.standard_normal()
        eta = h0 + H * x
        ys.append(eta + sd * rng.standard_normal() if obs == "gaussian" else rng.poisson(np.exp(eta)) if obs == "poisson"
                  else np.exp(eta / 2) * rng.standard_normal())
    return np.array(ys, dtype=np.float64)


def sisr_filter_1d(y, N, F, rng, A, b, L, m0, L0, h0=0.0, H=1.0, sd=1.0, obs="gaussian"):
    """F bootstrap filters of N particles on the model itself, stratified resampling at every observation: loglike_history [F, T] and
    state_est [F, T], the mean of the resampled particles"""
    x = m0 + L0 * rng.standard_normal((F, N))
    ll, llh, est = np.zeros(F), [], []
    rows = np.arange(F)[:, None]
    for yt in np.asarray(y, dtype=np.float64):
        x = A * x + b + L * rng.standard_normal((F, N))
        w = np.ones((F, N)) if np.isnan(yt) else np.exp(_obs_logpdf_1d(obs, yt, h0 + H * x, sd))
        ll = ll + np.log(w.mean(axis=1))
        llh.append(ll)
        c = np.cumsum(w, axis=1)
        c /= c[:, -1:]
        u = (np.arange(N)[None, :] + rng.random((F, N))) / N
        pick = np.searchsorted((c + rows).ravel(), (u + rows).ravel(), side="right").reshape(F, N)
        x = np.take_along_axis(x, np.minimum(pick - rows * N, N - 1), axis=1)
        est.append(x.mean(axis=1))
    return {"loglike_history": np.array(llh).T, "state_est": np.array(est).T}


# ---- any d and p, linear and Gaussian -----------------------------------------------------------------------------------------------------
def _nd_times(T, obs_times):
    return np.arange(1, T + 1) if obs_times is None else np.asarray(obs_times, dtype=np.int64)


def kalman_nd(y, A, b, L, m0, L0, h0, H, sd, b_t=None, h0_t=None, H_t=None, obs_times=None):
    """x_0 ~ N(m0, L0 L0'), x_tau = A x_{tau-1} + b + L z per unit of time, y_i | x ~ N(h0 + H x, diag(sd^2)) at the time of observation i.
    b_t [n_times, d] is indexed by absolute time (the transition TO tau reads b_t[tau - 1]), h0_t [T, p] and H_t [T, p, d] by observation
    row; obs_times (None: 1 .. T) may repeat a time (no transition in between) and leave gaps (one transition per unit).  A row of y with
    NaN components updates on the observed ones only; an empty row contributes 0.0.  Returns loglike_history [T] (cumulative) and
    filtered_mean [T, d]."""
    y = np.asarray(y, dtype=np.float64).reshape(len(y), -1)
    A, L, L0, H = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (A, L, L0, H))
    b, m0, h0 = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (b, m0, h0))
    d, p = len(m0), y.shape[1]
    sd = np.broadcast_to(np.asarray(sd, dtype=np.float64), (p,))
    m, P, Q = m0.copy(), L0 @ L0.T, L @ L.T
    ll, llh, means, now = 0.0, [], [], 0
    for i, t in enumerate(_nd_times(len(y), obs_times)):
        for tau in range(now + 1, int(t) + 1):
            m, P = A @ m + (b if b_t is None else np.asarray(b_t, dtype=np.float64)[tau - 1]), A @ P @ A.T + Q
        now = int(t)
        Hi = H if H_t is None else np.asarray(H_t, dtype=np.float64)[i].reshape(p, d)
        hi = h0 if h0_t is None else np.asarray(h0_t, dtype=np.float64)[i].reshape(p)
        seen = ~np.isnan(y[i])
        if seen.any():
            Hs = Hi[seen]
            S = Hs @ P @ Hs.T + np.diag(sd[seen] ** 2)
            ll += st.multivariate_normal.logpdf(y[i][seen], hi[seen] + Hs @ m, S)
            G = np.linalg.solve(S, Hs @ P).T                        # P Hs' S^-1 (S and P are symmetric)
            m, P = m + G @ (y[i][seen] - hi[seen] - Hs @ m), P - G @ Hs @ P
            P = 0.5 * (P + P.T)
        llh.append(ll)
        means.append(m.copy())
    return {"loglike_history": np.array(llh), "filtered_mean": np.array(means)}


def simulate_nd(T, rng, A, b, L, m0, L0, h0, H, sd, b_t=None, h0_t=None, H_t=None, obs_times=None):
    A, L, L0, H = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (A, L, L0, H))
    p, d = H.shape
    x, ys, now = np.asarray(m0) + L0 @ rng.standard_normal(d), [], 0
    for i, t in enumerate(_nd_times(T, obs_times)):
        for tau in range(now + 1, int(t) + 1):
            x = A @ x + (b if b_t is None else b_t[tau - 1]) + L @ rng.standard_normal(d)
        now = int(t)
        eta = (h0 if h0_t is None else h0_t[i]) + (H if H_t is None else H_t[i]) @ x
        ys.append(eta + np.broadcast_to(sd, (p,)) * rng.standard_normal(p))
    return np.array(ys)


def sisr_filter_nd(y, N, F, rng, A, b, L, m0, L0, h0, H, sd, b_t=None, h0_t=None, H_t=None, obs_times=None):
    """F bootstrap filters of N particles on the model itself, stratified resampling at every observation: loglike_history [F, T] and
    state_est [F, T, d], the mean of the resampled particles"""
    y = np.asarray(y, dtype=np.float64).reshape(len(y), -1)
    A, L, L0, H = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (A, L, L0, H))
    p, d = H.shape
    sd = np.broadcast_to(np.asarray(sd, dtype=np.float64), (p,))
    x = np.asarray(m0) + rng.standard_normal((F, N, d)) @ L0.T
    ll, llh, est, now = np.zeros(F), [], [], 0
    rows = np.arange(F)[:, None]
    for i, t in enumerate(_nd_times(len(y), obs_times)):
        for tau in range(now + 1, int(t) + 1):
            x = x @ A.T + (b if b_t is None else b_t[tau - 1]) + rng.standard_normal((F, N, d)) @ L.T
        now = int(t)
        eta = (h0 if h0_t is None else h0_t[i]) + x @ (H if H_t is None else H_t[i]).T
        seen = ~np.isnan(y[i])
        w = np.exp(st.norm.logpdf(y[i][seen], eta[..., seen], sd[seen]).sum(axis=-1))
        ll = ll + np.log(w.mean(axis=1))
        llh.append(ll)
        c = np.cumsum(w, axis=1)
        c /= c[:, -1:]
        u = (np.arange(N)[None, :] + rng.random((F, N))) / N
        pick = np.searchsorted((c + rows).ravel(), (u + rows).ravel(), side="right").reshape(F, N)
        x = np.take_along_axis(x, np.minimum(pick - rows * N, N - 1)[:, :, None], axis=1)
        est.append(x.mean(axis=1))
    return {"loglike_history": np.array(llh).T, "state_est": np.transpose(np.array(est), (1, 0, 2))}
