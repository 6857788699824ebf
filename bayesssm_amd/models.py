"""Built-in device models: the stand-ins for the reference's R closures.

The reference takes init_fn / transition_fn / log_likelihood_fn as arbitrary R
closures (R/particle_filter-doc.R:7-35).  Closures cannot run on a GPU, so the
device path takes DESCRIPTORS of built-in models with the same argument names;
model parameters still travel as named arguments (`phi=..., sigma_x=...`), as
they do through `...` in the reference.
"""


class ModelFn:
    """One of the three (four, with the APF) user functions of a built-in model."""

    def __init__(self, model, role, params):
        self.model = model          # "lg" | "ar1sin"
        self.role = role            # "init" | "transition" | "log_likelihood" | "aux_log_likelihood"
        self.params = tuple(params)  # model-specific named arguments this function reads

    def formals(self):
        """Argument names as the reference's .check_params_match sees them (R/utils.R:19-61)."""
        head = {"init": ["num_particles"], "transition": ["particles"],
                "log_likelihood": ["y", "particles"], "aux_log_likelihood": ["y", "particles"]}[self.role]
        return head + list(self.params)

    def __repr__(self):
        return "<%s %s_fn(%s)>" % (self.model, self.role, ", ".join(self.formals()))


class Model:
    PARAM_ORDER = ("phi", "sigma_x", "sigma_y")

    def __init__(self, name, doc):
        self.name = name
        self.__doc__ = doc
        self.init_fn = ModelFn(name, "init", ())
        self.transition_fn = ModelFn(name, "transition", ("phi", "sigma_x"))
        self.log_likelihood_fn = ModelFn(name, "log_likelihood", ("sigma_y",))
        self.aux_log_likelihood_fn = ModelFn(name, "aux_log_likelihood", ("phi", "sigma_y"))
        self.dim = 1
        self.param_order = self.PARAM_ORDER
        self.constants = ()

    def rw_move_fn(self, sd=0.1):
        return MoveFn(self.name, sd)


class SirModel(Model):
    """Stochastic SIR of vignettes/articles/stochastic-sir-model.Rmd:143-176,285-310: state (s, i), one Gillespie
    day per transition (rates lambda/n_total * s * i and gamma * i), y ~ Poisson(i).  `n_total` and the initial
    state are the vignette's globals (:143-148); the sampled parameters are (lambda, gamma)."""
    PARAM_ORDER = ("lambda", "gamma")

    def __init__(self, n_total=500, init_infected=70):
        self.name = "sir"
        self.init_fn = ModelFn("sir", "init", ())
        self.transition_fn = ModelFn("sir", "transition", ("lambda", "gamma"))
        self.log_likelihood_fn = ModelFn("sir", "log_likelihood", ())
        # look-ahead used by auxiliary_filter (the reference defines none for this model): Poisson at the one-day mean of i
        self.aux_log_likelihood_fn = ModelFn("sir", "aux_log_likelihood", ("lambda", "gamma"))
        self.dim = 2
        self.param_order = self.PARAM_ORDER
        self.constants = (float(n_total), float(n_total - init_infected), float(init_infected))
        for fn in (self.init_fn, self.transition_fn, self.log_likelihood_fn, self.aux_log_likelihood_fn):
            fn.owner = self


def sir(n_total=500, init_infected=70):
    return SirModel(n_total, init_infected)


class MoveFn:
    """Built-in move_fn of resample_move_filter: the random-walk Metropolis move of the reference's own example
    (R/resample_move_filter.R:166-176):  proposal = particle + rnorm(1, 0, sd);  accept when
    log(runif(1)) < log_likelihood(proposal) - log_likelihood(particle)."""

    def __init__(self, model, sd=0.1, params=("sigma_y",)):
        self.model, self.sd, self.params = model, float(sd), tuple(params)

    def formals(self):
        return ["particle", "y"] + list(self.params)


class LinearGaussianMV:
    """Multivariate linear-Gaussian family on the device (state dimension d <= 8, observation dimension p <= 8):

        init_fn           x0 = m0 + L0 z               (the reference's  matrix(rnorm(N d), ncol = d)  shifted and scaled)
        transition_fn     x' = A x + b + L z           L lower triangular: a Cholesky factor of the state noise covariance
        log_likelihood_fn p == 0: the constant c0      (tests/testthat/test-bootstrap_filter.R:211-230: rep(1, nrow(particles)))
                          p >  0: sum_k dnorm(y_k, h0_k + (H x)_k, sd_k, log = TRUE)
        aux_log_likelihood_fn  the log-likelihood at the transition mean A x + b (auxiliary_filter; the pattern of the
                          reference's APF test, tests/testthat/test-auxiliary_filter.R:24-27)
        rw_move_fn(sd)    the random-walk Metropolis move of resample_move_filter (see rw_move_fn)

    obs= selects the observation density over the linear predictor  eta_k = h0_k + (H x)_k  (p >= 1 unless "gaussian"):
        "gaussian" (default)  dnorm(y_k, eta_k, sd_k, log = TRUE)
        "poisson"             dpois(y_k, exp(eta_k), log = TRUE): counts through a log link (the observation of the reference's
                              stochastic-SIR vignette over a linear-Gaussian latent state); y must hold non-negative integers
        "logvar"              dnorm(y_k, 0, exp(eta_k / 2), log = TRUE): stochastic volatility; the canonical model is d = p = 1,
                              H = 1, A = phi, b = mu (1 - phi)
    The two new families do not read sd (it keeps its slot in the packed block: pack() is the same for every obs); the aux
    log-likelihood and the move's acceptance ratio use the family's density.

    missing= says what a NaN in y means (+-inf is refused always):
        "refuse" (default)    an error, as for every other model (the reference's assert_numeric(y, any.missing = FALSE))
        "skip"                y[i, k] = NaN: component k of observation i was not observed (a sensor dropped out, a quarterly series
                              next to monthly ones, counts not reported on weekends).  The log-likelihood of observation i is the sum
                              over its observed components only -- what a reference closure does that returns 0 for what was not
                              seen; a row with nothing observed gives every particle 0.0, and the filter goes through its usual
                              sequence (normalisation, ESS, resample decision, resampling), so every draw keeps its key.  The aux
                              log-likelihood and both terms of the move's ratio follow the same rule.  The Poisson family's
                              count checks cover the observed entries only.

    Pieces that change with time in a KNOWN way (control inputs, seasonal offsets, dynamic regression: the covariate row of
    time t is the observation matrix) are data next to y:  time_varying={"b": [n_times, d], "h0": [T, p], "H": [T, p, d]}, any
    subset.  Shorthands: a vector for "b" at d == 1 and for "h0" at p == 1 (one scalar per row), and a [T, d] matrix for "H" at
    p == 1 (one covariate row per observation); they are stored in the full shapes.  The reference hands every closure the time index (R/bootstrap_filter.R:142-148); here the transition TO absolute
    time tau (prev_t + step in the gap loop, R/particle_filter_core.R:125-136) reads b[tau - 1]; the APF's second transition and
    its aux transition mean read the row of the observation's time; h0 / H are indexed by observation row, as y is.  n_times
    must reach the last observation time (T without obs_times).  A, L, sd, m0, L0, c0 are constant.
    The arrays may depend on the sampled parameters too (an input gain  b_t = g u_t,  a seasonal amplitude  h0_t = a sin(w t)):
    `build(**params)` then returns, next to its constant pieces, "time_varying": {...} in the same forms; an array it returns
    replaces the constructor's of that name for that draw, the others keep the constructor's.  `has_param_tv` tells whether
    the model has such pieces; it is decided by the first call of `build` (any pack / tv_arrays with parameters), and `build`
    must then return the key for every draw or for none.

    Fixed pieces are given to the constructor (m0, P0 or L0, A, b, Q or L, c0, H, h0, sd); pieces that depend on sampled
    parameters come from `build(**params) -> dict of pieces` (e.g. the reference's multi-dimensional PMMH case,
    tests/testthat/test-pmmh.R:619-668:  linear_gaussian_mv(2, build=lambda phi: {"b": [phi, phi]}, param_names=("phi",))).
    The three descriptors carry the parameter names, so bootstrap_filter / pmmh take them as they take the scalar models."""

    OBS = ("gaussian", "poisson", "logvar")
    MISSING = ("refuse", "skip")

    def __init__(self, d, p=0, build=None, param_names=(), time_varying=None, obs="gaussian", missing="refuse", **pieces):
        import numpy as np
        if not (1 <= int(d) <= 8 and 0 <= int(p) <= 8):
            raise ValueError("linear_gaussian_mv: 1 <= d <= 8 and 0 <= p <= 8")
        if obs not in self.OBS:
            raise ValueError("linear_gaussian_mv: obs must be one of %s, got %r" % (", ".join('"%s"' % o for o in self.OBS), obs))
        if obs != "gaussian" and int(p) == 0:
            raise ValueError("linear_gaussian_mv: obs=%r needs observation components (p >= 1)" % obs)
        if missing not in self.MISSING:
            raise ValueError("linear_gaussian_mv: missing must be one of 'refuse', 'skip'")
        self.name, self.dim, self.p, self.obs, self.missing = "lgmv", int(d), int(p), obs, missing
        self.time_varying = self._check_time_varying(time_varying)
        self.build, self.param_order, self.constants = build, tuple(param_names), ()
        self._param_tv, self._built_last = (False if build is None else None), None
        self.pieces = {"m0": np.zeros(self.dim), "L0": np.eye(self.dim), "A": np.eye(self.dim), "b": np.zeros(self.dim), "L": np.eye(self.dim),
                       "c0": 0.0, "H": np.eye(self.p, self.dim), "h0": np.zeros(self.p), "sd": np.ones(self.p)}
        self._set(pieces)
        self.init_fn = ModelFn("lgmv", "init", ())
        self.transition_fn = ModelFn("lgmv", "transition", self.param_order)
        self.log_likelihood_fn = ModelFn("lgmv", "log_likelihood", ())
        self.aux_log_likelihood_fn = ModelFn("lgmv", "aux_log_likelihood", self.param_order)
        for fn in (self.init_fn, self.transition_fn, self.log_likelihood_fn, self.aux_log_likelihood_fn):
            fn.owner = self

    def rw_move_fn(self, sd=0.1):
        """The move of resample_move_filter on this family: the d-dimensional form of the reference example's random-walk
        Metropolis move (R/resample_move_filter.R:166-176) with d independent normals,
            proposal_c = particle_c + rnorm(1, 0, sd)   for every component c;
            accept when log(runif(1)) < log_likelihood(proposal) - log_likelihood(particle)   (p == 0: always).
        This is NOT what the R example does with an N x d matrix: there `particle + rnorm(1, 0, sd)` adds ONE normal, recycled,
        to every component of the row."""
        m = MoveFn("lgmv", sd, self.param_order)
        m.owner = self
        return m

    def _check_time_varying(self, tv):
        """{"b": [n_times, d], "h0": [T, p], "H": [T, p, d]} as contiguous float64 arrays (None when nothing is given)"""
        import numpy as np
        if tv is None:
            return None
        if not isinstance(tv, dict):
            raise TypeError("linear_gaussian_mv: time_varying must be a dict with keys among 'b', 'h0', 'H'")
        d, p = self.dim, self.p
        tails = {"b": (d,), "h0": (p,), "H": (p, d)}
        out = {}
        for k, v in tv.items():
            if k not in tails:
                raise TypeError("linear_gaussian_mv: unknown time-varying piece %r (b, h0 and H may vary with time)" % k)
            if v is None:
                continue
            if k != "b" and p == 0:
                raise ValueError("linear_gaussian_mv: time_varying[%r] given for a model without observation components (p == 0)" % k)
            a = np.ascontiguousarray(v, dtype=np.float64)
            if k != "H" and a.ndim == 1 and tails[k] == (1,):
                a = a.reshape(-1, 1)                                   # a vector of scalars for d == 1 / p == 1
            if k == "H" and a.ndim == 2 and p == 1 and a.shape[1] == d:
                a = a.reshape(-1, 1, d)                                # dynamic regression: one covariate row per observation
            if a.ndim != 1 + len(tails[k]) or a.shape[1:] != tails[k] or a.shape[0] < 1:
                raise ValueError("linear_gaussian_mv: time_varying[%r] must have shape (%s, %s), got %s"
                                 % (k, "n_times" if k == "b" else "T", ", ".join(str(n) for n in tails[k]), tuple(a.shape)))
            if not np.all(np.isfinite(a)):
                raise ValueError("linear_gaussian_mv: time_varying[%r] contains non-finite values" % k)
            out[k] = a
        return out or None

    @property
    def has_param_tv(self):
        """True when `build` returns parameter-dependent time-varying arrays.  Decided by the first call of `build` (the
        first pack / tv_arrays with parameters); False before it."""
        return bool(self._param_tv)

    def _built(self, params):
        """(constant pieces, checked time-varying arrays or None) that `build` returns for one draw; the last draw is kept, so
        that pack and tv_arrays of the same draw call `build` once"""
        missing = [k for k in self.param_order if k not in params]
        if missing:
            raise TypeError('argument "%s" is missing, with no default' % missing[0])
        key = tuple(float(params[k]) for k in self.param_order)
        last = self._built_last                      # (read once: chains on several threads share the descriptor)
        if last is not None and last[0] == key:
            return last[1], last[2]
        pieces = dict(self.build(**dict(zip(self.param_order, key))))
        has = "time_varying" in pieces
        if self._param_tv is None:
            self._param_tv = has
        elif has != self._param_tv:
            raise ValueError("linear_gaussian_mv: build must return 'time_varying' for every parameter draw or for none")
        tv = self._check_time_varying(pieces.pop("time_varying")) if has else None
        self._built_last = (key, pieces, tv)
        return pieces, tv

    def tv_arrays(self, T, obs_times=None, params=None):
        """(n_times, b_t, h0_t, H_t) for a run over T observations at obs_times (None: 1..T), checked against them: b_t must
        reach the last observation time, h0_t / H_t hold one row per observation.  None when the model has no such pieces.
        params: the parameter draw, for the arrays `build` returns (they replace the constructor's of the same name)."""
        tv = self.time_varying
        if params is not None and self.build is not None:
            drawn = self._built(params)[1]
            if drawn:
                tv = dict(tv or {}, **drawn)
        return self.tv_checked(tv, T, obs_times)

    def tv_checked(self, tv, T, obs_times=None):
        """tv_arrays for a dict of arrays that _check_time_varying returned (None: no such pieces)"""
        if tv is None:
            return None
        T = int(T)
        last = (int(obs_times[-1]) if obs_times is not None and len(obs_times) else T) if T > 0 else 0
        b = tv.get("b")
        if b is not None and b.shape[0] < last:
            raise ValueError("linear_gaussian_mv: time_varying['b'] has %d rows (n_times); the last observation time is %d"
                             % (b.shape[0], last))
        for k in ("h0", "H"):
            if tv.get(k) is not None and tv[k].shape[0] != T:
                raise ValueError("linear_gaussian_mv: time_varying[%r] has %d rows; y has %d observations (one row each)"
                                 % (k, tv[k].shape[0], T))
        return (0 if b is None else int(b.shape[0]), b, tv.get("h0"), tv.get("H"))

    def y_ok(self, y):
        """the host's finiteness check of y for this descriptor: no NaN and no +-inf; missing="skip" lets NaN through"""
        import numpy as np
        y = np.asarray(y, dtype=np.float64)
        return bool(np.all(np.isfinite(y) | np.isnan(y))) if self.missing == "skip" else bool(np.all(np.isfinite(y)))

    def check_y(self, y):
        """what the observation family asks of the data beyond finiteness: Poisson counts are non-negative integers
        (missing="skip": of the observed entries)"""
        import numpy as np
        if self.obs != "poisson":
            return
        y = np.asarray(y, dtype=np.float64)
        if self.missing == "skip":
            y = y[~np.isnan(y)]                          # the observed entries (+-inf stays among them and is refused)
        if not np.all(np.isfinite(y)):
            raise ValueError("linear_gaussian_mv: obs=\"poisson\": y contains non-finite values")
        if np.any(y < 0):
            raise ValueError("linear_gaussian_mv: obs=\"poisson\": y contains negative values (counts must be >= 0)")
        if np.any(y != np.floor(y)):
            raise ValueError("linear_gaussian_mv: obs=\"poisson\": y contains fractional values (counts must be integers)")

    def _set(self, pieces, into=None):
        import numpy as np
        tgt = self.pieces if into is None else into
        for k, v in pieces.items():
            if k == "P0":
                tgt["L0"] = np.linalg.cholesky(np.atleast_2d(np.asarray(v, dtype=np.float64)))
            elif k == "Q":
                tgt["L"] = np.linalg.cholesky(np.atleast_2d(np.asarray(v, dtype=np.float64)))
            elif k in self.pieces:
                tgt[k] = float(v) if k == "c0" else np.asarray(v, dtype=np.float64)
            else:
                raise TypeError("linear_gaussian_mv: unknown piece %r" % k)

    def pack(self, params):
        """the packed parameter block of include/bayesssm_amd.h (BSSM_MODEL_LGMV) for one parameter draw (the time-varying
        arrays `build` may return are data next to y, not part of the block: see tv_arrays)"""
        import numpy as np
        q = dict(self.pieces)
        if self.build is not None:
            self._set(self._built(params)[0], into=q)
        d, p = self.dim, self.p
        shapes = {"m0": (d,), "L0": (d, d), "A": (d, d), "b": (d,), "L": (d, d), "H": (p, d), "h0": (p,), "sd": (p,)}
        parts = [np.array([d, p], dtype=np.float64)]
        for k in ("m0", "L0", "A", "b", "L"):
            parts.append(np.broadcast_to(np.asarray(q[k], dtype=np.float64), shapes[k]).reshape(-1))
        parts[2] = np.tril(parts[2].reshape(d, d)).reshape(-1)          # (lower triangles: what a Cholesky factor is)
        parts[5] = np.tril(parts[5].reshape(d, d)).reshape(-1)
        parts.append(np.array([q["c0"]], dtype=np.float64))
        for k in ("H", "h0", "sd"):
            parts.append(np.broadcast_to(np.asarray(q[k], dtype=np.float64), shapes[k]).reshape(-1))
        return np.ascontiguousarray(np.concatenate(parts))


def linear_gaussian_mv(d, p=0, build=None, param_names=(), time_varying=None, obs="gaussian", missing="refuse", **pieces):
    return LinearGaussianMV(d, p, build, param_names, time_varying=time_varying, obs=obs, missing=missing, **pieces)


class ReactionNetwork:
    """Mass-action reaction network on the device (SEIR, SIRS, births and deaths, two strains, Lotka-Volterra, ...): d <= 8 species
    held as integer-valued doubles, R <= 8 reactions of order 0, 1 or 2, p <= 8 Poisson observation components.

        init_fn            every particle starts at x0
        transition_fn      one unit of time of Gillespie's direct method, as the built-in SIR runs its day: propensities
                           k (no reactant), k x[a] (one), (k x[a]) x[b] (two different species; A + A is refused), summed in the
                           order of `reactions`; rate constants arrive already scaled (SIR: beta = lambda / n_total)
        log_likelihood_fn  sum_k dpois(y_k, sum_c G_kc x_c, log = TRUE)
        aux_log_likelihood_fn  the same density at the one-unit Euler mean x + sum_r nu_r a_r(x), clamped at 0

    species    names, e.g. ("S", "E", "I", "R")
    reactions  triples (reactants, products, rate): dicts species -> count and a parameter name or a number,
               e.g. ({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"); a two-reactant propensity multiplies in the order the reactants are written
    x0         initial counts, one per species
    observe    G as a p x d matrix, or one {"I": rho} per observation component (a single dict: p = 1)
    counters   names of species that are set to 0.0 at the start of every observation interval (incidence): write the counter as an
               ordinary product of the reaction to be counted -- ({"E": 1}, {"I": 1, "C": 1}, "sigma") -- and observe it;
               y_t ~ Poisson(rho * firings since the previous report).  transition_fn(particles, t) zeroes the counters before its
               Gillespie loop if and only if it is the first call of the gap loop (t == prev_t + 1): over an obs_times gap a counter
               accumulates over the whole gap, at a repeated observation time nothing is reset, and the auxiliary filter's
               second-stage transition never resets (under the APF a counter spans gap + 1 units, the reference's double
               transition).  A counter may not be a reactant.  The state estimate and the histories report it like any species.
    missing    what a NaN in y means (+-inf is refused always): "refuse" (default) an error; "skip" component k of that observation
               was not observed -- the log-likelihood (and the APF look-ahead) sums over the observed components only, a row with
               nothing observed weighs every particle 0.0
    rate_schedule  time-varying rates (school terms, a season, a lockdown): multipliers M[n_times, R], finite and >= 0.  The
               transition TO absolute time tau runs with the rates k_r * M[tau - 1, r] (tau = prev_t + step in an obs_times gap;
               the observation's time for the auxiliary filter's second-stage transition and its look-ahead), so n_times must
               reach the last observation time.  Either the array, or a dict from a rate name or a reaction index to a vector
               [n_times]: reactions not named get 1.0, a name shared by several reactions applies to all of them.  A schedule of
               ones changes no bit of any output.  A multiplier of 0.0 switches a reaction off: writing a reaction twice with
               the rates "beta1", "beta2" and 0 / 1 indicator columns gives piecewise-constant learnable rates from a schedule
               that does not depend on the parameters.
    obs        the observation family: "poisson" (default), or "negbin" for overdispersed counts,
               y_k ~ NegBin(mean = mu_k, size = size_k) with variance mu + mu^2 / size: mu_k is the Poisson family's lambda_k (for the
               look-ahead at the Euler mean, clamped at 0), and the density is dnbinom(y, size = size_k, mu = mu_k, log = TRUE) as
               DESIGN.md section 1d states it.  Everything else (counters, missing, rate_schedule, obs_times) is as for "poisson".
    size       obs="negbin" only, and required there: the dispersion, a number or a parameter name for all p components, or a sequence
               of p of them; finite and > 0 (checked per draw).  Named sizes are parameters like named rates: they join param_order
               and are formals of log_likelihood_fn and aux_log_likelihood_fn, so pmmh learns them next to the rates.
    method     the transition: "gillespie" (default), Gillespie's direct method -- exact, one draw per event, so a unit of time in a
               population of n costs O(n) and stops silently at 2^20 events; or "tau_leap" for large populations: leaps=K leaps per
               unit of time, each with the propensities a_r of its start held fixed and, for r = 0 .. R-1 in order, n_r ~ Poisson(a_r / K)
               firings, cut at the smallest count among the species the reaction consumes (as the earlier reactions of the leap left
               them: no count goes below 0).  O(K R) per particle and unit of time whatever the population; biased for small K
               (DESIGN.md section 1d has a table for choosing K).  The Poisson sampler is inversion below lam = 10 and Hoermann's
               PTRS from there.  Densities, look-ahead, counters, missing, rate_schedule, obs_times and obs are as for "gillespie";
               the packed block is the same, K travels as the context option rn_leaps for the length of each library call.
               Or "euler_multinomial", the discretisation that pomp's reulermultinom made the default for compartmental models: per
               leap (leaps=K of them per unit of time, each from the state at its start) every individual of a compartment leaves
               with probability 1 - exp(-H / K), H the sum of the per-capita hazards of the compartment's exits (k, or k x[b] for an
               exit S + b -> ... + b that b catalyses), and the leavers are split over the exits multinomially, as a chain of
               conditional binomial draws.  Nothing goes negative, nothing is cut, and competing exits (I -> R next to I -> 0) are
               treated alike whatever the order they are written in; the mean of a linear death process is exact at any K.
               Reactions that consume nothing (0 -> A, X -> 2X) keep Poisson counts.  A reaction that consumes BOTH of its reactants
               (A + B -> C) has no place in this scheme and is refused: use "tau_leap".  The binomial sampler is inversion below a
               mean of 10 and Hoermann's BTRS from there (DESIGN.md section 1d states all of it).  K travels as rn_leaps, the method
               as the context option rn_method, both for the length of each library call.
    leaps      method="tau_leap" and method="euler_multinomial" only, and required there: an integer K, 1 <= K <= 1024.  `build` cannot
               change method or leaps.
    noise      method="euler_multinomial" only: gamma white noise on the rates (extra-demographic or environmental stochasticity; He,
               Ionides and King 2010, pomp's rgammawn next to reulermultinom), a non-empty dict {key: sigma}.  A key is a rate name or a
               reaction index, as in rate_schedule: all reactions whose rate is that name form one noise group and share one draw per
               leap (environmental noise is common to every stratum that the same beta infects); an index names a group of one; no
               reaction may be named twice.  A value is a number or a parameter name, finite and > 0 (checked per draw); a named sigma
               is a parameter like a named rate or a named size: it joins param_order, so pmmh learns it next to the rates.  Per leap
               the integrated hazard of a reaction of group g is h_r * w_g instead of h_r / K, w_g = sigma^2 Gamma(shape = 1 / (K sigma^2)):
               mean 1 / K, variance sigma^2 / K (DESIGN.md section 1d states the transition and the sampler, Marsaglia and Tsang's).
               Densities and the APF look-ahead are unchanged.  The packed block carries lead[R], sigma[R] after G (after size[p]
               with obs="negbin"); the method travels as the context options rn_method = 1 with rn_noise = 1.
    build(**params) may return "rates" (dict name -> value, or the full list), "x0", "G", "size" (a number, p numbers, or a dict name -> value),
    "noise_sigma" (a number for every group, or a dict noise key -> value)
    and "rate_schedule" (in the forms above,
    replacing the constructor's for that draw: an intervention effect applied from day 30, say; n_times is the constructor's if it
    gave a schedule, and the draws of one batched call or pmmh step must all give the same block length: pack_many raises a ValueError) for the draw; without it the named rates are the parameters themselves.  With d = 2 and the two SIR reactions
    the outputs equal models.sir()'s bit for bit."""

    MISSING = ("refuse", "skip")
    OBS = ("poisson", "negbin")
    METHODS = ("gillespie", "tau_leap", "euler_multinomial")
    MAX_LEAPS = 1024

    @property
    def rn_leaps(self):
        """the value of the context option rn_leaps for this descriptor's library calls: K, or 0 for Gillespie's direct method"""
        return self.leaps or 0

    @property
    def rn_method(self):
        """the method of this descriptor's library calls as Context.rn_method takes it: 1 for Euler-multinomial leaps, 2 for the same
        with gamma white noise on the rates (the context options rn_method = 1 and rn_noise = 1), else 0"""
        return (2 if self.noise is not None else 1) if self.method == "euler_multinomial" else 0

    def _noise(self, spec):
        """noise= as {group key: sigma} in the order given, checked, with the groups: noise_lead[r] = the lowest reaction index of r's
        group or -1, noise_key[r] = the key of r's group or None"""
        import numpy as np
        if self.method != "euler_multinomial":
            raise ValueError("reaction_network: noise (gamma white noise on the rates) needs method='euler_multinomial'")
        if not isinstance(spec, dict):
            raise ValueError("reaction_network: noise is a dict from a rate name or a reaction index to sigma (a number or a parameter name)")
        if not spec:
            raise ValueError("reaction_network: noise is empty: name at least one rate or reaction, or leave noise out")
        R = self.R
        self.noise_lead, self.noise_key, out = [-1] * R, [None] * R, {}
        for key, v in spec.items():
            if isinstance(key, str):
                hit = [r for r in range(R) if self.rates[r] == key]
                if not hit:
                    raise ValueError("reaction_network: noise names the unknown rate %r" % (key,))
            elif isinstance(key, (int, np.integer)) and not isinstance(key, bool):
                if not 0 <= key < R:
                    raise ValueError("reaction_network: noise names the unknown reaction index %r (0 .. %d)" % (key, R - 1))
                key = int(key)
                hit = [key]
            else:
                raise ValueError("reaction_network: noise names the unknown rate %r" % (key,))
            for r in hit:
                if self.noise_lead[r] >= 0:
                    raise ValueError("reaction_network: noise names reaction %d twice (through %r and %r)" % (r, self.noise_key[r], key))
                self.noise_lead[r], self.noise_key[r] = hit[0], key
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (str, int, float, np.integer, np.floating)):
                raise ValueError("reaction_network: a noise sigma is a number or a parameter name, got %r" % (v,))
            out[key] = v if isinstance(v, str) else float(v)
        self._check_sigma([1.0 if isinstance(v, str) else v for v in out.values()])
        return out

    @staticmethod
    def _check_sigma(sigma):
        import numpy as np
        sigma = np.asarray(sigma, dtype=np.float64)
        if not (np.all(np.isfinite(sigma)) and np.all(sigma > 0)):
            raise ValueError("reaction_network: a noise sigma must be finite and > 0")

    def _check_euler_multinomial(self):
        """the method's classification on the descriptor: every reaction has one source -- the one reactant it
        consumes; another reactant is a catalyst -- or consumes nothing"""
        for r in range(self.R):
            consumed = [c for c in (self.s1[r], self.s2[r]) if c >= 0 and self.nu[r, c] < 0]
            if len(consumed) == 2:
                raise ValueError("reaction_network: reaction %d consumes both of its reactants (%s + %s -> ...); method='euler_multinomial' splits the "
                                 "leavers of ONE compartment over its exits and has no place for it -- use method='tau_leap' for this network"
                                 % (r, self.species[consumed[0]], self.species[consumed[1]]))

    def __init__(self, species, reactions, x0, observe, build=None, param_names=(), counters=(), missing="refuse", rate_schedule=None,
                 obs="poisson", size=None, method="gillespie", leaps=None, noise=None):
        import numpy as np
        if missing not in self.MISSING:
            raise ValueError("reaction_network: missing must be one of 'refuse', 'skip'")
        if method not in self.METHODS:
            raise ValueError("reaction_network: method must be one of 'gillespie', 'tau_leap', 'euler_multinomial'")
        if leaps is not None and method == "gillespie":
            raise ValueError("reaction_network: leaps is the number of tau-leaps per unit of time; it needs method='tau_leap' or method='euler_multinomial'")
        if leaps is None and method != "gillespie":
            raise ValueError("reaction_network: method='%s' needs leaps (an integer K, 1 <= K <= %d)" % (method, self.MAX_LEAPS))
        if leaps is not None:
            if isinstance(leaps, (bool, np.bool_)):
                raise ValueError("reaction_network: leaps must be an integer count, not a bool")
            if not isinstance(leaps, (int, np.integer)):
                raise ValueError("reaction_network: leaps must be an integer, got %r" % (leaps,))
            if not 1 <= int(leaps) <= self.MAX_LEAPS:
                raise ValueError("reaction_network: leaps must lie in 1 .. %d, got %d" % (self.MAX_LEAPS, int(leaps)))
        self.method, self.leaps = method, (None if leaps is None else int(leaps))
        if obs not in self.OBS:
            raise ValueError("reaction_network: obs must be one of 'poisson', 'negbin'")
        if size is not None and obs != "negbin":
            raise ValueError("reaction_network: size is the negative-binomial dispersion; it needs obs='negbin'")
        if size is None and obs == "negbin":
            raise ValueError("reaction_network: obs='negbin' needs size (a number or a parameter name, or one per observation component)")
        self.missing, self.obs = missing, obs
        self.species = tuple(species)
        d, R = len(self.species), len(reactions)
        if not 1 <= d <= 8 or len(set(self.species)) != d:
            raise ValueError("reaction_network: 1 <= d <= 8 distinct species")
        if not 1 <= R <= 8:
            raise ValueError("reaction_network: 1 <= R <= 8 reactions")
        idx = {s: c for c, s in enumerate(self.species)}
        self.s1, self.s2, self.rates = [], [], []
        self.nu = np.zeros((R, d))
        for r, rx in enumerate(reactions):
            if len(rx) != 3:
                raise ValueError("reaction_network: a reaction is a triple (reactants, products, rate)")
            lhs, rhs, rate = rx
            for side in (lhs, rhs):
                for s, n in side.items():
                    if s not in idx:
                        raise ValueError("reaction_network: unknown species %r in reaction %d" % (s, r))
                    if n != int(n) or n < 0:
                        raise ValueError("reaction_network: stoichiometric counts are non-negative integers")
            used = [idx[s] for s, n in lhs.items() if n > 0]
            if any(n > 1 for n in lhs.values()):
                raise ValueError("reaction_network: reaction %d takes more than one molecule of a species (s1 == s2); dimerisation and higher orders are not supported" % r)
            if len(used) > 2:
                raise ValueError("reaction_network: reaction %d has more than two reactants" % r)
            self.s1.append(used[0] if len(used) > 0 else -1)
            self.s2.append(used[1] if len(used) > 1 else -1)
            for s, n in lhs.items():
                self.nu[r, idx[s]] -= int(n)
            for s, n in rhs.items():
                self.nu[r, idx[s]] += int(n)
            self.rates.append(rate if isinstance(rate, str) else float(rate))
        if isinstance(observe, dict):
            observe = [observe]
        if len(observe) and all(isinstance(o, dict) for o in observe):
            G = np.zeros((len(observe), d))
            for k, o in enumerate(observe):
                for s, v in o.items():
                    if s not in idx:
                        raise ValueError("reaction_network: unknown species %r in observe" % (s,))
                    G[k, idx[s]] = float(v)
        else:
            G = np.atleast_2d(np.asarray(observe, dtype=np.float64))
        if G.ndim != 2 or G.shape[1] != d or not 1 <= G.shape[0] <= 8:
            raise ValueError("reaction_network: observe gives 1 <= p <= 8 components over the %d species" % d)
        self.G = G
        self.x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
        if self.x0.shape != (d,):
            raise ValueError("reaction_network: x0 holds one count per species (%d)" % d)
        self.name, self.dim, self.R, self.p = "rnet", d, R, int(G.shape[0])
        if method == "euler_multinomial":
            self._check_euler_multinomial()
        self.counters = (counters,) if isinstance(counters, str) else tuple(counters)
        self.reset = np.zeros(d)
        for s in self.counters:
            if s not in idx:
                raise ValueError("reaction_network: unknown species %r in counters" % (s,))
            if self.reset[idx[s]] != 0.0:
                raise ValueError("reaction_network: counter %r is named twice" % (s,))
            if idx[s] in self.s1 or idx[s] in self.s2:
                raise ValueError("reaction_network: counter %r is a reactant of reaction %d (the reset would change the dynamics)"
                                 % (s, [r for r in range(R) if idx[s] in (self.s1[r], self.s2[r])][0]))
            self.reset[idx[s]] = 1.0
        self.rate_schedule = None if rate_schedule is None else self._schedule(rate_schedule)
        self.size = None
        if obs == "negbin":
            entries = list(size) if isinstance(size, (list, tuple, np.ndarray)) else [size] * self.p
            if len(entries) != self.p:
                raise ValueError("reaction_network: size holds one entry for all or one per observation component (%d), got %d" % (self.p, len(entries)))
            self.size = [q if isinstance(q, str) else float(q) for q in entries]
            self._check_size([1.0 if isinstance(q, str) else q for q in self.size])
        self.noise = None if noise is None else self._noise(noise)
        self.build, self.constants = build, ()
        named = [q for q in self.rates if isinstance(q, str)]
        named_sizes = [q for q in (self.size or ()) if isinstance(q, str)]
        named_sigmas = [q for q in (self.noise or {}).values() if isinstance(q, str)]
        self.param_order = tuple(param_names) if (build is not None or param_names) else tuple(dict.fromkeys(named + named_sizes + named_sigmas))
        self.has_param_tv = False
        # (the density reads the sizes: the named ones, or with a `build` -- which may return "size" from any parameter -- all of them)
        lik = () if obs != "negbin" else self.param_order if build is not None else tuple(dict.fromkeys(named_sizes))
        self.init_fn = ModelFn("rnet", "init", ())
        self.transition_fn = ModelFn("rnet", "transition", self.param_order)
        self.log_likelihood_fn = ModelFn("rnet", "log_likelihood", lik)
        self.aux_log_likelihood_fn = ModelFn("rnet", "aux_log_likelihood", self.param_order)
        for fn in (self.init_fn, self.transition_fn, self.log_likelihood_fn, self.aux_log_likelihood_fn):
            fn.owner = self
        self._check_block(self.x0, [0.0 if isinstance(q, str) else q for q in self.rates], self.G)

    @staticmethod
    def _check_block(x0, k, G):
        import numpy as np
        if not (np.all(np.isfinite(x0)) and np.all(np.isfinite(k)) and np.all(np.isfinite(G))):
            raise ValueError("reaction_network: x0, the rates and G must be finite")
        if np.any(np.asarray(k) < 0):
            raise ValueError("reaction_network: rate constants must be >= 0")

    @staticmethod
    def _check_size(size):
        import numpy as np
        size = np.asarray(size, dtype=np.float64)
        if not (np.all(np.isfinite(size)) and np.all(size > 0)):
            raise ValueError("reaction_network: size (the negative-binomial dispersion) must be finite and > 0")

    def _schedule(self, spec):
        """rate_schedule as the array M[n_times, R], checked: from the array itself, or from a dict rate name | reaction index ->
        vector [n_times] (1.0 for the reactions not named)"""
        import numpy as np
        R = self.R
        if isinstance(spec, dict):
            cols = {}
            for key, v in spec.items():
                if isinstance(key, str):
                    hit = [r for r in range(R) if self.rates[r] == key]
                    if not hit:
                        raise ValueError("reaction_network: rate_schedule names the unknown rate %r" % (key,))
                elif isinstance(key, (int, np.integer)) and not isinstance(key, bool):
                    if not 0 <= key < R:
                        raise ValueError("reaction_network: rate_schedule names the unknown reaction index %r (0 .. %d)" % (key, R - 1))
                    hit = [int(key)]
                else:
                    raise ValueError("reaction_network: rate_schedule names the unknown rate %r" % (key,))
                v = np.asarray(v, dtype=np.float64)
                if v.ndim != 1 or v.size < 1:
                    raise ValueError("reaction_network: rate_schedule has the wrong shape: a dict holds one vector [n_times] per entry")
                for r in hit:
                    cols[r] = v
            if not cols or len({v.size for v in cols.values()}) != 1:
                raise ValueError("reaction_network: rate_schedule has the wrong shape: the vectors of a dict have one length n_times >= 1")
            M = np.ones((next(iter(cols.values())).size, R))
            for r, v in cols.items():
                M[:, r] = v
        else:
            M = np.array(spec, dtype=np.float64)
            if M.ndim != 2 or M.shape[0] < 1 or M.shape[1] != R:
                raise ValueError("reaction_network: rate_schedule has the wrong shape: an array [n_times, %d] with n_times >= 1" % R)
        if not np.all(np.isfinite(M)) or np.any(M < 0):
            raise ValueError("reaction_network: rate_schedule multipliers must be finite and >= 0")
        return np.ascontiguousarray(M)

    def _base_size(self):
        # d, R, p, x0, k, s1, s2, nu, G [, size] [, lead, sigma]
        return (3 + self.dim + 3 * self.R + self.R * self.dim + self.p * self.dim + (self.p if self.obs == "negbin" else 0)
                + (2 * self.R if self.noise is not None else 0))

    def n_theta(self):
        """the length of this descriptor's packed block, or None when only pack() can tell (a `build` that may return a schedule).
        The descriptor keeps no memory of earlier packs: the draws of ONE call are compared with each other (pack_many)."""
        if self.rate_schedule is not None:
            return self._base_size() + self.dim + 1 + self.rate_schedule.size
        return None if self.build is not None else self._base_size() + (self.dim if self.counters else 0)

    def n_theta_ok(self, n):
        """whether a packed block of length n can be this descriptor's"""
        want = self.n_theta()
        if want is not None:
            return n == want
        tail = n - self._base_size() - self.dim - 1
        return n == self._base_size() + (self.dim if self.counters else 0) or (tail >= self.R and tail % self.R == 0)

    def check_times(self, n_theta, T, obs_times=None):
        """the schedule of a block of length n_theta (if it has one) must reach the last observation time (T without obs_times)"""
        tail = int(n_theta) - self._base_size() - self.dim - 1
        if tail < self.R or T < 1:
            return
        last = int(obs_times[-1]) if obs_times is not None and len(obs_times) else int(T)
        if tail // self.R < last:
            raise ValueError("reaction_network: rate_schedule has n_times = %d rows, short of the last observation time %d" % (tail // self.R, last))

    def rw_move_fn(self, sd=0.1):
        raise ValueError("reaction_network: resample_move_filter (RMPF) is not available: a move on integer states is not defined")

    def y_ok(self, y):
        """the host's finiteness check of y for this descriptor: no NaN and no +-inf; missing="skip" lets NaN through"""
        import numpy as np
        y = np.asarray(y, dtype=np.float64)
        return bool(np.all(np.isfinite(y) | np.isnan(y))) if self.missing == "skip" else bool(np.all(np.isfinite(y)))

    def check_y(self, y):
        """the counts the Poisson density asks for (the Poisson observation family's checks and wording); missing="skip": of the
        observed entries"""
        import numpy as np
        y = np.asarray(y, dtype=np.float64)
        if self.missing == "skip":
            y = y[~np.isnan(y)]                          # the observed entries (+-inf stays among them and is refused)
        if not np.all(np.isfinite(y)):
            raise ValueError("reaction_network: y contains non-finite values")
        if np.any(y < 0):
            raise ValueError("reaction_network: y contains negative values (counts must be >= 0)")
        if np.any(y != np.floor(y)):
            raise ValueError("reaction_network: y contains fractional values (counts must be integers)")

    def pack(self, params=None):
        """the packed parameter block of include/bayesssm_amd.h (BSSM_MODEL_RNET; obs="negbin": BSSM_MODEL_RNET_NB) for one parameter draw:
        d, R, p, x0[d], k[R], s1[R], s2[R], nu[R][d], G[p][d], with obs="negbin" size[p], with noise= lead[R], sigma[R] (lead[r]: the lowest
        reaction index of r's noise group or -1; sigma[r]: the group's sigma or 0.0), and with counters the tail reset[d] of 0.0 / 1.0
        (without: no tail); with a rate schedule reset[d] always (zeros without counters), then n_times, M[n_times][R]"""
        import numpy as np
        params = dict(params or {})
        missing = [k for k in self.param_order if k not in params]
        if missing:
            raise TypeError('argument "%s" is missing, with no default' % missing[0])
        x0, G, named = self.x0, self.G, {k: float(params[k]) for k in self.param_order}
        rates, sched, sizes, sigmas = None, self.rate_schedule, None, None
        if self.build is not None:
            built = dict(self.build(**named))
            unknown = set(built) - {"rates", "x0", "G", "rate_schedule", "size", "noise_sigma"}
            if unknown:
                raise TypeError("reaction_network: build may return 'rates', 'x0', 'G', 'size', 'noise_sigma' and 'rate_schedule', got %r" % sorted(unknown)[0])
            sigmas = built.get("noise_sigma")
            if sigmas is not None and self.noise is None:
                raise ValueError("reaction_network: build returned noise_sigma; it needs noise=")
            sizes = built.get("size")
            if sizes is not None and self.obs != "negbin":
                raise ValueError("reaction_network: build returned size, the negative-binomial dispersion; it needs obs='negbin'")
            if built.get("rate_schedule") is not None:
                sched = self._schedule(built["rate_schedule"])
            if "x0" in built:
                x0 = np.asarray(built["x0"], dtype=np.float64).reshape(-1)
            if "G" in built:
                G = np.atleast_2d(np.asarray(built["G"], dtype=np.float64))
            if x0.shape != (self.dim,) or G.shape != (self.p, self.dim):
                raise ValueError("reaction_network: build returned x0 / G of the wrong shape")
            rates = built.get("rates")
            if rates is not None and not isinstance(rates, dict):
                rates = [float(v) for v in rates]
                if len(rates) != self.R:
                    raise ValueError("reaction_network: build returned %d rates for %d reactions" % (len(rates), self.R))
        if isinstance(rates, list):
            k = rates
        else:
            look = dict(named, **(rates or {}))
            k = []
            for q in self.rates:
                if isinstance(q, str) and q not in look:
                    raise TypeError('argument "%s" is missing, with no default' % q)
                k.append(float(look[q]) if isinstance(q, str) else q)
        self._check_block(x0, k, G)
        tails = []
        if self.obs == "negbin":                              # size[p] directly after G, in front of the tails
            if isinstance(sizes, dict) or sizes is None:
                look = dict(named, **(sizes or {}))
                sz = []
                for q in self.size:
                    if isinstance(q, str) and q not in look:
                        raise TypeError('argument "%s" is missing, with no default' % q)
                    sz.append(float(look[q]) if isinstance(q, str) else q)
            else:
                sz = [float(v) for v in np.asarray(sizes, dtype=np.float64).reshape(-1)]
                sz = sz * self.p if len(sz) == 1 else sz
                if len(sz) != self.p:
                    raise ValueError("reaction_network: build returned %d sizes for %d observation components" % (len(sz), self.p))
            self._check_size(sz)
            tails.append(np.asarray(sz, dtype=np.float64))
        if self.noise is not None:                            # lead[R], sigma[R] after size[p], in front of the tails
            if sigmas is not None and not isinstance(sigmas, dict):
                sigmas = {key: float(sigmas) for key in self.noise}
            unknown = set(sigmas or {}) - set(self.noise)
            if unknown:
                raise ValueError("reaction_network: build returned noise_sigma for %r, which noise= does not name" % (sorted(unknown, key=str)[0],))
            look, sg = dict(named), {}
            for key, q in self.noise.items():
                if key in (sigmas or {}):
                    sg[key] = float(sigmas[key])
                elif isinstance(q, str):
                    if q not in look:
                        raise TypeError('argument "%s" is missing, with no default' % q)
                    sg[key] = float(look[q])
                else:
                    sg[key] = q
            self._check_sigma(list(sg.values()))
            tails.append(np.asarray(self.noise_lead, dtype=np.float64))
            tails.append(np.asarray([0.0 if key is None else sg[key] for key in self.noise_key], dtype=np.float64))
        if self.counters or sched is not None:
            tails.append(self.reset)
        if sched is not None:
            tails += [np.array([sched.shape[0]], dtype=np.float64), sched.reshape(-1)]
        block = np.ascontiguousarray(np.concatenate([
            np.array([self.dim, self.R, self.p], dtype=np.float64), x0, np.asarray(k, dtype=np.float64),
            np.asarray(self.s1, dtype=np.float64), np.asarray(self.s2, dtype=np.float64), self.nu.reshape(-1), G.reshape(-1)] + tails))
        if sched is not None and self.rate_schedule is not None and sched.shape != self.rate_schedule.shape:
            raise ValueError("reaction_network: n_theta changed between draws: build returned a rate_schedule of n_times = %d, the "
                             "constructor's has %d" % (sched.shape[0], self.rate_schedule.shape[0]))
        return block

    def pack_many(self, draws):
        """the blocks of the parameter draws of one call (a batched launch, the chains of a pmmh step) as an (F, n_theta) array; every
        draw must give the same n_theta: a rate_schedule returned by build keeps its n_times and is returned for every draw or for none"""
        import numpy as np
        blocks = [self.pack(q) for q in draws]
        sizes = [b.size for b in blocks]
        if len(set(sizes)) > 1:
            k = next(i for i, n in enumerate(sizes) if n != sizes[0])
            raise ValueError("reaction_network: n_theta changed between draws (%d, then %d at draw %d): a rate_schedule returned by build "
                             "keeps its n_times, and is returned for every draw or for none" % (sizes[0], sizes[k], k))
        return np.ascontiguousarray(np.array(blocks, dtype=np.float64).reshape(len(blocks), -1))


def reaction_network(species, reactions, x0, observe, build=None, param_names=(), counters=(), missing="refuse", rate_schedule=None,
                     obs="poisson", size=None, method="gillespie", leaps=None, noise=None):
    return ReactionNetwork(species, reactions, x0, observe, build, param_names, counters=counters, missing=missing, rate_schedule=rate_schedule,
                           obs=obs, size=size, method=method, leaps=leaps, noise=noise)


def linear_gaussian():
    """x0 ~ N(0,1); x' = phi x + N(0, sigma_x); y ~ N(x, sigma_y)
    (tests/testthat/test-pmmh_tuning.R:163-173 with free sigma_x, sigma_y; BASELINE C2/C3/C5)."""
    return Model("lg", linear_gaussian.__doc__)


def ar1_sin():
    """x0 ~ N(0,1); x' = phi x + sin(x) + N(0, sigma_x); y ~ N(x, sigma_y)   (README.md:137-146; BASELINE C1)."""
    return Model("ar1sin", ar1_sin.__doc__)


def resolve(init_fn, transition_fn, log_likelihood_fn, aux_log_likelihood_fn=None):
    """Check that the functions are descriptors of ONE built-in model and return its name."""
    fns = [("init_fn", init_fn, "init"), ("transition_fn", transition_fn, "transition"),
           ("log_likelihood_fn", log_likelihood_fn, "log_likelihood")]
    if aux_log_likelihood_fn is not None:
        fns.append(("aux_log_likelihood_fn", aux_log_likelihood_fn, "aux_log_likelihood"))
    for name, fn, role in fns:
        if not isinstance(fn, ModelFn):
            raise TypeError(
                "%s must be a built-in model descriptor from bayesssm_amd.models (arbitrary closures cannot run "
                "on the GPU; see DESIGN.md, 'user closures')" % name)
        if fn.role != role:
            raise ValueError("%s is a %s function, expected %s" % (name, fn.role, role))
    names = {fn.model for _, fn, _ in fns}
    if len(names) != 1:
        raise ValueError("init_fn, transition_fn and log_likelihood_fn belong to different models: %s" % sorted(names))
    return names.pop()


def theta_from_kwargs(fns, kwargs):
    """Collect the model's parameter vector from the named arguments the functions read
    (lg / ar1sin: phi, sigma_x, sigma_y;  sir: lambda, gamma, then the constants n_total, s0, i0)."""
    kwargs = dict(kwargs)
    if "lambda_" in kwargs:                       # `lambda` is a Python keyword
        kwargs["lambda"] = kwargs.pop("lambda_")
    needed = []
    for fn in fns:
        for p in fn.params:
            if p not in needed:
                needed.append(p)
    for p in needed:
        if p not in kwargs:
            raise TypeError('argument "%s" is missing, with no default' % p)   # R's message for a missing closure arg
    owner = getattr(fns[0], "owner", None)
    if owner is not None:
        return [float(kwargs.get(p, 1.0)) for p in owner.param_order] + list(owner.constants)
    return [float(kwargs.get(p, 1.0)) for p in Model.PARAM_ORDER]


def dim_of(model_name):
    return 2 if model_name == "sir" else 1            # ("lgmv": the dimension is the descriptor's, see filters.particle_filter_core)
