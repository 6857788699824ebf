"""What gamma white noise on the rates (models.reaction_network(..., method="euler_multinomial", leaps=K, noise={...})) changes in the numpy
restatement of the Euler-multinomial transition (tests/rnet_em_restated.py), from the definition in DESIGN.md section 1d and the head of
bayesssm_amd/csrc/rnet.hip.h alone.  fp64, in the order written; exp, log, log1p, expm1 are the C library's (math.*), element by element.

  block           lead[R], sigma[R] directly after G (after size[p] in a negative-binomial block), in front of the tails: lead[r] = -1 or the
                  lowest reaction index of r's noise group, sigma[r] the group's sigma.  strip() takes them out, so that every other
                  restatement reads the block it knows.
  transition      the Euler-multinomial transition with the integrated per-capita hazard of reaction r over leap l = h_r * w_r:
                    r in group g:  s2 = sigma_g * sigma_g;  sh = 1 / (K * s2);  w_r = s2 * rgamma(sh)      (one draw per particle, call, leap, group)
                    otherwise:     w_r = 1 / K
                    1. hw_r = h_r * w_r;  H = 0.0 + hw_{r_1} + hw_{r_2} + ...;  not H > 0: nothing drawn;  pe = -expm1(-H);  p_i = (hw_{r_i} / H) * pe;
                       clamp, rbinom, rem, prem as rnet_em_restated
                    2. sourceless r:  n = rpois(a_r * w_r)
  rgamma(sh)      Marsaglia and Tsang (2000), the normal by inversion (AS 241, PPND16).  Attempt a of leader g in leap l reads the Philox block at
                    (j, call, DRAW_TRANS | (1 << 27) | (((l * RNR + g) << 6 | a) << 8), stream);  u1 = u01(w.x, w.y), u2 = u01(w.z, w.w)
                  boost = sh < 1;  al = sh + 1 if boost else sh;  dd = al - 1 / 3;  cc = 1 / sqrt(9 * dd)
                  attempts a = 0 .. 62:  x = qnorm(u1);  v = 1 + cc * x;  reject if not v > 0;  v = v * v * v;  x2 = x * x
                    accept if u2 < 1 - 0.0331 * (x2 * x2);  otherwise accept if log(u2) < 0.5 * x2 + dd * ((1 - v) + log(v));  result dd * v
                  after 63 rejections the result is dd
                  boost:  result = result * exp(log(ub) / sh),  ub the u1 of the block at a = 63

Everything else -- densities, look-ahead, counters, missing observations, schedule rows, the filter core -- is the other restatements',
untouched: they reach the transition through rnet_restated.make, which gamma_noise(K, lead, sigma) rebinds for the length of a with block.

counts additionally collects, per gamma draw,
  "gamma"                  draws (one per particle, call, leap and group)
  "boost", "plain"         draws at sh < 1 and at sh >= 1
  "squeeze", "full"        attempts accepted by the squeeze and by the full test -- under counts["rgamma"], with
  "rejected", "v<=0"       attempts rejected by the full test and for v <= 0
  "fallback"               draws that ran out of attempts
(counts["rgamma"] is a dict of its own because rnet_em_restated's binomial counts use "squeeze", "full", "rejected" and "fallback" too)."""
import contextlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_em_restated as ER  # noqa: E402
import rnet_leap_restated as LR  # noqa: E402
import rnet_nb_restated as NB  # noqa: E402
import rnet_restated as RN  # noqa: E402
import rnet_tv_restated as RT  # noqa: E402
from rnet_em_restated import RNR, _exp, _expm1, _log, philox4x32_10, u01_from_bits  # noqa: E402
from rnet_restated import DRAW_TRANS, stream_word  # noqa: E402

GWN_BIT = 1 << 27
GKEYS = ("gamma", "boost", "plain", "squeeze", "full", "rejected", "v<=0", "fallback")


def new_counts():
    return {k: 0 for k in GKEYS}


def _horner(coef, r):
    v = coef[0] * r + coef[1]
    for c in coef[2:]:
        v = v * r + c
    return v


_A = (2.5090809287301226727e3, 3.3430575583588128105e4, 6.7265770927008700853e4, 4.5921953931549871457e4, 1.3731693765509461125e4,
      1.9715909503065514427e3, 1.3314166789178437745e2, 3.3871328727963666080e0)
_B = (5.2264952788528545610e3, 2.8729085735721942674e4, 3.9307895800092710610e4, 2.1213794301586595867e4, 5.3941960214247511077e3,
      6.8718700749205790830e2, 4.2313330701600911252e1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e0, 3.64784832476320460504e0,
      5.76949722146069140550e0, 4.63033784615654529590e0, 1.42343711074968357734e0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1, 6.89767334985100004550e-1,
      1.67638483018380384940e0, 2.05319162663775882187e0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2, 2.96560571828504891230e-1,
      1.78482653991729133580e0, 5.46378491116411436990e0, 6.65790464350110377720e0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4, 1.48753612908506148525e-2,
      1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def qnorm_as241(p, branches=None):
    """Wichura's AS 241 (PPND16), the published coefficients: the central branch |p - 0.5| <= 0.425, and the two tail branches on
    r = sqrt(-log(min(p, 1 - p))), r <= 5 and r > 5.  branches: a dict that collects how many arguments took each branch"""
    p = np.asarray(p, dtype=np.float64)
    q = p - 0.5
    out = np.empty(p.shape)
    mid = np.abs(q) <= 0.425
    if mid.any():
        r = 0.180625 - q[mid] * q[mid]
        out[mid] = q[mid] * _horner(_A, r) / _horner(_B, r)
    tail = ~mid
    n_far = 0
    if tail.any():
        qt = q[tail]
        r = np.sqrt(-_log(np.where(qt < 0, p[tail], 1.0 - p[tail])))
        near = r <= 5.0
        n_far = int((~near).sum())
        val = np.empty(r.shape)
        rn, rf = r[near] - 1.6, r[~near] - 5.0
        val[near] = _horner(_C, rn) / _horner(_D, rn)
        val[~near] = _horner(_E, rf) / _horner(_F, rf)
        out[tail] = np.where(qt < 0, -val, val)
    if branches is not None:
        for name, n in (("central", int(mid.sum())), ("near", int(tail.sum()) - n_far), ("far", n_far)):
            branches[name] = branches.get(name, 0) + n
    return out


def gamma_key(lg, a):
    """the third counter word of attempt a for lg = l * RNR + g"""
    return DRAW_TRANS | GWN_BIT | (((lg << 6) | a) << 8)


def uniforms(key, sw, j, call, lg, a):
    w = philox4x32_10(j, call, gamma_key(lg, a), sw, key)
    return u01_from_bits(w[0], w[1]), u01_from_bits(w[2], w[3])


def rgamma(key, sw, j, call, lg, sh, counts=None):
    """the draws of the particles j (an index array) for (call, lg = l * RNR + g) at the shapes sh[i]"""
    sh, j = np.asarray(sh, dtype=np.float64), np.asarray(j, dtype=np.uint64)
    c = counts if counts is not None else new_counts()
    boost = sh < 1.0
    al = np.where(boost, sh + 1.0, sh)
    dd = al - 1.0 / 3.0
    cc = 1.0 / np.sqrt(9.0 * dd)
    res = dd.copy()
    left = np.arange(sh.size)
    c["gamma"] += int(sh.size); c["boost"] += int(boost.sum()); c["plain"] += int((~boost).sum())
    for a in range(63):
        if left.size == 0:
            break
        u1, u2 = uniforms(key, sw, j[left], call, lg, a)
        x = qnorm_as241(u1)
        v = 1.0 + cc[left] * x
        pos = v > 0.0
        v = np.where(pos, v, 1.0)                          # (the rejected ones: any value, not used)
        v = v * v * v
        x2 = x * x
        squeeze = pos & (u2 < 1.0 - 0.0331 * (x2 * x2))
        test = pos & ~squeeze
        ok = np.zeros(left.size, dtype=bool)
        if test.any():
            ok[test] = _log(u2[test]) < 0.5 * x2[test] + dd[left[test]] * ((1.0 - v[test]) + _log(v[test]))
        acc = squeeze | ok
        res[left[acc]] = dd[left[acc]] * v[acc]
        c["squeeze"] += int(squeeze.sum()); c["full"] += int(ok.sum()); c["rejected"] += int((test & ~ok).sum()); c["v<=0"] += int((~pos).sum())
        left = left[~acc]
    c["fallback"] += int(left.size)
    if boost.any():
        i = np.nonzero(boost)[0]
        ub, _ = uniforms(key, sw, j[i], call, lg, 63)
        res[i] = res[i] * _exp(_log(ub) / sh[i])
    return res


def sample(seed, stream, call, leap, g, sh, counts=None):
    """what bssm_dump_rgamma returns: the draws that particles 0 .. len(sh)-1 take for (call, leap, g)"""
    sh = np.asarray(sh, dtype=np.float64).reshape(-1)
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    return rgamma(key, stream_word(stream), np.arange(sh.size), call, leap * RNR + g, sh, counts)


def strip(theta, nb=False):
    """(the block without lead[R], sigma[R], lead as ints, sigma)"""
    th = np.asarray(theta, dtype=np.float64)
    d, nr, p = int(th[0]), int(th[1]), int(th[2])
    o = 3 + d + 3 * nr + nr * d + p * d + (p if nb else 0)
    lead, sigma = th[o:o + nr].astype(int), th[o + nr:o + 2 * nr].copy()
    for r in range(nr):                                    # what the library checks
        assert lead[r] == -1 or (0 <= lead[r] <= r and lead[lead[r]] == lead[r] and sigma[r] > 0.0 and sigma[r] == sigma[lead[r]])
    return np.concatenate([th[:o], th[o + 2 * nr:]]), lead, sigma


_gillespie_make = RN.make


def make(K, lead, sigma, oracle, seed, stream, counts=None):
    """rnet_restated.make with the Euler-multinomial transition of K leaps under gamma white noise; the densities are rnet_restated's"""
    _, ll, aux = _gillespie_make(oracle, seed, stream, counts)
    if counts is not None:
        for name in ER.KEYS:
            counts.setdefault(name, 0)
        counts.setdefault("rpois", LR.new_counts())
        counts.setdefault("rgamma", new_counts())
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    sw = stream_word(stream)

    def transition(q, x, z):
        call = int(z[0, 0])
        x = np.array(x, dtype=np.float64)
        d, nr, N = q["d"], q["R"], x.shape[1]
        kr = [float(v) for v in q["k"]]
        nu = [[float(q["nu"][r, c]) for c in range(d)] for r in range(nr)]
        cls = ER.classify(q)
        j = np.arange(N)
        dK = float(K)

        def hazard(r):
            h = np.full(N, kr[r])
            if cls[r][1] >= 0:
                h = h * x[cls[r][1]]
            return np.where(h > 0.0, h, 0.0)

        for leap in range(K):
            drawn = {}                                     # (the draw is a pure function of its key: one per leader and leap)

            def weight(r):
                g = int(lead[r])
                if g < 0:
                    return np.full(N, 1.0 / dK)
                if g not in drawn:
                    s2 = float(sigma[r]) * float(sigma[r])
                    sh = 1.0 / (dK * s2)
                    drawn[g] = s2 * rgamma(key, sw, j, call, leap * RNR + g, np.full(N, sh), counts["rgamma"] if counts is not None else None)
                return drawn[g]

            xn = x.copy()
            for c in range(d):
                group = [r for r in range(nr) if cls[r][0] == c]
                if not group:
                    continue
                H = np.zeros(N)
                for r in group:
                    H = H + hazard(r) * weight(r)
                live = H > 0.0
                Hl = np.where(live, H, 1.0)              # (the particles with not H > 0 draw nothing: their q is put at 0.0 below)
                pe = -_expm1(-Hl)
                rem, prem = x[c].copy(), np.ones(N)
                for r in group:
                    p = ((hazard(r) * weight(r)) / Hl) * pe
                    with np.errstate(divide="ignore", invalid="ignore"):
                        qv = p / prem
                    qv = np.where(qv > 0.0, qv, 0.0)
                    qv = np.where(qv > 1.0, 1.0, qv)
                    qv = np.where(live, qv, 0.0)
                    sub = ER.new_counts() if counts is not None else None
                    n = ER.rbinom(key, sw, j, call, leap * RNR + r, rem, qv, sub)
                    if counts is not None:               # (a particle with not H > 0 makes no draw at all: it is no "zero" either)
                        sub["zero"] -= int((~live).sum())
                        for name in ER.KEYS:
                            counts[name] += sub[name]
                    rem = rem - n
                    prem = prem - p
                    for c2 in range(d):
                        xn[c2] = xn[c2] + nu[r][c2] * n
            for r in range(nr):
                if cls[r][0] >= 0:
                    continue
                a = np.full(N, kr[r])
                if q["s1"][r] >= 0:
                    a = a * x[q["s1"][r]]
                if q["s2"][r] >= 0:
                    a = a * x[q["s2"][r]]
                a = np.where(a > 0.0, a, 0.0)
                lam = a * weight(r)
                sub = counts["rpois"] if counts is not None else None
                n = np.array([LR.rpois(oracle, key, sw, jj, call, leap, r, float(lam[jj]), sub) for jj in range(N)])
                if counts is not None:
                    counts["poisson"] += N
                for c2 in range(d):
                    xn[c2] = xn[c2] + nu[r][c2] * n
            x = xn
        return x

    return transition, ll, aux


@contextlib.contextmanager
def gamma_noise(K, lead, sigma):
    """inside, every restatement of the family (rnet_restated and the modules that build on its make) runs the noisy transition"""
    assert isinstance(K, int) and 1 <= K <= 1024
    saved = RN.make
    RN.make = lambda oracle, seed, stream, counts=None: make(K, lead, sigma, oracle, seed, stream, counts)
    try:
        yield
    finally:
        RN.make = saved


def pf_run_rn(oracle, theta, y, N, u_res, K, nb=False, **kw):
    """rnet_em_restated.pf_run_rn for a block with lead[R], sigma[R]"""
    plain, lead, sigma = strip(theta, nb)
    with gamma_noise(K, lead, sigma):
        return (NB if nb else RT).pf_run_rn(oracle, plain, y, N, u_res, **kw)


def death_moments(h, sigma, x0):
    """mean and variance of x_1 for the linear death process X -> 0 at rate h under gamma white noise sigma, exact at any K: given the
    integrated noise Gamma(shape 1 / sigma^2, scale sigma^2) =: W, every individual survives with probability exp(-h W) independently"""
    s = (1.0 + sigma * sigma * h) ** (-1.0 / (sigma * sigma))
    s2 = (1.0 + 2.0 * sigma * sigma * h) ** (-1.0 / (sigma * sigma))
    return x0 * s, x0 * s * (1.0 - s) + x0 * (x0 - 1.0) * (s2 - s * s)
