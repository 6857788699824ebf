"""What Euler-multinomial leaps (models.reaction_network(..., method="euler_multinomial", leaps=K)) put in the place of Gillespie's direct
method in the numpy restatement of the reaction-network family (tests/rnet_restated.py and what rnet_inc_restated.py, rnet_tv_restated.py
and rnet_nb_restated.py add to it), from the definition in DESIGN.md section 1d alone.  fp64, in the order written; exp, log, log1p, expm1
and lgamma are the C library's (math.*), element by element.  Vectorised over the particles: the loops over leaps, species, reactions and
attempts are the definition's, every arithmetic step is one numpy operation over the particles that take it.

  classification  source(r): the one reactant c of {s1[r], s2[r]} with nu[r][c] == -1, the other reactant (if any) with nu >= 0 and no
                  species that is no reactant with nu < 0;  o(r): the other reactant.   sourceless: no species with nu < 0.   Everything
                  else (both reactants consumed, a reactant with nu < -1, a non-reactant with nu < 0) is refused: classify raises.
  transition      one unit of time, after the counters' reset (rnet_inc_restated, unchanged): for leap l = 0 .. K-1, x held, xn = x
                    1. for c = 0 .. d-1, over the reactions r_1 < r_2 < ... with source(r) == c:
                         h_r = kr[r] (times x[o(r)]), not > 0 counts as 0.0;   H = 0.0 + h_{r_1} + h_{r_2} + ...;   not H > 0: all counts 0.0
                         pe = -expm1(-H / K); rem = x[c]; prem = 1.0;  for each i:
                           p_i = (h_{r_i} / H) * pe;  q = p_i / prem;  not q > 0: q = 0.0;  q > 1: q = 1.0
                           n_i = rbinom(rem, q);  rem = rem - n_i;  prem = prem - p_i;  xn[c'] = xn[c'] + nu[r_i][c'] * n_i
                    2. for each sourceless r:  a_r = rnet_restated.propensities' value;  n = rpois(a_r / K) (rnet_leap_restated.rpois);
                       xn[c'] = xn[c'] + nu[r][c'] * n
                    3. x = xn
  rbinom(n, q)    for reaction r in leap l of call `call` and particle j, attempt a reads the Philox block at
                    (j, call, DRAW_TRANS | (((l * RNR + r) << 6 | a) << 8), stream),  u1 = u01(w.x, w.y),  u2 = u01(w.z, w.w),  RNR = 8
                  not n > 0 or not q > 0: 0.0.   q >= 1: n.   flip = q > 0.5;  qq = 1 - q if flip else q;  the result is n - k if flip else k
                  n * qq < 10: inversion by sequential search on u1 of attempt 0
                    pr = exp(n * log1p(-qq)); F = pr; k = 0; odds = qq / (1 - qq)
                    while u1 > F and k < n and k < 128: k = k + 1; pr = pr * ((n - k + 1) / k) * odds; F = F + pr
                  otherwise Hoermann's BTRS (1993)
                    spq = sqrt((n * qq) * (1 - qq)); b = 1.15 + 2.53 spq; a_ = (-0.0873 + 0.0248 b) + 0.01 qq; cc = n * qq + 0.5; vr = 0.92 - 4.2 / b
                    attempts a = 0 .. 63:  U = u1 - 0.5; V = u2; us = 0.5 - |U|; k = floor((2 a_ / us + b) U + cc)
                      accept if us >= 0.07 and V <= vr;  reject if k < 0 or k > n;  otherwise accept if, with
                      alpha = (2.83 + 5.1 / b) spq; m = floor((n + 1) qq); lr = log(qq / (1 - qq)),
                      log(V alpha / (a_ / us^2 + b)) <= (((lgamma(m + 1) + lgamma(n - m + 1)) - lgamma(k + 1)) - lgamma(n - k + 1)) + (k - m) lr
                    after 64 rejections k = floor(n * qq)

Everything else -- densities, look-ahead, counters, missing observations, schedule rows, the filter core -- is the other restatements',
untouched: they reach the transition through rnet_restated.make, which euler_multinomial(K) rebinds for the length of a with block.

counts (rnet_restated.make) additionally collects, per binomial draw,
  "zero", "all"            not n > 0 or not q > 0;  q >= 1
  "flip"                   draws sampled at 1 - q
  "inv", "btrs"            draws by branch
  "squeeze", "full"        BTRS accepts by the squeeze and by the full test
  "rejected"               BTRS attempts that were rejected
  "fallback"               BTRS draws that ran out of attempts
and "poisson", the draws of sourceless reactions (their own branches under counts["rpois"], rnet_leap_restated's keys)."""
import contextlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_leap_restated as LR  # noqa: E402
import rnet_nb_restated as NB  # noqa: E402
import rnet_restated as RN  # noqa: E402
import rnet_tv_restated as RT  # noqa: E402
from rnet_restated import DRAW_TRANS, stream_word  # noqa: E402

RNR = 8
KEYS = ("zero", "all", "flip", "inv", "btrs", "squeeze", "full", "rejected", "fallback", "poisson")
_M32 = np.uint64(0xFFFFFFFF)


def new_counts():
    return {k: 0 for k in KEYS}


def _elementwise(f):
    g = np.frompyfunc(f, 1, 1)
    return lambda v: g(np.asarray(v, dtype=np.float64)).astype(np.float64)


_exp, _log, _log1p, _expm1, _lgamma = (_elementwise(f) for f in (math.exp, math.log, math.log1p, math.expm1, math.lgamma))


def philox4x32_10(c0, c1, c2, c3, key):
    """Philox4x32-10 (Salmon et al. 2011) on arrays of counter words; key: the two key words.  Four uint64 arrays holding 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & _M32 for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                          # (32 x 32 bits: no overflow in 64)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def u01_from_bits(lo, hi):
    return ((((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def uniforms(key, sw, j, call, lr, a):
    """(u1, u2) of attempt a for the particles j"""
    w = philox4x32_10(j, call, DRAW_TRANS | (((lr << 6) | a) << 8), sw, key)
    return u01_from_bits(w[0], w[1]), u01_from_bits(w[2], w[3])


def rbinom(key, sw, j, call, lr, n, q, counts=None):
    """the draws of the particles j (an index array) for (call, lr = l * RNR + r) from n[i] trials at q[i]"""
    n, q, j = np.asarray(n, dtype=np.float64), np.asarray(q, dtype=np.float64), np.asarray(j, dtype=np.uint64)
    c = counts if counts is not None else new_counts()
    out = np.zeros(n.shape)
    zero = ~(n > 0.0) | ~(q > 0.0)
    every = ~zero & (q >= 1.0)
    out[every] = n[every]
    act = ~zero & ~every
    flip = act & (q > 0.5)
    qq = np.where(flip, 1.0 - q, q)
    inv = act & (np.where(act, n * qq, 0.0) < 10.0)
    btrs = act & ~inv
    k = np.zeros(n.shape)
    for name, mask in (("zero", zero), ("all", every), ("flip", flip), ("inv", inv), ("btrs", btrs)):
        c[name] = c.get(name, 0) + int(mask.sum())
    if inv.any():
        i = np.nonzero(inv)[0]
        u1, _ = uniforms(key, sw, j[i], call, lr, 0)
        ni, qi = n[i], qq[i]
        pr = _exp(ni * _log1p(-qi))
        F = pr.copy()
        kk = np.zeros(i.size)
        odds = qi / (1.0 - qi)
        for _ in range(128):
            go = (u1 > F) & (kk < ni) & (kk < 128.0)
            if not go.any():
                break
            kk[go] = kk[go] + 1.0
            pr[go] = pr[go] * ((ni[go] - kk[go] + 1.0) / kk[go]) * odds[go]
            F[go] = F[go] + pr[go]
        k[i] = kk
    if btrs.any():
        i = np.nonzero(btrs)[0]
        ni, qi = n[i], qq[i]
        spq = np.sqrt((ni * qi) * (1.0 - qi))
        b = 1.15 + 2.53 * spq
        a_ = (-0.0873 + 0.0248 * b) + 0.01 * qi
        cc = ni * qi + 0.5
        vr = 0.92 - 4.2 / b
        res = np.floor(ni * qi)
        left = np.arange(i.size)                           # (positions in i still without an accepted draw)
        for a in range(64):
            if left.size == 0:
                break
            u1, u2 = uniforms(key, sw, j[i[left]], call, lr, a)
            U, V = u1 - 0.5, u2
            us = 0.5 - np.abs(U)
            kk = np.floor((2.0 * a_[left] / us + b[left]) * U + cc[left])
            squeeze = (us >= 0.07) & (V <= vr[left])
            out_of_range = ~squeeze & ((kk < 0.0) | (kk > ni[left]))
            test = ~squeeze & ~out_of_range
            ok = np.zeros(left.size, dtype=bool)
            if test.any():
                t = left[test]
                nt, qt, kt, bt = ni[t], qi[t], kk[test], b[t]
                alpha = (2.83 + 5.1 / bt) * spq[t]
                m = np.floor((nt + 1.0) * qt)
                lr_ = _log(qt / (1.0 - qt))
                lhs = _log(V[test] * alpha / (a_[t] / (us[test] * us[test]) + bt))
                rhs = (((_lgamma(m + 1.0) + _lgamma(nt - m + 1.0)) - _lgamma(kt + 1.0)) - _lgamma(nt - kt + 1.0)) + (kt - m) * lr_
                ok[test] = lhs <= rhs
            acc = squeeze | ok
            res[left[acc]] = kk[acc]
            c["squeeze"] = c.get("squeeze", 0) + int(squeeze.sum())
            c["full"] = c.get("full", 0) + int(ok.sum())
            c["rejected"] = c.get("rejected", 0) + int((~acc).sum())
            left = left[~acc]
        c["fallback"] = c.get("fallback", 0) + int(left.size)
        k[i] = res
    out[act] = np.where(flip, n - k, k)[act]
    return out


def sample(oracle, seed, stream, call, leap, r, n, q, counts=None):
    """what bssm_dump_rbinom returns: the draws that particles 0 .. len(n)-1 take for (call, leap, r); oracle is not used (the Philox
    blocks are philox4x32_10's above, which tests/test_rnet_em_cpu.py holds against the oracle's)"""
    n, q = np.broadcast_arrays(np.asarray(n, dtype=np.float64), np.asarray(q, dtype=np.float64))
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    return rbinom(key, stream_word(stream), np.arange(n.size), call, leap * RNR + r, n.reshape(-1), q.reshape(-1), counts)


def classify(q):
    """per reaction (source, other): source = a species, or -1 for a sourceless reaction; other = the other reactant or -1.  Raises
    ValueError for a reaction that the method refuses"""
    out = []
    for r in range(q["R"]):
        s1, s2 = int(q["s1"][r]), int(q["s2"][r])
        nu = q["nu"][r]
        n1 = float(nu[s1]) if s1 >= 0 else 0.0
        n2 = float(nu[s2]) if s2 >= 0 else 0.0
        if n1 < 0.0 and n2 < 0.0:
            raise ValueError("reaction %d consumes both of its reactants" % r)
        if (n1 < 0.0 and n1 != -1.0) or (n2 < 0.0 and n2 != -1.0):
            raise ValueError("reaction %d: a consumed reactant has nu == -1" % r)
        if any(float(nu[c]) < 0.0 for c in range(q["d"]) if c not in (s1, s2)):
            raise ValueError("reaction %d: only a reactant may have nu < 0" % r)
        out.append((s1, s2) if n1 < 0.0 else (s2, s1) if n2 < 0.0 else (-1, -1))
    return out


_gillespie_make = RN.make


def make(K, oracle, seed, stream, counts=None):
    """rnet_restated.make with the Euler-multinomial transition of K leaps; the densities are rnet_restated's"""
    _, ll, aux = _gillespie_make(oracle, seed, stream, counts)
    if counts is not None:
        for name in KEYS:
            counts.setdefault(name, 0)
        counts.setdefault("rpois", LR.new_counts())
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    sw = stream_word(stream)

    def transition(q, x, z):
        call = int(z[0, 0])
        x = np.array(x, dtype=np.float64)
        d, nr, N = q["d"], q["R"], x.shape[1]
        kr = [float(v) for v in q["k"]]
        nu = [[float(q["nu"][r, c]) for c in range(d)] for r in range(nr)]
        cls = classify(q)
        j = np.arange(N)
        dK = float(K)

        def hazard(r):
            h = np.full(N, kr[r])
            if cls[r][1] >= 0:
                h = h * x[cls[r][1]]
            return np.where(h > 0.0, h, 0.0)

        for leap in range(K):
            xn = x.copy()
            for c in range(d):
                group = [r for r in range(nr) if cls[r][0] == c]
                if not group:
                    continue
                H = np.zeros(N)
                for r in group:
                    H = H + hazard(r)
                live = H > 0.0
                Hl = np.where(live, H, 1.0)              # (the particles with not H > 0 draw nothing: their q is put at 0.0 below)
                pe = -_expm1(-Hl / dK)
                rem, prem = x[c].copy(), np.ones(N)
                for r in group:
                    p = (hazard(r) / Hl) * pe
                    with np.errstate(divide="ignore", invalid="ignore"):
                        qv = p / prem
                    qv = np.where(qv > 0.0, qv, 0.0)
                    qv = np.where(qv > 1.0, 1.0, qv)
                    qv = np.where(live, qv, 0.0)
                    sub = None
                    if counts is not None:
                        sub = new_counts()
                    n = rbinom(key, sw, j, call, leap * RNR + r, rem, qv, sub)
                    if counts is not None:               # (a particle with not H > 0 makes no draw at all: it is no "zero" either)
                        sub["zero"] -= int((~live).sum())
                        for name in KEYS:
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
                lam = a / dK
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
def euler_multinomial(K):
    """inside, every restatement of the family (rnet_restated and the modules that build on its make) runs the Euler-multinomial transition"""
    assert isinstance(K, int) and 1 <= K <= 1024
    saved = RN.make
    RN.make = lambda oracle, seed, stream, counts=None: make(K, oracle, seed, stream, counts)
    try:
        yield
    finally:
        RN.make = saved


def pf_run_rn(oracle, theta, y, N, u_res, K, nb=False, **kw):
    """rnet_tv_restated.pf_run_rn (nb: rnet_nb_restated.pf_run_rn, for a negative-binomial block) with K Euler-multinomial leaps per unit of
    time, for the bootstrap and the auxiliary filter (algorithm=)"""
    with euler_multinomial(K):
        return (NB if nb else RT).pf_run_rn(oracle, theta, y, N, u_res, **kw)
