"""Negative-binomial observations of the reaction-network family (models.reaction_network(obs="negbin", size=)) without a GPU: the
restated density (tests/rnet_nb_restated.py) against closed forms, its normalisation and variance, and the packed block of
BSSM_MODEL_RNET_NB with every refusal of the host."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_nb_restated as NB  # noqa: E402
import rnet_tv_restated as RT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEIR_REACTIONS = [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1, "C": 1}, "sigma"), ({"I": 1}, {"R": 1}, "gamma")]
SEIR_PAR = dict(beta=0.004, sigma=0.5, gamma=0.3)
N_BASE = 3 + 5 + 3 * 3 + 3 * 5            # d, R, p, x0, k, s1, s2, nu: G starts here


def seir_c(B, observe=({"C": 0.6}, {"I": 0.3}), **kw):
    """the README's SEIR with the onset species C, p = 2"""
    return B.models.reaction_network(("S", "E", "I", "R", "C"), SEIR_REACTIONS, x0=(180, 8, 12, 0, 0), observe=list(observe), **kw)


# --- the density ------------------------------------------------------------------------------------------------------------------------
def test_size_one_is_the_geometric_distribution():
    """r = 1: y log(mu / (1 + mu)) - log(1 + mu), to 1e-13 relative"""
    for mu in (0.03, 0.4, 1.0, 3.5, 60.0):
        for y in (0.0, 1.0, 2.0, 7.0, 40.0):
            want = y * math.log(mu / (1.0 + mu)) - math.log(1.0 + mu)
            got = NB.dnbinom_log(y, mu, 1.0)
            assert abs(got - want) <= 1e-13 * abs(want), (mu, y, got, want)


def test_zero_count_and_zero_mean():
    for mu, r in ((3.5, 0.7), (0.4, 25.0), (2.0, 2.0)):
        want = r * math.log(r / (r + mu))
        assert abs(NB.dnbinom_log(0.0, mu, r) - want) <= 1e-13 * abs(want)
    counts = {k: 0 for k in NB.KEYS}
    assert NB.dnbinom_log(0.0, 0.0, 0.7, None, counts) == 0.0
    assert NB.dnbinom_log(3.0, 0.0, 0.7, None, counts) == -math.inf
    assert NB.dnbinom_log(1.0, -0.5, 0.7, None, counts) == -math.inf          # (never formed by the filters; as dpois_log treats lambda < 0)
    assert counts == {"lr_log": 0, "lr_log1p": 0, "y0": 1, "mu0_inf": 1, "clamped": 0}
    NB.dnbinom_log(2.0, 3.5, 0.7, None, counts); NB.dnbinom_log(0.0, 0.4, 25.0, None, counts)
    assert counts == {"lr_log": 1, "lr_log1p": 1, "y0": 2, "mu0_inf": 1, "clamped": 0}


@pytest.mark.parametrize("mu,r", [(3.5, 0.7), (0.4, 25.0)])
def test_normalisation_and_variance(mu, r):
    """over y = 0 .. 600: sum exp(l) = 1 to 1e-12 and the variance is mu + mu^2 / r to 1e-9 (the tails beyond 600 are below both bars:
    the heavier one, (3.5, 0.7), decays like (mu / (r + mu))^y = 0.833^y, 1e-47 at y = 600).  size and mu exchanged, or a wrong table
    entry c, fail both."""
    ys = np.arange(601, dtype=np.float64)
    pr = np.array([math.exp(NB.dnbinom_log(float(y), mu, r, NB.table_c(float(y), r))) for y in ys])
    total = math.fsum(pr)
    mean = math.fsum(pr * ys)
    var = math.fsum(pr * (ys - mean) ** 2)
    print("sum", total, "mean", mean, "variance", var, "want", mu + mu * mu / r)
    assert abs(total - 1.0) <= 1e-12
    assert abs(mean - mu) <= 1e-9 * mu
    assert abs(var - (mu + mu * mu / r)) <= 1e-9 * (mu + mu * mu / r)
    swapped = math.fsum(math.exp(NB.dnbinom_log(float(y), r, mu)) * (y - r) ** 2 for y in ys)
    assert abs(swapped - (mu + mu * mu / r)) > 1e-3                            # (the check can tell the two apart)


# --- the block ----------------------------------------------------------------------------------------------------------------------------
def test_pack_inserts_size_after_G_and_leaves_poisson_alone():
    import bayesssm_amd as B
    from bayesssm_amd import _lib
    M = 0.5 + ((7 * np.arange(9)[:, None] + 3 * np.arange(3)[None, :]) % 11) / 10.0
    for kw in ({}, {"counters": ("C",)}, {"rate_schedule": M}, {"counters": ("C",), "rate_schedule": M, "missing": "skip"}):
        pois = seir_c(B, **kw)
        nb = seir_c(B, obs="negbin", size=(0.8, 25.0), **kw)
        bp, bn = pois.pack(SEIR_PAR), nb.pack(SEIR_PAR)
        o = N_BASE + 2 * 5                                                     # the end of G
        assert bn.dtype == np.float64 and bn.size == bp.size + 2
        assert np.array_equal(bn[:o], bp[:o]) and np.array_equal(bn[o:o + 2], [0.8, 25.0]) and np.array_equal(bn[o + 2:], bp[o:])
        assert nb.n_theta() == bn.size and nb.n_theta_ok(bn.size) and not nb.n_theta_ok(bp.size)
        back, size = NB.split(bn)
        assert np.array_equal(back, bp) and np.array_equal(size, [0.8, 25.0])
        # obs="poisson" is the descriptor without the keyword, byte for byte
        assert seir_c(B, obs="poisson", **kw).pack(SEIR_PAR).tobytes() == bp.tobytes()
        assert pois.obs == "poisson" and pois.size is None and pois.log_likelihood_fn.params == ()
    assert _lib.RN_OBS_MODEL == {"poisson": 6, "negbin": 7} and _lib.MODEL["rnet"] == 6
    header = open(os.path.join(ROOT, "include", "bayesssm_amd.h")).read()
    assert re.search(r"#define\s+BSSM_MODEL_RNET_NB\s+7\b", header)
    assert "bssm_rn_nb_tables" in _lib.EXPORTED_SYMBOLS
    # one number for every component
    assert np.array_equal(NB.split(seir_c(B, obs="negbin", size=10.0).pack(SEIR_PAR))[1], [10.0, 10.0])
    # the schedule is still checked against the times behind the longer block
    m = seir_c(B, obs="negbin", size=3.0, rate_schedule=M)
    m.check_times(m.n_theta(), 6, (1, 2, 5, 5, 6, 9))
    with pytest.raises(ValueError, match="short of the last observation time"):
        m.check_times(m.n_theta(), 6, (1, 2, 5, 5, 6, 10))


def test_named_sizes_are_parameters():
    import bayesssm_amd as B
    m = seir_c(B, obs="negbin", size="r")
    assert m.param_order == ("beta", "sigma", "gamma", "r")
    assert m.log_likelihood_fn.params == ("r",) and "r" in m.log_likelihood_fn.formals()
    assert "r" in m.aux_log_likelihood_fn.formals() and "r" in m.transition_fn.params
    assert np.array_equal(NB.split(m.pack(dict(SEIR_PAR, r=4.5)))[1], [4.5, 4.5])
    with pytest.raises(TypeError, match='argument "r" is missing'):
        m.pack(SEIR_PAR)
    two = seir_c(B, obs="negbin", size=("r", 7.0))
    assert two.param_order == ("beta", "sigma", "gamma", "r") and np.array_equal(NB.split(two.pack(dict(SEIR_PAR, r=0.5)))[1], [0.5, 7.0])
    # from build: a number, one per component, or by name
    for ret, want in ((2.5, [2.5, 2.5]), ([0.5, 9.0], [0.5, 9.0]), ({"r": 6.0}, [6.0, 6.0])):
        b = seir_c(B, obs="negbin", size="r", param_names=("beta", "sigma", "gamma", "phi"),
                   build=lambda beta, sigma, gamma, phi, ret=ret: {"rates": {"beta": beta, "sigma": sigma, "gamma": gamma}, "size": ret})
        assert b.log_likelihood_fn.params == ("beta", "sigma", "gamma", "phi")
        assert np.array_equal(NB.split(b.pack(dict(SEIR_PAR, phi=1.0)))[1], want)
    # a named size that is a parameter of a descriptor with build: read from the draw
    b = seir_c(B, obs="negbin", size="r", build=lambda beta, sigma, gamma, r: {}, param_names=("beta", "sigma", "gamma", "r"))
    assert np.array_equal(NB.split(b.pack(dict(SEIR_PAR, r=3.0)))[1], [3.0, 3.0])


def test_pack_many_gives_each_draw_its_size():
    import bayesssm_amd as B
    m = seir_c(B, obs="negbin", size=("r", 25.0), counters=("C",))
    draws = [dict(SEIR_PAR, r=r, beta=0.004 + 0.001 * i) for i, r in enumerate((0.5, 4.0, 30.0))]
    blocks = m.pack_many(draws)
    o = N_BASE + 2 * 5
    assert blocks.shape == (3, m.n_theta()) and blocks.flags["C_CONTIGUOUS"]
    for i, q in enumerate(draws):
        assert np.array_equal(blocks[i], m.pack(q)) and np.array_equal(blocks[i, o:o + 2], [q["r"], 25.0])
        assert np.array_equal(blocks[i, o + 2:], [0, 0, 0, 0, 1])
        base, reset, sched = RT.split(NB.split(blocks[i])[0])
        assert sched is None and np.array_equal(reset, [0, 0, 0, 0, 1])


def test_refusals():
    import bayesssm_amd as B
    with pytest.raises(ValueError, match="obs must be one of"):
        seir_c(B, obs="binomial")
    with pytest.raises(ValueError, match="needs obs='negbin'"):
        seir_c(B, size=3.0)
    with pytest.raises(ValueError, match="needs obs='negbin'"):
        seir_c(B, obs="poisson", size="r")
    with pytest.raises(ValueError, match="obs='negbin' needs size"):
        seir_c(B, obs="negbin")
    for bad in ((1.0, 2.0, 3.0), (), ("r",)):
        with pytest.raises(ValueError, match="one per observation component"):
            seir_c(B, obs="negbin", size=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), (2.0, 0.0)):
        with pytest.raises(ValueError, match="must be finite and > 0"):
            seir_c(B, obs="negbin", size=bad)
    m = seir_c(B, obs="negbin", size="r")
    for bad in (0.0, -1.0, float("nan"), float("inf")):                       # per draw
        with pytest.raises(ValueError, match="must be finite and > 0"):
            m.pack(dict(SEIR_PAR, r=bad))
        with pytest.raises(ValueError, match="must be finite and > 0"):
            m.pack_many([dict(SEIR_PAR, r=2.0), dict(SEIR_PAR, r=bad)])
    b = seir_c(B, obs="negbin", size=2.0, build=lambda beta, sigma, gamma: {"size": [1.0, 2.0, 3.0]}, param_names=("beta", "sigma", "gamma"))
    with pytest.raises(ValueError, match="3 sizes for 2 observation components"):
        b.pack(SEIR_PAR)
    b = seir_c(B, build=lambda beta, sigma, gamma: {"size": 2.0}, param_names=("beta", "sigma", "gamma"))
    with pytest.raises(ValueError, match="needs obs='negbin'"):
        b.pack(SEIR_PAR)
