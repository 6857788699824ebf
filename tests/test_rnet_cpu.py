"""Reaction networks (models.reaction_network, BSSM_MODEL_RNET) without a GPU: the packed block, the SIR instance, the host's
refusals, the new ctypes prototypes against the header, and the numpy restatement of the family (tests/rnet_restated.py) at the
SIR instance against the oracle's own C restatement of the built-in SIR model."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_restated as RN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sir_instance(B, n_total=500, i0=70):
    """the built-in SIR as a network: infection S + I -> 2 I at lambda / n_total, removal I -> 0 at gamma, y ~ Poisson(I)"""
    return B.models.reaction_network(("S", "I"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {}, "gamma")],
                                     x0=(n_total - i0, i0), observe={"I": 1.0},
                                     build=lambda lam, gamma: {"rates": {"beta": lam / n_total, "gamma": gamma}}, param_names=("lam", "gamma"))


def test_pack_layout():
    import bayesssm_amd as B
    m = B.models.reaction_network(("S", "E", "I", "R"),
                                  [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"), ({"I": 1}, {"R": 1}, 0.25)],
                                  x0=(90, 4, 6, 0), observe=[{"I": 0.5}, {"E": 0.25, "I": 0.125}])
    assert (m.dim, m.R, m.p, m.param_order) == (4, 3, 2, ("beta", "sigma"))
    assert m.init_fn.model == m.transition_fn.model == m.log_likelihood_fn.model == m.aux_log_likelihood_fn.model == "rnet"
    b = m.pack({"beta": 0.004, "sigma": 0.5, "unrelated": 1})
    want = [4, 3, 2, 90, 4, 6, 0, 0.004, 0.5, 0.25, 0, 1, 2, 2, -1, -1,
            -1, 1, 0, 0, 0, -1, 1, 0, 0, 0, -1, 1, 0, 0, 0.5, 0, 0, 0.25, 0.125, 0]
    assert b.dtype == np.float64 and np.array_equal(b, np.array(want, dtype=np.float64))
    q = RN.unpack(b)
    assert np.array_equal(q["nu"][0], [-1, 1, 0, 0]) and np.array_equal(q["G"], [[0, 0, 0.5, 0], [0, 0.25, 0.125, 0]])
    with pytest.raises(TypeError, match='argument "sigma" is missing'):
        m.pack({"beta": 0.004})
    G = np.array([[0.0, 0, 1, 0]])
    assert np.array_equal(B.models.reaction_network(m.species, [({"I": 1}, {}, 1.0)], (1, 1, 1, 1), G).pack()[-4:], G[0])


def test_sir_instance_block():
    import bayesssm_amd as B
    b = sir_instance(B).pack({"lam": 0.5, "gamma": 0.2})
    assert np.array_equal(b, np.array([2, 2, 1, 430, 70, 0.5 / 500, 0.2, 0, 1, 1, -1, -1, 1, 0, -1, 0, 1], dtype=np.float64))


def test_refusals_without_a_gpu():
    import bayesssm_amd as B
    from bayesssm_amd import _lib
    assert _lib.MODEL["rnet"] == 6
    rn = B.models.reaction_network
    with pytest.raises(ValueError, match="s1 == s2"):
        rn(("A",), [({"A": 2}, {}, 1.0)], (5,), {"A": 1})
    with pytest.raises(ValueError, match="more than one molecule of a species"):
        rn(("A",), [({"A": 3}, {}, 1.0)], (5,), {"A": 1})
    with pytest.raises(ValueError, match="1 <= d <= 8"):
        rn(tuple("ABCDEFGHI"), [({"A": 1}, {}, 1.0)], (1,) * 9, {"A": 1})
    with pytest.raises(ValueError, match="1 <= R <= 8"):
        rn(("A",), [({"A": 1}, {}, 1.0)] * 9, (1,), {"A": 1})
    with pytest.raises(ValueError, match="1 <= R <= 8"):
        rn(("A",), [], (1,), {"A": 1})
    with pytest.raises(ValueError, match="1 <= p <= 8"):
        rn(("A",), [({"A": 1}, {}, 1.0)], (1,), [{"A": 1}] * 9)
    with pytest.raises(ValueError, match="1 <= p <= 8"):
        rn(("A",), [({"A": 1}, {}, 1.0)], (1,), np.zeros((0, 1)))
    with pytest.raises(ValueError, match="more than two reactants"):
        rn(("A", "B", "C"), [({"A": 1, "B": 1, "C": 1}, {}, 1.0)], (1, 1, 1), {"A": 1})
    with pytest.raises(ValueError, match=">= 0"):
        rn(("A",), [({"A": 1}, {}, -1.0)], (1,), {"A": 1})
    m = sir_instance(B)
    par = dict(lam=0.5, gamma=0.2)
    good = np.ones(5)
    for bad, match in ((-1.0, "negative"), (0.5, "fractional"), (np.nan, "non-finite"), (np.inf, "non-finite")):
        y = good.copy(); y[3] = bad
        with pytest.raises(ValueError, match=match):
            B.bootstrap_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, **par)
        with pytest.raises(ValueError, match=match):
            B.auxiliary_filter(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, **par)
        with pytest.raises(ValueError, match=match):
            B.bootstrap_filter_batch(y, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, [par] * 2, 1, [0, 1])
    with pytest.raises(ValueError, match="T x 1 matrix"):
        B.bootstrap_filter(np.ones((5, 2)), 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, **par)
    with pytest.raises(ValueError, match="RMPF"):                                   # no move on integer states
        m.rw_move_fn(0.1)
    lg = B.models.linear_gaussian()
    with pytest.raises(ValueError, match="RMPF"):
        B.resample_move_filter(good, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, lg.rw_move_fn(0.1), **par)
    with pytest.raises(ValueError, match="stratified / systematic"):
        B.bootstrap_filter(good, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_fn="multinomial", **par)
    with pytest.raises(ValueError, match="injected z_"):
        B.bootstrap_filter(good, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, draws={"z_init": np.zeros(200), "u_res": np.zeros(5)}, **par)
    with pytest.raises(ValueError, match="r_seed / r_stream"):
        B.bootstrap_filter(good, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, r_seed=1, **par)
    with pytest.raises(ValueError, match="bootstrap filter"):                       # batched APF
        B.auxiliary_filter_batch(good, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, m.aux_log_likelihood_fn, [par] * 2)
    with pytest.raises(TypeError, match='argument "gamma" is missing'):
        B.bootstrap_filter(good, 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, lam=0.5)


def test_new_prototypes_match_the_header():
    from bayesssm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bayesssm_amd.h")).read()
    assert re.search(r"#define\s+BSSM_MODEL_RNET\s+6\b", header)
    assert re.search(r"\bint\s+bssm_pf_batch_max_particles_rn\s*\(\s*int\s+d\s*\)\s*;", header)
    assert "bssm_pf_batch_max_particles_rn" in _lib.EXPORTED_SYMBOLS
    assert "d, R, p, x0[d], k[R], s1[R], s2[R], nu[R][d]" in header and "G[p][d]" in header
    import ctypes as C
    lib = _lib.load()
    assert lib.bssm_pf_batch_max_particles_rn.argtypes == [C.c_int]
    for d in range(1, 9):                                                           # a host-side constant: no device needed
        assert 1000 <= lib.bssm_pf_batch_max_particles_rn(d) <= 2048
    assert lib.bssm_pf_batch_max_particles_rn(0) == 0 and lib.bssm_pf_batch_max_particles_rn(9) == 0


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_restatement_equals_the_oracles_sir(oracle, algorithm):
    """the numpy restatement at the SIR instance against oracle.pf_run("sir", ...): the same draws, within 1e-12"""
    import bayesssm_amd as B
    rng = np.random.default_rng(3)
    N, T, seed, stream = 64, 6, 77, 5
    y = np.array([72, 80, 85, 95, 99, 110], dtype=np.float64)
    nres = 2 * T if algorithm == "APF" else T
    u = rng.random((nres, N))
    block = sir_instance(B).pack({"lam": 0.5, "gamma": 0.2})
    got = RN.pf_run_rn(oracle, block, y, N, u, seed=seed, stream=stream, algorithm=algorithm, resample_algorithm="SISAR")
    ref = oracle.pf_run("sir", [0.5, 0.2, 500, 430, 70], y, N, None, None, u, algorithm=algorithm, resample_algorithm="SISAR",
                        seed=seed, stream=stream)
    assert abs(got["loglike"] - ref["loglike"]) <= 1e-12 * abs(ref["loglike"])
    np.testing.assert_allclose(got["loglike_history"], ref["loglike_history"], rtol=1e-12)
    np.testing.assert_allclose(got["ess"], ref["ess"], rtol=1e-12)
    np.testing.assert_allclose(got["state_est"], ref["state_est"], rtol=1e-12)
    assert (got["resampled"] == ref["resampled"]).all()


# --- the restatement where tests/test_gpu_rnet_limits.py is the first to use it: d = R = p = 8, an order-0 reaction, d = 1 ---------
def test_full8_pack_layout():
    import bayesssm_amd as B
    import test_gpu_rnet_limits as L
    m = L.full8(B)
    b = m.pack(L.FULL8_PAR)
    assert (m.dim, m.R, m.p) == (8, 8, 8) and b.size == 163 == 3 + 8 + 3 * 8 + 64 + 64 and tuple(b[:3]) == (8, 8, 8)
    q = RN.unpack(b)
    assert np.array_equal(q["x0"], [6, 5, 7, 4, 5, 6, 5, 0]) and np.array_equal(q["k"], [L.FULL8_PAR["k%d" % r] for r in range(8)])
    assert q["s1"][0] == -1 and q["s2"][0] == -1                                   # 0 -> A: no reactant
    assert np.array_equal(q["s1"], [-1, 0, 1, 3, 4, 5, 7, 6]) and np.array_equal(q["s2"], [-1, -1, 2, -1, -1, 6, -1, -1])
    assert np.array_equal(q["nu"][0], [1, 0, 0, 0, 0, 0, 0, 0])
    assert np.array_equal(q["nu"][3], [0, 0, 0, -1, 1, 1, 0, 0])                   # D -> E + F
    assert np.all((q["G"] != 0).sum(axis=0) >= 1) and np.array_equal(q["G"][7], [0, 0, 0, 0, 0, 0, 0, 1])
    assert np.all((q["G"] != 0).sum(axis=1) <= 2)                                   # (what makes a species permutation exact)


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_restatement_is_equivariant_under_a_species_permutation(oracle, algorithm):
    """the restatement on full8 against itself with the species of slots 0..3 and 4..7 exchanged: equal after un-permuting, 1e-12"""
    import bayesssm_amd as B
    import test_gpu_rnet_limits as L
    N, T = 64, 3
    u = np.random.default_rng(11).random((2 * T if algorithm == "APF" else T, N))
    cols = [L.FULL8_PERM.index(s) for s in L.FULL8_SPECIES]
    kw = dict(seed=5, stream=2, algorithm=algorithm, resample_algorithm="SISAR", obs_times=L.OT[:T], return_particles=True)
    a = RN.pf_run_rn(oracle, L.full8(B).pack(L.FULL8_PAR), L.Y_FULL8[:T], N, u, **kw)
    b = RN.pf_run_rn(oracle, L.full8(B, L.FULL8_PERM).pack(L.FULL8_PAR), L.Y_FULL8[:T], N, u, **kw)
    assert np.isfinite(a["loglike"]) and a["ancestors"].size > 0
    for k in ("loglike", "loglike_history", "ess", "weights_history"):
        np.testing.assert_allclose(a[k], b[k], rtol=1e-12, err_msg=k)
    assert np.array_equal(a["ancestors"], b["ancestors"]) and np.array_equal(a["resampled"], b["resampled"])
    np.testing.assert_allclose(a["state_est"], b["state_est"][:, cols], rtol=1e-12, atol=1e-12)
    pa, pb = a["particles_history"].reshape(T + 1, 8, N), b["particles_history"].reshape(T + 1, 8, N)
    assert np.array_equal(pa, pb[:, cols]) and all((pa[:, c] != pa[0, c]).any() for c in range(8))


def test_restatement_has_the_birth_death_mean(oracle):
    """the restatement on bd1 (an order-0 reaction, d = 1) with G = 0, y = 0 under SIS: the state estimate is the sample mean of
    N = 4096 independent chains, within 6 sigma of the exact mean (test_gpu_rnet_limits.bd1_mean_and_bound)"""
    import bayesssm_amd as B
    import test_gpu_rnet_limits as L
    N, T = 4096, 5
    m = L.bd1(B, observe=np.zeros((1, 1)))
    res = RN.pf_run_rn(oracle, m.pack(L.BD1_PAR), np.zeros(T), N, np.zeros((T, N)), seed=3, stream=0, resample_algorithm="SIS", return_particles=True)
    assert res["loglike"] == 0.0 and res["state_est"].shape == (T + 1,) and not res["resampled"].any()
    exact, bound = L.bd1_mean_and_bound(np.arange(T + 1), N)
    err = np.abs(res["state_est"] - exact)
    print("errors", err, "bound", bound)
    assert np.all(err <= bound)
    ph = res["particles_history"]
    assert np.all(ph == np.floor(ph)) and ph.min() >= 0 and ph.max() > L.BD1_X0
