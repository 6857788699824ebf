"""CPU tests of the genealogy smoother's definition: the numpy restatement (tests/smooth_restated.py) against a
hand-enumerated case and against the exact (Rauch-Tung-Striebel) smoothed means, and the keyword refusals that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_restated as SR  # noqa: E402


def test_hand_case_against_brute_force_enumeration():
    """N = 4, T = 3: observation 1 made one ancestor row, observation 2 none (no resample), observation 3 two (the auxiliary
    filter's first and second stage).  Every lineage is followed by hand below; the numbers are written out."""
    P = np.array([[10.0, 20.0, 30.0, 40.0], [1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0], [9.0, 10.0, 11.0, 12.0]])
    wh = np.array([[0.25] * 4, [0.25] * 4, [0.4, 0.3, 0.2, 0.1], [0.1, 0.2, 0.3, 0.4]])
    row_obs1, first3, second3 = [2, 2, 4, 1], [1, 1, 3, 4], [2, 3, 3, 1]
    anc, call_obs = np.array([row_obs1, first3, second3]), np.array([1, 3, 3])
    # brute force: one loop per final particle
    b = np.zeros((4, 4), dtype=int)
    for j in range(4):
        b[3, j] = j
        b[2, j] = first3[second3[j] - 1] - 1        # two rows: first[second[j]]
        b[1, j] = b[2, j]                            # no row: the identity
        b[0, j] = row_obs1[b[1, j]] - 1
    assert b.tolist() == [[1, 3, 3, 1], [0, 2, 2, 0], [0, 2, 2, 0], [0, 1, 2, 3]]
    want = [sum(wh[3, j] * P[i, b[i, j]] for j in range(4)) for i in range(4)]
    np.testing.assert_allclose(want, [30.0, 2.0, 6.0, 11.0], rtol=1e-15)
    got = SR.smooth(P, wh, anc, call_obs)
    assert np.array_equal(got["b"], b)
    np.testing.assert_allclose(got["smoothed"][:, 0], [30.0, 2.0, 6.0, 11.0], rtol=1e-15)
    np.testing.assert_allclose(got["abs_sum"][:, 0], [30.0, 2.0, 6.0, 11.0], rtol=1e-15)
    assert got["n_lineages"].tolist() == [2, 2, 2, 4]
    # terminal indices: cum = (0.1, 0.3, 0.6, 1.0); the first j with cum[j] >= u; beyond the last cum: N
    idx = SR.terminal_indices(wh[3], [0.05, 0.25, 0.95, 0.61, 1.5])
    assert idx.tolist() == [1, 2, 4, 4, 4]
    assert SR.terminal_indices([0.5, 0.5], [0.5, np.nextafter(0.5, 1.0)]).tolist() == [1, 2]      # u == cum[j] takes j
    tr = SR.paths(P, got["b"], idx)
    assert tr.shape == (5, 4, 1)
    assert tr[0, :, 0].tolist() == [20.0, 1.0, 5.0, 9.0] and tr[1, :, 0].tolist() == [40.0, 3.0, 7.0, 10.0]
    assert tr[2, :, 0].tolist() == [20.0, 1.0, 5.0, 12.0]


def test_two_components_are_traced_together():
    """d = 2, component-major rows: both components follow the same lineage"""
    P = np.array([[1.0, 2.0, 3.0, 10.0, 20.0, 30.0], [4.0, 5.0, 6.0, 40.0, 50.0, 60.0]])
    wh = np.array([[1 / 3] * 3, [0.5, 0.25, 0.25]])
    got = SR.smooth(P, wh, np.array([[3, 3, 1]]), np.array([1]), d=2)
    np.testing.assert_allclose(got["smoothed"], [[0.5 * 3 + 0.25 * 3 + 0.25 * 1, 0.5 * 30 + 0.25 * 30 + 0.25 * 10], [4.75, 47.5]], rtol=1e-15)
    assert got["n_lineages"].tolist() == [2, 3]
    assert SR.paths(P, got["b"], [3], d=2).tolist() == [[[1.0, 10.0], [6.0, 60.0]]]


def test_rts_pass_against_the_joint_gaussian():
    """the backward pass: E[x | y] of the joint Gaussian of (x_0 .. x_T, y_1 .. y_T), by dense linear algebra"""
    A, b, L, m0, L0, h0, H, sd = 0.8, 0.1, 0.7, 0.3, 1.2, -0.2, 1.5, 0.6
    y = np.array([0.4, -0.3, 1.1, 0.2])
    T = y.size
    mean, cov = np.zeros(T + 1), np.zeros((T + 1, T + 1))
    mean[0], cov[0, 0] = m0, L0 * L0
    for t in range(1, T + 1):
        mean[t] = A * mean[t - 1] + b
        cov[t, :t] = A * cov[t - 1, :t]
        cov[:t, t] = cov[t, :t]
        cov[t, t] = A * A * cov[t - 1, t - 1] + L * L
    Cxy = H * cov[:, 1:]
    Cyy = H * H * cov[1:, 1:] + sd * sd * np.eye(T)
    want = mean + Cxy @ np.linalg.solve(Cyy, y - h0 - H * mean[1:])
    np.testing.assert_allclose(SR.rts_means_1d(y, A, b, L, m0, L0, h0, H, sd), want, rtol=1e-12)


def test_restatement_on_a_numpy_sisr_filter_meets_the_exact_smoothed_means():
    """T = 6, N = 4096, 32 fixed seeds: for every t the mean over the seeds of smoothed[t] lies within 5 standard errors (taken from
    the 32 replicates) of the Rauch-Tung-Striebel mean.  A condition, not a measurement: under normality a coordinate fails with
    probability about 6e-7."""
    q = SR.EXACT
    exact = SR.exact_means()
    reps = []
    for seed, _ in SR.EXACT_SEEDS:
        h = SR.sisr_histories_1d(SR.EXACT_Y, SR.EXACT_N, np.random.default_rng(seed), q["phi"], 0.0, q["sigma_x"], 0.0, 1.0, sd=q["sigma_y"])
        s = SR.smooth(h["particles_history"], h["weights_history"], h["ancestors"], h["call_obs"])
        assert s["n_lineages"][-1] == SR.EXACT_N and np.all(np.diff(s["n_lineages"]) >= 0)
        reps.append(s["smoothed"][:, 0])
    ok, z = SR.within_5_se(reps, exact)
    print("exact", exact, "mean", np.mean(reps, axis=0), "z", z)
    assert ok.all(), z


# ---- keyword refusals that are raised before any device work --------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


Y = np.array([0.1, -0.2, 0.3])
PAR = dict(phi=0.8, sigma_x=1.0, sigma_y=1.0)


def _closures():
    return (lambda num_particles, **k: np.zeros(num_particles), lambda particles, **k: particles, lambda y, particles, **k: np.zeros(particles.size))


@pytest.mark.parametrize("kw", [dict(smooth=True), dict(trajectories=3)])
def test_refused_outside_the_single_filter_device_path(B, kw):
    m = B.models.linear_gaussian()
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    with pytest.raises(ValueError, match="closure mode: smooth= / trajectories="):
        B.bootstrap_filter(Y, 16, *_closures(), **kw)
    with pytest.raises(ValueError, match="closure mode: smooth= / trajectories="):
        B.auxiliary_filter(Y, 16, *_closures(), lambda y, particles, **k: np.zeros(particles.size), **kw)
    with pytest.raises(ValueError, match="r_seed / r_stream: smooth= / trajectories="):
        B.bootstrap_filter(Y, 16, *fns, r_seed=1, **kw, **PAR)
    with pytest.raises(ValueError, match="bootstrap_filter_batch: smooth= / trajectories="):
        B.bootstrap_filter_batch(Y, 16, *fns, np.array([[0.8, 1.0, 1.0]]), **kw)
    with pytest.raises(ValueError, match="bootstrap_filter_batch: smooth= / trajectories="):
        B.auxiliary_filter_batch(Y, 16, *fns, m.aux_log_likelihood_fn, np.array([[0.8, 1.0, 1.0]]), **kw)
    with pytest.raises(ValueError, match="bootstrap_filter_multi: smooth= / trajectories="):
        B.bootstrap_filter_multi(Y, 16, *fns, np.array([[0.8, 1.0, 1.0]]), **kw)
    with pytest.raises(ValueError, match="bootstrap_filter_sharded: smooth= / trajectories="):
        B.bootstrap_filter_sharded(Y, 16, *fns, **kw, **PAR)
    with pytest.raises(ValueError, match="pmmh: smooth= / trajectories="):
        B.pmmh(B.bootstrap_filter, Y, 10, *fns, {}, [{}], 2, **kw)


@pytest.mark.parametrize("bad", [-1, 4097, 2.5, True])
def test_trajectories_must_be_a_count_up_to_4096(B, bad):
    m = B.models.linear_gaussian()
    with pytest.raises(ValueError, match="trajectories must be an integer in 0 .. 4096"):
        B.bootstrap_filter(Y, 16, m.init_fn, m.transition_fn, m.log_likelihood_fn, trajectories=bad, **PAR)


def test_the_library_exports_the_entry_point_and_the_structs_match_the_header(B):
    import ctypes as C
    from bayesssm_amd import _lib
    assert "bssm_pf_run_smooth" in _lib.EXPORTED_SYMBOLS
    assert C.sizeof(_lib.SmoothConfig) == C.sizeof(C.c_int) and C.sizeof(_lib.SmoothResult) == 7 * C.sizeof(C.c_void_p)
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "bayesssm_amd.h")) as f:
        text = f.read()
    body = text[text.index("} bssm_smooth_config;"):text.index("} bssm_smooth_result;")]
    names = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines() if ";" in ln and "(" not in ln.split(";")[0] and not ln.startswith("}")]
    assert names == [k for k, _ in _lib.SmoothResult._fields_], names
