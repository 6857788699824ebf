"""CPU tests of the batched smoother's host side: the path a PMMH chain carries (run_chains_host_lockstep with scripted filters and
scripted acceptances), the refusals of pmmh(return_latent_trajectories=True) and of bootstrap_smoother_batch that are raised before
any device work, and the ctypes struct against the header."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


class ScriptedRng:
    """standard_normal(p): the scripted proposal steps in order; random(): the scripted acceptance uniforms in order"""

    def __init__(self, steps, uniforms):
        self.steps, self.uniforms = list(steps), list(uniforms)

    def standard_normal(self, p):
        return np.full(p, self.steps.pop(0))

    def random(self):
        return self.uniforms.pop(0)


class FlatOn:
    """log prior 0 on [lo, hi], -inf outside"""
    kind = "uniform"

    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def __call__(self, x):
        return 0.0 if self.lo <= x <= self.hi else -np.inf


T1, D = 4, 2


def _path(theta, call):
    return np.full((T1, D), 100.0 * call + theta)


def _run(pmmh_mod, triples, steps, uniforms, m, with_tag=True):
    """one chain from theta = 0 with unit proposal variance (the proposal is cur + step) and a constant log-likelihood: the acceptance
    ratio is 0, so the scripted uniform alone decides (u < 1 accepts, u = 1 rejects: log(1) < 0 is false)"""
    calls = []

    def pf_batch(thetas, ns, who):
        out = []
        for th in thetas:
            calls.append(float(th[0]))
            r = (-1.0, np.full(T1, float(th[0])))
            if triples:
                r += (_path(float(th[0]), len(calls)),) + ((len(calls),) if with_tag else ())
            out.append(r)
        return out

    res = pmmh_mod.run_chains_host_lockstep(pf_batch, [[0.0]], [np.eye(1)], [10], ["identity"], [FlatOn(-5.0, 5.0)],
                                            [ScriptedRng(steps, uniforms)], m, return_latent_state_est=True)[0]
    return res, calls


def test_the_path_chain_follows_accept_and_reject(B):
    P = importlib.import_module("bayesssm_amd.pmmh")
    # iteration 1 accepts (+1), 2 rejects (+1), 3 proposes outside the prior support (+10: no filter, no uniform), 4 accepts (-0.5)
    steps, uniforms = [1.0, 1.0, 10.0, -0.5], [0.5, 1.0, 0.5]
    res, calls = _run(P, True, steps, uniforms, 5)
    assert calls == [0.0, 1.0, 2.0, 0.5]                                     # the initial filter, then one per proposal inside the support
    assert np.array_equal(res["theta_chain"][:, 0], [0.0, 1.0, 1.0, 1.0, 0.5]) and res["accepted"] == 2
    tc = res["trajectory_chain"]
    assert tc.shape == (5, T1, D)
    want = [_path(0.0, 1), _path(1.0, 2), _path(1.0, 2), _path(1.0, 2), _path(0.5, 4)]
    for i in range(5):
        assert np.array_equal(tc[i], want[i]), i
    assert np.array_equal(res["trajectory_tag"], [1, 2, 2, 2, 4])            # the filter call whose path is current
    # the path changes exactly where theta does (here every accepted proposal moves theta)
    moved = np.any(np.diff(res["theta_chain"], axis=0) != 0, axis=1)
    assert np.array_equal(np.any(tc[1:] != tc[:-1], axis=(1, 2)), moved)
    # triples without the tag: the path is carried, the tag chain is absent
    res3, _ = _run(P, True, steps, uniforms, 5, with_tag=False)
    assert np.array_equal(res3["trajectory_chain"], tc) and res3["trajectory_tag"] is None


def test_pairs_give_what_they_gave(B):
    P = importlib.import_module("bayesssm_amd.pmmh")
    steps, uniforms = [1.0, 1.0, 10.0, -0.5], [0.5, 1.0, 0.5]
    pairs, calls2 = _run(P, False, steps, uniforms, 5)
    triples, calls3 = _run(P, True, steps, uniforms, 5)
    assert calls2 == calls3
    assert sorted(pairs) == ["accepted", "device_ms", "state_est_chain", "theta_chain"]           # no new key for callers that return pairs
    for k in ("theta_chain", "state_est_chain", "accepted"):
        assert np.array_equal(pairs[k], triples[k]), k
    assert np.array_equal(pairs["state_est_chain"][:, 0], [0.0, 1.0, 1.0, 1.0, 0.5])


def _closures():
    return (lambda num_particles, **k: np.zeros(num_particles), lambda particles, **k: particles, lambda y, particles, **k: np.zeros(particles.size))


def test_return_latent_trajectories_is_refused_outside_the_two_families(B):
    y = np.array([0.1, -0.2, 0.3])
    msg = "return_latent_trajectories runs for the multivariate linear-Gaussian family .* and the reaction networks"
    pri = {"phi": B.prior_uniform(0, 1), "sigma_x": B.prior_exponential(1), "sigma_y": B.prior_exponential(1)}
    init = [{"phi": 0.5, "sigma_x": 1.0, "sigma_y": 1.0}]
    with pytest.raises(ValueError, match=msg):                                                    # closure model
        B.pmmh(B.bootstrap_filter, y, 10, *_closures(), {}, [{}], 2, num_chains=1, return_latent_trajectories=True)
    for m in (B.models.linear_gaussian(), B.models.ar1_sin()):
        with pytest.raises(ValueError, match=msg):                                                # scalar built-ins
            B.pmmh(B.bootstrap_filter, y, 10, m.init_fn, m.transition_fn, m.log_likelihood_fn, pri, init, 2, num_chains=1,
                   return_latent_trajectories=True)
    sir = B.models.sir()
    with pytest.raises(ValueError, match=msg):
        B.pmmh(B.bootstrap_filter, np.array([3.0, 4.0]), 10, sir.init_fn, sir.transition_fn, sir.log_likelihood_fn,
               {"lambda": B.prior_exponential(1), "gamma": B.prior_exponential(1)}, [{"lambda": 0.5, "gamma": 0.2}], 2, num_chains=1,
               return_latent_trajectories=True)
    m = B.models.linear_gaussian()
    with pytest.raises(ValueError, match=msg):                                                    # r_stream
        B.pmmh(B.bootstrap_filter, y, 10, m.init_fn, m.transition_fn, m.log_likelihood_fn, pri, init, 2, num_chains=1, seed=1, r_stream=True,
               return_latent_trajectories=True)


@pytest.mark.parametrize("bad", [-1, 4097, 2.5, True])
def test_smoother_batch_trajectories_must_be_a_count_up_to_4096(B, bad):
    m = B.models.linear_gaussian()
    with pytest.raises(ValueError, match="trajectories must be an integer in 0 .. 4096"):
        B.bootstrap_smoother_batch(np.zeros(3), 16, m.init_fn, m.transition_fn, m.log_likelihood_fn, np.array([[0.8, 1.0, 1.0]]), trajectories=bad)


def test_smoother_batch_refuses_the_scalar_models(B):
    for m, th in ((B.models.linear_gaussian(), [[0.8, 1.0, 1.0]]), (B.models.sir(), [[0.5, 0.2, 1000.0, 990.0, 10.0]])):
        with pytest.raises(ValueError, match="bootstrap_smoother_batch: the multivariate linear-Gaussian family .* and the reaction networks"):
            B.bootstrap_smoother_batch(np.array([3.0, 4.0, 5.0]), 16, m.init_fn, m.transition_fn, m.log_likelihood_fn, np.array(th), trajectories=1)
    with pytest.raises(TypeError):                                                                # closures are no descriptors
        B.bootstrap_smoother_batch(np.zeros(3), 16, *_closures(), np.array([[0.8, 1.0, 1.0]]))


def test_the_library_exports_the_entry_point_and_the_struct_matches_the_header(B):
    from bayesssm_amd import _lib
    assert "bssm_pf_run_batch_smooth" in _lib.EXPORTED_SYMBOLS
    assert C.sizeof(_lib.SmoothBatchResult) == 7 * C.sizeof(C.c_void_p)
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "bayesssm_amd.h")) as f:
        text = f.read()
    end = text.index("} bssm_smooth_batch_result;")
    body = text[text.rindex("typedef struct {", 0, end):end]
    names = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines() if ";" in ln and "(" not in ln.split(";")[0] and not ln.startswith("}")]
    assert names == [k for k, _ in _lib.SmoothBatchResult._fields_], names
    proto = text[text.index("int bssm_pf_run_batch_smooth("):]
    proto = proto[:proto.index(";")]
    assert proto.count(",") == 9 and "const bssm_mv_tv_batch* tv" in proto and "bssm_smooth_batch_result* sres" in proto
    lib = _lib.load()                                                                             # the built library has the symbol
    assert lib.bssm_pf_run_batch_smooth.argtypes is not None and len(lib.bssm_pf_run_batch_smooth.argtypes) == 10
