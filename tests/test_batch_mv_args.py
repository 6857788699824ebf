"""bootstrap_filter_batch on the multivariate linear-Gaussian family: argument errors are raised on the host, before any
context is created (no GPU needed), and the capacity of the batched kernel is a host-side number."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


def _model(B, d=3, p=2):
    return B.models.linear_gaussian_mv(d, p, build=lambda a: {"A": a * np.eye(d)}, param_names=("a",))


def _call(B, m, y, thetas, N=100, **kw):
    return B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, thetas, 1, **kw)


def test_y_shape_errors(B):
    m = _model(B)
    th = [{"a": 0.5}, {"a": 0.7}]
    with pytest.raises(ValueError, match="T x 2 matrix"):
        _call(B, m, np.zeros(10), th)                      # a vector for p = 2
    with pytest.raises(ValueError, match="T x 2 matrix"):
        _call(B, m, np.zeros((10, 3)), th)                 # the wrong number of columns
    with pytest.raises(ValueError, match="T x 2 matrix"):
        _call(B, m, np.zeros((10, 2, 1)), th)
    y = np.zeros((10, 2))
    y[4, 1] = np.nan
    with pytest.raises(ValueError, match="missing values"):
        _call(B, m, y, th)
    with pytest.raises(ValueError, match="obs_times"):
        _call(B, m, np.zeros((10, 2)), th, obs_times=np.arange(1, 10))


def test_thetas_forms_and_mixed_dimensions(B):
    m = _model(B)
    y = np.zeros((10, 2))
    blocks = np.array([m.pack({"a": 0.5}), m.pack({"a": 0.7})])
    with pytest.raises(ValueError, match="packed blocks"):
        _call(B, m, y, {"a": 0.5})                         # one dict, not a list of them
    with pytest.raises(ValueError, match="packed blocks"):
        _call(B, m, y, blocks[0])                          # one block, not an (F, n_theta) array
    with pytest.raises(ValueError, match="packed blocks"):
        _call(B, m, y, blocks[:, :-1])                     # the wrong block length
    with pytest.raises(ValueError, match="packed blocks"):
        _call(B, m, y, np.zeros((0, blocks.shape[1])))     # no filters
    with pytest.raises(TypeError, match='"a" is missing'):
        _call(B, m, y, [{"a": 0.5}, {"b": 0.7}])           # a dict without the model's parameter
    mixed = blocks.copy()
    mixed[1, :2] = (2, 3)                                  # another (d, p) with a block of the same length
    with pytest.raises(ValueError, match=r"\(d, p\) = \(3, 2\)"):
        _call(B, m, y, mixed)
    other = _model(B, 2, 1).pack({"a": 0.5})
    with pytest.raises(ValueError):
        _call(B, m, y, [blocks[0], other])                 # blocks of two models


def test_batch_capacity_is_a_host_number(B):
    assert B.batch_max_particles() == 2048                 # the scalar models: unchanged
    caps = [B.batch_max_particles(d) for d in range(1, 9)]
    assert all(c >= 2048 for c in caps[:4]) and all(c >= 1000 for c in caps)
    assert all(a >= b for a, b in zip(caps, caps[1:]))
    assert B.batch_max_particles(0) == 0 and B.batch_max_particles(9) == 0
