"""Parameter-dependent time-varying b / h0 / H of the multivariate linear-Gaussian family, host side (no GPU): `build` may
return "time_varying" next to its constant pieces; the arrays are checked as the constructor's are; bootstrap_filter_batch
raises its argument errors before any context is created; the C ABI's new entry and struct are bound."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, P, T = 3, 2, 12
OBS_TIMES = [1, 2, 2, 5, 6, 6, 7, 9, 10, 11, 13, 14]
_rng = np.random.default_rng(20260)
U = _rng.standard_normal((16, D))               # known inputs: more rows than the last observation time
S = _rng.standard_normal((T, P))                # seasonal pattern
H0 = _rng.standard_normal((T, P, D))
A0 = 0.5 * np.eye(D)


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


def _model(B, U_=U, S_=S, **kw):
    return B.models.linear_gaussian_mv(D, P, build=lambda g, a: {"A": A0, "time_varying": {"b": g * U_, "h0": a * S_}},
                                       param_names=("g", "a"), **kw)


def test_pack_ignores_the_time_varying_key(B):
    m = _model(B)
    plain = B.models.linear_gaussian_mv(D, P, build=lambda g, a: {"A": A0}, param_names=("g", "a"))
    q = {"g": 1.7, "a": 0.4}
    np.testing.assert_array_equal(m.pack(q), plain.pack(q))
    assert m.pack(q).size == 2 + D + 3 * D * D + D + 1 + P * D + 2 * P         # n_theta unchanged
    assert m.has_param_tv and not plain.has_param_tv


def test_has_param_tv_is_decided_by_the_first_build(B):
    m = _model(B)
    assert not m.has_param_tv                         # nothing built yet
    m.tv_arrays(T, OBS_TIMES, {"g": 1.0, "a": 1.0})
    assert m.has_param_tv
    assert not B.models.linear_gaussian_mv(D, P).has_param_tv
    flip = B.models.linear_gaussian_mv(D, P, build=lambda g: ({"time_varying": {"b": g * U}} if g > 0 else {}), param_names=("g",))
    flip.pack({"g": 1.0})
    with pytest.raises(ValueError, match="for every parameter draw or for none"):
        flip.pack({"g": -1.0})


def test_tv_arrays_of_a_draw(B):
    m = _model(B, time_varying={"H": H0, "b": np.zeros((20, D))})
    n_times, b, h0, H = m.tv_arrays(T, OBS_TIMES, {"g": 1.7, "a": 0.4})
    np.testing.assert_array_equal(b, 1.7 * U)          # build's b replaces the constructor's
    np.testing.assert_array_equal(h0, 0.4 * S)
    np.testing.assert_array_equal(H, H0)               # a piece build does not return keeps the constructor's
    assert n_times == 16 and b.flags.c_contiguous and b.dtype == np.float64
    # the two-argument call: the constructor's arrays, as before
    n2, b2, h02, H2 = m.tv_arrays(T, OBS_TIMES)
    assert n2 == 20 and h02 is None and H2 is H and not b2.any()
    assert _model(B).tv_arrays(T, OBS_TIMES) is None
    plain = B.models.linear_gaussian_mv(D, P, build=lambda g, a: {"A": A0}, param_names=("g", "a"), time_varying={"H": H0})
    assert plain.tv_arrays(T, None, {"g": 1.0, "a": 1.0})[3] is plain.tv_arrays(T)[3]
    with pytest.raises(TypeError, match='"a" is missing'):
        m.tv_arrays(T, OBS_TIMES, {"g": 1.0})


def test_same_validation_messages_as_the_constructor(B):
    q = {"g": 1.0, "a": 1.0}
    for bad_build, ctor_tv in (({"b": np.zeros((16, D + 1))}, None), ({"h0": np.zeros(T)}, None), ({"H": np.zeros((T, D))}, None)):
        with pytest.raises(ValueError, match="must have shape") as e_ctor:
            B.models.linear_gaussian_mv(D, P, time_varying=bad_build)
        m = B.models.linear_gaussian_mv(D, P, build=lambda g, a, tv=bad_build: {"time_varying": tv}, param_names=("g", "a"))
        with pytest.raises(ValueError) as e_build:
            m.tv_arrays(T, OBS_TIMES, q)
        assert str(e_build.value) == str(e_ctor.value)
    Un = U.copy()
    Un[3, 1] = np.inf
    with pytest.raises(ValueError, match=r"time_varying\['b'\] contains non-finite values"):
        _model(B, U_=Un).tv_arrays(T, OBS_TIMES, q)
    with pytest.raises(ValueError, match=r"time_varying\['b'\] contains non-finite values"):
        _model(B, U_=Un).pack(q)                       # the arrays are checked whenever build is called
    with pytest.raises(ValueError, match=r"time_varying\['b'\] has 13 rows \(n_times\); the last observation time is 14"):
        _model(B, U_=U[:13]).tv_arrays(T, OBS_TIMES, q)
    with pytest.raises(ValueError, match=r"time_varying\['h0'\] has 11 rows; y has 12 observations"):
        _model(B, S_=S[:11]).tv_arrays(T, OBS_TIMES, q)
    with pytest.raises(TypeError, match="unknown time-varying piece 'A'"):
        B.models.linear_gaussian_mv(D, P, build=lambda g: {"time_varying": {"A": A0}}, param_names=("g",)).pack({"g": 1.0})


def _call(B, m, thetas, F=None, **kw):
    return B.bootstrap_filter_batch(np.zeros((T, P)), 100, m.init_fn, m.transition_fn, m.log_likelihood_fn, thetas, 1,
                                    obs_times=OBS_TIMES, **kw)


def test_batch_argument_errors_need_no_device(B, monkeypatch):
    from bayesssm_amd import _lib

    def no_context(*a, **k):
        raise AssertionError("a context was requested before the arguments were checked")
    monkeypatch.setattr(_lib, "default_context", no_context)
    m = _model(B)
    blocks = np.array([m.pack({"g": 1.0 + k, "a": 0.5}) for k in range(3)])
    b2 = np.stack([U, 2 * U])
    with pytest.raises(ValueError, match="one set per filter"):
        _call(B, m, blocks, time_varying={"b": b2})                              # G = 2 sets for F = 3 filters, no tv_set
    with pytest.raises(ValueError, match="agree on the number of sets"):
        _call(B, m, blocks, time_varying={"b": b2, "h0": np.stack([S, S, S])})
    with pytest.raises(ValueError, match=r"set indices must lie in \[0, 2\)"):
        _call(B, m, blocks, time_varying={"b": b2}, tv_set=[0, 1, 2])
    with pytest.raises(ValueError, match=r"set indices must lie in \[0, 2\)"):
        _call(B, m, blocks, time_varying={"b": b2}, tv_set=[0, -1, 1])
    with pytest.raises(ValueError, match="one integer set index per filter"):
        _call(B, m, blocks, time_varying={"b": b2}, tv_set=[0, 1])
    with pytest.raises(ValueError, match="one integer set index per filter"):
        _call(B, m, blocks, time_varying={"b": b2}, tv_set=[0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="time_varying="):
        _call(B, m, blocks)                                                      # packed blocks, parameter-dependent arrays
    with pytest.raises(ValueError, match="tv_set is given without time_varying"):
        _call(B, B.models.linear_gaussian_mv(D, P), np.array([B.models.linear_gaussian_mv(D, P).pack({})] * 3), tv_set=[0, 0, 0])
    # every set is checked as one filter's arrays are
    with pytest.raises(ValueError, match=r"time_varying\['b'\] must have shape \(n_times, 3\)"):
        _call(B, m, blocks, time_varying={"b": np.zeros((3, 16, D + 1))})
    bn = np.stack([U, U, U])
    bn[1, 5, 0] = np.nan
    with pytest.raises(ValueError, match=r"time_varying\['b'\] contains non-finite values"):
        _call(B, m, blocks, time_varying={"b": bn})
    with pytest.raises(ValueError, match="the last observation time is 14"):
        _call(B, m, blocks, time_varying={"b": np.zeros((3, 13, D))})
    with pytest.raises(ValueError, match=r"time_varying\['h0'\] has 11 rows"):
        _call(B, m, blocks, time_varying={"h0": np.zeros((3, 11, P))})
    with pytest.raises(ValueError, match="the last observation time is 14"):
        _call(B, _model(B, U_=U[:13]), [{"g": 1.0, "a": 1.0}, {"g": 2.0, "a": 1.0}])     # the assembled sets too
    lg = B.models.linear_gaussian()
    with pytest.raises(ValueError, match="multivariate linear-Gaussian family only"):
        B.bootstrap_filter_batch(np.zeros(T), 100, lg.init_fn, lg.transition_fn, lg.log_likelihood_fn, np.ones((2, 3)), 1,
                                 time_varying={"b": U})


def test_sets_are_assembled_from_equal_draws(B):
    from bayesssm_amd import filters
    m = _model(B, time_varying={"H": H0})
    ot = np.asarray(OBS_TIMES, dtype=np.int32)
    draws = [{"g": 1.0, "a": 2.0}, {"g": 3.0, "a": 2.0}, {"g": 1.0, "a": 2.0}, {"g": 3.0, "a": 2.0}, {"g": 3.0, "a": 2.0}]
    m.pack(draws[0])
    n_times, n_sets, set_of, pieces = filters._mv_batch_tv(m, len(draws), T, ot, draws, None, None)
    assert (n_times, n_sets) == (16, 2) and set_of.dtype == np.int32 and set_of.tolist() == [0, 1, 0, 1, 1]
    np.testing.assert_array_equal(pieces["b"][0], np.stack([1.0 * U, 3.0 * U]))
    assert pieces["b"][1] == 16 * D and pieces["h0"][1] == T * P
    assert pieces["H"][0] is m.time_varying["H"] and pieces["H"][1] == 0        # the constructor's piece: one shared array
    # one set per filter in order needs no index array; one set for all is a shared array
    assert filters._mv_batch_tv(m, 2, T, ot, draws[:2], None, None)[2] is None
    n_times, n_sets, set_of, pieces = filters._mv_batch_tv(m, 2, T, ot, [draws[0], draws[2]], None, None)
    assert n_sets == 1 and set_of is None and all(stride == 0 for _, stride in pieces.values())


def test_c_abi_is_bound():
    from bayesssm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bayesssm_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} bssm_mv_tv_batch;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in _lib.MvTvBatch._fields_]
    assert names == ["n_times", "n_sets", "set_of", "b_t", "b_stride", "h0_t", "h0_stride", "H_t", "H_stride"]
    assert "bssm_pf_run_batch_tv" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.bssm_pf_run_batch_tv.argtypes[6]._type_ is _lib.MvTvBatch
    assert [f[0] for f in _lib.MvTv._fields_] == ["n_times", "b_t", "h0_t", "H_t"]          # the single-filter struct: untouched
