"""Rate schedules of the reaction-network family (models.reaction_network(rate_schedule=)) without a GPU: the packed block at its three
lengths, the dict and array forms, a schedule returned by `build`, every refusal, and the restatement of the definition
(tests/rnet_tv_restated.py): a schedule of ones is the existing restatement bit for bit, a column of zeros switches a reaction off."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_inc_restated as RI  # noqa: E402
import rnet_tv_restated as RT  # noqa: E402

OT = (1, 2, 5, 5, 6, 9)              # gap 1, gap 1, gap 3, a repeated time, gap 1, gap 3
NT = 9                               # the last observation time

SEIR_REACTIONS = [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1, "C": 1}, "sigma"), ({"I": 1}, {"R": 1}, "gamma")]
SEIR_PAR = dict(beta=0.004, sigma=0.5, gamma=0.3)


def seir_c(B, **kw):
    """the README's SEIR with the onset species C (a counter only with counters=("C",))"""
    return B.models.reaction_network(("S", "E", "I", "R", "C"), SEIR_REACTIONS, x0=(180, 8, 12, 0, 0), observe={"C": 0.6}, **kw)


def pattern(nt, R):
    """entries that all differ: a wrong row or column cannot pass"""
    return 0.5 + ((7 * np.arange(nt)[:, None] + 3 * np.arange(R)[None, :]) % 11) / 10.0


def test_pack_layout_at_the_three_lengths():
    import bayesssm_amd as B
    plain = seir_c(B).pack(SEIR_PAR)
    tail = seir_c(B, counters=("C",)).pack(SEIR_PAR)
    n = 3 + 5 + 3 * 3 + 3 * 5 + 5
    assert plain.size == n and tail.size == n + 5
    M = pattern(NT, 3)
    assert len(set(M.reshape(-1))) > 10
    for counters, reset in (((), [0, 0, 0, 0, 0]), (("C",), [0, 0, 0, 0, 1])):
        m = seir_c(B, counters=counters, rate_schedule=M)
        b = m.pack(SEIR_PAR)
        assert b.dtype == np.float64 and b.size == n + 5 + 1 + NT * 3 == m.n_theta()
        assert np.array_equal(b[:n], plain)                                   # without a schedule: today's bytes in front
        assert np.array_equal(b[n:n + 5], reset)                              # reset[d] always, zeros without counters
        assert b[n + 5] == NT and np.array_equal(b[n + 6:].reshape(NT, 3), M)
        base, rs, Ms = RT.split(b)
        assert np.array_equal(base, plain) and np.array_equal(rs, reset) and np.array_equal(Ms, M)
    assert RT.split(plain)[1:] == (None, None) and RT.split(tail)[2] is None
    # without a schedule pack() returns what it returned before, byte for byte
    assert seir_c(B, rate_schedule=None).pack(SEIR_PAR).tobytes() == plain.tobytes()
    assert seir_c(B, counters=("C",), rate_schedule=None).pack(SEIR_PAR).tobytes() == tail.tobytes()


def test_dict_and_array_forms():
    import bayesssm_amd as B
    v = np.linspace(0.2, 1.8, NT)
    M = np.ones((NT, 3)); M[:, 0] = v
    want = seir_c(B, rate_schedule=M).pack(SEIR_PAR)
    assert np.array_equal(seir_c(B, rate_schedule={"beta": v}).pack(SEIR_PAR), want)
    assert np.array_equal(seir_c(B, rate_schedule={0: list(v)}).pack(SEIR_PAR), want)
    both = seir_c(B, rate_schedule={"gamma": v, 1: 2 * v}).rate_schedule
    assert np.array_equal(both[:, 2], v) and np.array_equal(both[:, 1], 2 * v) and np.all(both[:, 0] == 1.0)
    # one name shared by two reactions applies to both; the reaction not named gets 1.0
    two = B.models.reaction_network(("S", "I"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"S": 1}, {"I": 1}, "beta"), ({"I": 1}, {}, "gamma")],
                                    x0=(50, 5), observe={"I": 1.0}, rate_schedule={"beta": v})
    assert np.array_equal(two.rate_schedule[:, 0], v) and np.array_equal(two.rate_schedule[:, 1], v) and np.all(two.rate_schedule[:, 2] == 1.0)
    # the descriptor keeps its own copy
    M2 = M.copy(); m = seir_c(B, rate_schedule=M2); M2[:] = 7.0
    assert np.array_equal(m.pack(SEIR_PAR), want)


def test_build_returns_a_schedule():
    import bayesssm_amd as B
    t0 = 4

    def build(beta, sigma, gamma, rho):
        col = np.ones(NT); col[t0:] = rho
        return {"rates": {"beta": beta, "sigma": sigma, "gamma": gamma}, "rate_schedule": {"beta": col}}

    m = seir_c(B, build=build, param_names=("beta", "sigma", "gamma", "rho"))
    assert m.n_theta() is None                                # only a pack can tell
    b = m.pack(dict(SEIR_PAR, rho=0.4))
    n = 3 + 5 + 3 * 3 + 3 * 5 + 5
    assert b.size == n + 5 + 1 + NT * 3 and m.n_theta_ok(b.size) and not m.n_theta_ok(b.size - 1)
    many = m.pack_many([dict(SEIR_PAR, rho=0.4), dict(SEIR_PAR, rho=0.7)])
    assert many.shape == (2, b.size) and np.array_equal(many[0], b) and RT.split(many[1])[2][t0, 0] == 0.7
    Ms = RT.split(b)[2]
    assert np.all(Ms[:t0, 0] == 1.0) and np.all(Ms[t0:, 0] == 0.4) and np.all(Ms[:, 1:] == 1.0)
    assert RT.split(m.pack(dict(SEIR_PAR, rho=0.7)))[2][t0, 0] == 0.7     # each draw packs its own
    # the build's schedule replaces the constructor's for the draw
    m2 = seir_c(B, build=build, param_names=("beta", "sigma", "gamma", "rho"), rate_schedule=np.full((NT, 3), 2.0))
    assert RT.split(m2.pack(dict(SEIR_PAR, rho=0.4)))[2][0, 1] == 1.0

    def shrinking(beta, sigma, gamma, rho):
        return {"rate_schedule": np.ones((NT if rho < 0.5 else NT - 1, 3))}

    # the draws of one call are compared with each other; the descriptor itself remembers nothing between calls
    m3 = seir_c(B, build=shrinking, param_names=("beta", "sigma", "gamma", "rho"))
    lo, hi = dict(SEIR_PAR, rho=0.4), dict(SEIR_PAR, rho=0.6)
    assert m3.pack(lo).size == m3.pack(hi).size + 3 == m3.pack(lo).size
    fns3 = (m3.init_fn, m3.transition_fn, m3.log_likelihood_fn)
    with pytest.raises(ValueError, match="n_theta changed between draws"):
        m3.pack_many([lo, lo, hi])
    with pytest.raises(ValueError, match="n_theta changed between draws"):
        B.bootstrap_filter_batch(np.array([3.0, 4, 2, 5, 1, 6]), 64, *fns3, [lo, hi], 1, [0, 1])

    def sometimes(beta, sigma, gamma, rho):
        return {"rate_schedule": np.ones((NT, 3))} if rho < 0.5 else {}

    m4 = seir_c(B, build=sometimes, param_names=("beta", "sigma", "gamma", "rho"))
    with pytest.raises(ValueError, match="n_theta changed between draws"):
        m4.pack_many([lo, hi])
    with pytest.raises(ValueError, match="n_theta changed between draws"):   # against the constructor's n_times
        seir_c(B, build=shrinking, param_names=("beta", "sigma", "gamma", "rho"), rate_schedule=np.ones((NT, 3))).pack(dict(SEIR_PAR, rho=0.6))
    with pytest.raises(TypeError, match="build may return"):
        seir_c(B, build=lambda **kw: {"schedule": 1}, param_names=("beta", "sigma", "gamma")).pack(SEIR_PAR)


def test_refusals():
    import bayesssm_amd as B
    ok = np.ones((NT, 3))
    for bad in (np.ones(NT), np.ones((NT, 2)), np.ones((NT, 4)), np.ones((0, 3)), np.ones((2, NT, 3))):
        with pytest.raises(ValueError, match="rate_schedule has the wrong shape"):
            seir_c(B, rate_schedule=bad)
    for bad in ({"beta": np.ones((NT, 1))}, {"beta": np.ones(NT), "gamma": np.ones(NT - 1)}, {}, {"beta": []}):
        with pytest.raises(ValueError, match="rate_schedule has the wrong shape"):
            seir_c(B, rate_schedule=bad)
    with pytest.raises(ValueError, match="rate_schedule names the unknown rate 'delta'"):
        seir_c(B, rate_schedule={"delta": np.ones(NT)})
    for idx in (3, -1):
        with pytest.raises(ValueError, match="rate_schedule names the unknown reaction index"):
            seir_c(B, rate_schedule={idx: np.ones(NT)})
    for v in (-0.5, np.nan, np.inf):
        bad = ok.copy(); bad[4, 1] = v
        with pytest.raises(ValueError, match="rate_schedule multipliers must be finite and >= 0"):
            seir_c(B, rate_schedule=bad)
        with pytest.raises(ValueError, match="rate_schedule multipliers must be finite and >= 0"):
            seir_c(B, rate_schedule={"sigma": bad[:, 1]})
        with pytest.raises(ValueError, match="rate_schedule multipliers must be finite and >= 0"):
            seir_c(B, build=lambda beta, sigma, gamma: {"rate_schedule": bad}, param_names=("beta", "sigma", "gamma")).pack(SEIR_PAR)
    # n_times short of the last observation time: refused by every entry point before a context exists (none can: no GPU here)
    y = np.array([3.0, 4, 2, 5, 1, 6])
    short = seir_c(B, rate_schedule=np.ones((NT - 1, 3)))
    fns = (short.init_fn, short.transition_fn, short.log_likelihood_fn)
    msg = "rate_schedule has n_times = 8 rows, short of the last observation time 9"
    with pytest.raises(ValueError, match=msg):
        B.bootstrap_filter(y, 64, *fns, obs_times=OT, **SEIR_PAR)
    with pytest.raises(ValueError, match=msg):
        B.auxiliary_filter(y, 64, *fns, short.aux_log_likelihood_fn, obs_times=OT, **SEIR_PAR)
    with pytest.raises(ValueError, match=msg):
        B.bootstrap_filter_batch(y, 64, *fns, [SEIR_PAR] * 2, 1, [0, 1], obs_times=OT)
    with pytest.raises(ValueError, match=msg):
        B.bootstrap_filter_batch(y, 64, *fns, np.stack([short.pack(SEIR_PAR)] * 2), 1, [0, 1], obs_times=OT)
    with pytest.raises(ValueError, match=msg):
        B.pmmh(B.bootstrap_filter, y, 3, *fns, {k: (lambda v: 0.0) for k in SEIR_PAR}, [dict(SEIR_PAR)] * 2, burn_in=1, num_chains=2, obs_times=OT)
    five = seir_c(B, rate_schedule=np.ones((5, 3)))                  # without obs_times the last time is T = 6
    with pytest.raises(ValueError, match="n_times = 5 rows, short of the last observation time 6"):
        B.bootstrap_filter(y, 64, five.init_fn, five.transition_fn, five.log_likelihood_fn, **SEIR_PAR)
    with pytest.raises(ValueError, match="n_times = 5 rows, short of the last observation time 6"):
        B.pmmh(B.bootstrap_filter, y, 3, five.init_fn, five.transition_fn, five.log_likelihood_fn, {k: (lambda v: 0.0) for k in SEIR_PAR},
               [dict(SEIR_PAR)] * 2, burn_in=1, num_chains=2)
    # a batched call's packed blocks have the descriptor's length
    full = seir_c(B, rate_schedule=ok)
    with pytest.raises(ValueError, match="array of packed blocks"):
        B.bootstrap_filter_batch(y, 64, full.init_fn, full.transition_fn, full.log_likelihood_fn, np.stack([full.pack(SEIR_PAR)[:-1]] * 2), 1, [0, 1],
                                 obs_times=OT)


def _check_call_times():
    """the rows by call number: BPF gaps 1, 1, 3, 0, 1, 3; the APF's second-stage call and its look-ahead take the observation's time.
    (The restatement's own bookkeeping: called from the test below, which runs the library's pack() as well.)"""
    calls, aux = RT.call_times(6, OT, "BPF")
    assert [calls[k][0] for k in range(9)] == [1, 2, 3, 4, 5, 6, 7, 8, 9] and all(v[1] == "gap" for v in calls.values()) and aux == list(OT)
    calls, aux = RT.call_times(6, OT, "APF")
    assert [calls[k] for k in range(15)] == [(1, "gap"), (1, "second"), (2, "gap"), (2, "second"), (3, "gap"), (4, "gap"), (5, "gap"), (5, "second"),
                                             (5, "second"), (6, "gap"), (6, "second"), (7, "gap"), (8, "gap"), (9, "gap"), (9, "second")]
    assert aux == list(OT)
    assert RT.call_times(3, None, "APF")[0] == {0: (1, "gap"), 1: (1, "second"), 2: (2, "gap"), 3: (2, "second"), 4: (3, "gap"), 5: (3, "second")}


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_restated_ones_equal_the_existing_restatement(oracle, algorithm):
    """a schedule of ones in the restatement = rnet_inc_restated on the block without it, every output bit for bit, with the counter,
    the gaps and the repeated time (k * 1.0 is exact); and the rows the calls read are the definition's"""
    import bayesssm_amd as B
    _check_call_times()
    N, T = 24, len(OT)
    y = np.array([1, 2, 6, 5, 3, 8], dtype=np.float64)
    u = np.random.default_rng(5).random((2 * T, N))
    par = dict(beta=0.0015, sigma=0.25, gamma=0.1)
    kw = dict(seed=7, stream=1, algorithm=algorithm, resample_algorithm="SISAR", obs_times=OT, return_particles=True)
    ref = RI.pf_run_rn(oracle, seir_c(B, counters=("C",)).pack(par), y, N, u, **kw)
    counts = {}
    got = RT.pf_run_rn(oracle, seir_c(B, counters=("C",), rate_schedule=np.ones((NT, 3))).pack(par), y, N, u, counts=counts, **kw)
    assert np.isfinite(ref["loglike"]) and got["loglike"] == ref["loglike"]
    for k in ("state_est", "ess", "loglike_history", "resampled", "ancestors", "particles_history", "weights_history"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert ref["particles_history"].reshape(T + 1, 5, N)[-1, 4].sum() > 0          # (the counter counted)
    rows = counts["rows"]
    assert [r[2] for r in rows if r[0] == "gap"] == list(range(9))
    if algorithm == "APF":
        assert [r[2] for r in rows if r[0] == "second"] == [t - 1 for t in OT] == [r[2] for r in rows if r[0] == "aux"]
    else:
        assert not [r for r in rows if r[0] != "gap"]
    # without a schedule the new restatement is the old one too
    plain = RT.pf_run_rn(oracle, seir_c(B, counters=("C",)).pack(par), y, N, u, **kw)
    np.testing.assert_array_equal(plain["particles_history"], ref["particles_history"])


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_restated_zero_column_switches_the_infection_off(oracle, algorithm):
    """a column of zeros for the infection: S stays at x0 exactly in every particle at every observation, while the other reactions
    fire; rows with nonzero infection multipliers elsewhere would have moved S (the same run with ones does)"""
    import bayesssm_amd as B
    N, T = 16, len(OT)
    y = np.array([1, 2, 6, 5, 3, 8], dtype=np.float64)
    u = np.random.default_rng(6).random((2 * T, N))
    M = pattern(NT, 3); M[:, 0] = 0.0
    counts = {}
    kw = dict(seed=9, stream=2, algorithm=algorithm, resample_algorithm="SISR", obs_times=OT, return_particles=True)
    res = RT.pf_run_rn(oracle, seir_c(B, rate_schedule=M).pack(SEIR_PAR), y, N, u, counts=counts, **kw)
    ph = res["particles_history"].reshape(-1, 5, N)
    assert np.all(ph[:, 0] == 180.0)
    assert counts["fired"].get(0, 0) == 0 and counts["fired"].get(1, 0) > 0 and counts["fired"].get(2, 0) > 0
    ones = RT.pf_run_rn(oracle, seir_c(B, rate_schedule=np.ones((NT, 3))).pack(SEIR_PAR), y, N, u, **kw)
    assert np.any(ones["particles_history"].reshape(-1, 5, N)[:, 0] < 180.0)
