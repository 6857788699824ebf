"""Counter species and missing observations of the reaction-network family (models.reaction_network(counters=, missing=)) without a
GPU: the packed block with and without the tail reset[d], the new refusals, and the restatement of the definition
(tests/rnet_inc_restated.py) on a pure birth network, where a counter must equal the growth since the previous observation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_inc_restated as RI  # noqa: E402

OT = (1, 2, 5, 5, 6, 9)              # gap 1, gap 3, a repeated time, gap 3 at the end

SEIR_REACTIONS = [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1, "C": 1}, "sigma"), ({"I": 1}, {"R": 1}, "gamma")]
SEIR_PAR = dict(beta=0.004, sigma=0.5, gamma=0.3)


def seir_c(B, **kw):
    """the README's SEIR with the onset counter C"""
    return B.models.reaction_network(("S", "E", "I", "R", "C"), SEIR_REACTIONS, x0=(180, 8, 12, 0, 0), observe={"C": 0.6}, **kw)


def birth(B, **kw):
    return B.models.reaction_network(("X", "C"), [({}, {"X": 1, "C": 1}, "b")], x0=(3, 0), observe={"C": 0.5}, counters=("C",), **kw)


def test_no_counters_and_refuse_is_todays_block():
    """without counters the block is the one built by hand in the layout d, R, p, x0, k, s1, s2, nu, G -- whatever `missing` says"""
    import bayesssm_amd as B
    want = np.array([5, 3, 1, 180, 8, 12, 0, 0, 0.004, 0.5, 0.3, 0, 1, 2, 2, -1, -1,
                     -1, 1, 0, 0, 0, 0, -1, 1, 0, 1, 0, 0, -1, 1, 0, 0, 0, 0, 0, 0.6], dtype=np.float64)
    assert want.size == 3 + 5 + 3 * 3 + 3 * 5 + 5
    for kw in ({}, {"counters": ()}, {"missing": "refuse"}, {"counters": (), "missing": "skip"}):
        m = seir_c(B, **kw)
        b = m.pack(SEIR_PAR)
        assert b.dtype == np.float64 and np.array_equal(b, want), kw
        assert m.counters == () and m.missing == kw.get("missing", "refuse")


def test_tail_layout():
    import bayesssm_amd as B
    plain = seir_c(B).pack(SEIR_PAR)
    m = seir_c(B, counters=("C",))
    b = m.pack(SEIR_PAR)
    assert b.size == plain.size + 5 and np.array_equal(b[:plain.size], plain) and np.array_equal(b[plain.size:], [0, 0, 0, 0, 1])
    base, reset = RI.split(b)
    assert np.array_equal(base, plain) and np.array_equal(reset, [0, 0, 0, 0, 1]) and RI.split(plain)[1] is None
    two = B.models.reaction_network(("A", "B", "C"), [({}, {"A": 1, "B": 1}, 1.0), ({"A": 1}, {"C": 1}, 0.5)], x0=(1, 0, 0), observe={"B": 1.0},
                                    counters=["C", "B"])
    assert np.array_equal(two.pack()[-3:], [0, 1, 1])
    assert np.array_equal(B.models.reaction_network(("A", "B"), [({}, {"A": 1, "B": 1}, 1.0)], (0, 0), {"B": 1.0}, counters="B").pack()[-2:], [0, 1])


def test_new_refusals():
    import bayesssm_amd as B
    with pytest.raises(ValueError, match="unknown species 'Q' in counters"):
        seir_c(B, counters=("Q",))
    with pytest.raises(ValueError, match="counter 'C' is named twice"):
        seir_c(B, counters=("C", "C"))
    with pytest.raises(ValueError, match="counter 'I' is a reactant of reaction 0"):
        seir_c(B, counters=("I",))
    with pytest.raises(ValueError, match="counter 'E' is a reactant of reaction 1"):
        seir_c(B, counters=("C", "E"))
    with pytest.raises(ValueError, match="missing must be one of"):
        seir_c(B, missing="drop")
    good = np.array([3.0, 4, 2, 5, 1, 6])
    for m in (seir_c(B, counters=("C",)), seir_c(B, counters=("C",), missing="skip")):
        fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
        for bad in ((np.nan, np.inf, -np.inf) if m.missing == "refuse" else (np.inf, -np.inf)):
            y = good.copy(); y[2] = bad
            with pytest.raises(ValueError, match="reaction_network: y contains non-finite values"):
                B.bootstrap_filter(y, 64, *fns, **SEIR_PAR)
            with pytest.raises(ValueError, match="reaction_network: y contains non-finite values"):
                B.auxiliary_filter(y, 64, *fns, m.aux_log_likelihood_fn, **SEIR_PAR)
            with pytest.raises(ValueError, match="reaction_network: y contains non-finite values"):
                B.bootstrap_filter_batch(y, 64, *fns, [SEIR_PAR] * 2, 1, [0, 1])
        assert m.y_ok(good) and not m.y_ok(np.array([1.0, np.inf]))
        assert m.y_ok(np.array([1.0, np.nan])) == (m.missing == "skip")
        y = good.copy(); y[1] = np.nan; y[4] = -1.0                  # (the counts' checks cover the observed entries)
        with pytest.raises(ValueError, match="non-finite" if m.missing == "refuse" else "negative"):
            B.bootstrap_filter(y, 64, *fns, **SEIR_PAR)
    y = good.copy(); y[0] = np.nan                                    # pmmh's own check of y: NaN under "refuse"
    m = seir_c(B, counters=("C",))
    with pytest.raises(ValueError, match="Contains missing values"):
        B.pmmh(B.bootstrap_filter, y, 3, m.init_fn, m.transition_fn, m.log_likelihood_fn, {k: (lambda v: 0.0) for k in SEIR_PAR},
               [dict(SEIR_PAR)] * 2, burn_in=1, num_chains=2)
    with pytest.raises(ValueError, match="Contains missing values"):
        ms = seir_c(B, counters=("C",), missing="skip")
        B.pmmh(B.bootstrap_filter, np.where(np.isnan(y), np.inf, y), 3, ms.init_fn, ms.transition_fn, ms.log_likelihood_fn,
               {k: (lambda v: 0.0) for k in SEIR_PAR}, [dict(SEIR_PAR)] * 2, burn_in=1, num_chains=2)


def test_first_calls():
    """the call numbers at which a gap loop starts: BPF gaps 1, 1, 3, 0, 1, 3; the APF's second-stage call follows every observation"""
    assert RI.first_calls(6, OT, "BPF") == {0, 1, 2, 5, 6}
    assert RI.first_calls(6, OT, "APF") == {0, 2, 4, 9, 11}
    assert RI.first_calls(3, None, "BPF") == {0, 1, 2} and RI.first_calls(3, None, "APF") == {0, 2, 4}


@pytest.mark.parametrize("ra", ["SIS", "SISR"])
def test_restated_counter_is_the_growth_since_the_previous_observation(oracle, ra):
    """pure birth 0 -> X + C of order 0 in the restated bootstrap filter: C_i == X_i - X_{i-1} for every particle at every
    observation with gap >= 1 (X_{i-1} through the ancestors when the filter resamples), C unchanged at the repeated time, and a gap
    of 3 holds more than one unit's births"""
    import bayesssm_amd as B
    N, T, b = 32, len(OT), 2.0
    y = np.array([1, np.nan, 3, 2, 1, 4], dtype=np.float64)
    u = np.random.default_rng(5).random((T, N))
    res = RI.pf_run_rn(oracle, birth(B, missing="skip").pack({"b": b}), y, N, u, seed=7, stream=1, resample_algorithm=ra, obs_times=OT,
                       return_particles=True)
    ph = res["particles_history"].reshape(T + 1, 2, N)
    assert res["early_return_step"] == 0 and np.array_equal(ph[0], np.repeat([[3.0], [0.0]], N, axis=1))
    assert res["loglike_history"][1] == res["loglike_history"][0]             # (the unobserved row adds exactly 0.0)
    prev_t, kres = 0, 0
    for i in range(1, T + 1):
        gap, prev_t = OT[i - 1] - prev_t, OT[i - 1]
        src = np.arange(N)
        if res["resampled"][i - 1]:
            src = res["ancestors"][kres] - 1; kres += 1
        if gap >= 1:
            np.testing.assert_array_equal(ph[i, 1], ph[i, 0] - ph[i - 1, 0][src], err_msg="observation %d" % i)
        else:
            np.testing.assert_array_equal(ph[i], ph[i - 1][:, src])
    assert kres == res["ancestors"].shape[0] == (T if ra == "SISR" else 0)
    assert ph[3, 1].mean() > b + 4 * np.sqrt(3 * b / N) and ph[6, 1].mean() > b + 4 * np.sqrt(3 * b / N)


def test_restated_apf_counter_spans_the_double_transition(oracle):
    """under the reference's APF the second-stage transition never resets: with no resampling information lost (pure birth, every
    particle traced through both ancestor draws) C_i == X_i - X_{i-1} still holds where gap >= 1, now over gap + 1 units"""
    import bayesssm_amd as B
    N, T = 16, len(OT)
    y = np.array([2, 3, 8, 5, 4, 9], dtype=np.float64)
    u = np.random.default_rng(6).random((2 * T, N))
    res = RI.pf_run_rn(oracle, birth(B).pack({"b": 2.0}), y, N, u, seed=9, stream=2, algorithm="APF", resample_algorithm="SISR", obs_times=OT,
                       return_particles=True)
    ph = res["particles_history"].reshape(T + 1, 2, N)
    anc = res["ancestors"] - 1
    assert anc.shape[0] == 2 * T
    prev_t = 0
    for i in range(1, T + 1):
        gap, prev_t = OT[i - 1] - prev_t, OT[i - 1]
        src = anc[2 * i - 2][anc[2 * i - 1]]                          # first stage, then the resampling after the weights
        grown = ph[i, 0] - ph[i - 1, 0][src]
        if gap >= 1:
            np.testing.assert_array_equal(ph[i, 1], grown)
        else:                                                         # the repeated time: the second-stage unit adds to the old count
            np.testing.assert_array_equal(ph[i, 1], ph[i - 1, 1][src] + grown)
