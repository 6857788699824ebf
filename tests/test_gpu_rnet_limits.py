"""GPU tests of the reaction-network family at its limits (rnet.hip.h, pf_run_rn, k_pf_batch_rn): d = R = p = 8 with every species
live and every reaction firing, reactions of order 0, three live species under DM = 4, d = 1, gaps and a repeated observation time,
two blocks, and particle sets of which only a part has the log-weight -inf.  The reference is the numpy restatement
(tests/rnet_restated.py) on the same Philox blocks; a species permutation, the batched = single identity, an exact mean and the
identity "a reaction of rate 0 adds nothing to the running sum" cover the rest.  tests/test_gpu_rnet.py holds the family's pins at
d <= 4 live species; its helpers run() and same() and its SCHEDULES are used here."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnet_restated as RN  # noqa: E402
from test_gpu_rnet import SCHEDULES, run, same  # noqa: E402

pytestmark = pytest.mark.gpu

OT = [1, 2, 2, 4, 5]                 # a repeated time (a weight-only step) and a gap (two transitions before one weighting)


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 15, 8)
    yield c
    c.close()


# --- full8: d = R = p = 8, reactions of all three orders -----------------------------------------------------------------------
FULL8_SPECIES = tuple("ABCDEFGH")
FULL8_X0 = dict(zip(FULL8_SPECIES, (6.0, 5.0, 7.0, 4.0, 5.0, 6.0, 5.0, 0.0)))
FULL8_REACTIONS = [({}, {"A": 1}, "k0"),                        # 0 -> A           order 0
                   ({"A": 1}, {"B": 1}, "k1"),                  # A -> B
                   ({"B": 1, "C": 1}, {"D": 1}, "k2"),          # B + C -> D       order 2
                   ({"D": 1}, {"E": 1, "F": 1}, "k3"),          # D -> E + F
                   ({"E": 1}, {"G": 1}, "k4"),                  # E -> G
                   ({"F": 1, "G": 1}, {"H": 1}, "k5"),          # F + G -> H       order 2
                   ({"H": 1}, {}, "k6"),                        # H -> 0
                   ({"G": 1}, {"C": 1}, "k7")]                  # G -> C           (the reaction taken "otherwise")
FULL8_PAR = dict(k0=1.5, k1=0.4, k2=0.08, k3=0.5, k4=0.4, k5=0.06, k6=0.3, k7=0.35)
# G: component k < 7 counts species k and species k + 3 (two entries a row: a sum of two terms is the same in either order, so a
# species permutation changes no bit); the last component is H alone, coefficient 1.  Every column has an entry.
FULL8_OBSERVE = [{FULL8_SPECIES[k]: 0.06, FULL8_SPECIES[(k + 3) % 8]: 0.03} for k in range(7)] + [{"H": 1.0}]
# column 7 = (0, 1, 0, 2, 1): H starts at 0, so row 1 meets lambda == 0 with y == 0 and row 2 gives the particles that still have no
# H the log-weight -inf, and only those
Y_FULL8 = np.array([[1, 0, 0, 0, 0, 0, 0, 0],
                    [1, 0, 0, 3, 0, 0, 0, 1],
                    [0, 1, 2, 1, 0, 0, 0, 0],
                    [0, 0, 1, 0, 1, 0, 0, 2],
                    [1, 1, 1, 1, 0, 1, 0, 1]], dtype=np.float64)
FULL8_PERM = ("F", "H", "E", "G", "C", "A", "D", "B")            # slots 0..3 <-> slots 4..7


def full8(B, order=FULL8_SPECIES):
    return B.models.reaction_network(order, FULL8_REACTIONS, x0=[FULL8_X0[s] for s in order], observe=FULL8_OBSERVE)


# --- sirs3: three live species under DM = 4, p = 2 ------------------------------------------------------------------------------
SIRS3_PAR = dict(beta=0.02, gamma=0.4, rho=0.3)
Y_SIRS3 = np.array([[2, 3], [7, 2], [2, 4], [8, 1], [3, 3]], dtype=np.float64)       # (7 and 8 surprise the filter: SISAR resamples there)


def sirs3(B):
    return B.models.reaction_network(("S", "I", "R"), [({"S": 1, "I": 1}, {"I": 2}, "beta"), ({"I": 1}, {"R": 1}, "gamma"), ({"R": 1}, {"S": 1}, "rho")],
                                     x0=(40, 6, 4), observe=[{"I": 0.3}, {"S": 0.05, "R": 0.2}])


# --- bd1: d = 1, births (order 0) and deaths ---------------------------------------------------------------------------------------
BD1_PAR = dict(b=2.0, m=0.25)
BD1_X0 = 12.0
Y_BD1 = np.array([5, 13, 3, 7, 1], dtype=np.float64)                                             # (13 and 1: SISAR resamples there)


def bd1(B, observe={"A": 0.5}):
    return B.models.reaction_network(("A",), [({}, {"A": 1}, "b"), ({"A": 1}, {}, "m")], x0=(BD1_X0,), observe=observe)


def bd1_mean_and_bound(t, N, b=BD1_PAR["b"], m=BD1_PAR["m"], x0=BD1_X0):
    """the exact mean of bd1 at the times t, and the 6-sigma bound of a sample mean over N chains.  The state is a binomial count of
    the x0 first molecules' survivors plus an independent Poisson count of the born ones: its variance
    x0 e^{-mt} (1 - e^{-mt}) + (b / m)(1 - e^{-mt}) is at most x0 / 4 + b / m."""
    e = np.exp(-m * np.asarray(t, dtype=np.float64))
    return x0 * e + (b / m) * (1.0 - e), 6.0 * np.sqrt((x0 / 4.0 + b / m) / N)


NETS = {"full8": (full8, FULL8_PAR, Y_FULL8), "sirs3": (sirs3, SIRS3_PAR, Y_SIRS3), "bd1": (bd1, BD1_PAR, Y_BD1)}


# --- 1. against the restatement ---------------------------------------------------------------------------------------------------
def u_res_for(algorithm, T, N, resample_fn):
    ncalls = 2 * T if algorithm == "APF" else T
    rng = np.random.default_rng(17)
    return rng.random(ncalls) if resample_fn == "systematic" else rng.random((ncalls, N))


def restated(oracle, m, par, y, N, algorithm, ra, rf, seed, stream, ot=OT):
    """the restatement's run, its counts (rnet_restated.make) and the u_res it used"""
    u = u_res_for(algorithm, len(y), N, rf)
    counts = {}
    t0 = time.perf_counter()
    ref = RN.pf_run_rn(oracle, m.pack(par), y, N, u, seed=seed, stream=stream, algorithm=algorithm, counts=counts, resample_algorithm=ra,
                       resample_fn=rf, obs_times=ot, return_particles=True)
    print("restatement: %.2f s" % (time.perf_counter() - t0))
    return ref, counts, u


def compare_with_restatement(got, ref):
    """the bars of test_gpu_rnet.test_seir_against_the_restatement, with the integer states compared exactly and the coarse branch
    open only to runs in which at most 1 in 1000 ancestor entries differ"""
    print("loglike", got["loglike"], ref["loglike"])
    print("loglike_history", got["loglike_history"], ref["loglike_history"])
    assert got["_extras"]["early_return_step"] == ref["early_return_step"] == 0
    anc_g, anc_r = got["_extras"]["ancestors"], ref["ancestors"]
    assert anc_g.shape == anc_r.shape
    n_diff = int(np.sum(anc_g != anc_r))
    print("differing ancestors: %d of %d" % (n_diff, anc_r.size))
    assert abs(got["loglike"] - ref["loglike"]) <= 1e-6 * abs(ref["loglike"])
    np.testing.assert_allclose(got["loglike_history"], ref["loglike_history"], rtol=1e-6)
    assert (got["_extras"]["resampled"] == ref["resampled"]).all()
    assert got["state_est"].shape == ref["state_est"].shape
    if n_diff == 0:
        np.testing.assert_allclose(got["ess"], ref["ess"], rtol=1e-9)
        np.testing.assert_allclose(got["state_est"], ref["state_est"], rtol=1e-9, atol=1e-9)
        # integers from the same Philox blocks: a difference is a wrong draw key, reaction choice or stoichiometry row, not rounding
        np.testing.assert_array_equal(got["particles_history"], ref["particles_history"])
    else:
        assert n_diff * 1000 <= anc_r.size, "more than 1 in 1000 ancestors differ from the restatement's"
        np.testing.assert_allclose(got["ess"], ref["ess"], rtol=1e-6)
        np.testing.assert_allclose(got["state_est"], ref["state_est"], rtol=1e-6, atol=1e-8)


def full8_properties(ref, counts, N, ra):
    """what makes full8 a test of the limits, asserted on the restatement's output"""
    ph = ref["particles_history"].reshape(ref["particles_history"].shape[0], 8, N)
    assert all((ph[:, c] != ph[0, c, 0]).any() for c in range(8)), "a species never changes"
    assert all(counts["fired"].get(r, 0) > 0 for r in range(8)), counts["fired"]
    assert np.isfinite(ref["loglike"])
    print("fired", sorted(counts["fired"].items()), "particles at -inf per observation", counts["n_inf"])
    assert any(1 <= n <= N - 1 for n in counts["n_inf"])
    if ra == "SISAR":
        assert ref["resampled"].any() and not ref["resampled"].all()


@pytest.mark.parametrize("N,ra,rf", [(385, "SISAR", "stratified"), (2561, "SISAR", "stratified"), (2561, "SISR", "systematic")])
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
def test_full8_against_the_restatement(B, ctx, oracle, algorithm, N, ra, rf):
    """d = R = p = 8 against the numpy restatement, one and two blocks, with a repeated observation time and a gap: log-likelihood
    and its history 1e-6 relative, `resampled` equal, and where every ancestor agrees ESS and state estimates at 1e-9 and the
    integer states exactly.  (Catches, for one: rn_transition's walk ending at r = 5, so that reaction 6 never fires; k_gather_rn
    reading component c & 3; rn_loglik's loop over the observation components taken for k < 4 only.)"""
    m = full8(B)
    ref, counts, u = restated(oracle, m, FULL8_PAR, Y_FULL8, N, algorithm, ra, rf, seed=23, stream=4)
    full8_properties(ref, counts, N, ra)
    got = run(B, m, algorithm, Y_FULL8, N, ctx, FULL8_PAR, resample_algorithm=ra, resample_fn=rf, obs_times=OT, seed=23, stream=4, draws={"u_res": u})
    compare_with_restatement(got, ref)


@pytest.mark.parametrize("algorithm,N", [("BPF", 385), ("APF", 385), ("BPF", 2561)])
@pytest.mark.parametrize("net", ["sirs3", "bd1"])
def test_small_nets_against_the_restatement(B, ctx, oracle, net, algorithm, N):
    """three live species under DM = 4, and d = 1 (DM = 2 behind the c < d guards, a 1-D state estimate), at the bars of
    test_full8_against_the_restatement.  (Catches, for one: the `s1 >= 0` test of rn_propensities dropped -- rn_pick(x, -1) is 0.0,
    so no birth ever happens.)"""
    make, par, y = NETS[net]
    m = make(B)
    ref, counts, u = restated(oracle, m, par, y, N, algorithm, "SISAR", "stratified", seed=29, stream=3)
    assert np.isfinite(ref["loglike"]) and all(counts["fired"].get(r, 0) > 0 for r in range(m.R))
    if algorithm == "BPF":                                  # (the APF's first stage resamples at every observation)
        assert ref["resampled"].any() and not ref["resampled"].all()
    got = run(B, m, algorithm, y, N, ctx, par, resample_algorithm="SISAR", resample_fn="stratified", obs_times=OT, seed=29, stream=3, draws={"u_res": u})
    assert got["state_est"].ndim == (1 if net == "bd1" else 2)
    compare_with_restatement(got, ref)


def test_bd1_early_return_gives_zeros(B, ctx, oracle):
    """d = 1 after an early return: no births and a fast death, so every particle is at 0 when y > 0 arrives.  The scalar state's
    estimate is zeros (not NaN) from the dead step on, ESS 0, at the restatement's step -- single and batched.  (Catches: NaN
    written for d = 1 by pf_run_rn or pf_run_batch_rn.)"""
    N, par, y = 100, dict(b=0.0, m=5.0), np.array([0.0, 0.0, 0.0, 2.0, 0.0])
    m = bd1(B)
    ref, _, u = restated(oracle, m, par, y, N, "BPF", "SISAR", "stratified", seed=31, stream=2, ot=None)
    k = ref["early_return_step"]
    assert k == 4 and ref["loglike"] == -np.inf
    got = run(B, m, "BPF", y, N, ctx, par, seed=31, stream=2, draws={"u_res": u})
    bat = B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, [par] * 2, 31, [2, 2], ctx=ctx)
    assert got["loglike"] == -np.inf and got["_extras"]["early_return_step"] == k
    assert got["state_est"].shape == (len(y) + 1,)
    assert np.all(got["state_est"][k:] == 0.0) and np.all(got["ess"][k:] == 0.0)
    np.testing.assert_allclose(got["state_est"], ref["state_est"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got["ess"], ref["ess"], rtol=1e-9)
    assert got["particles_history"].shape[0] == k
    assert np.all(bat["loglike"] == -np.inf) and np.all(bat["early_return_step"] == k)
    assert np.all(bat["state_est"][:, k:] == 0.0) and np.all(bat["ess"][:, k:] == 0.0)
    one = run(B, m, "BPF", y, N, ctx, par, seed=31, stream=2)                # (the batched filters draw their own u_res)
    assert one["_extras"]["early_return_step"] == k and np.all(one["state_est"][k:] == 0.0)
    for f in range(2):
        np.testing.assert_array_equal(bat["state_est"][f].reshape(-1), one["state_est"])
        np.testing.assert_array_equal(bat["ess"][f], one["ess"])


# --- 2. species permutation at d = 8 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("N", [1, 7, 2561])
def test_full8_permuted_species_give_permuted_outputs(B, ctx, N, algorithm):
    """full8 against itself with the species of slots 0..3 and 4..7 exchanged (reactions in the same order), under every schedule:
    the padding test of test_gpu_rnet.py with live species -- every run goes through all observations and no species stays
    constant over time, at N = 1 too.  (Catches, for one: the Euler mean of rn_loglik<AUX> taken for c < 4 only, or rn_pick
    comparing s & 3 -- a padded species is no reactant and has nu = 0, so the padding test cannot see either.)"""
    cols = [FULL8_PERM.index(s) for s in FULL8_SPECIES]
    assert sorted(cols[:4]) == [4, 5, 6, 7] and sorted(cols[4:]) == [0, 1, 2, 3]
    T = Y_FULL8.shape[0]
    for ra, rf, ot in SCHEDULES:
        kw = dict(resample_algorithm=ra, resample_fn=rf, obs_times=None if ot is None else ot[:T], seed=5, stream=N)
        a = run(B, full8(B), algorithm, Y_FULL8, N, ctx, FULL8_PAR, **kw)
        b = run(B, full8(B, FULL8_PERM), algorithm, Y_FULL8, N, ctx, FULL8_PAR, **kw)
        same(a, b, cols=cols)
        early = a["_extras"]["early_return_step"]
        assert early == 0 and np.isfinite(a["loglike"])
        ph = a["particles_history"].reshape(T + 1, 8, N)
        assert all((ph[:, c] != ph[0, c]).any() for c in range(8)), "a species is constant over time"


# --- 3. batched = single at the limits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["full8", "sirs3", "bd1"])
def test_batched_equals_single_at_the_limits(B, ctx, net):
    """k_pf_batch_rn = pf_run_rn bit for bit at d = 8, 3 and 1: N in {1, 7, 385, capacity}, both sides of batch_literal_max, with
    the repeated observation time and the gap, two filters of different parameters, seeds and streams.  (Catches, for one:
    k_pf_batch_rn's gather or carry leaving out the components c >= 4 -- a padded species is 3.0 gathered or not.)"""
    make, par, y = NETS[net]
    m = make(B)
    cap = B.batch_max_particles(m.dim, "rnet")
    assert 385 < cap <= 2048
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    last = list(par)[-1]
    pars = [par, dict(par, **{last: 1.25 * par[last]})]
    cases = [(1, "SISAR", "stratified"), (7, "SISR", "systematic"), (385, "SISAR", "stratified"), (385, "SIS", "stratified"),
             (cap, "SISAR", "systematic"), (cap, "SISR", "stratified")]
    for lit in (0, 512):                                   # N above / at most batch_literal_max: block scan / in-order sums
        ctx.set_option("batch_literal_max", lit)
        try:
            for N, ra, rf in cases:
                bat = B.bootstrap_filter_batch(y, N, *fns, pars, [11, 12], [3, 4], obs_times=OT, resample_algorithm=ra, resample_fn=rf, ctx=ctx)
                assert np.all(bat["status"] == 0)
                for f in range(2):
                    one = B.bootstrap_filter(y, N, *fns, obs_times=OT, resample_algorithm=ra, resample_fn=rf, ctx=ctx, return_particles=False,
                                             seed=11 + f, stream=3 + f, **pars[f])
                    assert bat["loglike"][f] == one["loglike"], (net, N, ra, rf, lit)
                    np.testing.assert_array_equal(bat["loglike_history"][f], one["loglike_history"])
                    np.testing.assert_array_equal(bat["ess"][f], one["ess"])
                    np.testing.assert_array_equal(bat["state_est"][f].reshape(one["state_est"].shape), one["state_est"])
                    assert bat["n_res_calls"][f] == one["_extras"]["n_res_calls"]
                    assert bat["early_return_step"][f] == one["_extras"]["early_return_step"]
                    if N >= 385:
                        assert np.isfinite(one["loglike"]), (net, N, ra, rf)
        finally:
            ctx.set_option("batch_literal_max", 512)


# --- 4. exact mean with an order-0 reaction ---------------------------------------------------------------------------------------
def test_birth_death_has_the_exact_mean(B, ctx):
    """bd1 with G = 0, y = 0: every log-weight is 0.0, so the SIS state estimate is the sample mean of N = 2^14 independent chains
    and lies within bd1_mean_and_bound's 6 sigma of x0 e^{-mt} + (b / m)(1 - e^{-mt}).  (Catches: an order-0 propensity of 0.0,
    as with the `s1 >= 0` test dropped, or of k x[0] -- the mean then decays to 0 or grows without the b / m limit.)"""
    N, T = 1 << 14, 5
    m = bd1(B, observe=np.zeros((1, 1)))
    res = B.bootstrap_filter(np.zeros(T), N, m.init_fn, m.transition_fn, m.log_likelihood_fn, resample_algorithm="SIS", ctx=ctx, seed=3, stream=0, **BD1_PAR)
    assert res["loglike"] == 0.0 and np.all(res["weights_history"] == 1.0 / N)
    assert res["state_est"].shape == (T + 1,)
    exact, bound = bd1_mean_and_bound(np.arange(T + 1), N)
    err = np.abs(res["state_est"] - exact)
    print("errors", err, "bound", bound)
    assert np.all(err <= bound)
    ph = res["particles_history"]
    assert ph.shape == (T + 1, N) and np.all(ph == np.floor(ph)) and ph.min() >= 0
    assert ph[1:].max() > BD1_X0                           # (the order-0 reaction fired)


# --- 5. the last-reaction branch in isolation -------------------------------------------------------------------------------------
def _one_live_reaction(B, R, live):
    """d = 2, R reactions of which only `live` (A -> B) has a rate: the others, of all three orders, have rate 0"""
    idle = [({}, {"A": 1}, 0.0), ({"B": 1}, {"A": 1}, 0.0), ({"A": 1, "B": 1}, {"B": 2}, 0.0), ({"A": 1}, {}, 0.0)]
    reactions = [idle[r % 4] for r in range(R)]
    reactions[live] = ({"A": 1}, {"B": 1}, 0.5)
    return B.models.reaction_network(("A", "B"), reactions, x0=(40, 3), observe=[{"B": 0.5}, {"A": 0.25, "B": 0.125}])


@pytest.mark.parametrize("algorithm", ["BPF", "APF"])
@pytest.mark.parametrize("N", [7, 2561])
def test_zero_rate_reactions_leave_the_choice(B, ctx, N, algorithm):
    """A -> B as the only reaction (R = 1) = the same reaction at index 7 of 8 behind seven of rate 0 (chosen by the "reaction R-1
    otherwise" initialiser alone: the walk ends at r = 6) = at index 3 with zeros on both sides (chosen at r = 3 after three
    additions of 0.0 to the running sum).  rn_transition: zero propensities add nothing to the running sum.  (Catches, for one:
    the stoichiometry row read at (rsel & 3) * d.)"""
    y = np.array([[3, 2], [8, 5], [9, 4], [12, 6], [14, 5]], dtype=np.float64)
    for ra, rf, ot in (("SISAR", "stratified", OT), ("SISR", "systematic", None)):
        kw = dict(resample_algorithm=ra, resample_fn=rf, obs_times=ot, seed=13, stream=6)
        ref = run(B, _one_live_reaction(B, 1, 0), algorithm, y, N, ctx, {}, **kw)
        assert np.isfinite(ref["loglike"])
        ph = ref["particles_history"]
        assert (ph[-1, :N] < 40).any() and (ph[-1, N:] > 3).any()
        same(ref, run(B, _one_live_reaction(B, 8, 7), algorithm, y, N, ctx, {}, **kw))
        same(ref, run(B, _one_live_reaction(B, 8, 3), algorithm, y, N, ctx, {}, **kw))
