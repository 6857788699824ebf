"""pmmh(..., return_latent_trajectories=True) on the two device families: one path x_{0:T} per iteration, drawn from the particle
system of the filter last accepted (the batched smoother in the lock-step route, the single-filter smoother with trajectories=1 in
the one-at-a-time route).  The keyword moves no other draw; the path changes exactly where the chain accepted; every path can be
replayed from (seed, trajectory_stream, theta); both routes give the same chain of paths."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, BURN, T = 30, 5, 10


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


def _lgmv(B):
    """(d, p) = (2, 1): rho scales A, s the observation sd"""
    A0 = np.array([[0.7, 0.1], [0.0, 0.5]])
    m = B.models.linear_gaussian_mv(2, 1, build=lambda rho, s: {"A": rho * A0, "sd": [0.7 * s]}, param_names=("rho", "s"), L=0.5 * np.eye(2),
                                    H=np.array([[1.0, 0.5]]))
    rng = np.random.default_rng(8)
    x, ys = np.zeros(2), []
    for _ in range(T):
        x = 0.8 * A0 @ x + 0.5 * rng.standard_normal(2)
        ys.append([x[0] + 0.5 * x[1] + 0.7 * rng.standard_normal()])
    priors = {"rho": B.prior_uniform(0.0, 1.2), "s": B.prior_exponential(1.0)}
    kw = dict(param_transform={"rho": "identity", "s": "log"}, seed=77,
              tune_control=B.default_tune_control(pilot_m=20, pilot_n=100, pilot_reps=2, pilot_burn_in=5, pilot_proposal_sd=0.3))
    return m, np.array(ys), priors, [{"rho": 0.5, "s": 1.0}, {"rho": 0.9, "s": 0.7}], kw, 2


def _seir(B):
    # (a small share of S is counted too: the Poisson mean stays positive when a proposal lets the epidemic die out)
    m = B.models.reaction_network(("S", "E", "I", "R"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"),
                                                         ({"I": 1}, {"R": 1}, "gamma")], x0=[180.0, 8.0, 12.0, 0.0], observe=({"I": 0.6, "S": 0.01},))
    priors = {"beta": B.prior_exponential(100.0), "sigma": B.prior_exponential(1.0), "gamma": B.prior_exponential(1.0)}
    kw = dict(param_transform={k: "log" for k in priors}, seed=7,
              tune_control=B.default_tune_control(pilot_m=20, pilot_burn_in=5, pilot_n=100, pilot_reps=2, pilot_proposal_sd=0.05))
    y = np.array([8, 9, 12, 13, 17, 19, 20, 24, 22, 25], dtype=np.float64)
    return m, y, priors, [dict(beta=0.004, sigma=0.5, gamma=0.3), dict(beta=0.0045, sigma=0.45, gamma=0.33)], kw, 4


@pytest.fixture(scope="module", params=["lgmv", "seir"])
def runs(B, request):
    m, y, priors, init, kw, d = (_lgmv if request.param == "lgmv" else _seir)(B)
    args = (B.bootstrap_filter, y, M, m.init_fn, m.transition_fn, m.log_likelihood_fn, priors, init, BURN)
    kw = dict(kw, num_chains=2, print_result=False, return_latent_state_est=True)
    with_kw = B.pmmh(*args, return_latent_trajectories=True, **kw)
    without = B.pmmh(*args, **kw)
    one_at_a_time = B.pmmh(*args, return_latent_trajectories=True, batch_chains=False, **kw)
    return dict(m=m, y=y, names=list(priors), d=d, a=with_kw, plain=without, seq=one_at_a_time)


def test_the_keyword_moves_no_other_draw(runs):
    a, plain = runs["a"], runs["plain"]
    assert "latent_trajectory_chain" not in plain and not any("trajectory_stream" in lc for lc in plain["_extras"]["local_chains"].values())
    assert a["_extras"]["batched"] is True and a["_extras"]["batched_launches"] > 0
    for k in runs["names"]:
        assert np.array_equal(np.asarray(a["theta_chain"][k]), np.asarray(plain["theta_chain"][k])), k
    for c in (0, 1):
        assert np.array_equal(a["latent_state_chain"][c], plain["latent_state_chain"][c], equal_nan=True)
        la, lp = a["_extras"]["local_chains"][c], plain["_extras"]["local_chains"][c]
        assert la["accepted"] == lp["accepted"] and np.array_equal(la["theta_chain"], lp["theta_chain"])
        assert a["latent_trajectory_chain"][c].shape == (M - BURN, T + 1, runs["d"])
        assert np.array_equal(a["latent_trajectory_chain"][c], la["trajectory_chain"][BURN:])
        assert la["trajectory_stream"].shape == (M,)


def test_the_path_changes_exactly_where_the_chain_accepted(runs):
    total = 0
    for c, lc in runs["a"]["_extras"]["local_chains"].items():
        th, tr, st = lc["theta_chain"], lc["trajectory_chain"], lc["trajectory_stream"]
        assert np.all(np.isfinite(tr))
        moved = np.any(th[1:] != th[:-1], axis=1)
        assert np.array_equal(np.any(tr[1:] != tr[:-1], axis=(1, 2)), moved)
        assert np.array_equal(st[1:] != st[:-1], moved) and np.all(np.diff(st) >= 0)
        assert int(moved.sum()) == lc["accepted"]
        total += lc["accepted"]
    assert total > 0                                              # (otherwise nothing above was exercised)


def test_every_path_replays_from_its_stream(B, runs):
    m, seeds = runs["m"], runs["a"]["_extras"]["seeds"]
    for c, lc in runs["a"]["_extras"]["local_chains"].items():
        first = [0] + [i for i in range(1, M) if lc["trajectory_stream"][i] != lc["trajectory_stream"][i - 1]]
        for i in first:
            one = B.bootstrap_filter(runs["y"], int(lc["pilot"]["target_n"]), m.init_fn, m.transition_fn, m.log_likelihood_fn, trajectories=1,
                                     return_particles=False, seed=int(seeds[c]), stream=int(lc["trajectory_stream"][i]),
                                     **dict(zip(runs["names"], [float(v) for v in lc["theta_chain"][i]])))
            assert np.array_equal(one["trajectories"][0], lc["trajectory_chain"][i]), (c, i)


def test_the_one_at_a_time_route_gives_the_same_paths(runs):
    a, seq = runs["a"], runs["seq"]
    assert seq["_extras"]["batched"] is False
    for c in (0, 1):
        assert np.array_equal(a["latent_trajectory_chain"][c], seq["latent_trajectory_chain"][c])
        assert np.array_equal(a["_extras"]["local_chains"][c]["trajectory_stream"], seq["_extras"]["local_chains"][c]["trajectory_stream"])
        assert np.array_equal(a["_extras"]["local_chains"][c]["theta_chain"], seq["_extras"]["local_chains"][c]["theta_chain"])
