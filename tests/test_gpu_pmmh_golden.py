"""pmmh() through every route of its dispatcher against fixtures recorded on the GPU from the build BEFORE pmmh.py's loops,
marshalling, argument checks and result assembly were put into shared functions (tools/record_pmmh_golden.py): the posterior columns,
diagnostics and seeds; per chain theta_chain, loglike_chain, state_est_chain, accepted, the path flag and every array of its pilot;
the "_extras" flags and launch counts; the warnings; stdout (as a multiset of lines where chains run on worker threads) -- byte for
byte, text by equality; device_ms is not compared.  Every case: T = 8, m = 10, pilot_m = 12, pilot_n = 64, pilot_reps = 4, two or
three chains.  Routes: built-in LG with the lock-step pilot and bssm_pmmh_chains_batch (also with latent states), one chain at a time,
one chain, 4096 particles on streams and in bssm_pmmh_chains_multi, SIR over the auxiliary filter, an injected chain runner, r_stream on a
built-in model (also with latent states), Python closures (plain, latent states, r_stream), an lgmv descriptor batched (also with latent
states) and one at a time, an rnet descriptor batched."""
import pytest

import tools.record_pmmh_golden as rec

pytestmark = pytest.mark.gpu

GPU_CASES = [name for name, (kind, _, _) in rec.CASES.items() if kind.startswith("gpu")]


@pytest.mark.parametrize("name", GPU_CASES)
def test_pmmh_equal_to_parent_build(name):
    want = rec.load_case(name)
    diffs = rec.differences(name, rec.run_case(name), want)
    assert not diffs, "\n".join(diffs)


def test_recorded_routes():
    """the fixtures took the routes they are named after"""
    flag = lambda name, key: key in rec.load_case(name)["chain0/keys"].split()      # noqa: E731
    assert flag("gpu_lg_lockstep", "batched") and not flag("gpu_lg_one_at_a_time", "batched")
    assert flag("gpu_lg_large_lockstep", "lockstep_launches") and not flag("gpu_lg_large_streams", "lockstep_launches")
    assert flag("gpu_sir_apf", "batched") and flag("gpu_lg_one_chain", "pilot") and not flag("gpu_lg_large_streams", "pilot")
    assert "injected runner: chain 1" in rec.load_case("gpu_lg_chain_runner")["text/stdout"]
    assert int(rec.load_case("gpu_ar1sin_r_stream")["extras/r_stream"][0]) == 1
    for name, batched in (("gpu_lgmv_batched", 1), ("gpu_rnet_batched", 1), ("gpu_lgmv_one_at_a_time", 0), ("gpu_closures", 0)):
        z = rec.load_case(name)
        assert int(z["extras/batched"][0]) == batched and (("extras/batched_launches" in z) == bool(batched))
    for name in ("gpu_lg_lockstep_latent", "gpu_ar1sin_r_stream_latent", "gpu_closures_latent", "gpu_lgmv_batched_latent"):
        assert "latent/0" in rec.load_case(name) and "latent/0" not in rec.load_case(name.replace("_latent", ""))
