"""pmmh.py's host side against fixtures recorded from the build BEFORE its loops, marshalling, argument checks and result assembly were
put into shared functions (tools/record_pmmh_golden.py; no GPU): the pilot and main-chain loops, one chain and lock-step, over a
synthetic filter -- every returned array, the sequence of filter calls (theta, n, tag, chain), how many draws each generator gave and
its next draw, stdout and the error, byte for byte and text by equality -- and every refusal of pmmh()'s argument checks for a built-in
model, Python closures, an lgmv and an rnet descriptor: exception type, text and warnings."""
import json

import pytest

import tools.record_pmmh_golden as rec

CPU_CASES = [name for name, (kind, _, _) in rec.CASES.items() if kind == "cpu"]


@pytest.mark.parametrize("name", CPU_CASES)
def test_host_loops_equal_parent_build(name):
    want = rec.load_case(name)
    rec.happened(name, want)              # the recording holds what the case is there for: redraws, skipped filters, subsets of chains
    diffs = rec.differences(name, rec.run_case(name), want)
    assert not diffs, "\n".join(diffs)


def test_lockstep_with_lapack_mvrnorm_is_the_single_chain():
    """run_chains_host_lockstep(mvrnorm=_mvrnorm_lapack) with one chain against the recording of run_chain_host(mvrnorm=_mvrnorm_lapack) over
    R's generator: the same chain, the same filter calls, the same number of draws"""
    want = rec.load_case("main_single_dense_rstream")
    got = rec.main_case(kind="lockstep", cov="dense", K=1, r_stream=True, lapack=True, latent=False)
    want.pop("calls/batch"), got.pop("calls/batch")          # (which of the two entry points called the filter)
    diffs = rec.differences("main_single_dense_rstream", got, want)
    assert not diffs, "\n".join(diffs)


with open(rec.golden_path("refusals.json")) as _f:
    REFUSALS = json.load(_f)


def test_refusal_table_is_the_recorders():
    assert sorted(REFUSALS) == sorted(rec.refusal_names())
    assert {k.split("/")[0] for k in REFUSALS} == {"builtin", "closures", "lgmv", "rnet"}
    assert any(v["warnings"] for v in REFUSALS.values())      # the unsupported-transform warning is among them


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_pmmh_refuses_as_parent_build(name):
    assert rec.run_refusal(name) == REFUSALS[name]
