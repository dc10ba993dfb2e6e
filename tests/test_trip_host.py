"""The path engine's query trip on the host (pt_query.h q_trip / q_run_trip, PT_TUNE
qengine=trip): a step and up to aux_extra more aux-node steps that leave a lane at a decision
in phase Q_DECIDE, then the trip's one q_decide -- the schedule of k_wpath's query waves
(pt_path.hip path_query_wave), one thread per ray.

Deferring the decide must change nothing: the six seeded ray sets of test_query_step.py
(stacked triangles with their overflow passes and exact hand-overs, +-0 direction components,
infinite margins, the two bulk sets on the dragon fixture) give the oracle's ids and hit bits
and that file's PARENT_COUNTERS (reference node records, primitive tests, aux visits, exact-DFS
fallbacks), with 0, 1 and 2 extra aux-node steps per trip.
"""
import pytest

import test_query_step as QS

SETS = ["stack", "stack_few", "zero", "wide", "bulk1", "bulk2"]


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("trip_host")


@pytest.mark.parametrize("aux_extra", [0, 1, 2])
@pytest.mark.parametrize("name", SETS)
def test_trip_schedule_same_answers_and_parent_counters(tmp_root, monkeypatch, name, aux_extra):
    monkeypatch.setenv("PT_TUNE", "qengine=trip,aux_extra=%d" % aux_extra)
    # (host_query checks the ids and the hit bits against the oracle's)
    _, _, ctr = QS.host_query(name, tmp_root)
    assert ctr["errors"] == 0
    QS.assert_parent_counters(name, ctr)
