"""The aux step's short body on the host (pt_query.h q_exec_aux / q_aux_entries): the per-entry
bookkeeping without the range test, taken when no lane of the wave is in a later pass (lb != 0)
or holds a full list -- the only lanes for which the test decides anything.  The body is picked
by a wave-uniform test; on the host a "wave" is the one thread, so a ray takes the short body
exactly on the steps where its own state allows it.

Both bodies must compute the same: the six seeded ray sets of test_query_step.py give the
oracle's ids and hit bits and that file's PARENT_COUNTERS (reference node records, primitive
tests, aux visits, exact-DFS fallbacks), in single steps and in the path engine's trips with 0,
1 and 2 extra aux-node steps -- once with the body the state picks, once with PT_TUNE
qforms=general, a host-only switch that forces the general body on every step.  The stack set
(60 stacked triangles: dozens of hitting leaves, overflow passes, exact hand-overs) needs the
general body on two thirds of its aux steps; the dragon sets never do.

(A short form of q_decide for lanes without an entered hit was built and measured with this one
and did not clear the bench margin: profiles/r27_qtrip.)
"""
import pytest

import test_query_step as QS

SETS = ["stack", "stack_few", "zero", "wide", "bulk1", "bulk2"]
SCHEDULES = ["steps", "trip0", "trip1", "trip2"]


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("decide_host")


@pytest.mark.parametrize("forms", ["picked", "general"])
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", SETS)
def test_short_and_general_bodies_same_answers_and_parent_counters(tmp_root, monkeypatch, name, schedule, forms):
    tune = [] if schedule == "steps" else ["qengine=trip", "aux_extra=%s" % schedule[4:]]
    if forms == "general":
        tune.append("qforms=general")
    monkeypatch.setenv("PT_TUNE", ",".join(tune))
    # (host_query checks the ids and the hit bits against the oracle's)
    _, _, ctr = QS.host_query(name, tmp_root)
    assert ctr["errors"] == 0
    QS.assert_parent_counters(name, ctr)
