"""q_decide against its reference and the aux entries' ready-made words, on the host (pt_query.h;
tests/test_decide_slots_gpu.py has the device's side).

The host self-test states q_decide as the plain loop over the hit list, apart from pt_query.h's
text: pt_selftest_decide runs both on seeded decision states (ne <= nh <= PT_QHK, sorted lists
with 0xffffffff in the empty slots, thresholds and t's on both sides of the bounds, both values
of overflow, lists full of entered hits with overflow set) and compares the whole Query byte for
byte.  The check was written for a slot-indexed q_decide (slot j examined in iteration j by the
lanes whose ne is j, selects and a wave-uniform exit), which passed it and did not clear the
bench margin alone (profiles/r29_decide); pt_query.h's q_decide is the loop today, and the check
holds whatever form replaces it.

The query blob's wide aux entries hold their last two words ready-made: w7 the item as it is
taken or pushed (child node, PT_LEAFQ | bundle ordinal, 0xffffffff empty), w6 the packed leaf
range or the leaf's reference index.  pt_selftest_aux_words compares every entry with what the
host-form array's code and range and the leaf's ordinal give.
"""
import pytest

import _util as U
import test_query_step as QS

SEEDS = [1, 2, 3]
N = 100000


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("decide_slots_host")


@pytest.mark.parametrize("seed", SEEDS)
def test_decide_equals_the_plain_loop_on_seeded_states(seed):
    pt = U.ptrace()
    r = pt.selftest_decide(seed, N)
    _, exits, slots = pt.selftest_decide_states(seed, N)
    print("seed %d: %r, exits %r, deciding slots %r" % (seed, r, exits, slots))
    assert r["states"] == N
    assert r["mismatches"] == 0
    assert 0 < r["examined"] < N                       # lanes that came with ne == nh as well
    assert sum(exits.values()) == N
    assert all(exits[k] > 0 for k in pt.DECIDE_EXITS)  # leaf check, pass done, another pass, exact
    assert len(slots) >= 2 and all(c > 0 for c in slots)   # every slot 0 .. PT_QHK - 1 decided some state
    assert sum(slots) == r["examined"]


@pytest.mark.parametrize("scene", ["stack", "dragon"])
def test_blob_aux_entries_hold_the_item_and_the_leaf_index(tmp_root, scene):
    pt = U.ptrace()
    path = QS.ray_set("stack", tmp_root)[0] if scene == "stack" else U.golden_scene_path(QS.DRAGON)
    with pt.Scene.load(path) as s:
        r = pt.selftest_aux_words(s)
    print("%s: %r" % (scene, r))
    assert r["mismatches"] == 0
    assert r["empty"] > 0 and r["leaf"] > 0 and r["internal"] > 0
    assert r["empty"] + r["leaf"] + r["internal"] == r["entries"]
