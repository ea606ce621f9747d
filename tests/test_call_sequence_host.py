"""The call-sequence harness of tests/handle_states.py on a NumPy stand-in (tests/handle_stub.py): the state builders, the
capture / load round trip, the replay of writers and the path_switch chain all run without a GPU, and a stand-in with a planted
fault of each kind the harness exists for is caught by the (state, guest) pair one would expect."""
import pytest

from tests import handle_states as H
from tests.handle_stub import StubModel

# one variant per state (the first that the plan lists) keeps this quick; the GPU suite runs them all
_FIRST = {}
for _v in H.VARIANTS:
    _FIRST.setdefault(_v["state"], _v)
_RUN = [(v, g) for v, g in H.cases(stub_only=True)[0] if v is _FIRST[v["state"]]]


def _make(U, I, D, **kw):
    return StubModel(U, I, D, **kw)


@pytest.mark.parametrize("v,guest", _RUN, ids=["%s-%s" % (v["id"], g) for v, g in _RUN])
def test_harness_on_the_stand_in(v, guest):
    H.run_case(_make, v, guest)


def test_every_kind_of_guest_runs_on_the_stand_in():
    assert {H.GUESTS[g].kind for _, g in _RUN} == {H.RO, H.WRITER, H.IDENTITY}
    assert {v["state"] for v, _ in _RUN} == set(H.STATES)


@pytest.mark.parametrize("shape", sorted(H.PATH_SWITCHES))
def test_path_switch_on_the_stand_in(shape):
    chain = H.path_switch_chain(_make, H.PATH_SWITCHES[shape])
    seen, end = H.path_switch_live(_make, len(H.PATH_SWITCH_STEPS), H.PATH_SWITCHES[shape])
    for k, s in enumerate(seen):
        H.same(s, chain[k][0], "step %d" % (k + 1))
    H.same(end, chain[-1][1], "tables after the last step")


def _broken(defect):
    def make(U, I, D, **kw):
        return StubModel(U, I, D, defect=defect, **kw)
    make.__name__ = "stub_" + defect                      # (a cache key of its own in handle_states)
    return make


def _variant(state, way=None):
    return [v for v in H.VARIANTS if v["state"] == state and (way is None or v["way"] == way)][0]


@pytest.mark.parametrize("defect,state,way,guest,where", [
    ("stale_forward", "two_table", None, "forward", "the guest's result"),            # a reader that does not settle
    ("kept_sort", "tile_lookahead", "staged", "upload_other_store", "training after"),     # a look-ahead sort that survives
    ("run_ahead", "tile_lookahead", "drawn9", "draw_ids", "the guest's result"),      # a draw that does not cancel the run-ahead
])
def test_a_planted_fault_is_caught(defect, state, way, guest, where):
    with pytest.raises(AssertionError) as e:
        H.run_case(_broken(defect), _variant(state, way), guest)
    assert where in str(e.value), str(e.value)
    H.run_case(_make, _variant(state, way), guest)           # and the sound stand-in passes the same pair


def test_same_tells_bits_apart():
    import numpy as np
    H.same(np.float32([1, np.nan]), np.float32([1, np.nan]), "nan")
    with pytest.raises(AssertionError):
        H.same(np.float32([0.0]), np.float32([-0.0]), "signed zero")
    with pytest.raises(AssertionError):
        H.same({"t3": np.zeros(2, np.float32)}, {"t3": np.ones(2, np.float32)}, "a table")
