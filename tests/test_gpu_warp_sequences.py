"""A WARP step as a guest of every state earlier calls leave behind on the model it is bound to (tests/handle_states.py names
the states).  The trainer's entry points take a ``tfr_warp*``, so tests/test_call_sequence_coverage.py does not list them
and they are not registered in ``handle_states.GUESTS``; what that suite exists to check is checked here: in every state
with a variant that is not tf1 Adam, ``train_warp_step`` and ``train_warp_steps_drawn`` give what they give on a
history-free handle carrying the same bits, and the training that follows equals, bit for bit, the same continuation on a
fresh handle loaded with the capture taken after the WARP calls."""
import copy

import numpy as np
import pytest

import tfrecomm_amd as T
from tests import handle_states as H
from tests.handle_states import BUILDERS, VARIANTS, capture, continue_training, reference, same

pytestmark = pytest.mark.gpu

RUN = [v for v in VARIANTS if not (v["opt"] == "adam" and v["mode"] == "tf1")]
assert {v["state"] for v in RUN} == set(BUILDERS)


def _make(U, I, D, **kw):
    return T.SvdModel(U, I, D, device=0, **kw)


def _warp_calls(m, g):
    indptr, items = g.env.positives
    e = g.randint(0, items.size, g.n)
    u = (np.searchsorted(indptr, e, side="right") - 1).astype(np.int32)
    m.set_warp(0.5)
    neg, trials, loss, reg, skipped = m.train_warp_step(u, items[e])
    assert (neg >= 0).any()
    return H._bytes(neg, trials, np.float32(loss), np.float32(reg), np.int64(skipped), m.train_warp_steps_drawn(g.n, 2, want_loss=True))


@pytest.mark.parametrize("v", RUN, ids=[v["id"] for v in RUN])
def test_warp_steps_in_state(v):
    snap, env0, _ = reference(_make, v)
    seed = H._seed("guest", "warp")
    live, env = H._built(_make, v)
    with live:
        got = _warp_calls(live, H.GuestRng(seed, env, v["n"]))
        left = capture(live, v)
        after = (continue_training(live, env), capture(live, v))
    fenv = copy.copy(env0)
    with H.new_handle(_make, v) as fresh:
        H.load(fresh, fenv, snap)
        want = _warp_calls(fresh, H.GuestRng(seed, fenv, v["n"]))
        mid = capture(fresh, v)
    same(got, want, "WARP steps in %s: their results against a fresh handle" % v["id"])
    same(left, mid, "WARP steps in %s: what they leave against a fresh handle" % v["id"])
    with H.new_handle(_make, v) as again:
        H.load(again, fenv, left)
        replay = (continue_training(again, fenv), capture(again, v))
    what = "WARP steps in %s: training after them against a replay on a fresh handle" % v["id"]
    same(after[0], replay[0], what + ", reported losses / logits")
    same(after[1], replay[1], what)
