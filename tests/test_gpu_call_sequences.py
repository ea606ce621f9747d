"""Every public entry point of the SVD handle, run as a guest in each kind of state earlier calls leave behind
(tests/handle_states.py names the states, the guests and the three statements).  The reference is the library's own kernel on
identical bits from a history-free handle, so every comparison is exact: no tolerance.

Also here: the value of ``last_batch_auc`` and what every other call between the step and it may do to it, and the
``path_switch`` sequence, the one place where a handle alternates between the tile, counting-sort and fused two-table step
(and their capacities) with nothing read in between."""
import functools

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import handle_states as H

pytestmark = pytest.mark.gpu

_RUN, _WHY = H.cases()


def _make(U, I, D, **kw):
    return T.SvdModel(U, I, D, device=0, **kw)


def _stop_at_a_device_error(test):
    """a HIP error (a fault among them) ends the session: nothing more is started on a device that reported one"""
    @functools.wraps(test)
    def run(*a, **k):
        try:
            return test(*a, **k)
        except T.TfrError as e:
            if e.code == L.ERR_HIP:
                pytest.exit("the device reported an error, stopping: %s" % e, returncode=3)
            raise
    return run


@pytest.mark.parametrize("v,guest", _RUN, ids=["%s-%s" % (v["id"], g) for v, g in _RUN])
@_stop_at_a_device_error
def test_guest_in_state(v, guest):
    H.run_case(_make, v, guest)


# ----------------------------------------------------------------------------- path_switch
@pytest.mark.parametrize("shape", sorted(H.PATH_SWITCHES))
@_stop_at_a_device_error
def test_path_switch_steps_take_the_paths_they_name(shape):
    H.path_switch_chain(_make, H.PATH_SWITCHES[shape])    # asserts kernel_plan per step


@pytest.mark.parametrize("nsteps", range(1, len(H.PATH_SWITCH_STEPS) + 1))
@pytest.mark.parametrize("shape", sorted(H.PATH_SWITCHES))
@_stop_at_a_device_error
def test_path_switch(shape, nsteps):
    """tiles, csort, fused (two tables), tiles, fused, csort on one lazy-Adam handle: each step's logits, loss and regulariser,
    and the tables and slots after step ``nsteps``, against the same step on a fresh handle loaded with the state before it.
    Step 4 and step 6 are where a step that is not the two-table one meets rows in the alternate item table - at 16000 items
    (``path_switch_items``); at 200 every run is cut at a block boundary and no row moves (tests/handle_states.py)."""
    v = H.PATH_SWITCHES[shape]
    chain = H.path_switch_chain(_make, v)
    seen, end = H.path_switch_live(_make, nsteps, v)
    for k in range(nsteps):
        H.same(seen[k], chain[k][0], "path_switch step %d (batch %d, %s): logits, loss, regulariser" % ((k + 1,) + H.PATH_SWITCH_STEPS[k]))
    H.same(end, chain[nsteps - 1][1], "path_switch after step %d" % nsteps)


# ----------------------------------------------------------------------------- last_batch_auc
STAGE_MAX = 1 << 20                                      # csrc/api.hip: larger host batches take the plain copies and d_r


def _auc_model(mode="lazy"):
    v = H._v("tile_lookahead", 300, 200, 16, 700, "adam", mode, "nll", "fed")
    env = H.Env(v)
    m = H.new_handle(_make, v)
    H._start(m, env)
    return m, env, v


def _batch(B, seed=5):
    rs = np.random.RandomState(seed)
    # few distinct users and items on purpose: equal logits (ties) by the thousand
    return rs.randint(0, 300, B).astype(np.int32), rs.randint(0, 200, B).astype(np.int32), (rs.rand(B) < 0.4).astype(np.float32)


@pytest.mark.parametrize("B", [700, STAGE_MAX, STAGE_MAX + 1], ids=["staged-700", "staged-2^20", "plain-2^20+1"])
@_stop_at_a_device_error
def test_last_batch_auc_is_the_auc_of_the_returned_logits(B):
    """to 1e-12 of sklearn's roc_auc_score on the logits the step returned (the bound tests/test_gpu_session.py uses for
    eval_binary: the rank sum is integer arithmetic); batches up to STAGE_MAX keep their rates in the staging buffer, larger
    ones in d_r"""
    from sklearn.metrics import roc_auc_score
    from tfrecomm_amd import adaptive_test as AT
    u, i, r = _batch(B)
    m, env, v = _auc_model()
    with m:
        lg, _, _ = m.train_step(u, i, r)
        got = m.last_batch_auc()
        again = m.last_batch_auc()
    want = roc_auc_score(r, lg.astype(np.float64))
    print("last_batch_auc B=%d: device %.17g sklearn %.17g diff %.3g" % (B, got, want, abs(got - want)))
    assert abs(got - want) <= 1e-12
    assert again == got
    if B <= 700:
        assert abs(got - AT.roc_auc(r, lg)) <= 1e-12


@_stop_at_a_device_error
def test_last_batch_auc_after_train_steps_repeat():
    from sklearn.metrics import roc_auc_score
    u, i, r = _batch(700, seed=6)
    m, env, v = _auc_model()
    with m:
        lg, loss = m.train_steps_repeat(u, i, r, 3)
        got = m.last_batch_auc()
    want = roc_auc_score(r, lg.astype(np.float64))
    print("last_batch_auc after train_steps_repeat: device %.17g sklearn %.17g" % (got, want))
    assert abs(got - want) <= 1e-12


@_stop_at_a_device_error
def test_last_batch_auc_needs_a_kept_batch():
    u, i, r = _batch(700)
    m, env, v = _auc_model()
    with m:
        with pytest.raises(T.TfrError) as e:
            m.last_batch_auc()
        assert e.value.code == H.ERR_STATE
        m.train_step(u, i, r, want_logits=False)
        with pytest.raises(T.TfrError) as e:
            m.last_batch_auc()
        assert e.value.code == H.ERR_STATE


_AUC_FIRST = {}


def _auc_first(mode):
    if mode not in _AUC_FIRST:
        from sklearn.metrics import roc_auc_score
        u, i, r = _batch(700)
        m, env, v = _auc_model(mode)
        with m:
            lg, _, _ = m.train_step(u, i, r)
            _AUC_FIRST[mode] = m.last_batch_auc()
        assert abs(_AUC_FIRST[mode] - roc_auc_score(r, lg.astype(np.float64))) <= 1e-12
    return _AUC_FIRST[mode]


def _between(mode):
    v = H._v("tile_lookahead", 300, 200, 16, 700, "adam", mode, "nll", "fed")
    # (train_step and train_steps_repeat with logits keep a batch of their own: the value tests above are theirs)
    return [g for g in sorted(H.GUESTS) if H.GUESTS[g].reason_not(v) is None and not H.GUESTS[g].stale
            and g not in ("train_step", "train_steps_repeat")]


_BETWEEN = [(g, "lazy") for g in _between("lazy")] + [(g, "tf1") for g in _between("tf1") if g not in _between("lazy")]
_BETWEEN += [("train_steps_drawn", "lazy"), ("train_steps_staged", "lazy"), ("train_step_no_logits", "lazy")]


@pytest.mark.parametrize("n", [256, 3000])
@pytest.mark.parametrize("guest,mode", _BETWEEN, ids=[g for g, _ in _BETWEEN])
@_stop_at_a_device_error
def test_last_batch_auc_after_another_call(guest, mode, n):
    """train_step with logits, any other call, last_batch_auc: that batch's AUC exactly, or TFR_ERR_STATE - never another
    number.  n = 3000 exceeds the workspace the step of 700 left (capacity 1024): the call in between reallocates it."""
    want = _auc_first(mode)
    u, i, r = _batch(700)
    m, env, v = _auc_model(mode)
    with m:
        m.train_step(u, i, r)
        if guest == "train_steps_drawn":
            m.train_steps_drawn(n, 2)
        elif guest == "train_steps_staged":
            m.stage_ids(np.random.RandomState(1).randint(0, H.N_STORE, 2 * n).astype(np.int64))
            m.train_steps_staged(0, n, 2)
        elif guest == "train_step_no_logits":
            m.train_step(*[c[:n % 700 + 100] for c in _batch(700, seed=9)], want_logits=False)
        else:
            H.GUESTS[guest].fn(m, H.GuestRng(H._seed("auc", guest), env, n))
        try:
            got = m.last_batch_auc()
        except T.TfrError as e:
            assert e.code == H.ERR_STATE, e
            print("last_batch_auc after %s (n=%d): refused" % (guest, n))
            return
    print("last_batch_auc after %s (n=%d): kept" % (guest, n))
    assert got == want, "last_batch_auc after %s returned %.17g, the batch's AUC is %.17g" % (guest, got, want)
