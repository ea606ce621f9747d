"""Drawn steps whose ids come in large chunks (tfr_train_steps_drawn, api.hip IdsReady: on the small-table path a chunk
grows to 256 steps, TFR_CHUNK_STEPS=<n> for A/B): calls long enough for the chunks to reach their cap, against the same
steps on ids drawn by NumPy on the host - per-step losses, all five tables and the generator's state afterwards, bit for
bit - and the cap's other settings (one step per chunk, the former six) against the default.  The
switch is read once per process: those runs are child processes."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import tfrecomm_amd as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(m):
    h = hashlib.sha256()
    for k, v in sorted(m.tables().items()):
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def _store(U, I, N):
    rs = np.random.RandomState(3)
    return rs.randint(0, U, N).astype(np.int32), rs.randint(0, I, N).astype(np.int32), rs.randint(1, 6, N).astype(np.float32)


# chunk sizes grow by a third of what is drawn: a 256-step chunk first appears after 768 steps.
@pytest.mark.parametrize("U,I,D,B,N,calls", [
    (6040, 3952, 64, 10000, 900188, (40, 1100)),                 # the headline shape; the second call starts on ids drawn ahead
    (300, 200, 20, 1000, (1 << 19) + 1, (1100,)),                # ~50 % rejection; early chunks by the one-workgroup draw, late
])                                                               # ones (up to 256000 ids) by the wide form
def test_long_drawn_calls_equal_host_drawn_steps(U, I, D, B, N, calls):
    su, si, sr = _store(U, I, N)
    steps = sum(calls)
    out = []
    for device_draw in (False, True):
        with T.SvdModel(U, I, D, adam_mode="tf1", device=0) as m:
            m.init_tables(seed=5)
            m.upload_triples(su, si, sr)
            np.random.seed(13575)
            if device_draw:
                m.rng_from_numpy()
                loss = np.concatenate([m.train_steps_drawn(B, k, want_loss=True) for k in calls])
                m.rng_to_numpy()
            else:
                loss = m.train_steps_resident(np.random.randint(0, N, (steps, B)), B)
            tail = np.random.randint(0, 1 << 30, 8)              # the host stream continues identically
            out.append((np.asarray(loss, np.float32), _digest(m), tail.tolist()))
    assert out[0][0].shape == (steps,) and np.isfinite(out[0][0]).all()
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1:] == out[1][1:]


_SCRIPT = r"""
import hashlib
import numpy as np, torch
torch.cuda.init(); torch.zeros(1, device='cuda')
import tfrecomm_amd as T
U, I, D, B, N = 6040, 3952, 64, 10000, 900188
rs = np.random.RandomState(3)
su, si, sr = rs.randint(0, U, N).astype(np.int32), rs.randint(0, I, N).astype(np.int32), rs.randint(1, 6, N).astype(np.float32)
h = hashlib.sha256()
with T.SvdModel(U, I, D, adam_mode="tf1", device=0) as m:
    m.init_tables(seed=5)
    m.upload_triples(su, si, sr)
    m.rng_seed(13575)
    for k in (3, 280):
        h.update(np.asarray(m.train_steps_drawn(B, k, want_loss=True), np.float32).tobytes())
    for _, v in sorted(m.tables().items()):
        h.update(np.ascontiguousarray(v).tobytes())
    key, pos = m.rng_get_state()
    h.update(np.asarray(key).tobytes()); h.update(str(int(pos)).encode())
print("digest", h.hexdigest())
"""


def test_every_chunk_cap_gives_the_same_steps():
    got = {}
    for cap in (None, "1", "6"):
        env = dict(os.environ)
        env.pop("TFR_CHUNK_STEPS", None)
        if cap:
            env["TFR_CHUNK_STEPS"] = cap
        p = subprocess.run([sys.executable, "-c", _SCRIPT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "digest" in p.stdout, p.stderr[-2000:]
        got[cap] = p.stdout.split("digest")[1].split()[0]
    assert len(set(got.values())) == 1, got
