"""What a child process of tests/test_gpu_switches.py runs: the workloads of tests/switch_cases.py under the environment the
parent gave it, written to one .npz.  Arrays above 4096 elements are kept as their sha256 (key + "#sha256"): the parent
compares bits, not values.  ``meta`` (JSON) holds the kernel plans, the violated statements of tests/step_ref.py, the
k_gather_triples counts and the times."""
import hashlib
import json
import sys
import time

import numpy as np

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import step_cases as S
from tests import step_ref as R
from tests import switch_cases as C

FLAGS = dict(loss="mse", item_abs=False, reg_bias=False)


def _put(out, key, arr):
    arr = np.ascontiguousarray(arr)
    if arr.size > 4096:
        out[key + "#sha256"] = np.frombuffer(hashlib.sha256(arr.tobytes()).digest(), np.uint8)
    else:
        out[key] = arr


def _snapshot(m, adam):
    snap = {}
    for name in R.NAMES:
        tid = R.TID[name]
        d = dict(w=m.get_table(tid))
        if adam:
            d["m"], d["v"] = m.get_table(tid | L.SLOT_M), m.get_table(tid | L.SLOT_V)
        snap[name] = d
    return snap


def _put_snapshot(out, key, snap):
    for name, d in snap.items():
        for slot, arr in d.items():
            _put(out, "%s/%s.%s" % (key, name, slot), arr)


def _plan(m, B):
    return ";".join("%s=%s" % kv for kv in m.kernel_plan(B).items())


def _steps(out, meta, key, U, I, D, opt, tables, bat, check):
    """host-fed single steps (each held to tests/step_ref.py where ``check``), then the same batches staged: the batches of
    the leading size in one train_steps_staged call, a ragged last one restaged for a call of its own"""
    adam = opt[0] == "adam"
    lr = S.ADAM_LR if adam else S.SGD_LR
    kw = dict(optimizer=opt[0], adam_mode=opt[1], lr=lr, reg=S.REG, **FLAGS)

    def model():
        m = T.SvdModel(U, I, D, **kw)
        m.set_tables(tables["mu"], tables["bu"], tables["bi"], tables["P"], tables["Q"])
        return m

    B = bat[0][0].size
    with model() as m:
        meta["plan"][key] = _plan(m, B)
        before = _snapshot(m, adam) if check else None
        for s, (u, i, r) in enumerate(bat):
            powers = m.get_step()[1:]
            logits, loss, reg = m.train_step(u, i, r)
            _put(out, "%s/host/logits%d" % (key, s), logits)
            _put(out, "%s/host/loss%d" % (key, s), np.array([loss, reg], np.float32))
            if check:
                after = _snapshot(m, adam)
                bad = R.check_step(before, after, u, i, r, opt=opt[0], mode=opt[1], lam=S.REG, lr=lr, powers=powers, fresh=s == 0, **FLAGS)
                meta["bad"] += ["%s, step %d: %s" % (key, s, b) for b in bad]
                before = after
        _put_snapshot(out, key + "/host", _snapshot(m, adam))
    full = [b for b in bat if b[0].size == B]
    with model() as m:
        m.upload_triples(*(np.concatenate([b[c] for b in bat]) for c in range(3)))
        m.stage_ids(np.arange(len(full) * B, dtype=np.int64))
        _put(out, key + "/staged/loss", m.train_steps_staged(0, B, len(full), want_loss=True))
        at = len(full) * B
        for b in bat[len(full):]:
            m.stage_ids(np.arange(at, at + b[0].size, dtype=np.int64))
            _put(out, key + "/staged/loss_ragged", m.train_steps_staged(0, b[0].size, 1, want_loss=True))
            at += b[0].size
        _put_snapshot(out, key + "/staged", _snapshot(m, adam))
        # a separate k_gather_triples launch shows in the profile's gather slot; profiling turns the look-ahead off, so it
        # is switched on only now, for one more staged step that is not compared
        m.profile(True)
        m.stage_ids(np.arange(B, dtype=np.int64))
        m.train_steps_staged(0, B, 1)
        m.sync()
        meta["gather"][key] = int(m.profile_read()["gather"][1])


def big_key(D, opt, B):
    return "big/D%d-%s_%s-B%d" % (D, opt[0], opt[1], B)


def run_big(out, meta, widths, check):
    for D in widths:
        for opt in C.BIG_OPTS:
            key = big_key(D, opt, C.BIG_B)
            if key not in meta["plan"]:
                _steps(out, meta, key, C.BIG_U, C.BIG_I, D, opt, C.big_tables(D), C.big_batches(C.BIG_B), check)


def run_big_long(out, meta, check):
    for D, opt in C.BIG_LONG:
        _steps(out, meta, big_key(D, opt, C.BIG_LONG_B), C.BIG_U, C.BIG_I, D, opt, C.big_tables(D), C.big_batches(C.BIG_LONG_B), check)


def tile_key(D, B):
    return "tiles/D%d-B%d" % (D, B)


def run_tiles(out, meta, check):
    for D, B in C.TILE_SHAPES:
        tables = C.rand_tables(np.random.RandomState(100 + D), C.TILE_U, C.TILE_I, D, scale=0.3 / np.sqrt(max(D, 16) / 16))
        rs = np.random.RandomState(B)
        bat = [(C.dup_heavy_ids(rs, C.TILE_U, B), C.dup_heavy_ids(rs, C.TILE_I, B), rs.randint(1, 6, B).astype(np.float32)) for _ in range(3)]
        _steps(out, meta, tile_key(D, B), C.TILE_U, C.TILE_I, D, ("adam", "tf1"), tables, bat, check)


def run_sort(out, meta, name, shapes):
    """sort_segments against np.argsort(kind="stable"); meta["sort"][name] lists (n, B, positions equal, keys equal)"""
    rows = meta["sort"].setdefault(name, [])
    for n, sizes in shapes:
        with T.SvdModel(n, 16, 4, optimizer="sgd") as m:
            for B in sizes:
                ids = C.sort_ids(n, B)
                t0 = time.time()
                want = np.argsort(ids, kind="stable").astype(np.int32)
                t1 = time.time()
                ks, ps = m.sort_segments(0, ids)
                t2 = time.time()
                rows.append([n, B, bool(np.array_equal(ps, want)), bool(np.array_equal(ks, ids[want]))])
                meta["plan"]["sort/B%d" % B] = m.kernel_plan(B)["sort"]
                meta["times"]["sort/n%d-B%d" % (n, B)] = dict(argsort=round(t1 - t0, 3), device=round(t2 - t1, 3))
                del want, ks, ps, ids


def run_draw(out, meta):
    """tests/test_gpu_rng.py's draws, as test_draw_matches_numpy_and_leaves_numpy_state checks them"""
    from tests.test_gpu_rng import DRAW_CASES
    rows = meta["draw"] = []
    with T.SvdModel(50, 40, 8, device=0) as m:
        np.random.seed(13575)
        m.rng_seed(13575)
        for high, count in DRAW_CASES:
            want = np.random.randint(0, high, (count,))
            t0 = time.time()
            got = m.draw_ids(high, count)
            dt = time.time() - t0
            key, pos = m.rng_get_state()
            st = np.random.get_state()
            rows.append([high, count, bool(got.dtype == want.dtype == np.int64 and np.array_equal(got, want)),
                         bool(pos == st[2] and np.array_equal(key, st[1])), round(dt, 3)])


def main(path, names):
    t0 = time.time()
    out, meta = {}, dict(plan={}, bad=[], gather={}, sort={}, times={}, workloads=list(names))
    check = "check" in names                      # hold every host-fed step to tests/step_ref.py
    for name in names:
        t1 = time.time()
        if name == "big_general":
            run_big(out, meta, C.BIG_GENERAL, check)
        elif name == "big_stream":
            run_big(out, meta, C.BIG_STREAM, check)
        elif name == "big_long":
            run_big_long(out, meta, check)
        elif name == "tiles":
            run_tiles(out, meta, check)
        elif name == "sort_wide_min":
            run_sort(out, meta, name, [(n, C.SORT_WIDE_MIN_B) for n in C.SORT_WIDE_MIN_N])
        elif name == "sort_narrow":
            run_sort(out, meta, name, [(C.SORT_NARROW_N, C.SORT_NARROW_B)])
        elif name == "sort_narrow_pref":
            run_sort(out, meta, name, [(C.SORT_NARROW_PREF_N, C.SORT_NARROW_PREF_B)])
        elif name == "sort_plans":                 # the default side of the sort workloads: which pass each size takes
            with T.SvdModel(C.SORT_NARROW_N, 16, 4, optimizer="sgd") as m:
                for B in C.SORT_WIDE_MIN_B + C.SORT_NARROW_B + C.SORT_NARROW_PREF_B:
                    meta["plan"]["sort/B%d" % B] = m.kernel_plan(B)["sort"]
        elif name == "draw":
            run_draw(out, meta)
        elif name != "check":
            raise ValueError(name)
        meta["times"][name] = round(time.time() - t1, 2)
    meta["times"]["total"] = round(time.time() - t0, 2)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez(path, **out)
    print("CHILD OK %.1f s" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
