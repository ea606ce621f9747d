"""Call sequences on one SVD handle: the states earlier calls leave behind, the entry points that arrive in them (guests) and
the three statements tests/test_gpu_call_sequences.py holds for every (state, guest), bit for bit:

  1. the guest's result equals the same call on a fresh handle loaded with everything the long-lived one reports;
  2. training afterwards is what it is without the guest (read-only and identity guests) or what replay on fresh handles
     gives (writers: load, guest, read back, load, continue);
  3. an identity write changes nothing in 1 or 2.

A state is built by a named function below, at the smallest shape that reaches it; each builder asserts the step path
(``kernel_plan`` against ``tests/step_cases.path_of``), so a builder that drifts onto another path fails.  Reading a handle
is itself a guest (get_table brings the item rows back from the alternate table, rng_get_state cancels the run-ahead), so
nothing here reads the long-lived handle before its guest: the state is built a second time on a probe handle, which is the
one that is read ("capture"), and the states are deterministic functions of their variant.

The model class is a parameter (``make``): tests/test_call_sequence_host.py runs the same harness on a float32 NumPy stand-in
(tests/handle_stub.py), without a GPU."""
import copy
import zlib

import numpy as np

from tests import step_cases as SC

MU, BU, BI, P, Q = 0, 1, 2, 3, 4                         # include/tfrecomm.h
SLOT_M, SLOT_V = 8, 16
TIDS = (MU, BU, BI, P, Q)
NAMES = {MU: "mu", BU: "bu", BI: "bi", P: "P", Q: "Q"}
ERR_STATE = -4
FROZEN_BUT_USER = (1 << MU) | (1 << BI) | (1 << Q)       # what tfr_finetune_users asks for
RO, WRITER, IDENTITY = "read-only", "writer", "identity"
N_STORE, N_EVAL = 40000, 3000


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7fffffff


def _bytes(*xs):
    """the bits of every array / number, in order (NaN-safe, -0.0 is not +0.0)"""
    out = []
    for x in xs:
        if x is None:
            out.append(b"<none>")
        elif isinstance(x, bytes):
            out.append(x)
        elif isinstance(x, dict):
            out.append(_bytes(*[x[k] for k in sorted(x)]))
        elif isinstance(x, (tuple, list)):
            out.append(_bytes(*x))
        else:
            a = np.ascontiguousarray(np.asarray(x))
            out.append(a.dtype.str.encode() + a.tobytes())
    return b"|".join(out)


# ----------------------------------------------------------------------------- variants
def _v(state, U, I, D, B, opt, mode, loss, way, item_abs=False, n=256, cont=3, tag=""):
    v = dict(state=state, U=U, I=I, D=D, B=B, opt=opt, mode=mode, loss=loss, way=way, item_abs=item_abs, n=n, cont=cont)
    v["id"] = "%s-%s%s-D%d-B%d-%s_%s-%s%s-n%d" % (state, way, tag, D, B, opt, mode, loss, "-abs" if item_abs else "", n)
    return v


LAZY, TF1, SGD = ("adam", "lazy"), ("adam", "tf1"), ("sgd", "tf1")
BIG = 17000                                              # just above CSORT_MAX_BINS rows: the radix sort and the fused step
VARIANTS = [
    # two_table: two host-fed fused steps; rows live in both item tables, runs are cut at block boundaries
    _v("two_table", BIG, BIG, 16, 1500, *LAZY, "mse", "fed"),
    _v("two_table", BIG, BIG, 33, 1500, *SGD, "nll", "fed", item_abs=True),
    # small tables past the counting sort's batch limit (path_switch's shape over 16000 items) take the same two-table step;
    # here the guests that follow are on the TILE path, which reads item_features with no forward launch in front
    _v("two_table", 16000, 16000, 8, 65537, *SGD, "mse", "fed", tag="_small_tables"),
    # + the side-stream look-ahead and the run-ahead draw
    _v("two_table_drawn", BIG, BIG, 16, 1500, *LAZY, "nll", "drawn5", cont=3),
    _v("two_table_drawn", BIG, BIG, 33, 1500, *SGD, "mse", "drawn5", cont=3),
    # tile_lookahead: one and three sort tiles; three ways into the state
    _v("tile_lookahead", 300, 200, 16, 700, *TF1, "mse", "drawn9", cont=9),
    _v("tile_lookahead", 300, 200, 16, 2500, *LAZY, "nll", "drawn3", cont=3),
    _v("tile_lookahead", 300, 200, 16, 2500, *TF1, "nll", "staged", cont=3),
    _v("tile_lookahead", 300, 200, 16, 700, *LAZY, "mse", "staged", cont=3),
    # in_flight: four asynchronous steps and no sync before the guest
    _v("in_flight", 300, 200, 16, 700, *LAZY, "nll", "ids", cont=2),
    _v("in_flight", 300, 200, 16, 2500, *TF1, "mse", "ids", cont=2),
    # grown: capacity 1024 with a published look-ahead sort; the guest stays below it (256) or forces reallocation (3000)
    _v("grown", 300, 200, 16, 700, *TF1, "nll", "staged", n=256),
    _v("grown", 300, 200, 16, 700, *TF1, "nll", "staged", n=3000),
    _v("grown", 300, 200, 16, 700, *LAZY, "mse", "staged", n=256),
    _v("grown", 300, 200, 16, 700, *LAZY, "mse", "staged", n=3000),
]
STATES = ("two_table", "two_table_drawn", "tile_lookahead", "in_flight", "grown")
assert len({v["id"] for v in VARIANTS}) == len(VARIANTS) and {v["state"] for v in VARIANTS} == set(STATES)


def opts_of(v):
    adam = v["opt"] == "adam"
    return dict(loss=v["loss"], item_abs=v["item_abs"], reg_bias=False, optimizer=v["opt"], adam_mode=v["mode"],
                lr=3e-3 if adam else 2.0 ** -12, reg=0.02)


def plan_word(path):
    """what tfr_kernel_plan (csrc/api.hip) says on the branch ``tests/step_cases.path_of`` names"""
    if path.startswith("tiles"):
        return "k_tile_step<"
    if path.startswith("fused"):
        return ", true, true, "                          # k_seg_reduce with the forward inside (fwd_in_reduce)
    if path == "csort":
        return "k_front<"
    return "k_forward<"


def assert_path(m, v, B, path):
    assert SC.path_of(v["U"], v["I"], B, v["opt"], v["mode"]).startswith(path), (v["id"], B, SC.path_of(v["U"], v["I"], B, v["opt"], v["mode"]))
    plan = ";".join("%s=%s" % kv for kv in sorted(m.kernel_plan(B).items()))
    assert plan_word(path) in plan, "%s: batch %d is not on the %s path: %s" % (v["id"], B, path, plan)


# ----------------------------------------------------------------------------- what a builder gives a handle
class Env(object):
    """everything a builder handed to the handle that no call reports back, and the plan of the training that follows"""

    def __init__(self, v):
        self.v = v
        rs = np.random.RandomState(_seed("env", v["U"], v["I"], v["D"]))
        U, I, D = v["U"], v["I"], v["D"]
        self.t0 = dict(mu=np.float32(0.3), bu=rs.normal(0, .3, U).astype(np.float32), bi=rs.normal(0, .3, I).astype(np.float32),
                       P=rs.normal(0, .2, (U, D)).astype(np.float32), Q=rs.normal(0, .2, (I, D)).astype(np.float32))
        # a store whose items repeat (a tenth of it on 40 hot items, one of them on a tenth of that)
        hot = rs.randint(0, I, 40)
        su = rs.randint(0, U, N_STORE).astype(np.int32)
        si = np.where(rs.rand(N_STORE) < 0.3, hot[rs.randint(0, 40, N_STORE)], rs.randint(0, I, N_STORE)).astype(np.int32)
        si[rs.rand(N_STORE) < 0.1] = hot[0]
        self.hot = hot
        self.store = (su, si, self._rates(rs, N_STORE))
        self.evalset = (rs.randint(0, U, N_EVAL).astype(np.int32), rs.randint(0, I, N_EVAL).astype(np.int32), self._rates(rs, N_EVAL))
        key = np.unique(su[:6000].astype(np.int64) * I + si[:6000])
        self.positives = (np.searchsorted(key // I, np.arange(U + 1)).astype(np.int64), (key % I).astype(np.int32))
        self.sampler = (12345, 8)
        self.frozen, self.hyper = 0, (opts_of(v)["lr"], opts_of(v)["reg"])
        self.staged, self.next_step = None, 0
        self.seed = 4321
        self.pre_snapshot = False
        self.item_pool = hot                             # item rows the state's steps surely touched

    def _rates(self, rs, n):
        return (rs.rand(n) < 0.45).astype(np.float32) if self.v["loss"] == "nll" else rs.randint(1, 6, n).astype(np.float32)

    def fed_batch(self, k):
        """host-fed batch k of the two_table plan: about half of its items repeat batch k - 1's, one takes a tenth"""
        v = self.v
        rs = np.random.RandomState(_seed("fed", v["id"].split("-n")[0], 0))
        u = i = r = None
        for s in range(k + 1):
            prev = i
            u = rs.randint(0, v["U"], v["B"]).astype(np.int32)
            i = rs.randint(0, v["I"], v["B"]).astype(np.int32)
            if prev is not None:
                i = np.where(rs.rand(v["B"]) < 0.5, prev[rs.randint(0, v["B"], v["B"])], i).astype(np.int32)
            i[rs.rand(v["B"]) < 0.1] = self.hot[0]
            r = self._rates(rs, v["B"])
        return u, i, r

    def ids_batch(self, k):
        return np.random.RandomState(_seed("ids", k)).randint(0, N_STORE, self.v["B"]).astype(np.int64)


def give(m, env):
    """what every state starts from, on a new handle: the things ``load`` also gives a fresh one (except tables and counters)"""
    m.set_frozen(env.frozen)
    m.set_hyper(*env.hyper)
    m.upload_triples(*env.store)
    m.upload_eval_triples(*env.evalset)
    if hasattr(m, "set_positives"):
        m.set_positives(env.positives)
        m.set_bpr_sampler(*env.sampler)
    if env.staged is not None:
        m.stage_ids(env.staged)


def capture(m, v):
    """what a handle reports: the five tables and their Adam slots, the step counters, the generator state"""
    snap = {"t%d" % t: m.get_table(t) for t in TIDS}
    if v["opt"] == "adam":
        for t in TIDS:
            snap["m%d" % t], snap["v%d" % t] = m.get_table(t | SLOT_M), m.get_table(t | SLOT_V)
    snap["step"] = m.get_step()
    key, pos = m.rng_get_state()
    snap["rng_key"], snap["rng_pos"] = key, pos
    return snap


def load(m, env, snap):
    give(m, env)
    for k, x in snap.items():
        if k[0] in "tmv" and k[1:].isdigit():
            m.set_table(int(k[1:]) | {"t": 0, "m": SLOT_M, "v": SLOT_V}[k[0]], x)
    m.set_step(*snap["step"])
    m.rng_set_state(snap["rng_key"], snap["rng_pos"])


def same(a, b, what):
    """two captures / results carry the same bits; names what differs"""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in sorted(a):
            same(a[k], b[k], "%s[%s]" % (what, NAMES.get(int(k[1:]), k) + k[0] if k[0] in "tmv" and k[1:].isdigit() else k))
        return
    ba, bb = _bytes(a), _bytes(b)
    if ba != bb:
        n = sum(x != y for x, y in zip(ba, bb)) if len(ba) == len(bb) else -1
        first = next((k for k, (x, y) in enumerate(zip(ba, bb)) if x != y), min(len(ba), len(bb)))
        show = (lambda x: x[max(0, first - 8):first + 24]) if isinstance(a, bytes) else (lambda x: np.ravel(np.asarray(x))[:4])
        raise AssertionError("%s differs (%d of %d bytes, the first at %d): %r against %r"
                             % (what, n, len(ba), first, show(a), show(b)))


# ----------------------------------------------------------------------------- the states
def new_handle(make, v):
    return make(v["U"], v["I"], v["D"], **opts_of(v))


def _start(m, env):
    t = env.t0
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    if env.pre_snapshot:
        m.snapshot_bf16()                                # the stale-snapshot guests ask it after the state is built
    give(m, env)
    m.rng_seed(env.seed)


def two_table(m, env):
    """two host-fed fused big-table steps: updated item rows sit in the alternate table (q_dirty), about half of the second
    step's items were the first's, so some rows have flipped twice; the hot item's run is cut at block boundaries"""
    v = env.v
    _start(m, env)
    assert_path(m, v, v["B"], "fused_small" if v["U"] <= SC.CSORT_MAX_BINS else "fused_big")
    for k in range(2):
        m.train_step(*env.fed_batch(k), want_logits=False)
    env.item_pool = np.unique(np.concatenate([env.fed_batch(k)[1] for k in range(2)]))


def two_table_drawn(m, env):
    """the same rows in two tables, left by five drawn steps: the big-table look-ahead on the side stream has run, ids for
    the next call are drawn ahead into the alternate id buffer"""
    v = env.v
    _start(m, env)
    assert_path(m, v, v["B"], "fused_big")
    m.train_steps_drawn(v["B"], 5)


def tile_lookahead(m, env):
    """the small-table step (k_tile_step) after a drawn call of nine or three steps (run-ahead ids), or after four of twelve
    staged steps: the last staged step's launch sorted batch four and published it (pf_valid)"""
    v = env.v
    path = "tiles"
    if v["way"] == "staged":
        env.staged = np.random.RandomState(_seed("staged", v["B"])).randint(0, N_STORE, 12 * v["B"]).astype(np.int64)
        env.next_step = 4
    _start(m, env)
    assert_path(m, v, v["B"], path)
    assert -(-v["B"] // SC.CSORT_TILE) == {700: 1, 2500: 3}[v["B"]]
    if v["way"] == "staged":
        m.train_steps_staged(0, v["B"], 4)
    else:
        m.train_steps_drawn(v["B"], int(v["way"][5:]))


def in_flight(m, env):
    """four asynchronous steps on host-drawn ids, nothing waited for: the guest's work queues behind them"""
    v = env.v
    _start(m, env)
    assert_path(m, v, v["B"], "tiles")
    for k in range(4):
        m.train_step_ids(env.ids_batch(k))
    env.next_step = 4


def grown(m, env):
    """tile_lookahead's staged form at batch 700: the workspace holds 1024 entries and a published look-ahead sort lives in
    it; the guest's own batch (variant ``n``) stays below the capacity or exceeds it, which reallocates every buffer"""
    assert env.v["B"] == 700 and env.v["n"] in (256, 3000)
    tile_lookahead(m, env)


BUILDERS = dict(two_table=two_table, two_table_drawn=two_table_drawn, tile_lookahead=tile_lookahead, in_flight=in_flight,
                grown=grown)


def continue_training(m, env):
    """the training that follows the guest, in the state's own form; returns what it reports (losses, logits)"""
    v = env.v
    way = v["way"]
    if way == "fed":
        lg, loss, reg = m.train_step(*env.fed_batch(2))
        return _bytes(lg, np.float32(loss), np.float32(reg))
    if way.startswith("drawn"):
        return _bytes(m.train_steps_drawn(v["B"], v["cont"], want_loss=True))
    if way == "staged":
        return _bytes(m.train_steps_staged(env.next_step, v["B"], v["cont"], want_loss=True))
    for k in range(v["cont"]):
        m.train_step_ids(env.ids_batch(env.next_step + k))
    m.sync()
    return b""


# ----------------------------------------------------------------------------- guests
class GuestRng(np.random.RandomState):
    """the guest's seeded inputs; ``env`` is the handle's own copy (a guest that replaces the store says so there)"""

    def __init__(self, seed, env, n):
        super(GuestRng, self).__init__(seed)
        self.env, self.n, self.v = env, n, env.v

    def users(self, n=None):
        return self.randint(0, self.v["U"], n or self.n).astype(np.int32)

    def items(self, n=None):
        n = n or self.n
        pool = self.env.item_pool
        return np.where(self.rand(n) < 0.5, pool[self.randint(0, pool.size, n)], self.randint(0, self.v["I"], n)).astype(np.int32)

    def rates(self, n=None):
        return self.env._rates(self, n or self.n)


GUESTS = {}


class Guest(object):
    def __init__(self, name, fn, kind, entries, needs=None, stub=False, stale=False):
        self.name, self.fn, self.kind, self.entries, self.needs, self.stub, self.stale = name, fn, kind, tuple(entries), needs, stub, stale

    def reason_not(self, v):
        """None, or why this guest cannot run in variant v"""
        return self.needs(v) if self.needs else None


def guest(kind, *entries, **kw):
    def deco(fn):
        name = fn.__name__.lstrip("_")
        assert name not in GUESTS
        GUESTS[name] = Guest(name, fn, kind, entries, **kw)
        return fn
    return deco


def _nll(v):
    return None if v["loss"] == "nll" else "eval_binary needs the binary-outcome model: runs in the nll variants of the state"


def _not_tf1(v):
    return "SGD or lazy Adam only (tf1 Adam couples the rows)" if (v["opt"], v["mode"]) == TF1 else None


def _dense(v):
    return "data-parallel steps need dense semantics (tf1 Adam or SGD)" if (v["opt"], v["mode"]) == LAZY else None


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(*arrays):
    torch, dev = _torch()
    out = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    torch.cuda.synchronize()
    return out


def _host(m, *tensors):
    m.sync()
    torch, _ = _torch()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


# -- forward and evaluation
@guest(RO, "tfr_forward", stub=True)
def _forward(m, g):
    return _bytes(m.forward(g.users(), g.items()))


@guest(RO, "tfr_forward_dev")
def _forward_dev(m, g):
    torch, dev = _torch()
    u, i = _dev(g.users(), g.items())
    out = torch.zeros(g.n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m.forward_dev(u.data_ptr(), i.data_ptr(), g.n, out.data_ptr())
    return _bytes(*_host(m, out))


@guest(RO, "tfr_forward_resident", stub=True)
def _forward_resident(m, g):
    lo = int(g.randint(0, N_STORE - g.n))
    return _bytes(m.forward_resident(lo, lo + g.n))


@guest(RO, "tfr_eval", stub=True)
def _eval(m, g):
    return _bytes(np.float64(m.eval(g.users(), g.items(), g.rates())))


@guest(RO, "tfr_eval_resident", stub=True)
def _eval_resident(m, g):
    return _bytes(np.float64(m.eval_resident()))


def _dict_bytes(d):
    return _bytes(*[np.float64(d[k]) for k in sorted(d)])


@guest(RO, "tfr_eval_binary", needs=_nll)
def _eval_binary(m, g):
    return _dict_bytes(m.eval_binary(g.users(), g.items(), g.rates()))


@guest(RO, "tfr_eval_binary_resident", needs=_nll)
def _eval_binary_resident(m, g):
    return _dict_bytes(m.eval_binary_resident())


@guest(RO, "tfr_auc_dev")
def _auc_dev(m, g):
    sc = (g.randint(-9, 10, g.n) * 0.25).astype(np.float32)
    lab = (g.rand(g.n) < 0.4).astype(np.float32)
    s, l = _dev(sc, lab)
    return _bytes(np.float64(m.auc_dev(s.data_ptr(), l.data_ptr(), g.n)))


# -- top-K, ranking, neighbours
def _targets(g, nu):
    items = np.sort(np.stack([g.items(nu), g.items(nu), g.items(nu)], 1), 1)
    keep = np.concatenate([np.ones((nu, 1), bool), items[:, 1:] != items[:, :-1]], 1)
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), items[keep].astype(np.int32)


@guest(RO, "tfr_topk")
def _recommend(m, g):
    return _bytes(*m.recommend(g.users(min(g.n, 96)), k=10))


@guest(RO, "tfr_topk_dev")
def _recommend_dev(m, g):
    (u,) = _dev(g.users(min(g.n, 96)))
    items, scores = m.recommend_dev(u, k=10)
    return _bytes(*_host(m, items, scores))


@guest(RO, "tfr_rank_items")
def _rank_items(m, g):
    nu = min(g.n, 96)
    return _bytes(m.rank_items(g.users(nu), _targets(g, nu)))


def _similar(m, g, suffix=""):
    out = []
    for metric in ("cosine", "dot"):
        out += list(getattr(m, "similar_items" + suffix)(g.items(64), k=8, metric=metric))
        out += list(getattr(m, "similar_users" + suffix)(g.users(64), k=8, metric=metric))
    return out


@guest(RO, "tfr_neighbours")
def _similar_host(m, g):
    return _bytes(*_similar(m, g))


@guest(RO, "tfr_neighbours_dev")
def _similar_dev(m, g):
    out = []
    for metric in ("cosine", "dot"):
        i, u = _dev(g.items(64), g.users(64))
        out += list(m.similar_items_dev(i, k=8, metric=metric)) + list(m.similar_users_dev(u, k=8, metric=metric))
    return _bytes(*_host(m, *out))


# -- bf16 snapshot: taken by the guest, or before the state was built (stale: the queries see the tables of that moment)
def _bf16_queries(m, g):
    nu = min(g.n, 96)
    out = [m.forward_bf16(g.users(), g.items()), np.float64(m.eval_bf16(g.users(), g.items(), g.rates()))]
    out += list(m.recommend_bf16(g.users(nu), k=10)) + [m.rank_items_bf16(g.users(nu), _targets(g, nu))] + _similar(m, g, "_bf16")
    out += [m.bf16_rows(P), m.bf16_rows(Q)]
    return _bytes(*out)


_BF16 = ("tfr_bf16_forward", "tfr_bf16_eval", "tfr_bf16_topk", "tfr_bf16_rank_items", "tfr_bf16_neighbours", "tfr_bf16_get_rows")


@guest(RO, "tfr_bf16_snapshot", *_BF16)
def _bf16_snapshot(m, g):
    m.snapshot_bf16()
    return _bf16_queries(m, g)


@guest(RO, *_BF16, stale=True)
def _bf16_stale(m, g):
    return _bf16_queries(m, g)


@guest(RO, "tfr_bf16_snapshot", "tfr_bf16_forward_dev", "tfr_bf16_topk_dev", "tfr_bf16_neighbours_dev", "tfr_bf16_drop")
def _bf16_dev(m, g):
    torch, dev = _torch()
    m.snapshot_bf16()
    u, i, q = _dev(g.users(), g.items(), g.users(64))
    lg = torch.zeros(g.n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m.forward_bf16_dev(u.data_ptr(), i.data_ptr(), g.n, lg.data_ptr())
    out = [lg] + list(m.recommend_bf16_dev(q, k=10)) + list(m.similar_users_bf16_dev(q, k=8)) + list(m.similar_items_bf16_dev(i[:64].contiguous(), k=8))
    got = _bytes(*_host(m, *out))
    m.drop_bf16()
    return got


# -- sort, draws, streams, uploads
@guest(RO, "tfr_sort_segments")
def _sort_segments(m, g):
    return _bytes(*(m.sort_segments(0, g.users()) + m.sort_segments(1, g.items())))


@guest(WRITER, "tfr_draw_ids", stub=True)                # the generator moves: what follows is held against replay
def _draw_ids(m, g):
    return _bytes(m.draw_ids(12345, g.n))


@guest(WRITER, "tfr_draw_ids_dev", "tfr_join_draws", "tfr_join_draw")
def _draw_ids_dev(m, g):
    torch, dev = _torch()
    a = torch.zeros(g.n, dtype=torch.int64, device=dev)
    b = torch.zeros(g.n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    m.draw_ids_dev(N_STORE, g.n, a.data_ptr())
    m.join_draw(1)
    m.draw_ids_dev(777, g.n, b.data_ptr())
    m.join_draws()
    return _bytes(*_host(m, a, b))


@guest(RO, "tfr_rng_get_state", stub=True)
def _rng_get_state(m, g):
    return _bytes(*m.rng_get_state())


@guest(RO, "tfr_rng_get_state", "tfr_rng_set_state", stub=True)
def _rng_numpy_round_trip(m, g):
    keep = np.random.get_state()
    try:
        m.rng_to_numpy()
        st = np.random.get_state()
        m.rng_from_numpy()
    finally:
        np.random.set_state(keep)
    return _bytes(st[1], np.int64(st[2]))


@guest(RO, "tfr_stage_ids", "tfr_staged_ids_devptr", stub=True)
def _stage_ids(m, g):
    """the staged ids again (or, where the state staged none, new ones: nothing that follows reads them)"""
    if g.env.staged is None:
        g.env.staged = g.randint(0, N_STORE, 4 * g.n).astype(np.int64)
    m.stage_ids(g.env.staged)
    return _bytes(np.int64(m.staged_ids_devptr()[1]))


def _view(ptr, n, typestr):
    torch, dev = _torch()
    holder = type("_V", (), {"__cuda_array_interface__": {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}})()
    return torch.as_tensor(holder, device=dev)


@guest(RO, "tfr_table_devptr", "tfr_staged_ids_devptr", "tfr_scalars_devptr")
def _devptrs(m, g):
    """the tables through their device addresses (item_features settled first), the staged ids where the state staged some"""
    import ctypes
    out = []
    for t in (Q, P, BI):
        ptr, n = m.table_devptr(t)
        m.sync()
        out.append(_view(ptr, n, "<f4").cpu().numpy())
    ptr, n = m.staged_ids_devptr()
    if g.env.staged is not None:
        out.append(_view(ptr, n, "<i8").cpu().numpy())
    p = ctypes.c_void_p()
    assert m._lib.tfr_scalars_devptr(m._h, ctypes.byref(p)) == 0 and p.value
    return _bytes(*out)


@guest(RO, "tfr_upload_triples", stub=True)
def _upload_same_store(m, g):
    m.upload_triples(*g.env.store)
    return b""


@guest(RO, "tfr_set_triples_dev")
def _set_same_store_dev(m, g):
    u, i, r = _dev(*g.env.store)
    m.set_triples_dev(u.data_ptr(), i.data_ptr(), r.data_ptr(), N_STORE)
    m.sync()
    return b""


@guest(RO, "tfr_upload_eval_triples", "tfr_eval_resident", stub=True)
def _upload_eval(m, g):
    g.env.evalset = (g.users(500), g.items(500), g.rates(500))
    m.upload_eval_triples(*g.env.evalset)
    return _bytes(np.float64(m.eval_resident()))


@guest(RO, "tfr_bpr_negatives", "tfr_bpr_set_positives", "tfr_bpr_set_sampler")
def _bpr_negatives(m, g):
    m.set_positives(g.env.positives)
    m.set_bpr_sampler(*g.env.sampler)
    return _bytes(m.bpr_negatives(g.users(), step=17))


# -- writers
def _schedule(g):
    """three users, the smallest schedule tests/test_gpu_finetune.py builds: rows, rounds of growing prefixes"""
    users, rows = [3, 9, 4], [5, 6, 2]
    row_ptr, items, rates, round_ptr, ask, prefix = [0], [], [], [0], [], []
    for n in rows:
        items.append(g.items(n)); rates.append((g.rand(n) < 0.5).astype(np.float32))
        row_ptr.append(row_ptr[-1] + n)
        pre = np.unique(np.linspace(1, n, min(3, n)).astype(np.int64))
        prefix += pre.tolist(); ask += g.items(pre.size).tolist()
        round_ptr.append(round_ptr[-1] + pre.size)
    return (np.asarray(users, np.int32), np.asarray(row_ptr, np.int64), np.concatenate(items).astype(np.int32), np.concatenate(rates),
            np.asarray(round_ptr, np.int64), np.asarray(ask, np.int32), np.asarray(prefix, np.int32), 4)


@guest(WRITER, "tfr_finetune_users", needs=_not_tf1)
def _finetune_users(m, g):
    m.set_frozen(FROZEN_BUT_USER)
    out = m.finetune_users(*_schedule(g))
    m.set_frozen(g.env.frozen)
    return _bytes(*out)


@guest(WRITER, "tfr_bpr_train_step", needs=_not_tf1)
def _train_bpr_step(m, g):
    indptr, items = g.env.positives
    e = g.randint(0, items.size, g.n)
    u = (np.searchsorted(indptr, e, side="right") - 1).astype(np.int32)
    neg, loss, reg, skipped = m.train_bpr_step(u, items[e])
    return _bytes(neg, np.float32(loss), np.float32(reg), np.int64(skipped))


@guest(WRITER, "tfr_bpr_train_step_dev", "tfr_bpr_train_steps_drawn", needs=_not_tf1)
def _train_bpr_dev_and_drawn(m, g):
    indptr, items = g.env.positives
    e = g.randint(0, items.size, g.n)
    u, i = _dev((np.searchsorted(indptr, e, side="right") - 1).astype(np.int32), items[e])
    neg = m.train_bpr_step_dev(u, i, want_negatives=True)
    (neg,) = _host(m, neg)
    return _bytes(neg, m.train_bpr_steps_drawn(g.n, 2, want_loss=True))


@guest(WRITER, "tfr_train_step", stub=True)
def _train_step(m, g):
    lg, loss, reg = m.train_step(g.users(), g.items(), g.rates())
    return _bytes(lg, np.float32(loss), np.float32(reg))


@guest(WRITER, "tfr_train_steps_repeat", stub=True)
def _train_steps_repeat(m, g):
    return _bytes(*m.train_steps_repeat(g.users(), g.items(), g.rates(), 3))


@guest(WRITER, "tfr_train_step_dev")
def _train_step_dev(m, g):
    torch, dev = _torch()
    u, i, r = _dev(g.users(), g.items(), g.rates())
    lg = torch.zeros(g.n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m.train_step_dev(u.data_ptr(), i.data_ptr(), r.data_ptr(), g.n, lg.data_ptr())
    return _bytes(*_host(m, lg))


@guest(WRITER, "tfr_train_steps_resident", "tfr_train_step_ids", stub=True)
def _train_steps_resident(m, g):
    """resident steps on the guest's own ids (they replace the staged ids, as the call documents), then one asynchronous step"""
    ids = g.randint(0, N_STORE, 2 * g.n).astype(np.int64)
    loss = m.train_steps_resident(ids, g.n)
    m.train_step_ids(ids[:g.n])
    m.sync()
    if g.env.staged is not None:                         # put the state's staged ids back for the steps that follow
        m.stage_ids(g.env.staged)
    return _bytes(loss)


@guest(WRITER, "tfr_dp_hint_next", "tfr_dp_local_grads", "tfr_dp_apply", "tfr_dp_flat_size", needs=_dense)
def _dp_steps(m, g):
    """two data-parallel steps of one replica on store ids: the first hints the second's ids, the second takes the hinted sort"""
    torch, dev = _torch()
    (ids,) = _dev(g.randint(0, N_STORE, 2 * g.n).astype(np.int64))
    flat = torch.zeros(m.dp_flat_size(), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    out = []
    for s in range(2):
        if s == 0:
            m.dp_hint_next(ids.data_ptr() + 8 * g.n)
        m.dp_local_grads(None, None, None, g.n, ids.data_ptr() + 8 * g.n * s, flat.data_ptr())
        out += _host(m, flat)
        m.dp_apply(flat.data_ptr())
        m.sync()
    return _bytes(*out)


def _shard_step(m, g, split):
    """one row-sharded step of a world of one rank (every exchange is the identity): the stages of tests/shard_world.World.step"""
    torch, dev = _torch()
    v, n = g.v, g.n
    u, i, r = _dev(g.users(), g.items(), g.rates())
    stride = m.shard_row_stride()
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
    ns = min(v["I"], n)                                  # request slots: tfrecomm_amd/sharded.py capacities, small batches
    req, rows, grad, logits, scal = z(ns, torch.int32), z((ns, stride)), z((ns, stride)), z(n), z(4)
    torch.cuda.synchronize()
    m.shard_select(0)
    m.shard_route(u.data_ptr(), i.data_ptr(), r.data_ptr(), n, 0, 1, v["U"], v["I"], n, ns, req.data_ptr())
    ptrs = m.shard_routed_devptrs()
    m.sync()
    counts = _view(ptrs[3], 3, "<i4").cpu().numpy()
    if split:
        m.shard_presort(req.data_ptr(), ns)
    m.shard_gather(req.data_ptr(), ns, rows.data_ptr())
    if split:
        m.shard_forward_items(rows.data_ptr(), logits.data_ptr(), grad.data_ptr(), scal.data_ptr())
        m.shard_reduce_users(rows.data_ptr())
    else:
        m.shard_forward_reduce(rows.data_ptr(), logits.data_ptr(), grad.data_ptr(), scal.data_ptr())
    m.shard_apply_items(req.data_ptr(), grad.data_ptr(), ns)
    m.shard_finish_step(scal.data_ptr())
    return _bytes(counts, *_host(m, req, rows, grad, logits, scal))


_SHARD = ("tfr_shard_select", "tfr_shard_route", "tfr_shard_routed_devptrs", "tfr_shard_gather", "tfr_shard_apply_items",
          "tfr_shard_finish_step", "tfr_shard_row_stride")


@guest(WRITER, "tfr_shard_forward_reduce", *_SHARD)
def _shard_step_fused(m, g):
    return _shard_step(m, g, False)


@guest(WRITER, "tfr_shard_forward_items", "tfr_shard_reduce_users", "tfr_shard_presort", *_SHARD)
def _shard_step_split(m, g):
    return _shard_step(m, g, True)


@guest(WRITER, "tfr_init_tables", stub=True)
def _init_tables(m, g):
    m.init_tables(seed=7)
    return b""


@guest(WRITER, "tfr_get_table", "tfr_set_table", stub=True)
def _set_table_changed(m, g):
    q = m.get_table(Q)
    q[g.env.item_pool[:50]] *= np.float32(0.5)
    m.set_table(Q, q)
    return b""


@guest(WRITER, "tfr_upload_triples", stub=True)
def _upload_other_store(m, g):
    su, si, sr = g.env.store
    p = g.permutation(N_STORE)
    g.env.store = (su[p], si[p], sr[p])
    m.upload_triples(*g.env.store)
    return b""


# -- identity writes
@guest(IDENTITY, "tfr_get_table", "tfr_set_table", stub=True)
def _set_table_same(m, g):
    slots = (0, SLOT_M, SLOT_V) if g.v["opt"] == "adam" else (0,)
    for t in TIDS:
        for s in slots:
            m.set_table(t | s, m.get_table(t | s))
    return b""


@guest(IDENTITY, "tfr_get_step", "tfr_set_step", stub=True)
def _set_step_same(m, g):
    m.set_step(*m.get_step())
    return b""


@guest(IDENTITY, "tfr_set_frozen", "tfr_set_hyper", stub=True)
def _set_frozen_hyper_same(m, g):
    m.set_frozen(g.env.frozen)
    m.set_hyper(*g.env.hyper)
    return b""


@guest(IDENTITY, "tfr_set_stream", "tfr_switch_stream", "tfr_get_stream", "tfr_sync")
def _streams_and_back(m, g):
    torch, dev = _torch()
    own = m.get_stream()
    side = torch.cuda.Stream(device=dev)
    m.set_stream(side.cuda_stream)                       # drains the stream in use
    m.set_stream(None)
    assert m.get_stream() == own
    m.switch_stream(side.cuda_stream)                    # nothing is queued on the side stream: no ordering is owed
    m.switch_stream(None)
    assert m.get_stream() == own
    return b""


@guest(RO, "tfr_get_table", "tfr_get_step", "tfr_rng_get_state", stub=True)
def _capture(m, g):
    """what the harness itself does to the probe handle: read every table, slot, counter and the generator"""
    return _bytes(capture(m, g.v))


# ----------------------------------------------------------------------------- the three statements
_CACHE = {}


def _built(make, v, pre_snapshot=False):
    env = Env(v)
    env.pre_snapshot = pre_snapshot
    m = new_handle(make, v)
    BUILDERS[v["state"]](m, env)
    return m, env


def reference(make, v):
    """per variant, once: the probe's capture of the state, and what training gives when no guest comes between"""
    key = (make, v["id"])
    if key not in _CACHE:
        m, env = _built(make, v)
        with m:
            snap = capture(m, v)
        m, env2 = _built(make, v)
        with m:
            after = (continue_training(m, env2), capture(m, v))
        _CACHE[key] = (snap, env, after)
    return _CACHE[key]


def run_case(make, v, guest_name):
    g = GUESTS[guest_name]
    assert g.reason_not(v) is None, g.reason_not(v)
    snap, env0, plain = reference(make, v)
    seed = _seed("guest", guest_name)
    # the long-lived handle: state, guest, the training that follows
    live, env = _built(make, v, pre_snapshot=g.stale)
    with live:
        got = g.fn(live, GuestRng(seed, env, v["n"]))
        after = (continue_training(live, env), capture(live, v))
    # the same call on a history-free handle with the same bits
    fenv = copy.copy(env0)
    with new_handle(make, v) as fresh:
        if g.stale:                                      # the snapshot belongs to the tables of before the state
            t = fenv.t0
            fresh.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
            fresh.snapshot_bf16()
        load(fresh, fenv, snap)
        want = g.fn(fresh, GuestRng(seed, fenv, v["n"]))
        mid = capture(fresh, v) if g.kind == WRITER else None
    same(got, want, "%s in %s: the guest's result against a fresh handle" % (guest_name, v["id"]))
    if g.kind == WRITER:                                 # replay: load what the guest left, continue
        with new_handle(make, v) as again:
            load(again, fenv, mid)
            plain = (continue_training(again, fenv), capture(again, v))
    what = "%s in %s: training after the guest against %s" % (guest_name, v["id"], "replay on fresh handles" if g.kind == WRITER else "the same plan without it")
    same(after[0], plain[0], what + ", reported losses / logits")
    same(after[1], plain[1], what)


def cases(stub_only=False):
    """[(variant, guest name)] that run, and {(state, guest name): reason} for the pairs that run in no variant of a state"""
    run, why = [], {}
    for name, g in sorted(GUESTS.items()):
        if stub_only and not g.stub:
            continue
        for state in STATES:
            ok = [v for v in VARIANTS if v["state"] == state and g.reason_not(v) is None]
            run += [(v, name) for v in ok]
            if not ok:
                why[(state, name)] = [g.reason_not(v) for v in VARIANTS if v["state"] == state][0]
    return run, why


# ----------------------------------------------------------------------------- path_switch
PATH_SWITCH = dict(U=16000, I=200, D=8, opt="adam", mode="lazy", loss="mse", item_abs=False, state="path_switch", id="path_switch")
# At 200 items every item's run in a batch of 65537 (~330 entries) is longer than a reduce block (1024 / G = 256 entries): each
# is cut at a block boundary and finished in place by k_apply_rows, so no row ever moves to the alternate table and the
# `!dual && settle_q` transition has nothing to bring back.  The same plan over 16000 items (runs of ~4 entries, whole inside a
# block) leaves most rows there: this is the shape at which that transition does work.
PATH_SWITCH_ITEMS = dict(PATH_SWITCH, I=16000, id="path_switch_items")
PATH_SWITCHES = {v["id"]: v for v in (PATH_SWITCH, PATH_SWITCH_ITEMS)}
# (65537 entries: 65 tiles x 16384 bins exceed the counting sort's table, so the small tables take the radix sort and the fused
#  step - path_of's "fused_small" -, which is the two-table form at any table size)
PATH_SWITCH_STEPS = [(700, "tiles"), (16385, "csort"), (65537, "fused_small"), (700, "tiles"), (65537, "fused_small"), (16385, "csort")]


def path_switch_batch(v, k):
    B = PATH_SWITCH_STEPS[k][0]
    rs = np.random.RandomState(_seed("path_switch", k))
    return rs.randint(0, v["U"], B).astype(np.int32), rs.randint(0, v["I"], B).astype(np.int32), rs.randint(1, 6, B).astype(np.float32)


def path_switch_chain(make, v=PATH_SWITCH):
    """step k on a fresh handle loaded with the state before it, for every k: [(logits, loss, reg, capture after)]"""
    key = (make, v["id"])
    if key not in _CACHE:
        env = Env(v)
        out, snap = [], None
        for k, (B, path) in enumerate(PATH_SWITCH_STEPS):
            with new_handle(make, v) as m:
                if snap is None:
                    _start(m, env)
                else:
                    load(m, env, snap)
                assert_path(m, v, B, path)
                lg, loss, reg = m.train_step(*path_switch_batch(v, k))
                snap = capture(m, v)
            out.append((_bytes(lg, np.float32(loss), np.float32(reg)), snap))
        _CACHE[key] = out
    return _CACHE[key]


def path_switch_live(make, nsteps, v=PATH_SWITCH):
    """the first nsteps steps on ONE handle with nothing read in between: (what each step reported, capture at the end)"""
    env = Env(v)
    with new_handle(make, v) as m:
        _start(m, env)
        seen = []
        for k in range(nsteps):
            lg, loss, reg = m.train_step(*path_switch_batch(v, k))
            seen.append(_bytes(lg, np.float32(loss), np.float32(reg)))
        return seen, capture(m, v)
