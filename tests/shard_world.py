"""An in-process world for the row-sharded step (TEST ONLY): ``world`` shard backends in one process - ``HipShard`` on one
GPU, tests/fake_shard_backend.OracleShard on the CPU - driven through one global step stage by stage, every intermediate
kept per rank.  An equal-split all-to-all is a reshuffle of tensor chunks (``out[r].chunk(w) = inp[w].chunk(r)``), the scalar
all-reduce a sum over the ranks in rank order; no torch.distributed, no child process.

Beside the world: the per-stage statements (gather, forward outputs, gradient rows, the owner's apply), shared by
tests/test_gpu_shard_stages.py and tests/test_shard_stages_host.py.  Every limit is ``step_ref.limit_from`` of the float32
oracle on the same inputs, or an exact-bits statement.  NumPy and torch only."""
import numpy as np
import torch

from oracle import svd_oracle as so
from tests import step_ref as R
from tests.util import RTOL, rel_err
from tfrecomm_amd import _lib as L
from tfrecomm_amd import sharded

ITEM_SIDE = ("Q", "bi")


class _Comm(object):                     # ShardedSvd.capacities / pair_capacity need only rank and world
    def __init__(self, rank, world):
        self.rank, self.world = rank, world


def geometry(D):
    """(G, VEC) of the row kernels (csrc/svd_kernels.h geometry), as tests/test_width_coverage.py restates it"""
    vec = 4 if D % 4 == 0 else 1
    lanes, g = -(-D // vec), 4
    while g < lanes:
        g *= 2
    return g, vec


def exchange(parts):
    """the equal-split all-to-all of ``parts[rank]`` (each ``world`` equal chunks along dim 0): chunk w of out[r] = chunk r of
    parts[w].  Torch indexing on the current stream."""
    world = len(parts)
    cut = [p.reshape((world, -1) + tuple(p.shape[1:])) for p in parts]
    return [torch.cat([cut[w][r] for w in range(world)], dim=0).contiguous() for r in range(world)]


def _np(t):
    return t.detach().cpu().numpy().copy()


class World(object):
    """``factory(u_rows, i_rows, dim)`` builds one rank's backend.  ``step`` runs one global step and returns its record:
    per stage a list over the ranks of NumPy copies."""

    def __init__(self, U, I, D, world, factory, device="cpu"):
        self.U, self.I, self.D, self.world = U, I, D, world
        self.device = torch.device(device)
        self.sh = [sharded.ShardedSvd(U, I, D, _Comm(r, world), factory, device=self.device) for r in range(world)]
        self.be = [s.backend for s in self.sh]
        self.hip = hasattr(self.be[0], "model")
        self.per_u, self.per_i = self.sh[0].per_u, self.sh[0].per_i

    def close(self):
        for be in self.be:
            if self.hip:
                be.model.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state ---------------------------------------------------------------------------------
    def set_tables(self, t):
        for s in self.sh:
            s.set_tables_from_global(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])

    def set_frozen(self, mask):
        for be in self.be:
            if self.hip:
                be.model.set_frozen(mask)
            else:
                be.o.frozen = mask

    def set_hyper(self, lr, reg):
        for be in self.be:
            if self.hip:
                be.model.set_hyper(lr, reg)
            else:
                be.o.lr, be.o.reg = lr, reg

    def get_step(self, rank):
        """(step, beta1 power, beta2 power) of one rank"""
        be = self.be[rank]
        if self.hip:
            return be.model.get_step()
        return be.o.step, float(be.o.b1p), float(be.o.b2p)

    def sync(self):
        for be in self.be:
            be.sync()

    def _read(self, rank, tid, slot):
        be = self.be[rank]
        if self.hip:
            return be.model.get_table(tid | {"w": 0, "m": L.SLOT_M, "v": L.SLOT_V}[slot])
        o = be.o
        return np.array(o.tables()[tid] if slot == "w" else getattr(o.slots[tid], slot))

    def local(self, rank, name, adam):
        """{w, m, v} of one rank's shard of a table, the dummy row of an empty shard dropped"""
        s = self.sh[rank]
        rows = None if name == "mu" else (s.u_hi - s.u_lo if name in ("P", "bu") else s.i_hi - s.i_lo)
        out = {}
        for slot in ("w", "m", "v") if adam else ("w",):
            a = self._read(rank, R.TID[name], slot)
            out[slot] = a if rows is None else a[:rows]
        return out

    def snapshot(self, adam, names=R.NAMES):
        """the global tables (and Adam slots) assembled from the shard slices, following shard_range"""
        self.sync()
        out = {}
        for name in names:
            parts = [self.local(r, name, adam) for r in range(self.world)]
            if name == "mu":
                for p in parts[1:]:
                    for slot in p:
                        assert R.same_bits(p[slot], parts[0][slot]) or np.array_equal(p[slot], parts[0][slot]), "mu.%s differs between ranks" % slot
                out[name] = parts[0]
            else:
                out[name] = {slot: np.concatenate([p[slot] for p in parts], axis=0) for slot in parts[0]}
        return out

    # -- one step ------------------------------------------------------------------------------
    def capacities(self, Bg, form):
        sh = self.sh[0]
        if form != "recs":
            return sh.capacities(Bg) + (None,)
        assert Bg % self.world == 0, "pre-split batches: the global batch divides by the world"
        b_loc = Bg // self.world
        pair_cap = sh.pair_capacity(b_loc)
        sample_cap, slot_cap = sh.capacities(b_loc * self.world)
        return min(sample_cap, self.world * pair_cap), slot_cap, pair_cap

    def step(self, u, i, r, form="route", split=False, presort=False, sample_cap_of=None, adam=None):
        """one global step on the batch (u, i, r).  ``form``: "route" (batch columns), "route_ids" (rows of a store every rank
        holds), "recs" (pre-split: rank k brings the k-th slice of the batch, bucket_ids then route_recs).  ``split``:
        forward_items + reduce_users for forward_reduce.  ``sample_cap_of``: {rank: sample capacity} in place of the computed
        one (the void-step case).  ``adam`` (True / False): also read the item-side shards right behind apply_items."""
        W, dev = self.world, self.device
        B = u.size
        sample_cap, slot_cap, pair_cap = self.capacities(B, form)
        caps = [(sample_cap_of or {}).get(k, sample_cap) for k in range(W)]
        rec = dict(sample_cap=caps, slot_cap=slot_cap, form=form)
        tu, ti, tr = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (u, i, r))
        keep = [tu, ti, tr]
        if form == "route":
            req = [self.be[k].route(tu, ti, tr, k, W, self.U, self.I, caps[k], slot_cap) for k in range(W)]
            src = None
        else:
            # a store the batch is rows of: scattered among other rows, so that a kernel reading the wrong row shows
            rs = np.random.RandomState(B)
            Ns = B + 37
            ids = rs.permutation(Ns)[:B].astype(np.int64)
            su, si = rs.randint(0, self.U, Ns).astype(np.int32), rs.randint(0, self.I, Ns).astype(np.int32)
            sr = rs.randint(1, 6, Ns).astype(np.float32)
            su[ids], si[ids], sr[ids] = u, i, r
            store = [torch.from_numpy(x).to(dev) for x in (su, si, sr)]
            keep += store
            self._store = store                           # the backends keep pointers into it
            for be in self.be:
                be.set_store(*store)
            if form == "route_ids":
                tids = torch.from_numpy(ids).to(dev)
                keep.append(tids)
                req = [self.be[k].route_ids(tids, k, W, self.U, self.I, caps[k], slot_cap) for k in range(W)]
                src = None
            else:
                b_loc = B // W
                send = []
                for k in range(W):
                    tids = torch.from_numpy(ids[k * b_loc:(k + 1) * b_loc].copy()).to(dev)
                    keep.append(tids)
                    send.append(self.be[k].bucket_ids(tids, W, self.U, pair_cap).clone())
                recv = exchange(send)
                keep += recv
                req = [self.be[k].route_recs(recv[k], k, W, self.U, self.I, caps[k], slot_cap) for k in range(W)]
                # position p of a rank's received buffer came from sender p // pair_cap, whose record names its own batch row
                src = [np.arange(W * pair_cap) // pair_cap * b_loc + _np(recv[k])[:, 3] for k in range(W)]
        req = [q.clone() for q in req]
        rec["req"] = [_np(q) for q in req]
        routed = [self.be[k].routed() for k in range(W)]
        rec["counts"] = [_np(p["counts"]) for p in routed]
        rec["slot"] = [_np(p["slot"]) for p in routed]
        rec["u_local"] = [_np(p["u_local"]) for p in routed]
        mine = [_np(p["mine"]) for p in routed]
        rec["mine"] = mine
        # the rank's samples as positions of the global batch, in routed order (what its logits are indexed by)
        rec["own"] = []
        for k in range(W):
            n = min(int(rec["counts"][k][0]), caps[k])
            rec["own"].append((mine[k][:n] if src is None else src[k][mine[k][:n]]).astype(np.int64))
        req_recv = exchange(req)
        rec["req_recv"] = [_np(q) for q in req_recv]
        if presort:
            for k in range(W):
                self.be[k].presort(req_recv[k])
        rows_out = [self.be[k].gather(req_recv[k]).clone() for k in range(W)]
        rec["rows_out"] = [_np(x) for x in rows_out]
        item_rows = exchange(rows_out)
        rec["item_rows"] = [_np(x) for x in item_rows]
        grad, scal, logits = [], [], []
        for k in range(W):
            if split:
                g, sc, lg = self.be[k].forward_items(item_rows[k])
                g, sc, lg = g.clone(), sc.clone(), lg.clone()
                self.be[k].reduce_users(item_rows[k])
            else:
                g, sc, lg = (x.clone() for x in self.be[k].forward_reduce(item_rows[k]))
            grad.append(g); scal.append(sc); logits.append(lg)
        rec["grad"] = [_np(x) for x in grad]
        rec["scal"] = [_np(x) for x in scal]
        rec["logits"] = [_np(x) for x in logits]
        grad_recv = exchange(grad)
        rec["grad_recv"] = [_np(x) for x in grad_recv]
        for k in range(W):
            self.be[k].apply_items(req_recv[k], grad_recv[k])
        if adam is not None:
            self.sync()
            rec["item_side"] = [{name: self.local(k, name, adam) for name in ITEM_SIDE} for k in range(W)]
        total = scal[0].clone()
        for k in range(1, W):                             # rank order
            total = total + scal[k]
        rec["scal_sum"] = _np(total)
        self._finish = (total, keep)
        return rec

    def finish(self):
        total, keep = self._finish
        for be in self.be:
            be.finish_step(total)
            if not self.hip:                              # the library keeps the beta powers in float32: so does the stand-in here
                be.o.b1p, be.o.b2p = (be.o.dt.type(np.float32(x)) for x in (be.o.b1p, be.o.b2p))
        if self.hip:
            torch.cuda.synchronize()
        del keep


# ----------------------------------------------------------------------------- the statements, stage by stage
def exact_f32(a, b):
    return R.same_bits(a, b)


def exact_any(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def slot_kinds(slot, n, G):
    """(whole, cut, most pieces): the request slots of a rank's n routed samples whose run in the order sorted by slot lies in one reduce
    block of 1024 / G entries (written straight to the exchange buffer by the reduce), and those a block boundary cuts (left
    to k_apply_rows in its emit form), and the largest number of pieces a slot is cut into - csrc/api.hip
    shard_forward_reduce_part, nblk"""
    epb = 1024 // G
    s = np.sort(np.asarray(slot[:n], np.int64), kind="stable")
    if s.size == 0:
        return 0, 0, 0
    heads = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))
    tails = np.concatenate((heads[1:], [s.size])) - 1
    pieces = tails // epb - heads // epb + 1
    return int((pieces == 1).sum()), int((pieces > 1).sum()), int(pieces.max())


def check_gather(rec, before, world, exact=exact_f32):
    """rows_out[j] = [Q[id] | bi[id] | flag = 0 | zero padding]; an unused slot is all zero"""
    bad = []
    D = before["Q"]["w"].shape[1]
    for k in range(world.world):
        ids = rec["req_recv"][k].astype(np.int64)
        rows = rec["rows_out"][k]
        want = np.zeros(rows.shape, rows.dtype)
        ok = ids >= 0
        gid = world.sh[k].i_lo + ids[ok]
        want[ok, :D] = before["Q"]["w"][gid]
        want[ok, D] = before["bi"]["w"][gid]
        if not exact(rows, want):
            bad.append("gather, rank %d: %d rows differ from the owner's Q row and bias (or carry a flag / non-zero padding)"
                       % (k, int((rows != want).any(axis=1).sum())))
    return bad


def _rank_inputs(rec, k, u, i, r):
    own = rec["own"][k]
    return u[own], i[own], r[own]


def slot_gids(rec, k, world):
    """global item id of every request slot of rank k (-1: unused)"""
    req = rec["req"][k].astype(np.int64)
    owner = np.arange(req.size) // rec["slot_cap"]
    return np.where(req >= 0, owner * world.per_i + req, -1)


def check_forward(rec, before, world, u, i, r, s, *, loss, item_abs, reg_bias, lam, report=None):
    """logits, local scalars and gradient rows of every rank against float64 over that rank's own samples"""
    bad = []
    tabs = {name: before[name]["w"] for name in R.NAMES}
    w = R.f64_tables(tabs)
    D = w["Q"].shape[1]
    tol = 2 * RTOL * (s + 1)                              # as tests/test_gpu_step_gradients.py holds logits, loss and reg
    for k in range(world.world):
        uk, ik, rk = _rank_inputs(rec, k, u, i, r)
        n = uk.size
        gid = slot_gids(rec, k, world)
        # the routing fed the compute stages what the batch says
        if not np.array_equal(gid[rec["slot"][k][:n]], ik) or not np.array_equal(rec["u_local"][k][:n] + world.sh[k].u_lo, uk):
            bad.append("rank %d: the routed samples do not name their own user rows / item slots" % k)
            continue
        ref, x, _ = R.step_grads(tabs, uk, ik, rk, loss, item_abs, reg_bias, lam)
        f32 = R.f32_oracle_grads(tabs, uk, ik, rk, loss, item_abs, reg_bias, lam)
        scal = rec["scal"][k]
        if n:
            e = rel_err(rec["logits"][k][:n], x)
            if not e <= tol:
                bad.append("rank %d logits: scale-relative error %.3e > %.1e" % (k, e, tol))
            want = (so.data_loss(x, rk.astype(np.float64), loss),
                    so.regularizer(w["P"], w["Q"], w["bu"], w["bi"], uk.astype(np.int64), ik.astype(np.int64), reg_bias))
            for what, got, wv in (("loss", scal[0], want[0]), ("reg", scal[1], want[1])):
                if not abs(got - wv) <= tol * abs(wv):
                    bad.append("rank %d local %s: %r against %r" % (k, what, float(got), float(wv)))
        elif scal[0] != 0 or scal[1] != 0 or scal[2] != 0:
            bad.append("rank %d has no samples and non-zero local scalars %r" % (k, scal[:3]))
        if scal[3] != 0:
            bad.append("rank %d: the fourth scalar word is %r, not zero" % (k, float(scal[3])))
        # sum g and the gradient rows: step_ref.ratio with E of the rank's samples, limit from the float32 oracle on the same
        rows = rec["grad"][k]
        used = gid >= 0
        dev = dict(Q=np.zeros(w["Q"].shape), bi=np.zeros(w["bi"].shape), mu=np.reshape(np.float64(scal[2]), (1,)))
        dev["Q"][gid[used]] = rows[used, :D]
        dev["bi"][gid[used]] = rows[used, D]
        if not np.array_equal(np.sort(gid[used]), np.unique(ik)):
            bad.append("rank %d: the slots in use are not the distinct items of its samples" % k)
        for name in ("Q", "bi", "mu"):
            G, E, cnt = ref[name]
            ref32 = f32[name]
            if name == "mu":
                G, E, cnt, ref32 = (np.reshape(a, (1,)) for a in (G, E, cnt, ref32))
            c_ref = R.ratio(ref32, G, E, cnt)
            lim = R.limit_from(c_ref)
            got = R.ratio(dev[name], G, E, cnt)
            if report is not None:
                report["rank%d %s rows" % (k, name)] = dict(c_ref=c_ref, dev=got)
            for cls in ("short", "long"):
                if not got[cls] <= lim[cls]:
                    bad.append("rank %d %s gradient rows, %s runs: %.1f x eps32 x E, limit %.1f (float32 oracle %.1f)"
                               % (k, name, cls, got[cls], lim[cls], c_ref[cls]))
        # what the reduce does not write must be zero on the wire: unused slots whole, and every word behind the bias
        if np.any(rows[~used] != 0):
            bad.append("rank %d: %d unused gradient slots are not zero" % (k, int((rows[~used] != 0).any(axis=1).sum())))
        if np.any(rows[:, D + 1:] != 0):
            bad.append("rank %d: non-zero words behind the bias gradient" % k)
    return bad


def check_apply_items(rec, before, world, *, opt, mode, lr, fresh, frozen, report=None):
    """the owner's summed gradient - recovered from its own m, or from w under SGD, as check_step does - against the float64
    sum of the rows it received, per item row; the float32 reference adds them in buffer (= rank) order"""
    bad = []
    adam, tf1 = opt == "adam", opt == "adam" and mode == "tf1"
    after = rec["item_side"]
    for k in range(world.world):
        sh = world.sh[k]
        rows_n = sh.i_hi - sh.i_lo
        if rows_n == 0:
            continue
        ids = rec["req_recv"][k].astype(np.int64)
        ok = ids >= 0
        recv = rec["grad_recv"][k]
        D = world.D
        for name, col in (("Q", slice(0, D)), ("bi", D)):
            if frozen >> R.TID[name] & 1:
                continue
            b = {slot: a[sh.i_lo:sh.i_hi] for slot, a in before[name].items()}
            a = after[k][name]
            vals = np.ascontiguousarray(recv[ok][:, col], np.float64)
            G = R.seg_sum(vals, ids[ok], rows_n)
            E = R.seg_sum(np.abs(vals), ids[ok], rows_n)
            cnt = np.bincount(ids[ok], minlength=rows_n)
            cnt = cnt[:, None] if name == "Q" else cnt
            f32 = np.zeros(G.shape, np.float32)
            np.add.at(f32, ids[ok], vals.astype(np.float32))
            if adam:
                g, extra = R.grad_from_fresh_adam(a["m"]) if fresh else R.grad_from_adam(a["m"], b["m"])
            else:
                g, extra = R.grad_from_sgd(b["w"], a["w"], lr)
            touched = np.broadcast_to(cnt > 0, G.shape)
            if not tf1:
                extra = np.where(touched, extra, 0.0)
            c_ref = R.ratio(f32, G, E, cnt)
            lim = R.limit_from(c_ref)
            got = R.ratio(g, G, E + extra, np.broadcast_to(cnt, G.shape))
            if report is not None:
                report["rank%d %s owner" % (k, name)] = dict(c_ref=c_ref, dev=got)
            for cls in ("short", "long"):
                if not got[cls] <= lim[cls]:
                    bad.append("rank %d %s: the owner's sum of the received rows, %s runs: %.1f x eps32 x E, limit %.1f"
                               % (k, name, cls, got[cls], lim[cls]))
    return bad


# ----------------------------------------------------------------------------- the data-parallel stages
# the read-back of g from m (or from w under SGD) against the buffer it was computed from, in units of eps32 x (the
# read-back's own first-order bound ``extra`` of step_ref.grad_from_* + |g|): limit_from's floor
READ_BACK_LIMIT = R.limit_from({"x": 0.0})["x"]


def dp_parts(flat, U, I, D):
    """the flat buffer [P | Q | bu | bi | loss, reg, sum g, 0] as views (csrc/api.hip tfr_dp_flat_size)"""
    a, b, c, d = U * D, U * D + I * D, U * D + I * D + U, U * D + I * D + U + I
    return dict(P=flat[:a].reshape(U, D), Q=flat[a:b].reshape(I, D), bu=flat[b:c], bi=flat[c:d], tail=flat[d:])


def check_dp_local_grads(got, tabs, u, i, r, s, *, loss, item_abs, reg_bias, lam, report=None, tag=""):
    """one replica's buffer after dp_local_grads on its half (u, i, r): every table's part against the float64 sum over that
    half, limit from the float32 oracle on the same half; rows the half does not touch exactly zero; the tail"""
    bad = []
    ref, x, _ = R.step_grads(tabs, u, i, r, loss, item_abs, reg_bias, lam)
    f32 = R.f32_oracle_grads(tabs, u, i, r, loss, item_abs, reg_bias, lam)
    for name in ("P", "Q", "bu", "bi", "mu"):
        G, E, n = ref[name]
        dev, ref32 = (got["tail"][2:3], f32[name]) if name == "mu" else (got[name], f32[name])
        if name == "mu":
            G, E, n, ref32 = (np.reshape(a, (1,)) for a in (G, E, n, ref32))
        c_ref = R.ratio(ref32, G, E, n)
        lim, dv = R.limit_from(c_ref), R.ratio(dev, G, E, n)
        if report is not None:
            report["%s%s" % (tag, name)] = dict(c_ref=c_ref, dev=dv)
        for cls in ("short", "long"):
            if not dv[cls] <= lim[cls]:
                bad.append("%s, %s runs: %.1f x eps32 x E, limit %.1f (float32 oracle %.1f)" % (name, cls, dv[cls], lim[cls], c_ref[cls]))
        if name != "mu" and np.any(dev[np.broadcast_to(np.asarray(n) == 0, np.shape(G))] != 0):
            bad.append("%s: rows outside this half's batch are not zero" % name)
    w = R.f64_tables(tabs)
    tol = 2 * RTOL * (s + 1)                              # as tests/test_gpu_step_gradients.py holds loss and reg
    want = (so.data_loss(x, r.astype(np.float64), loss),
            so.regularizer(w["P"], w["Q"], w["bu"], w["bi"], u.astype(np.int64), i.astype(np.int64), reg_bias))
    for what, gv, wv in (("loss", got["tail"][0], want[0]), ("reg", got["tail"][1], want[1])):
        if not abs(gv - wv) <= tol * abs(wv):
            bad.append("local %s: %r against %r" % (what, float(gv), float(wv)))
    if got["tail"][3] != 0:
        bad.append("the fourth scalar word is not zero")
    return bad


def check_dp_apply(before, after, gsum, *, opt, lr, powers, fresh):
    """one replica around dp_apply on the summed buffer ``gsum`` (dp_parts): the gradient it applied, read back from its own
    m (or w under SGD), is the buffer's; v and w follow by the moments and apply statements of tests/step_ref.py"""
    bad = []
    adam = opt == "adam"
    alpha = R.alpha_f32(lr, *powers) if adam else 0.0
    for name in R.NAMES:
        gs = np.reshape(gsum["tail"][2], (1,)) if name == "mu" else gsum[name]
        b, a = ({k: np.reshape(v, np.shape(gs)) for k, v in d[name].items()} for d in (before, after))
        if adam:
            g, extra = R.grad_from_fresh_adam(a["m"]) if fresh else R.grad_from_adam(a["m"], b["m"])
        else:
            g, extra = R.grad_from_sgd(b["w"], a["w"], lr)
        got = R.ratio(g, gs, extra + np.abs(gs), np.ones(np.shape(gs), np.int64))["short"]
        if not got <= READ_BACK_LIMIT:
            bad.append("%s: the gradient applied is not the summed buffer (%.1f x eps32 x the read-back's bound, limit %.1f)"
                       % (name, got, READ_BACK_LIMIT))
        if adam:
            ex = R.moments_excess(b["v"], a["v"], gs)
            if not ex <= 1:
                bad.append("%s: v does not follow from the summed buffer and the previous v (%.2f x its allowance)" % (name, ex))
            ex = R.apply_excess(b["w"], a["w"], a["m"], a["v"], alpha)
            if not ex <= 1:
                bad.append("%s: w does not follow from m and v (%.2f x its allowance)" % (name, ex))
    return bad


def assert_hot(case, recs):
    """a hot case reaches, on some rank, slots written whole by the reduce, slots a block boundary cuts, and a slot cut into
    three pieces or more (uniform ids cut short runs in two at most: a hot case that went uniform fails here)"""
    G = geometry(case["D"])[0]
    kinds = [slot_kinds(rec["slot"][k], rec["own"][k].size, G) for rec in recs for k in range(case["world"])]
    assert any(w > 0 and c > 0 and p >= 3 for w, c, p in kinds), "%s: (whole, cut, most pieces) per rank and step %r" % (case["id"], kinds)


def run_two_steps(world, case, cases, exact=exact_f32, report=None, split=False, presort=None, stage_checks=True):
    """two successive steps of a case on a fresh world, every stage statement after each; returns (records, final snapshot)"""
    adam = case["opt"] == "adam"
    flags = dict(loss=case["loss"], item_abs=case["item_abs"], reg_bias=case["reg_bias"])
    lr, reg = cases.hyper_of(case, 0)
    world.set_tables(cases.tables_of(case))
    if case["frozen"]:
        world.set_frozen(case["frozen"])
    before = world.snapshot(adam)
    recs = []
    for s in range(2):
        if s == 1 and case["hyper2"]:
            world.set_hyper(*case["hyper2"])
        lr, reg = cases.hyper_of(case, s)
        u, i, r = cases.batch_of(case, s)
        _, b1p, b2p = world.get_step(0)
        rec = world.step(u, i, r, form=case["form"], split=split, presort=case["presort"] if presort is None else presort, adam=adam)
        world.finish()
        after = world.snapshot(adam)
        recs.append(rec)
        if stage_checks:
            rep = {} if report is not None else None
            bad = check_gather(rec, before, world, exact)
            bad += check_forward(rec, before, world, u, i, r, s, lam=reg, report=rep, **flags)
            bad += check_apply_items(rec, before, world, opt=case["opt"], mode=case["mode"], lr=lr, fresh=s == 0,
                                     frozen=case["frozen"], report=rep)
            bad += R.check_step(before, after, u, i, r, opt=case["opt"], mode=case["mode"], lam=reg, lr=lr, powers=(b1p, b2p),
                                fresh=s == 0, frozen=case["frozen"], report=rep, **flags)
            for k in range(world.world):
                if world.get_step(k)[0] != s + 1:
                    bad.append("rank %d: step counter %d after step %d" % (k, world.get_step(k)[0], s))
            if report is not None:
                report["step%d" % s] = rep
            assert not bad, "%s, step %d:\n  %s" % (case["id"], s, "\n  ".join(bad))
        before = after
    if case["ids"] == "hot":
        assert_hot(case, recs)
    return recs, before


def print_report(case, report, seconds):
    """the measured ratios per case, table and run-length class, as tests/test_gpu_step_gradients.py prints them"""
    for step, rep in sorted(report.items()):
        for name, v in sorted(rep.items()):
            print("RATIO %s %s %s dev short %.2f long %.2f | c_ref short %.2f long %.2f" % (
                case["id"], step, name, v["dev"]["short"], v["dev"]["long"], v["c_ref"]["short"], v["c_ref"]["long"]))
    print("TIME %s %.1f s" % (case["id"], seconds))
