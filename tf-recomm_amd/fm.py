"""Second-order FM on the GPU: prediction (reference: forward.py:14-22), training, and the five-fold driver of fm.py.

``FmModel.fma(X)`` is the reference's ``fma(x)``: X is a scipy.sparse CSR design matrix
(fm.py:61-93), the result ``mu + X.W + 0.5 * (||X V||^2 - (X*X).(V*V).1)`` per row.

``run(...)`` is fm.py:113-181: users split five ways, one model per fold trained on rows that stay on the device
(``upload_rows`` / ``train_steps_resident``), ACC / AUC / NLL of the held-out users from ``eval_binary_resident``.
``python -m tfrecomm_amd.fm --dataset NAME --d D --users --items --iter N`` runs it on a prepared data set.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


class FmModel(object):
    def __init__(self, n_features, dim, device=0, loss="nll", optimizer="sgd", lr=0.01, reg=0.0):
        self._lib = L.load()
        self._h = L._p()
        self.n_features, self.dim = int(n_features), int(dim)
        self._row_lengths = {}                         # "train" / "eval" -> the uploaded store's row lengths (sizes the outputs)
        o = L.TfrOpts()
        self._lib.tfr_default_opts(C.byref(o))
        o.loss, o.optimizer, o.adam_mode = L.LOSS[loss], L.OPTIMIZER[optimizer], L.ADAM_MODE["lazy"]
        o.device, o.lr, o.reg = int(device), lr, reg
        self._check(self._lib.tfr_fm_create(C.byref(self._h), self.n_features, self.dim, C.byref(o)))

    def _check(self, rc):
        if rc != L.OK:
            text = self._lib.tfr_fm_last_error().decode("utf-8", "replace")
            raise (L.OutOfRangeError if rc == L.ERR_OOB else L.TfrError)(rc, text)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tfr_fm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set(self, mu, W, V):
        """the bundle fm_mangaki.py:39-45 pickles: {'mu', 'W', 'V'}"""
        W, V = L.as_f32(W).reshape(-1), L.as_f32(V)
        if W.size != self.n_features or V.shape != (self.n_features, self.dim):
            raise ValueError("W must be [%d], V [%d, %d]" % (self.n_features, self.n_features, self.dim))
        self._check(self._lib.tfr_fm_set(self._h, float(mu), L.ptr_f32(W), L.ptr_f32(V.reshape(-1))))

    def get(self):
        mu = np.empty(1, np.float32)
        W = np.empty(self.n_features, np.float32)
        V = np.empty(self.n_features * self.dim, np.float32)
        self._check(self._lib.tfr_fm_get(self._h, L.ptr_f32(mu), L.ptr_f32(W), L.ptr_f32(V)))
        return float(mu[0]), W, V.reshape(self.n_features, self.dim)

    def get_table(self, which):
        """one table or Adam slot: ``which`` = MU, BU (= W) or P (= V) of ``_lib``, optionally | SLOT_M / SLOT_V"""
        t = which & 7
        shape = {L.MU: (), L.BU: (self.n_features,), L.P: (self.n_features, self.dim)}.get(t, (0,))
        out = np.empty(int(np.prod(shape, dtype=np.int64)), np.float32)
        self._check(self._lib.tfr_fm_get_table(self._h, int(which), L.ptr_f32(out), out.size))
        return out.reshape(shape)

    def get_step(self):
        """(steps taken, beta1^t, beta2^t) as the next step will use them"""
        s, a, b = C.c_int64(), C.c_float(), C.c_float()
        self._check(self._lib.tfr_fm_get_step(self._h, C.byref(s), C.byref(a), C.byref(b)))
        return s.value, a.value, b.value

    def train_step(self, x, y):
        """One minibatch of SGD / lazy-Adam training on CSR rows ``x`` with targets ``y``.
        Returns (predictions before the update, data loss)."""
        x = x.tocsr()
        indptr = np.ascontiguousarray(x.indptr, np.int64)
        indices = np.ascontiguousarray(x.indices, np.int32)
        data = np.ascontiguousarray(x.data, np.float32)
        y = L.as_f32(y)
        n = indptr.size - 1
        if y.shape != (n,) or x.shape[1] != self.n_features:
            raise ValueError("x must be [n, %d] and y [n]" % self.n_features)
        pred, loss = np.empty(n, np.float32), C.c_float()
        self._check(self._lib.tfr_fm_train_step(self._h, L.ptr_i64(indptr), L.ptr_i32(indices), L.ptr_f32(data),
                                                L.ptr_f32(y), n, L.ptr_f32(pred), C.byref(loss)))
        return pred, loss.value

    def train_step_dev(self, d_indptr, d_indices, d_data, d_y, n_rows, nnz, d_pred=None):
        self._check(self._lib.tfr_fm_train_step_dev(self._h, d_indptr, d_indices, d_data, d_y, n_rows, nnz, d_pred))

    # ---- the trainer: rows resident on the device, minibatches gathered there
    _WHICH = {"train": 0, "eval": 1}

    def upload_rows(self, x, y, which="train"):
        """Copy the CSR design rows ``x`` and targets ``y`` to the device once, as the ``train`` or the ``eval`` store
        (a second upload replaces the first)."""
        x = x.tocsr()
        indptr = np.ascontiguousarray(x.indptr, np.int64)
        indices = np.ascontiguousarray(x.indices, np.int32)
        data = np.ascontiguousarray(x.data, np.float32)
        y = L.as_f32(y)
        n = indptr.size - 1
        if y.shape != (n,) or x.shape[1] != self.n_features:
            raise ValueError("x must be [n, %d] and y [n]" % self.n_features)
        self._check(self._lib.tfr_fm_upload_rows(self._h, self._WHICH[which], L.ptr_i64(indptr), L.ptr_i32(indices),
                                                 L.ptr_f32(data), L.ptr_f32(y), n))
        self._row_lengths[which] = np.diff(indptr)

    def gather_rows(self, ids, which="train"):
        """The minibatch the device builds for store rows ``ids``: scipy's ``(X[ids], y[ids])``."""
        import scipy.sparse as sp
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        lengths = self._row_lengths.get(which)
        # (a bad id or a missing store is the library's to refuse: size the outputs for the ids that are in range)
        ok = ids[(ids >= 0) & (ids < (0 if lengths is None else lengths.size))]
        cap = int(lengths[ok].sum()) if ok.size else 0
        indptr, yb = np.empty(ids.size + 1, np.int64), np.empty(ids.size, np.float32)
        indices, data = np.empty(cap, np.int32), np.empty(cap, np.float32)
        self._check(self._lib.tfr_fm_gather_rows(self._h, self._WHICH[which], L.ptr_i64(ids), ids.size, L.ptr_i64(indptr),
                                                 L.ptr_i32(indices), L.ptr_f32(data), L.ptr_f32(yb), cap))
        return sp.csr_matrix((data, indices, indptr), shape=(ids.size, self.n_features)), yb

    def train_steps_resident(self, ids, batch, want_loss=True):
        """``len(ids) // batch`` training steps, step ``s`` on train-store rows ``ids[s*batch:(s+1)*batch]``: the same
        bits as ``train_step(X[ids_s], y[ids_s])`` per step.  Returns the per-step data losses, or (``want_loss=False``)
        None with the steps queued."""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        batch = int(batch)
        if batch < 1 or ids.size % batch:
            raise ValueError("ids must hold a whole number of batches of %d" % batch)
        nsteps = ids.size // batch
        loss = np.empty(nsteps, np.float32) if want_loss else None
        self._check(self._lib.tfr_fm_train_steps_resident(self._h, L.ptr_i64(ids), batch, nsteps,
                                                          L.ptr_f32(loss) if want_loss else None))
        return loss

    def predict_resident(self, which="eval"):
        return self._predict_resident(self._lib.tfr_fm_predict_resident, which)

    def predict_resident_bf16(self, which="eval"):
        """``predict_resident`` from the bf16 snapshot (``snapshot_bf16``)."""
        return self._predict_resident(self._lib.tfr_fm_bf16_predict_resident, which)

    def _predict_resident(self, entry, which):
        n = self._row_lengths.get(which)
        out = np.empty(0 if n is None else n.size, np.float32)
        self._check(entry(self._h, self._WHICH[which], L.ptr_f32(out)))
        return out

    def eval_binary_resident(self):
        """Accuracy, mean sigmoid cross-entropy and AUC of the eval store (fm.py:162-166), computed on the device."""
        return self._eval_binary_resident(self._lib.tfr_fm_eval_binary_resident)

    def eval_binary_resident_bf16(self):
        """``eval_binary_resident`` of the predictions ``predict_resident_bf16`` makes."""
        return self._eval_binary_resident(self._lib.tfr_fm_bf16_eval_binary_resident)

    def _eval_binary_resident(self, entry):
        neq, n, nll, auc = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        self._check(entry(self._h, C.byref(neq), C.byref(nll), C.byref(auc), C.byref(n)))
        return {"acc": neq.value / n.value, "mean_nll": nll.value / n.value, "auc": auc.value, "n": n.value}

    # ---- the bf16 snapshot: forward, resident predict / eval and top-K at half the row bytes (bf16.py)
    def snapshot_bf16(self):
        """Build or refresh the bf16 copy of ``V`` (with ``W`` and ``mu`` of the same moment) the ``*_bf16`` calls score
        from; training, ``set`` and ``init`` do not move it."""
        self._check(self._lib.tfr_fm_bf16_snapshot(self._h))

    def drop_bf16(self):
        self._check(self._lib.tfr_fm_bf16_drop(self._h))

    def bf16_rows(self):
        """The snapshot's ``V`` as the library stores it: uint16 [n_features, DP] (``bf16.pack_rows(V)``)."""
        from . import bf16
        out = np.empty((self.n_features, bf16.row_stride(self.dim)), np.uint16)
        self._check(self._lib.tfr_fm_bf16_get_rows(self._h, out.ctypes.data_as(C.POINTER(C.c_uint16)), out.size))
        return out

    def init(self, seed=0, stddev=0.1):
        self._check(self._lib.tfr_fm_init(self._h, int(seed), stddev))

    def forward_csr(self, indptr, indices, data):
        return self._forward_csr(self._lib.tfr_fm_forward, indptr, indices, data)

    def forward_csr_bf16(self, indptr, indices, data):
        """``forward_csr`` from the bf16 snapshot (``snapshot_bf16``): the same formula on ``V`` as the snapshot holds it,
        with the snapshot's ``W`` and ``mu`` (include/tfrecomm.h tfr_fm_bf16_forward)."""
        return self._forward_csr(self._lib.tfr_fm_bf16_forward, indptr, indices, data)

    def _forward_csr(self, entry, indptr, indices, data):
        indptr = np.ascontiguousarray(indptr, np.int64)
        indices = np.ascontiguousarray(indices, np.int32)
        data = np.ascontiguousarray(data, np.float32)
        n = indptr.size - 1
        out = np.empty(n, np.float32)
        self._check(entry(self._h, L.ptr_i64(indptr), L.ptr_i32(indices), L.ptr_f32(data), n, L.ptr_f32(out)))
        return out

    def fma(self, x):
        """forward.py:21-22 on a scipy.sparse matrix (any format; converted to CSR)."""
        return self.forward_csr(*self._csr_arrays(x))

    def fma_bf16(self, x):
        """``fma`` from the bf16 snapshot."""
        return self.forward_csr_bf16(*self._csr_arrays(x))

    def _csr_arrays(self, x):
        x = x.tocsr()
        if x.shape[1] != self.n_features:
            raise ValueError("X has %d columns, the model %d features" % (x.shape[1], self.n_features))
        return x.indptr, x.indices, x.data

    def topk(self, user_features, item_lo, item_hi, k=50, exclude=None, return_scores=True):
        """The ``k`` best item features ``j`` in ``[item_lo, item_hi)`` for each user feature ``u``: forward.py:21-22 on the
        two-hot row ``e_u + e_j``, computed as ``((V[u].V[j] + mu) + W[u]) + W[j]``.  Item ids (returned and in ``exclude``)
        are relative to ``item_lo``; ``exclude`` as in ``SvdModel.recommend`` (a sparse matrix is indexed by user feature)."""
        return self._topk(self._lib.tfr_fm_topk, user_features, item_lo, item_hi, k, exclude, return_scores)

    def topk_bf16(self, user_features, item_lo, item_hi, k=50, exclude=None, return_scores=True):
        """``topk`` from the bf16 snapshot (``snapshot_bf16``): the same arguments and return values, the scores of the
        snapshot's tables with the dot taken 16 features per bf16 matrix instruction (include/tfrecomm.h tfr_fm_bf16_topk)."""
        return self._topk(self._lib.tfr_fm_bf16_topk, user_features, item_lo, item_hi, k, exclude, return_scores)

    def _topk(self, entry, user_features, item_lo, item_hi, k, exclude, return_scores):
        from .engine import exclusion_csr
        u = L.as_i32(user_features, "user features").reshape(-1)
        indptr, excl = exclusion_csr(exclude, u)
        items = np.empty((u.size, int(k)), np.int32)
        scores = np.empty((u.size, int(k)), np.float32) if return_scores else None
        self._check(entry(self._h, L.ptr_i32(u), u.size, int(item_lo), int(item_hi), int(k),
                          None if indptr is None else L.ptr_i64(indptr), None if excl is None else L.ptr_i32(excl),
                          L.ptr_i32(items), None if scores is None else L.ptr_f32(scores)))
        return (items, scores) if return_scores else items

    def similar_features(self, features, lo=0, hi=None, k=10, metric="cosine", exclude=None, return_scores=True):
        """The ``k`` features in ``[lo, hi)`` most like each of ``features`` over the rows of ``V``, best first, equal scores
        by feature id, a feature never its own neighbour (``SvdModel.similar_items``).  The range picks a block of the design
        matrix: with the reference's layout (user ``u`` at feature ``u``, item ``i`` at ``user_num + i``),
        ``similar_features([user_num + i], user_num, user_num + item_num)`` asks for the items like item ``i``.  Ids
        (returned and in ``exclude``) are feature ids, whatever the range."""
        from . import neighbours as nb

        def call(*args):
            self._check(self._lib.tfr_fm_neighbours(self._h, *args))
        return nb.query_host(call, features, self.n_features, k, metric, exclude, lo, hi, return_scores, "feature ids")

    def rank_items(self, user_features, item_lo, item_hi, targets, exclude=None):
        """``SvdModel.rank_items`` for the ``topk`` scores: item features ``[item_lo, item_hi)``, ids (in ``targets`` and
        ``exclude``) relative to ``item_lo``; a sparse ``targets`` / ``exclude`` is indexed by user feature."""
        from .engine import rank_call
        u = L.as_i32(user_features, "user features").reshape(-1)

        def call(ip, it, xp, xi, out):
            self._check(self._lib.tfr_fm_rank_items(self._h, L.ptr_i32(u), u.size, int(item_lo), int(item_hi), ip, it, xp,
                                                    xi, out))
        return rank_call(call, u, targets, exclude)

    def get_ranking(self, encoded_user_id, user_num, item_num, k=50, exclude=None):
        """forward.py:47-61 ``get_ranking``: the reference's design rows put user ``u`` at feature ``u`` and item ``i`` at
        feature ``user_num + i``; returns (items [k] best first, their scores)."""
        items, scores = self.topk([int(encoded_user_id)], int(user_num), int(user_num) + int(item_num), k, exclude)
        return items[0], scores[0]

    def get_ranking_bf16(self, encoded_user_id, user_num, item_num, k=50, exclude=None):
        """``get_ranking`` from the bf16 snapshot (``topk_bf16``)."""
        items, scores = self.topk_bf16([int(encoded_user_id)], int(user_num), int(user_num) + int(item_num), k, exclude)
        return items[0], scores[0]

    def forward_dev(self, d_indptr, d_indices, d_data, n_rows, d_out):
        self._check(self._lib.tfr_fm_forward_dev(self._h, d_indptr, d_indices, d_data, n_rows, d_out))

    def forward_bf16_dev(self, d_indptr, d_indices, d_data, n_rows, d_out):
        self._check(self._lib.tfr_fm_bf16_forward_dev(self._h, d_indptr, d_indices, d_data, n_rows, d_out))

    def sync(self):
        ms = C.c_float()
        self._check(self._lib.tfr_fm_sync(self._h, C.byref(ms)))
        return ms.value


AGENTS = ["users", "items", "skills", "attempts", "wins", "fails", "item_wins", "item_fails"]   # dataio.py:67 order


def df_to_sparse(df, user_num, item_num, active_agents, qmatrix=None, skill_wins=None, skill_fails=None):
    """The FM design matrix of fm.py:61-93 as one CSR ``[n_events, sum of block widths]``:

    ``users`` / ``items`` one-hot blocks (fm.py:74-75); ``skills`` = the q-matrix rows of the events'
    items (fm.py:76; identity q-matrix when none is given, fm.py:44-47); ``item_wins`` /
    ``item_fails`` = the item one-hot pattern carrying the event's win / fail counts
    (fm.py:78-81); ``attempts`` / ``wins`` / ``fails`` = per-skill counters supplied as matrices
    (fm.py:83-89).  Blocks are concatenated in the order of ``AGENTS`` restricted to
    ``active_agents`` (dataio.py:63-72, fm.py:91).  Host code (scipy), like the reference."""
    import scipy.sparse as sp
    n = len(df["user"])
    rows = np.arange(n)
    user = np.asarray(df["user"], np.int64)
    item = np.asarray(df["item"], np.int64)
    ones = np.ones(n, np.float32)
    blocks = {"users": sp.coo_matrix((ones, (rows, user)), shape=(n, user_num)),
              "items": sp.coo_matrix((ones, (rows, item)), shape=(n, item_num))}
    q = qmatrix if qmatrix is not None else sp.identity(item_num, dtype=np.float32, format="csr")
    blocks["skills"] = q.tocsr()[item]
    if "wins" in df:
        blocks["item_wins"] = sp.coo_matrix((np.asarray(df["wins"], np.float32), (rows, item)), shape=(n, item_num))
        blocks["item_fails"] = sp.coo_matrix((np.asarray(df["fails"], np.float32), (rows, item)), shape=(n, item_num))
    if skill_wins is not None:
        blocks["attempts"] = skill_wins + skill_fails
        blocks["wins"] = skill_wins
        blocks["fails"] = skill_fails
    chosen = [a for a in AGENTS if a in active_agents]
    missing = [a for a in chosen if a not in blocks]
    if missing:
        raise ValueError("no data for blocks %s" % missing)
    x = sp.hstack([blocks[a] for a in chosen]).tocsr().astype(np.float32)
    x.data = np.nan_to_num(x.data)                     # fm.py:126,130
    return x


def kfold_by_user(users, n_splits=5, seed=0):
    """fm.py:114-119's split of the users: the unique users in order of first appearance, shuffled by
    ``np.random.RandomState(seed).permutation`` and cut by ``np.array_split``; fold ``k`` tests on part ``k`` and trains on
    the rest.  Returns ``[(users_train, users_test)] * n_splits``; every user is in exactly one test part."""
    users = np.asarray(users)
    uniq, first = np.unique(users, return_index=True)
    uniq = uniq[np.argsort(first, kind="stable")]
    if n_splits < 2 or n_splits > uniq.size:
        raise ValueError("n_splits must lie in [2, %d users]" % uniq.size)
    parts = np.array_split(uniq[np.random.RandomState(seed).permutation(uniq.size)], n_splits)
    return [(np.concatenate(parts[:k] + parts[k + 1:]), parts[k]) for k in range(n_splits)]


def plan_steps(row_lengths, ids, batch):
    """The non-zeros of each step of ``train_steps_resident(ids, batch)``: the sum of the step's rows' lengths - what the
    library computes on the host to size each step's launches.  Raises IndexError on an id outside the store."""
    row_lengths = np.asarray(row_lengths, np.int64)
    ids = np.asarray(ids, np.int64).reshape(-1)
    if batch < 1 or ids.size % batch:
        raise ValueError("ids must hold a whole number of batches of %d" % batch)
    if ids.size and (ids.min() < 0 or ids.max() >= row_lengths.size):
        raise IndexError("row id out of range [0, %d)" % row_lengths.size)
    return row_lengths[ids].reshape(-1, batch).sum(axis=1)


def run(df, user_num, item_num, active_agents, d, num_iter, batch, lr, reg, optimizer, seed, out_dir=None, qmatrix=None,
        skill_wins=None, skill_fails=None, experiment_args=None, device=0, log=None):
    """fm.py:113-181 on the device.  For each of five folds of the users: the rows of the train users and of the test users
    are uploaded, a ``d``-dimensional model is initialised (``init(seed + fold)``) and trained for ``num_iter`` epochs of
    ``len(train) // batch`` minibatches drawn with replacement (``np.random.RandomState(seed + fold).randint``, one
    ``train_steps_resident`` call per epoch), then evaluated on the test rows.  (The epoch is this project's, as its SGD /
    lazy-Adam step is: the reference trains by MCMC inside libFM.)  With ``out_dir``, ``<out_dir>/<fold>/results.json``
    gets the reference's keys.  Returns one dict per fold: ``metrics`` {ACC, AUC, NLL}, ``pred`` (the final model's
    predictions of the test rows), ``y`` (their outcomes), ``test_rows`` and ``loss`` (per step)."""
    import json
    import os
    from . import dataio
    if d < 1:
        raise ValueError("d = %d: the reference fits sklearn's LogisticRegression there (fm.py:139-152); this driver "
                         "trains the factorization machine only, d >= 1" % d)
    x = df_to_sparse(df, user_num, item_num, active_agents, qmatrix, skill_wins, skill_fails)
    y = np.asarray(df["outcome"], np.float32)
    users = np.asarray(df["user"])
    args = dict(experiment_args) if experiment_args is not None else dict(
        {a: a in active_agents for a in AGENTS}, d=d, iter=num_iter, batch=batch, lr=lr, reg=reg, optimizer=optimizer,
        seed=seed)
    short, full, latex, _ = dataio.get_legend(dict({a: a in active_agents for a in AGENTS}, d=d))
    folds = []
    for fold, (_, users_test) in enumerate(kfold_by_user(users, 5, seed)):
        test = np.isin(users, users_test)
        i_train, i_test = np.flatnonzero(~test), np.flatnonzero(test)
        steps = i_train.size // batch
        if steps < 1:
            raise ValueError("fold %d trains on %d rows: fewer than one batch of %d" % (fold, i_train.size, batch))
        with FmModel(x.shape[1], d, device=device, loss="nll", optimizer=optimizer, lr=lr, reg=reg) as model:
            model.upload_rows(x[i_train], y[i_train], "train")
            model.upload_rows(x[i_test], y[i_test], "eval")
            model.init(seed + fold)
            rs = np.random.RandomState(seed + fold)
            losses = []
            for _ in range(num_iter):
                losses.append(model.train_steps_resident(rs.randint(0, i_train.size, (steps * batch,)), batch))
            ev = model.eval_binary_resident()
            pred = model.predict_resident("eval")
        metrics = {"ACC": ev["acc"], "AUC": ev["auc"], "NLL": ev["mean_nll"]}
        if log:
            log("fold %d: %d train rows, %d test rows, ACC %.4f AUC %.4f NLL %.4f"
                % (fold, i_train.size, i_test.size, metrics["ACC"], metrics["AUC"], metrics["NLL"]))
        if out_dir is not None:
            dataio.prepare_folder(os.path.join(out_dir, str(fold)))
            with open(os.path.join(out_dir, str(fold), "results.json"), "w") as f:
                f.write(json.dumps({"args": args, "legends": {"short": short, "full": full, "latex": latex},
                                    "metrics": metrics}, indent=4))
        folds.append({"metrics": metrics, "pred": pred, "y": y[i_test], "test_rows": i_test,
                      "loss": np.concatenate(losses) if losses else np.empty(0, np.float32)})
    return folds


def main(argv=None):
    import argparse
    import os
    from . import dataio
    ap = argparse.ArgumentParser(description="Knowledge Tracing Machines: five-fold FM training on the GPU (fm.py)")
    ap.add_argument("--dataset", type=str, default="dummy")
    ap.add_argument("--data_folder", type=str, default="data")
    ap.add_argument("--d", type=int, required=True)
    for a in AGENTS:
        ap.add_argument("--" + a, action="store_true")
    ap.add_argument("--iter", type=int, default=500)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--reg", type=float, default=0.0)
    ap.add_argument("--optimizer", choices=sorted(L.OPTIMIZER), default="adam")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    o = ap.parse_args(argv)
    if o.d == 0:
        raise ValueError("--d 0 is the reference's logistic-regression baseline (fm.py:139-152), which this driver does not "
                         "have: give --d >= 1")
    import scipy.sparse as sp
    folder, _, config_file, q_npz, sw_npz, sf_npz = dataio.build_new_paths(o.dataset, o.data_folder)
    config = dataio.get_config(config_file)
    df = dataio.get_new_data(o.dataset, o.data_folder)
    qmatrix = sp.load_npz(q_npz) if os.path.isfile(q_npz) else None
    both = os.path.isfile(sw_npz) and os.path.isfile(sf_npz)
    skill_wins, skill_fails = (sp.load_npz(sw_npz), sp.load_npz(sf_npz)) if both else (None, None)
    args = vars(o)
    short, _, _, active = dataio.get_legend(args)
    run(df, config["USER_NUM"], config["ITEM_NUM"], active, o.d, o.iter, o.batch, o.lr, o.reg, o.optimizer, o.seed,
        out_dir=os.path.join(folder, short), qmatrix=qmatrix, skill_wins=skill_wins, skill_fails=skill_fails,
        experiment_args=args, device=o.device, log=print)


if __name__ == "__main__":
    main()
