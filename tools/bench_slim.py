"""SLIM timings (tfr_slim_gram, tfr_slim_solve): one JSON object per run, on bench_itemknn.py's ML-1M-shaped synthetic pairs
(6040 users x 3706 items, about 1 M distinct pairs, items drawn from a Zipf law, users uniform) - the pairs of bench_ease.py.

``gram_ms`` / ``solve_ms``: the two device times tfr_slim_solve reports (events around the Gram launches, and around the
zeroing of W and the solver launch), medians and minima of ``--reps`` (9) fits after 3 warm-up fits.  Beside them what the
solver did, means over the item columns: sweeps, coordinate updates (each reads one row of the Gram matrix) and non-zero
weights, and the share of columns that met the stopping rule.
``host_*``: the wall time of sklearn's ``ElasticNet(precompute=Gram, positive=True)`` under the header's mapping (alpha =
(l1 + l2) / U, l1_ratio = l1 / (l1 + l2), column j of X zeroed, the same ``tol`` and ``max_iter``) on ``--sample`` columns
spread evenly over the catalogue, one fit each, at most 16 threads; where sklearn does not import, of the NumPy restatement
(tests/slim_ref.py solve_column).  ``host_ms_extrapolated`` scales the sample's total to the catalogue: it is an
extrapolation, not a measurement of a whole host fit.  The two stopping rules differ (sklearn also asks for a duality gap),
so the sample's largest weight difference is recorded, not asserted.  These are records; no ratio is a gate.
python tools/bench_slim.py [--l1 X] [--l2 X] [--reps N] [--sample N] [--out profiles/bench_slim.jsonl]"""
import argparse
import json
import os
import sys
import time
import warnings

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tfrecomm_amd as T
from tools.bench_itemknn import synthetic, U, I


def host_columns(x, A, cols, l1, l2, max_iter, tol):
    """(name, per-column wall ms, per-column float64 weights) of the host baseline on the columns `cols`"""
    try:
        from sklearn.linear_model import ElasticNet
    except ImportError:
        from tests import slim_ref
        ms, ws = [], []
        for j in cols:
            t = time.perf_counter()
            w = slim_ref.solve_column(A, j, l1, True, max_iter, tol)[0]
            ms.append((time.perf_counter() - t) * 1e3)
            ws.append(w)
        return "numpy restatement", ms, ws
    X = np.asfortranarray(x.toarray().astype(np.float64))
    G = A - l2 * np.eye(A.shape[0])                        # sklearn adds its own L2 term to the Gram matrix it is given
    ms, ws = [], []
    for j in cols:
        y = X[:, j].copy()
        row = G[j].copy()
        X[:, j] = 0.0                                      # w[j] = 0: the column is not a feature of its own regression
        G[j, :] = 0.0
        G[:, j] = 0.0
        en = ElasticNet(alpha=(l1 + l2) / U, l1_ratio=l1 / (l1 + l2), positive=True, fit_intercept=False, precompute=G,
                        copy_X=False, max_iter=max_iter, tol=tol)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                # a column that runs out of sweeps is timed as it is
            t = time.perf_counter()
            en.fit(X, y)
            ms.append((time.perf_counter() - t) * 1e3)
        ws.append(en.coef_.copy())
        X[:, j] = y
        G[j, :] = row
        G[:, j] = row
    return "sklearn ElasticNet(precompute=Gram, positive=True)", ms, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--l1", type=float, default=1.0)
    ap.add_argument("--l2", type=float, default=5.0)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default="profiles/bench_slim.jsonl")
    a = ap.parse_args()
    torch.cuda.init()
    x = synthetic()
    with T.SLIM(U, I, l1=a.l1, l2=a.l2, max_iter=a.max_iter, tol=a.tol) as m:
        m.load(x)
        parts = {"gram": [], "solve": []}
        for r in range(3 + a.reps):
            m.fit()
            if r >= 3:
                for name in parts:
                    parts[name].append(m.fit_ms_parts[name])
        W, sweeps, updates, conv = m.weights(), m.sweeps(), m.updates(), m.converged()
        A = m.gram()
    cols = [int(c) for c in np.linspace(0, I - 1, a.sample).round()]
    host, ms, ws = host_columns(x, A, cols, a.l1, a.l2, a.max_iter, a.tol)
    diff = max(float(np.abs(w - W[:, j].astype(np.float64)).max()) for j, w in zip(cols, ws))
    plan = T.slim.plan(I)
    rec = dict(what="fit", users=U, items=I, pairs=int(x.nnz), l1=a.l1, l2=a.l2, positive=True, max_iter=a.max_iter, tol=a.tol,
               reps=a.reps, window=plan["window"], grid=plan["grid"], lds=plan["lds"], w_in_lds=plan["w_in_lds"],
               gram_ms_median=round(float(np.median(parts["gram"])), 3), gram_ms_min=round(float(np.min(parts["gram"])), 3),
               solve_ms_median=round(float(np.median(parts["solve"])), 3), solve_ms_min=round(float(np.min(parts["solve"])), 3),
               sweeps_mean=round(float(sweeps.mean()), 2), sweeps_max=int(sweeps.max()), updates_mean=round(float(updates.mean()), 1),
               nonzeros_mean=round(float((W != 0).sum(axis=0).mean()), 1), converged_share=round(float(conv.mean()), 4),
               updates_per_second=round(float(updates.sum()) / (float(np.median(parts["solve"])) * 1e-3), 0),
               host=host, host_sample_columns=cols, host_sample_ms_total=round(float(np.sum(ms)), 1),
               host_ms_extrapolated=round(float(np.sum(ms)) * I / len(cols), 0), host_note="extrapolated from the sample to %d columns" % I,
               host_extrapolated_over_device_solve=round(float(np.sum(ms)) * I / len(cols) / float(np.median(parts["solve"])), 1),
               host_sample_max_weight_difference=diff)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
