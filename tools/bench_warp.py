"""WARP step timings: one JSON line per shape and phase, the WARP drawn step and the BPR drawn step
alternating in one process at the same shape.

    python tools/bench_warp.py [--shapes ml1m,ml10m] [--steps 500] [--runs 5] [--train 2000] [--out profiles/bench_warp.jsonl]
    python tools/bench_warp.py --trace-only ...        # the timed calls alone, for rocprofv3 --kernel-trace --stats

At batch 10000, D 64, lazy Adam, on the two synthetic shapes of tools/bench_bpr.py.  What WARP adds to a BPR step is the
violator search, so the comparison is with BPR's drawn step in the same process: per phase, ``runs`` alternating pairs of
(WARP call of ``steps`` steps, BPR call of ``steps`` steps), each ending in the loss copy's synchronise, medians reported.
Two phases: ``fresh`` tables (a search ends after about two candidates) and ``trained``, after ``train`` WARP steps
(searches run long, some triples find no violator).  Each timed call starts from the same saved tables and optimiser
slots, so neither model's steps change what the other is timed on.  Per phase the mean trial count per live triple and the
skipped share come from searches alone on the phase's tables (not timed), and again on the tables a timed WARP window
leaves, since the window itself trains them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_bpr import SHAPES, pairs   # noqa: E402


def _save(m, L):
    return [(t | s, m.get_table(t | s)) for t in (L.BI, L.P, L.Q) for s in (0, L.SLOT_M, L.SLOT_V)], m.get_step()


def _restore(m, snap):
    for which, x in snap[0]:
        m.set_table(which, x)
    m.set_step(*snap[1])


def _search_stats(m, rs, batch, rowof, items, nnz):
    """(mean trials per live triple, skipped share) of three batches searched on the current tables (not timed)"""
    live = trials = 0
    for _ in range(3):
        e = rs.randint(0, nnz, batch)
        neg, n = m.warp_negatives(rowof[e], items[e])
        live += int((neg >= 0).sum())
        trials += int(n.sum())
    return trials / max(live, 1), 1.0 - live / (3.0 * batch)


def _phase(m, L, row, phase, batch, steps, runs, rowof, items, nnz, trace_only):
    snap = _save(m, L)
    rs = np.random.RandomState(5)
    if not trace_only:
        row["mean_trials_per_live_triple"], row["skipped_share"] = _search_stats(m, rs, batch, rowof, items, nnz)
    t = {"warp": [], "bpr": []}
    calls = {"warp": m.train_warp_steps_drawn, "bpr": m.train_bpr_steps_drawn}
    for r in range(-1, runs):                                              # run -1 warms both up
        for name in ("warp", "bpr"):
            _restore(m, snap)
            m.sync()
            t0 = time.perf_counter()
            calls[name](batch, steps, want_loss=True)                      # the loss copy synchronises
            if r >= 0:
                t[name].append((time.perf_counter() - t0) / steps * 1e6)
            if name == "warp" and r == runs - 1 and not trace_only:     # the window trains the tables: where its searches end
                row["mean_trials_at_window_end"], row["skipped_share_at_window_end"] = _search_stats(m, rs, batch, rowof, items, nnz)
    _restore(m, snap)
    for name in t:
        row["%s_drawn_step_us" % name] = statistics.median(t[name])
        row["%s_drawn_step_us_min_max" % name] = [min(t[name]), max(t[name])]
    row["warp_over_bpr"] = row["warp_drawn_step_us"] / row["bpr_drawn_step_us"]
    row["search_adds_us"] = row["warp_drawn_step_us"] - row["bpr_drawn_step_us"]
    return dict(row, phase=phase)


def run_shape(name, a):
    import tfrecomm_amd as T
    from tfrecomm_amd import _lib as L
    U, I, n = SHAPES[name]
    u, i = pairs(U, I, n)
    X = T.rated_matrix(u, i, U, I)
    nnz = int(X.nnz)
    rowof = np.repeat(np.arange(U, dtype=np.int32), np.diff(X.indptr))
    items = np.asarray(X.indices, np.int32)
    row = dict(shape=name, users=U, items=I, positives=nnz, dim=a.dim, batch=a.batch, steps=a.steps, runs=a.runs, margin=a.margin)
    out = []
    with T.SvdModel(U, I, a.dim, optimizer="adam", adam_mode="lazy", lr=5e-3, reg=0.005) as m:
        m.init_tables(seed=0, feature_stddev=0.1)
        m.set_table(L.BI, np.zeros(I, np.float32))
        m.set_positives(X)
        m.set_warp(a.margin)
        m.rng_seed(1)
        out.append(_phase(m, L, dict(row), "fresh", a.batch, a.steps, a.runs, rowof, items, nnz, a.trace_only))
        m.train_warp_steps_drawn(a.batch, a.train)
        m.sync()
        out.append(_phase(m, L, dict(row, trained_steps=a.train), "trained", a.batch, a.steps, a.runs, rowof, items, nnz, a.trace_only))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,ml10m")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--train", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--trace-only", action="store_true", help="skip the search statistics: the timed calls alone")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.runs < 5 and not a.trace_only:
        ap.error("medians of at least 5 runs")
    fh = open(a.out, "a") if a.out else None
    for name in a.shapes.split(","):
        for row in run_shape(name, a):
            line = json.dumps({k: ([round(x, 2) for x in v] if isinstance(v, list) else round(v, 4) if isinstance(v, float) else v)
                               for k, v in row.items()})
            print(line, flush=True)
            if fh:
                fh.write(line + "\n")
                fh.flush()
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
