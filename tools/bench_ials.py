"""Implicit ALS iteration timings: one JSON line per width, every leg on the same pairs in the same process.

    python tools/bench_ials.py [--dims 32,64] [--iters 10] [--out profiles/bench_ials.jsonl]
    python tools/bench_ials.py --solver cg --cg-steps 3 --dims 32,64,128,256 --also-cholesky 32,64 --cap 1024,256 \
        --out profiles/bench_ials_cg.jsonl                                      
    python tools/bench_ials.py --fold-in --out profiles/bench_ials_fold.jsonl   

Data: ML-1M-shaped synthetic pairs (6040 x 3706, 1 M draws, item popularity p(i) ~ 1 / (i + 50), as tools/bench_bpr.py),
values 1 .. 5.  Legs: ImplicitALS.sweep (device time per iteration from the library's events) and each half on its own
(tfr_ials_half); MangakiALS3's iteration on the same pairs as ratings, at d = 32 only (its limit); and the NumPy float64
restatement of one iteration on one core (the CPU baseline; a few hundred users and items timed, scaled to the whole).
With --solver cg the rows are the conjugate-gradient path's (dims up to 256; no MangakiALS3 and no NumPy leg): the iteration,
each half, and the loss after 15 iterations from the library's initialisation.  --also-cholesky adds the Cholesky path's rows
at those dims in the same process; --cap N[,M] adds a further row per width and length on the same pairs with every item's list cut to its
first N users (popularity capped), which takes the longest lists (one block each) out of the halves.
With --fold-in the rows are fold-in's, at d = 64 (Cholesky) and d = 128 (conjugate gradient), one per n in 1, 256, 6040: the
rows of the first n users' lists by fold_in_users against a second ImplicitALS(n, ...) with set_factors, load and a
half-sweep, and their top-10 by recommend_lists against a second SvdModel set through the host; medians of --reps repeats,
the ways alternating in one process.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"                                   # the NumPy leg is the one-core baseline

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = (6040, 3706, 1000209)


def pairs(U, I, n, seed=0):
    rs = np.random.RandomState(seed)
    w = 1.0 / (np.arange(I) + 50.0)
    u = rs.randint(0, U, n).astype(np.int32)
    i = rs.choice(I, n, p=w / w.sum()).astype(np.int32)
    return u, i, rs.randint(1, 6, n).astype(np.float64)


def numpy_half_seconds(other, x, lam, alpha, sample, rs):
    """one half-sweep in NumPy float64 (G + corrections, LAPACK's Cholesky solve per row): `sample` rows timed, scaled to all"""
    n = x.shape[0]
    rows = rs.choice(n, min(sample, n), replace=False)
    t0 = time.perf_counter()
    G = other.T @ other + lam * np.eye(other.shape[1])
    tg = time.perf_counter() - t0
    t0 = time.perf_counter()
    for r in rows:
        j, v = x.indices[x.indptr[r]:x.indptr[r + 1]], x.data[x.indptr[r]:x.indptr[r + 1]]
        Y = other[j]
        w = alpha * v
        A = G + (Y * w[:, None]).T @ Y
        b = (1.0 + w) @ Y
        np.linalg.solve(A, b)
    return tg + (time.perf_counter() - t0) * n / rows.size


def capped(x, cap):
    """the CSR with every item's list (column) cut to its first `cap` users: popularity capped, the users' lists barely change"""
    t = x.T.tocsr()
    t.sort_indices()
    keep = np.arange(t.nnz) - np.repeat(t.indptr[:-1], np.diff(t.indptr)) < cap
    t.data[~keep] = 0.0
    t.eliminate_zeros()
    x = t.T.tocsr()
    x.sort_indices()
    return x


def run_solver(d, iters, solver, cg_steps, cap=0):
    """one row of the --solver cg form: either solver, device times only"""
    import scipy.sparse as sp
    import tfrecomm_amd as T
    U, I, n = SHAPE
    u, i, v = pairs(U, I, n)
    x = sp.csr_matrix((v, (u, i)), shape=(U, I))
    x.sum_duplicates()
    x.sort_indices()
    if cap:
        x = capped(x, cap)
    xt = x.T.tocsr()
    row = dict(users=U, items=I, pairs=int(x.nnz), d=d, iters=iters, lam=0.01, alpha=40.0, solver=solver, cap=cap,
               longest_user_list=int(np.diff(x.indptr).max()), longest_item_list=int(np.diff(xt.indptr).max()))
    kw = dict(solver="cg", cg_steps=cg_steps) if solver == "cg" else {}
    if solver == "cg":
        row["cg_steps"] = cg_steps
    with T.ImplicitALS(U, I, factors=d, regularization=0.01, alpha=40.0, **kw) as m:
        m.load(x)
        m.init_factors(0)
        m.sweep(2)                                          # warm-up: code objects, buffers
        row["ials_iter_ms"] = m.sweep(iters) / iters
        h = [0.0, 0.0]
        for _ in range(iters):
            h[0] += m.half_sweep(0)
            h[1] += m.half_sweep(1)
        row["ials_user_half_ms"], row["ials_item_half_ms"] = h[0] / iters, h[1] / iters
        m.init_factors(0)
        m.sweep(15)
        row["ials_loss_after_15"] = m.loss()
    return row


def run_dim(d, iters, sample):
    import scipy.sparse as sp
    import tfrecomm_amd as T
    from tfrecomm_amd import _lib as L
    U, I, n = SHAPE
    u, i, v = pairs(U, I, n)
    x = sp.csr_matrix((v, (u, i)), shape=(U, I))
    x.sum_duplicates()
    x.sort_indices()
    row = dict(users=U, items=I, pairs=int(x.nnz), d=d, iters=iters, lam=0.01, alpha=40.0, chunk=512)
    with T.ImplicitALS(U, I, factors=d, regularization=0.01, alpha=40.0) as m:
        m.load(x)
        m.init_factors(0)
        m.sweep(2)                                          # warm-up: code objects, buffers
        row["ials_iter_ms"] = m.sweep(iters) / iters
        h = [0.0, 0.0]
        for _ in range(iters):
            h[0] += m.half_sweep(0)
            h[1] += m.half_sweep(1)
        row["ials_user_half_ms"], row["ials_item_half_ms"] = h[0] / iters, h[1] / iters
        t0 = time.perf_counter()
        m.sweep(iters)
        row["ials_iter_wall_ms"] = (time.perf_counter() - t0) / iters * 1e3
        row["ials_loss"] = m.loss()
        X, Y = m.user_factors, m.item_factors
    if d <= 32:
        als = T.MangakiALS3(nb_components=d, nb_iterations=1, lambda_=0.1, verbose=False)
        als.nb_users, als.nb_works = U, I
        np.random.seed(0)
        als.init_vars()
        rowof = np.repeat(np.arange(U, dtype=np.int64), np.diff(x.indptr))
        uu, ww, yy = np.ascontiguousarray(rowof), np.ascontiguousarray(x.indices, np.int64), np.ascontiguousarray(x.data)
        als._check(als._lib.tfr_als_load(als._h, L.ptr_i64(uu), L.ptr_i64(ww), als._p64(yy), yy.size))
        ms = C.c_float()
        als._check(als._lib.tfr_als_sweep(als._h, 2, C.byref(ms)))
        als._check(als._lib.tfr_als_sweep(als._h, iters, C.byref(ms)))
        row["als3_iter_ms"] = ms.value / iters
        row["ials_over_als3"] = row["ials_iter_ms"] / row["als3_iter_ms"]
        als.close()
    rs = np.random.RandomState(1)
    xt = x.T.tocsr()
    xt.sort_indices()
    sec = numpy_half_seconds(Y, x, 0.01, 40.0, sample, rs) + numpy_half_seconds(X, xt, 0.01, 40.0, sample, rs)
    row["numpy_f64_iter_ms"] = sec * 1e3
    row["numpy_threads"] = 1
    row["numpy_rows_timed"] = sample
    row["numpy_over_ials"] = row["numpy_f64_iter_ms"] / row["ials_iter_ms"]
    return row


def _wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def run_fold_in(d, solver, cg_steps, reps, guests=256):
    """one row per n: the rows of the first n users' stored lists by fold_in_users (first call after the item factors were
    set, which pays the Gram, and later calls) against a second ImplicitALS(n, ...) with set_factors, load and a half-sweep;
    and their top-10 by recommend_lists against a second SvdModel set through the host.  Wall-clock medians, the two ways
    alternating in one process; the device times are the library's events."""
    import scipy.sparse as sp
    import tfrecomm_amd as T
    U, I, npairs = SHAPE
    u, i, v = pairs(U, I, npairs)
    x = sp.csr_matrix((v, (u, i)), shape=(U, I))
    x.sum_duplicates()
    x.sort_indices()
    kw = dict(solver="cg", cg_steps=cg_steps) if solver == "cg" else {}
    rows = []
    with T.ImplicitALS(U, I, factors=d, regularization=0.01, alpha=40.0, **kw) as m:
        m.load(x)
        m.init_factors(0)
        m.sweep(3)
        Y = m.item_factors
        half_ms = float(np.median([m.half_sweep(0) for _ in range(reps)]))
        m.gram(1)
        with m.to_svd_model(extra_users=guests) as svd:
            for n in (1, 256, U):
                lists = x[:n]
                row = dict(users=U, items=I, pairs=int(x.nnz), d=d, solver=solver, n=n, reps=reps, guests=guests,
                           user_half_device_ms=half_ms)
                if solver == "cg":
                    row["cg_steps"] = cg_steps

                def first():
                    m.set_factors(Y=Y)                     # the Gram in the handle is no longer the item table's
                    t0 = time.perf_counter()
                    m.fold_in_users(lists)
                    return (time.perf_counter() - t0) * 1e3, m.fold_ms

                def second_model():
                    with T.ImplicitALS(n, I, factors=d, regularization=0.01, alpha=40.0, **kw) as m2:
                        m2.set_factors(Y=Y)
                        m2.load(lists)
                        m2.half_sweep(0)
                        return m2.user_factors

                def second_svd():
                    got = m.fold_in_users(lists)
                    with T.SvdModel(n, I, d, device=m.device) as s2:
                        s2.set_tables(np.float32(0.0), np.zeros(n, np.float32), np.zeros(I, np.float32), got.astype(np.float32),
                                      Y.astype(np.float32))
                        return s2.recommend(np.arange(n, dtype=np.int32), 10, exclude=lists)

                assert second_model().tobytes() == m.fold_in_users(lists).tobytes()        # both ways give the same rows
                a = m.recommend_lists(svd, lists, k=10)
                b = second_svd()
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                t = dict(first=[], first_dev=[], later=[], later_dev=[], kept_dev=[], model=[], lists=[], svd=[])
                for _ in range(reps):
                    w, dev = first()
                    t["first"].append(w); t["first_dev"].append(dev)
                    t["later"].append(_wall_ms(lambda: m.fold_in_users(lists))); t["later_dev"].append(m.fold_ms)
                    t["model"].append(_wall_ms(second_model))
                    t["lists"].append(_wall_ms(lambda: m.recommend_lists(svd, lists, k=10)))
                    t["kept_dev"].append(m.fold_ms)        # recommend_lists' fold-in copies no rows to the host
                    t["svd"].append(_wall_ms(second_svd))
                med = {k: float(np.median(val)) for k, val in t.items()}
                row.update(fold_in_first_ms=med["first"], fold_in_first_device_ms=med["first_dev"], fold_in_later_ms=med["later"],
                           fold_in_later_device_ms=med["later_dev"], fold_in_rows_kept_device_ms=med["kept_dev"],
                           second_model_half_ms=med["model"],
                           second_model_over_fold_in=med["model"] / med["later"], recommend_lists_ms=med["lists"],
                           second_svd_model_ms=med["svd"], second_svd_over_recommend_lists=med["svd"] / med["lists"])
                rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="32,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--numpy-rows", type=int, default=400)
    ap.add_argument("--solver", choices=("cholesky", "cg"))
    ap.add_argument("--cg-steps", type=int, default=3)
    ap.add_argument("--also-cholesky", default="", help="with --solver cg: dims at which the Cholesky path runs too")
    ap.add_argument("--cap", default="", help="with --solver: a further row per width and per listed length, every item's list cut to it")
    ap.add_argument("--fold-in", action="store_true",
                    help="fold-in and recommend_lists against a second model, n = 1, 256, 6040: d = 64 Cholesky and d = 128 CG (DESIGN §29)")
    ap.add_argument("--reps", type=int, default=9, help="with --fold-in: alternated repeats behind each median")
    ap.add_argument("--out")
    a = ap.parse_args()
    fh = open(a.out, "a") if a.out else None
    if a.fold_in:
        jobs = [lambda: run_fold_in(64, "cholesky", 0, a.reps), lambda: run_fold_in(128, "cg", a.cg_steps, a.reps)]
    elif a.solver is None:
        jobs = [lambda d=int(d): [run_dim(d, a.iters, a.numpy_rows)] for d in a.dims.split(",")]
    else:
        legs = [(a.solver, int(d)) for d in a.dims.split(",")] + [("cholesky", int(d)) for d in a.also_cholesky.split(",") if d]
        jobs = [lambda s=s, d=d, cap=cap: [run_solver(d, a.iters, s, a.cg_steps, cap)] for s, d in legs for cap in [0] + [int(c) for c in a.cap.split(",") if c]]
    for job in jobs:
        for row in job():
            line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
            print(line, flush=True)
            if fh:
                fh.write(line + "\n")
                fh.flush()
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
