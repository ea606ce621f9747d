"""SVD++ step, top-K and ranking timings: one JSON line per shape, every leg at the same shape in the same process.

    python tools/bench_svdpp.py [--shapes ml1m,ml10m] [--steps 50] [--out profiles/bench_svdpp.jsonl]

Legs: the SVD++ step (train_step_dev, batch on the device) next to SvdModel's (train_step_dev and the host-fed train_step),
recommend_dev(k=10) for every user and rank_items of 10 held-out items per user for both models, and a vectorised NumPy
float32 host restatement of one SVD++ step (the CPU baseline; its thread count is reported).  Shapes are synthetic:
ML-1M-shaped (6040 x 3706, 1 M ratings) and ML-10M-shaped (71567 x 10681, 10 M ratings); N(u) = the training items.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"ml1m": (6040, 3706, 1000209), "ml10m": (71567, 10681, 10000054)}


def ratings(U, I, n, seed=0):
    """Uniform users; item popularity p(i) ~ 1 / (i + 50), whose head (0.46 % of the ratings at 3706 items, 0.37 % at 10681)
    is MovieLens's most-rated item (ML-1M: 3.4 k of 1 M ratings)."""
    rs = np.random.RandomState(seed)
    w = 1.0 / (np.arange(I) + 50.0)
    u = rs.randint(0, U, n).astype(np.int32)
    i = rs.choice(I, n, p=w / w.sum()).astype(np.int32)
    r = rs.randint(1, 6, n).astype(np.float32)
    return u, i, r


def host_step_f32(t, Nc, s_all, u, i, r, lam, lr):
    """One SVD++ SGD step in vectorised NumPy float32 (scipy.sparse for the implicit sums); updates t in place."""
    P, Q, Y, bu, bi = t["P"], t["Q"], t["Y"], t["bu"], t["bi"]
    users, inv = np.unique(u, return_inverse=True)
    Na = Nc[users]
    z = (Na @ Y) * s_all[users][:, None]
    e = P[users][inv] + z[inv]
    x = np.einsum("kd,kd->k", e, Q[i]) + t["mu"] + bu[u] + bi[i]
    g = (x - r).astype(np.float32)
    gq = g[:, None] * Q[i]
    W = np.zeros((users.size, P.shape[1]), np.float32)
    np.add.at(W, inv, gq)
    c = np.bincount(inv).astype(np.float32)
    W *= s_all[users][:, None]
    GY = (Na.T @ W) + lam * (Na.T @ c)[:, None] * Y
    dP = np.zeros_like(P)
    np.add.at(dP, u, gq + lam * P[u])
    dQ = np.zeros_like(Q)
    np.add.at(dQ, i, g[:, None] * e + lam * Q[i])
    P -= lr * dP
    Q -= lr * dQ
    Y -= lr * GY
    np.subtract.at(bu, u, lr * g)
    np.subtract.at(bi, i, lr * g)
    t["mu"] -= lr * g.sum()


def timed(fn, sync, reps):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps * 1e6


def run_shape(name, steps, batch, dim, host_reps):
    import torch
    import scipy.sparse as sp
    import tfrecomm_amd as T
    U, I, n = SHAPES[name]
    u, i, r = ratings(U, I, n)
    cut = int(0.9 * n)
    N = T.rated_matrix(u[:cut], i[:cut], U, I)
    nnz = int(N.nnz)
    rs = np.random.RandomState(1)
    d = torch.device("cuda")
    batches = [rs.randint(0, cut, batch) for _ in range(steps)]
    dev = [(torch.from_numpy(u[b]).to(d), torch.from_numpy(i[b]).to(d), torch.from_numpy(r[b]).to(d)) for b in batches]
    all_users = torch.arange(U, dtype=torch.int32, device=d)
    held = (rs.randint(0, I, U)[:, None] + np.arange(10) * (I // 10)) % I      # 10 distinct held-out items per user
    held.sort(axis=1)
    tgt = (np.arange(0, 10 * U + 1, 10), held.reshape(-1).astype(np.int32))
    row = dict(shape=name, users=U, items=I, ratings=n, implicit_nnz=nnz, dim=dim, batch=batch, steps=steps)
    kw = dict(optimizer="adam", adam_mode="lazy", lr=1e-3, reg=0.05)
    with T.SvdppModel(U, I, dim, **kw) as m:
        m.init_tables(seed=0)
        m.set_implicit(N)
        it = iter(range(10 ** 9))

        def pp_step():
            k = next(it) % steps
            m.train_step_dev(*dev[k])
        row["svdpp_step_us"] = timed(pp_step, lambda: (torch.cuda.synchronize(), m.sync()), steps)
        hb = [(u[b], i[b], r[b]) for b in batches]
        row["svdpp_step_host_us"] = timed(lambda: m.train_step(*hb[next(it) % steps], want_logits=False), m.sync, steps)
        row["svdpp_topk10_all_users_us"] = timed(lambda: m.recommend_dev(all_users, k=10, return_scores=False),
                                                 lambda: (torch.cuda.synchronize(), m.sync()), 5)
        row["svdpp_rank_10_per_user_us"] = timed(lambda: m.rank_items(np.arange(U, dtype=np.int32), tgt), m.sync, 3)
    with T.SvdModel(U, I, dim, **kw) as s:
        s.init_tables(seed=0)
        it2 = iter(range(10 ** 9))

        def svd_step():
            k = next(it2) % steps
            s.train_step_dev(dev[k][0].data_ptr(), dev[k][1].data_ptr(), dev[k][2].data_ptr(), batch)
        torch.cuda.synchronize()
        row["svd_step_us"] = timed(svd_step, s.sync, steps)
        row["svd_step_host_us"] = timed(lambda: s.train_step(*hb[next(it2) % steps], want_logits=False), s.sync, steps)
        row["svd_topk10_all_users_us"] = timed(lambda: s.recommend_dev(all_users, k=10, return_scores=False),
                                               lambda: (torch.cuda.synchronize(), s.sync()), 5)
        row["svd_rank_10_per_user_us"] = timed(lambda: s.rank_items(np.arange(U, dtype=np.int32), tgt), s.sync, 3)
    # CPU baseline: vectorised NumPy float32 SVD++ SGD step
    Nc = sp.csr_matrix((np.ones(nnz, np.float32), N.indices, N.indptr), shape=(U, I))
    cnt = np.diff(N.indptr).astype(np.float32)
    s_all = np.where(cnt > 0, 1.0 / np.sqrt(np.maximum(cnt, 1)), 0).astype(np.float32)
    rs2 = np.random.RandomState(2)
    t = dict(P=rs2.normal(0, .02, (U, dim)).astype(np.float32), Q=rs2.normal(0, .02, (I, dim)).astype(np.float32),
             Y=rs2.normal(0, .02, (I, dim)).astype(np.float32), bu=np.zeros(U, np.float32), bi=np.zeros(I, np.float32),
             mu=np.float32(3.5))
    t0 = time.perf_counter()
    for k in range(host_reps):
        b = batches[k % steps]
        host_step_f32(t, Nc, s_all, u[b], i[b], r[b], np.float32(0.05), np.float32(1e-3))
    row["numpy_f32_step_us"] = (time.perf_counter() - t0) / host_reps * 1e6
    row["numpy_threads"] = int(os.environ.get("OMP_NUM_THREADS", "1"))
    row["svdpp_over_svd_step"] = row["svdpp_step_us"] / row["svd_step_us"]
    row["numpy_over_svdpp_step"] = row["numpy_f32_step_us"] / row["svdpp_step_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,ml10m")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    fh = open(a.out, "a") if a.out else None
    for name in a.shapes.split(","):
        row = run_shape(name, a.steps, a.batch, a.dim, a.host_reps)
        line = json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items()})
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
