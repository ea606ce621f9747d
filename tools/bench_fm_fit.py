"""FM trainer timings: resident steps against host-fed steps, one JSON line per shape, in one process.

    python tools/bench_fm_fit.py [--steps 50] [--rounds 5] [--out profiles/bench_fm_fit.jsonl]
    python tools/bench_fm_fit.py --profile-steps 8           # resident steps only (2 warm-up steps, then one call of 8), to
                                                             # run under rocprofv3 --kernel-trace --stats, or with
                                                             # TFR_CALL_TRACE=1 for the host phases of the call
    python tools/bench_fm_fit.py --stats-csv profiles/fm_fit_kernel_stats.csv --stats-steps 10 ...
                                                             # adds the gather kernels' time and rate from that run's CSV

The tool is one process and sets no time limit of its own: run each invocation under `timeout` (the default shape takes
about two minutes, most of it the host-fed leg and building the store).

Shape (BASELINE config 5): F = 10^6 features, D = 64, a resident store of 2^22 rows x 8 non-zeros, batches of 2^20 rows,
nll loss, lazy Adam.  The two legs alternate, `rounds` times after a warm-up of each; the medians are reported:

  resident   train_steps_resident(ids, batch): ids uploaded once, every minibatch gathered on the device
  host-fed   train_step(X[ids_s], y[ids_s]) per step: scipy slices the rows, three arrays cross to the device

Also: the host time of plan_steps (NumPy) per step, the time a resident call takes to return when it does not wait for the
losses (ids checked, sized and uploaded, all steps queued), and the box's own copy rate (tfr_device_copy_rate) beside the
bytes the gather moves (ids, two indptr reads, indptr / y / indices / data written, indices / data read).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GATHER_KERNELS = ("k_fm_len_sums", "k_fm_chunk_scan", "k_fm_indptr", "k_fm_gather_copy")


def make_store(F, rows, nnz_per_row, seed=0):
    import scipy.sparse as sp
    rs = np.random.RandomState(seed)
    indptr = np.arange(rows + 1, dtype=np.int64) * nnz_per_row
    indices = rs.randint(0, F, rows * nnz_per_row).astype(np.int32)
    data = np.ones(rows * nnz_per_row, np.float32)
    y = (rs.rand(rows) < 0.5).astype(np.float32)
    return sp.csr_matrix((data, indices, indptr), shape=(rows, F)), y


def gather_bytes(batch, nnz):
    """bytes one minibatch gather reads and writes: three passes over the ids and the rows' two indptr words, the targets,
    indptr out (written, then read by the copy), and the entries in and out"""
    return 3 * batch * (8 + 16) + batch * (4 + 4) + 2 * (batch + 1) * 8 + 2 * nnz * 8


def gather_stats(path):
    """{kernel: total ns} of the gather kernels from a rocprofv3 --stats kernel_stats CSV"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for k in GATHER_KERNELS:
                if k in name:
                    out[k] = out.get(k, 0.0) + float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
    return out


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--nnz", type=int, default=8)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--stats-csv")
    ap.add_argument("--stats-steps", type=int, help="resident steps the --stats-csv run took (its warm-up steps included)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.stats_csv and (a.stats_steps is None or a.stats_steps < 1):
        ap.error("--stats-csv needs --stats-steps >= 1: the number of resident steps behind the CSV's totals")
    import tfrecomm_amd as T
    from tfrecomm_amd import fm
    if T._lib.load().tfr_device_count() < 1:
        raise SystemExit("no HIP device: this tool measures on the GPU only")
    x, y = make_store(a.features, a.rows, a.nnz)
    lengths = np.diff(x.indptr)
    rs = np.random.RandomState(1)
    nsteps = a.profile_steps or a.steps
    ids = rs.randint(0, a.rows, nsteps * a.batch).astype(np.int64)
    row = dict(shape="c5", features=a.features, dim=a.dim, store_rows=a.rows, nnz_per_row=a.nnz, batch=a.batch, steps=nsteps,
               rounds=a.rounds, loss="nll", optimizer="adam")
    with T.FmModel(a.features, a.dim, loss="nll", optimizer="adam", lr=1e-3, reg=0.0) as m:
        m.init(0)
        m.upload_rows(x, y)
        if a.profile_steps:
            m.train_steps_resident(ids[:2 * a.batch], a.batch)                   # warm-up: buffers and code objects
            m.train_steps_resident(ids, a.batch)
            print(json.dumps(dict(row, profile_only=True, resident_steps_run=nsteps + 2)), flush=True)
            return

        def host_fed(n):
            for s in range(n):
                e = ids[s * a.batch:(s + 1) * a.batch]
                m.train_step(x[e], y[e])

        m.train_steps_resident(ids[:3 * a.batch], a.batch)                   # warm-up: buffers and code objects
        host_fed(2)
        res, fed, enq, plan = [], [], [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            m.train_steps_resident(ids, a.batch)                             # returns with the losses: the steps are done
            res.append((time.perf_counter() - t0) / nsteps * 1e3)
            t0 = time.perf_counter()
            host_fed(nsteps)                                                 # every call synchronises
            fed.append((time.perf_counter() - t0) / nsteps * 1e3)
            t0 = time.perf_counter()
            m.train_steps_resident(ids, a.batch, want_loss=False)
            enq.append((time.perf_counter() - t0) / nsteps * 1e3)
            m.sync()
            t0 = time.perf_counter()
            fm.plan_steps(lengths, ids, a.batch)
            plan.append((time.perf_counter() - t0) / nsteps * 1e3)
    nnz = a.batch * a.nnz
    best, mean = T.device_copy_rate(0, 1 << 30, 10)
    row.update(resident_ms_per_step=median(res), host_fed_ms_per_step=median(fed), resident_rounds_ms=res, host_fed_rounds_ms=fed,
               resident_call_return_ms_per_step=median(enq), plan_steps_numpy_ms_per_step=median(plan),
               host_fed_over_resident=median(fed) / median(res), gather_bytes_per_step=gather_bytes(a.batch, nnz),
               device_copy_gbs_best=best, device_copy_gbs_mean=mean, timing="host clock around calls that end in a synchronise")
    if a.stats_csv:
        st = gather_stats(a.stats_csv)
        n = a.stats_steps
        total_us = sum(st.values()) / n / 1e3
        row.update(gather_kernels_us_per_step={k: v / n / 1e3 for k, v in st.items()}, gather_us_per_step=total_us,
                   gather_gbs=(gather_bytes(a.batch, nnz) / (total_us * 1e-6) / 1e9) if total_us > 0 else None)
        if row["gather_gbs"]:
            row["gather_over_copy_rate"] = row["gather_gbs"] / best
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
