#!/usr/bin/env python3
"""The headline step's k_tile_step launches from a rocprofv3 --kernel-trace csv, by what the id stream ran beside them:
nothing, the generator (k_mt_blocks), the wide draw's count / emit kernels, the record gather, the one-workgroup draw.  A
launch counts under every id-stream kernel whose [begin, end) overlaps its own; "several" are launches that met more than one.
    python tools/trace_c2.py <dir with *_kernel_trace.csv> [launches to skip at the start]"""
import csv
import glob
import sys

import numpy as np

d = sys.argv[1]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 25
f = sorted(glob.glob(d + "/**/*_kernel_trace.csv", recursive=True))[-1]
rows = list(csv.DictReader(open(f)))
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows)
SIDE = (("k_mt_blocks", "k_mt_blocks"), ("k_mt_count", "count/emit"), ("k_mt_emit", "count/emit"), ("k_gather_recs", "k_gather_recs"),
        ("k_mt_draw", "k_mt_draw"))
side = [(s, e, lab) for s, e, nm in ev for key, lab in SIDE if key in nm]
starts = np.array([s for s, _, _ in side])


def stats(name, us):
    us = np.asarray(us)
    if us.size == 0:
        print("  %-16s n=0" % name)
        return
    print("  %-16s n=%4d  mean %6.2f  median %6.2f  min %6.2f  max %6.2f  sigma %5.2f us" % (name, us.size, us.mean(), np.median(us), us.min(),
                                                                                        us.max(), us.std()))


for kern in ("k_tile_step", "k_dense_tiles"):
    mine = [(s, e) for s, e, nm in ev if kern in nm][skip:]
    print("%s: %d launches (first %d skipped)" % (kern, len(mine), skip))
    stats("all", [(e - s) / 1e3 for s, e in mine])
    groups = {}
    for s, e in mine:
        # id-stream kernels that begin before this launch ends and end after it begins (they are few: scan those that start before e)
        hi = int(np.searchsorted(starts, e))
        met = sorted({lab for ss, se, lab in side[max(0, hi - 64):hi] if se > s})
        key = "none" if not met else met[0] if len(met) == 1 else "several"
        groups.setdefault(key, []).append((e - s) / 1e3)
        if len(met) > 1:
            for lab in met:
                groups.setdefault("  with " + lab, []).append((e - s) / 1e3)
    for key in ("none", "k_mt_blocks", "count/emit", "k_gather_recs", "k_mt_draw", "several"):
        stats(key, groups.get(key, []))
    for key in sorted(k for k in groups if k.startswith("  with ")):
        stats(key.strip(), groups[key])
    # by position in the run: bench.py's legs follow each other (timed drawn steps, staged ids, host-fed single steps that sort
    # inside their own launch, drawn steps under HIP events), and a per-kernel mean over the whole trace mixes them
    allk = [(e - s) / 1e3 for s, e, nm in ev if kern in nm]
    for lo in range(0, len(allk), 100):
        stats("launches %d.." % lo, allk[lo:lo + 100])
busy = sum(e - s for s, e, _ in side)
span = ev[-1][1] - ev[0][0]
print("id stream busy %.2f ms of %.2f ms traced (%.0f %%)" % (busy / 1e6, span / 1e6, 100.0 * busy / max(span, 1)))
