# The id stream beside the headline step ("the id stream's share"), every leg inside one call on the GPU box:
#   bash tools/ab_sidestream.sh gap       drawn ids against ids staged before the clock, three alternations, 900 steps after 90
#   bash tools/ab_sidestream.sh trace     one rocprofv3 --kernel-trace pass (no counters), reduced by tools/trace_c2.py
#   bash tools/ab_sidestream.sh wt        TFR_WT settings (WT_SET) of the in-tree build, three alternations
#   bash tools/ab_sidestream.sh chunks    TFR_CHUNK_STEPS settings (CHUNK_SET) of the in-tree build, three alternations
#   bash tools/ab_sidestream.sh builds    tools/ab/libtfrecomm_hip_{base,new}.so copied over the in-tree one: c2 (900/90 and 20/5) and c3
# Several legs may be given; each GPU step runs under its own time limit and the script stops at the first that fails.
# The trace leg's files go to $AB_OUT (default build/sidestream, which git ignores).
set -e -o pipefail
cd "$(dirname "$0")/.."
OUT=${AB_OUT:-build/sidestream}
mkdir -p $OUT
C2="--steps 900 --warmup 90 --no-configs --no-north-star --no-cpu-baseline --no-convergence"
us_per_step() { python -c "
import json,sys
d=json.loads(sys.stdin.readline()); k=d['roofline']['kernels']
print('  %s: %.3f us/step  val_rmse %s' % (sys.argv[1], d['ms_per_step']*1e3, d.get('val_rmse_after_timed_steps')), {s: round(v['us_per_step'],2) for s,v in k.items()})" "$1"; }

for leg in "$@"; do
case $leg in
gap)
  # (a) the same model, the same 990 steps: drawn on the id stream inside the clock, or read from ids staged before it
  timeout -k 10 300 python - <<'EOF'
import time, sys
import numpy as np, torch
sys.path.insert(0, ".")
import bench, tfrecomm_amd as T
wl = bench.WORKLOADS["c2"]
U, I, D, B, K, W = wl["U"], wl["I"], wl["D"], wl["B"], 900, 90
train, val = bench.synth_movielens(U, I, wl["N"])
m = T.SvdModel(U, I, D, optimizer="adam", adam_mode=wl["adam_mode"], lr=wl["lr"], reg=wl["reg"], device=0)
m.init_tables(seed=13575)
m.upload_triples(*train)
np.random.seed(13575)
m.rng_from_numpy()
ids = np.random.RandomState(1).randint(0, len(train[0]), (W + K, B))
def timed(run_w, run_k):
    run_w(); m.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter(); run_k(); m.sync(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e6
drawn, staged = [], []
for rep in range(3):
    drawn.append(timed(lambda: m.train_steps_drawn(B, W), lambda: m.train_steps_drawn(B, K)))
    m.stage_ids(ids); m.sync()
    staged.append(timed(lambda: m.train_steps_staged(0, B, W), lambda: m.train_steps_staged(W, B, K)))
print("drawn  us/step:", " ".join("%.3f" % x for x in drawn))
print("staged us/step:", " ".join("%.3f" % x for x in staged))
print("gap (mean drawn - mean staged) %.3f us; spread of the drawn runs %.3f us" % (np.mean(drawn) - np.mean(staged), max(drawn) - min(drawn)))
EOF
  ;;
trace)
  # (b) which id-stream kernel ran beside each k_tile_step launch (kernel trace only: begin / end stamps, no counters)
  rm -rf $OUT/trace
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 bench.py --steps 200 --warmup 20 --no-cpu-baseline --no-north-star --no-convergence --no-configs > $OUT/bench_trace.json 2> $OUT/trace.log
  python3 tools/trace_c2.py $OUT/trace | tee $OUT/trace_c2.txt
  cp "$(ls $OUT/trace/*/*kernel_stats.csv | head -1)" $OUT/kernel_stats_c2_${TRACE_TAG:-run}.csv
  rm -rf $OUT/trace
  ;;
wt)
  # which write-through hand-offs pay (TFR_WT_* in csrc/svd_kernels.h): WT_SET="31 15 ..." picks the settings to alternate
  for rep in 1 2 3; do
    for v in ${WT_SET:-31 15}; do
      TFR_WT=$v timeout -k 10 200 python bench.py $C2 2>/dev/null | us_per_step "TFR_WT=$v"
    done
  done
  ;;
chunks)
  # steps per chunk of drawn ids at most on the small-table path (api.hip tfr_train_steps_drawn): CHUNK_SET="6 64 ..."
  for rep in 1 2 3; do
    for v in ${CHUNK_SET:-6 16 64 400}; do
      TFR_CHUNK_STEPS=$v timeout -k 10 200 python bench.py $C2 2>/dev/null | us_per_step "TFR_CHUNK_STEPS=$v"
    done
  done
  ;;
builds)
  for rep in 1 2 3; do
    for v in base new; do
      cp tools/ab/libtfrecomm_hip_$v.so tf-recomm_amd/csrc/libtfrecomm_hip.so
      timeout -k 10 200 python bench.py $C2 2>/dev/null | us_per_step "build=$v c2 900/90"
      timeout -k 10 200 python bench.py --steps 20 --warmup 5 --no-configs --no-north-star --no-cpu-baseline --no-convergence 2>/dev/null | us_per_step "build=$v c2 20/5"
      timeout -k 10 300 python bench.py --workload c3 --steps 40 --warmup 8 --no-cpu-baseline --no-north-star 2>/dev/null | us_per_step "build=$v c3 40/8"
    done
  done
  cp tools/ab/libtfrecomm_hip_new.so tf-recomm_amd/csrc/libtfrecomm_hip.so
  ;;
*) echo "unknown leg $leg"; exit 2 ;;
esac
done
