# A/B of two builds of the library - the parent's and one whose three-round sweep fetches a row's 4-byte words in one
# request per round - inside one GPU visit:
#   tools/ab_sweep_words.sh <parent libtfrecomm_hip.so> <new libtfrecomm_hip.so>
# Alternating three times: the headline (c2) over 900 steps and in the driver's 20-step form, and the sha256 of the five
# tables after 12 drawn headline steps; in the first turn also the headline at dim 128 (k_dense_tiles<32,4,false,10>) and
# a short run with the 30-epoch leg (val_rmse_converged), once for each build.  What the steps write to stderr is kept in $AB_LOG (default build/ab_sweep_words.log, which git ignores):
# when one faults or runs into its limit, the reason is there.  Each build is copied over the in-tree library for its
# turn; the in-tree one is put back at the end.  Every GPU step runs under its own time limit on a line of its own, so
# that `set -e -o pipefail` ends the script, with a non-zero status, at the first one that fails: nothing more starts on the card.
set -e -o pipefail
cd "$(dirname "$0")/.."
PARENT=$1; NEW=$2
[ -f "$PARENT" ] && [ -f "$NEW" ] || { echo "usage: $0 <parent .so> <new .so>"; exit 2; }
LIB=tf-recomm_amd/csrc/libtfrecomm_hip.so
LOG=${AB_LOG:-build/ab_sweep_words.log}
mkdir -p "$(dirname "$LOG")"; : > "$LOG"
KEEP=$(mktemp); cp $LIB $KEEP
trap 'cp $KEEP $LIB; rm -f $KEEP' EXIT
HASH='
import hashlib, sys
import numpy as np
sys.path.insert(0, ".")
import tfrecomm_amd as T
U, I, D, B, N = 6040, 3952, 64, 10000, 1000209
rs = np.random.RandomState(0)
with T.SvdModel(U, I, D, optimizer="adam", adam_mode="tf1", lr=1e-3, reg=0.05) as m:
    m.init_tables(seed=3)
    m.upload_triples(rs.randint(0, U, N).astype(np.int32), rs.randint(0, I, N).astype(np.int32), rs.randint(1, 6, N).astype(np.float32))
    m.rng_seed(7)
    m.train_steps_drawn(B, 12)
    t = m.tables()
print("  tables after 12 drawn steps: sha256", hashlib.sha256(b"".join(np.ascontiguousarray(t[k]).tobytes() for k in sorted(t))).hexdigest())
'
C2='
import json, sys
d = json.loads(sys.stdin.readline())
print("  c2 %4d steps: %.3f us/step" % (d["steps"], d["ms_per_step"] * 1e3), {k: round(v["us_per_step"], 2) for k, v in d["roofline"]["kernels"].items()},
      "val_rmse_after_timed_steps", d.get("val_rmse_after_timed_steps"), "val_rmse_converged", d.get("val_rmse_converged"))
'
ARGS="--no-configs --no-north-star --no-cpu-baseline --no-convergence"
for turn in 1 2 3; do
  for v in parent new; do
    if [ $v = parent ]; then cp "$PARENT" $LIB; else cp "$NEW" $LIB; fi
    echo "turn $turn build=$v"
    timeout -k 10 120 python bench.py --steps 900 --warmup 90 $ARGS 2>>"$LOG" | python -c "$C2"
    timeout -k 10 120 python bench.py --steps 20 --warmup 5 $ARGS 2>>"$LOG" | python -c "$C2"
    timeout -k 10 120 python -c "$HASH" 2>>"$LOG"
    if [ $turn = 1 ]; then
      echo -n "  dim 128:"
      timeout -k 10 120 python bench.py --dim 128 --steps 900 --warmup 90 $ARGS 2>>"$LOG" | python -c "$C2"
      echo -n "  with the 30-epoch leg:"
      timeout -k 10 300 python bench.py --steps 20 --warmup 5 --no-configs --no-north-star --no-cpu-baseline 2>>"$LOG" | python -c "$C2"
    fi
  done
done
