# Interleaved bench.py A/B of two libdeig builds (measurement tooling):
#   bash tools/bench_ab.sh TAG LIB_A LIB_B CONFIG [CONFIG ...]   (LIB "shipped" = in-tree)
# runs A, B, A, B per config; one JSON summary line per run in $DEIG_OUT_DIR/TAG/bench_ab.log
# (DEIG_OUT_DIR defaults to out/)
set -o pipefail
TAG=$1; A=$2; B=$3; shift 3
OUT=${DEIG_OUT_DIR:-out}/$TAG
mkdir -p $OUT
for c in "$@"; do
  for lib in $A $B $A $B; do
    if [ "$lib" = shipped ]; then unset DEIG_LIB_PATH; else export DEIG_LIB_PATH=$lib; fi
    timeout -k 10 400 python -u bench.py --config $c --full --no-cpu-baseline > $OUT/b.json 2> $OUT/b.err \
      || { tail -20 $OUT/b.err; exit 1; }
    python -c "import json,sys; d=json.load(open('$OUT/b.json')); b=d.get('breakdown',{}); print(json.dumps({'config':'$c','lib':'$lib','value':d['value'],'step_ms':d['step_ms']['median'],'eig_ms':b.get('worker_eig_ms_per_worker'),'sweeps':b.get('worker_sweeps'),'acc':d.get('accuracy')}))" >> $OUT/bench_ab.log
  done
done
