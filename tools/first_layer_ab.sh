# A/B on one box, back to back, for the first transformer layer of the writers:
#   tools/first_layer_ab.sh            (atom, position) rows (default) vs tokens (GRAPPA_FIRST_LAYER_ROWS=0)
#   tools/first_layer_ab.sh indexed    on (atom, position) rows: q | k | v read through the table index and the multi-row token sums (default)
#                                      vs the token-level copy of q | k | v (GRAPPA_FIRST_LAYER_INDEXED=0); four pairs of the plain bench command,
#                                      every ms_per_step and final_loss to $OUT_DIR/first_layer_index_ab.txt
set -e
if [ "$1" = indexed ]; then
  OUT_DIR=${OUT_DIR:-results}
  mkdir -p $OUT_DIR
  O=$OUT_DIR/first_layer_index_ab.txt
  : > $O
  for i in 1 2 3 4; do
    for v in 0 1; do
      echo -n "GRAPPA_FIRST_LAYER_INDEXED=$v  " >> $O
      GRAPPA_FIRST_LAYER_INDEXED=$v python bench.py --gpus 1 --steps 20 --warmup 5 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('ms_per_step', round(d['ms_per_step'],3), 'final_loss', repr(d.get('final_loss')))" >> $O
    done
  done
  cat $O
  exit 0
fi
B="python bench.py --full --no-cpu-baseline --no-extras --alt-precision= --steps 20 --warmup 5"
show() { python -c "import sys,json; b=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$1', round(b['ms_per_step'],2), 'ms/step; products', round(b['roofline']['kernel_ms_per_step'],2), 'ms,', round(b['roofline']['achieved'],1), 'TFLOP/s')"; }
for i in 1 2 3; do
  GRAPPA_FIRST_LAYER_ROWS=0 $B 2>/dev/null | show "tokens          "
  GRAPPA_FIRST_LAYER_ROWS=1 $B 2>/dev/null | show "(atom, pos) rows"
done
