#!/bin/bash
# Same-box A/B on the plain bench (the headline alone, 20 steps): the tree's build against
# HONK_LIB variants in exp/_var (libhonk_NAME.so: a parent commit's library, or an
# exp/build_vf_variant.sh build), three alternating runs each; per run the value, ms per step
# and ms per layer.  The first run of each build dumps its logits; they are compared bitwise.
#   exp/plain_ab.sh parent [NAME ...]
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-$PWD/last_ab_out/plain_ab}
mkdir -p $OUT
for rep in 1 2 3; do
for v in "$@" default; do
  if [ $v = default ]; then unset HONK_LIB; else export HONK_LIB=$PWD/exp/_var/libhonk_$v.so; fi
  EXTRA=""; [ $rep = 1 ] && EXTRA="--dump-outputs $OUT/dump_$v"
  timeout -k 10 240 python -u bench.py --steps 20 --warmup 2 $EXTRA > $OUT/b_${v}_$rep.json 2> $OUT/b_${v}_$rep.err || { tail -20 $OUT/b_${v}_$rep.err; exit 1; }
  python -c "import json; d=json.load(open('$OUT/b_${v}_$rep.json')); print('$v', $rep, d['value'], d.get('ms_per_step'), d.get('roofline', {}).get('avg_ms_per_layer'))"
done
done
for v in "$@"; do
  python -c "import numpy as np; a=np.load('$OUT/dump_$v/logits.npy'); b=np.load('$OUT/dump_default/logits.npy'); print('logits $v vs default: array_equal', bool(np.array_equal(a, b)), a.shape)"
done
