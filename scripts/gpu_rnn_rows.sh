#!/bin/bash
# RNN rows-per-block experiment: tick (1 frame/call) and pipelined throughput at several batch sizes.
set -u
OUT=${OUT:-out}
mkdir -p $OUT
for S in ${STREAMS:-1024 4096 16384}; do for R in 64 32 16; do
  NNN_RNN_ROWS=$R timeout 300 python bench.py --full --streams $S --steps 30 --warmup 3 --no-cpu-baseline > $OUT/rows_${S}_$R.json 2>$OUT/rows_${S}_$R.err
  python -c "import json; d=json.load(open('$OUT/rows_${S}_$R.json')); print('S=$S rows=$R value=%.3e tick=%.3e k_rnn=%.1f us' % (d['value'], d['tick']['value'], d['kernels']['k_rnn']['avg_us']))"
done; done
