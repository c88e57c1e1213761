#!/bin/bash
# Interleaved A/B of the stream's pinned slice on one box (profiles/ab_stream_pin.txt):
# per round the parent's library (tools/exp/parent.so, tools/build_variant.sh on
# the parent commit) and the in-tree library at every ABNN_STREAM_PIN_MB, each a
# fresh process of tools/pass_times.py (300 back-to-back passes, every launch
# timed).  usage: tools/ab_stream_pin.sh [ROUNDS]
set -o pipefail
export ABNN_LIB_ANY_ABI=1
ROUNDS=${1:-3}
log=$(mktemp)
trap 'rm -f "$log"' EXIT
one() {  # name lib MiB round
  ABNN_LIB=$PWD/$2 ABNN_STREAM_PIN_MB=$3 timeout -k 10 150 python -u tools/pass_times.py 300 1 > "$log" 2>&1 || { tail -20 "$log"; exit 1; }
  printf "%-12s r%s %s\n" "$1" "$4" "$(grep launches "$log" | sed 's/.*us: //')"
}
for r in $(seq 1 "$ROUNDS"); do
  [ -f tools/exp/parent.so ] && one parent tools/exp/parent.so 0 "$r"
  for mb in 0 64 96 128 160 192; do
    one "pin_mb=$mb" abnn_amd/libabnn_hip.so "$mb" "$r"
  done
done
