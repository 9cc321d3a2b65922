# A/B of march libraries, alternating, three rounds: variants/libmnv_<name>.so for every name in AB_LIBS but "new", which is the tree's own
# library.  Per round and library: the batched launch of every workload in AB_WORKLOADS, then cfg2 frame by frame on 1 and 3 streams.
# Stops at the first run that fails.   usage: [AB_LIBS="head step1 new"] [AB_WORKLOADS="cfg2 fog"] bash tools/ab_march.sh
set -o pipefail
for i in 1 2 3; do
 for lib in ${AB_LIBS:-head new}; do
  if [ $lib = new ]; then unset MNV_LIB_PATH; else export MNV_LIB_PATH=$PWD/variants/libmnv_$lib.so; fi
  for wl in ${AB_WORKLOADS:-cfg2 cfg3 fog}; do
   timeout -k 10 300 python bench.py --no-extras --no-cpu-baseline --workload $wl --laps $([ $wl = cfg2 ] && echo 4 || echo 1) --steps 10 --warmup 3 2>/dev/null | python -c "
import sys,json; d=json.loads(sys.stdin.read()); print('$lib $wl batch', d['value'], d['ms_per_step'])" || exit 1
  done
  timeout -k 10 300 python bench.py --no-extras --no-cpu-baseline --per-frame --frame-streams 1 --steps 5 --warmup 2 2>/dev/null | python -c "
import sys,json; d=json.loads(sys.stdin.read()); print('$lib cfg2 per-frame 1 stream', d['value'], d['ms_per_step'])" || exit 1
  timeout -k 10 300 python bench.py --no-extras --no-cpu-baseline --per-frame --frame-streams 3 --steps 5 --warmup 2 2>/dev/null | python -c "
import sys,json; d=json.loads(sys.stdin.read()); print('$lib cfg2 per-frame 3 streams', d['value'], d['ms_per_step'])" || exit 1
 done
done
