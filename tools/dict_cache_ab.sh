#!/bin/bash
# Evidence for the dictionary table reuse (profiles/dict_cache/): this tree
# against a checkout of its parent commit built beside it, on one box.
#   bash tools/dict_cache_ab.sh <parent tree> [pairs] [full pairs]
# <parent tree>: a directory holding the parent commit's files and its built
# lib/ (the Python binding checks the library's exports, so the parent's
# library runs under the parent's own package).
#   prof_{parent,new}/     single-proof kernel stats (rocprofv3 --kernel-trace --stats, --inflight 1)
#   pmc_{parent,new}/      VALU counters in a counter-only run of their own (pmc_valu.py, per_proof.py pmc)
#   overlap_{parent,new}/  kernel trace of a default run (three in flight): overlap.py on a window of the timed steps
#   ab/                    alternating plain bench.py runs: parent, new, new with SEZKP_DICT_CACHE=0
#   full/                  alternating bench.py --full runs: parent, new
# Each step has its own time limit; the first failure ends the script.
# The same A/B serves any change that has an off switch:
#   SEZKP_AB_OUT=<dir>       output directory (default out/dict_cache)
#   SEZKP_AB_OFF=<VAR=value> the third headline arm's switch (default SEZKP_DICT_CACHE=0;
#                            none: a change without a switch, such as a refactor, has no third arm)
#   SEZKP_AB_STEPS="prof ab full"  the steps to run (default all three)
set -euo pipefail
export TMPDIR=/tmp
ROOT=$PWD
PARENT=$(cd "$1" && pwd)
R=${2:-3}
RF=${3:-3}
O=${SEZKP_AB_OUT:-$ROOT/out/dict_cache}
OFF=${SEZKP_AB_OFF:-SEZKP_DICT_CACHE=0}
STEPS=${SEZKP_AB_STEPS:-prof ab full}
mkdir -p $O/ab $O/full
O=$(cd $O && pwd)
want() { case " $STEPS " in *" $1 "*) return 0;; *) return 1;; esac; }
P1="python3 bench.py --full --inflight 1 --no-cpu-baseline --no-configs --no-worst-case --no-host-rows --no-sharded --dntt-log-n 0"
for arm in parent new; do
  want prof || break
  if [ $arm = parent ]; then cd $PARENT; else cd $ROOT; fi
  mkdir -p $O/prof_$arm $O/pmc_$arm $O/overlap_$arm
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$arm/trace -o run -- \
    $P1 --steps 20 --detail $O/prof_$arm/if1.json > $O/prof_$arm/if1.log 2>&1
  cp $O/prof_$arm/trace/run_kernel_stats.csv $O/prof_$arm/kernel_stats_if1.csv
  timeout -s KILL 150 rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU \
    SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_$arm/valu -o run -- \
    $P1 --steps 6 --warmup 2 --no-host-to-proof --detail $O/pmc_$arm/pmc.detail.json > $O/pmc_$arm/valu.log 2>&1
  timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/overlap_$arm/trace -o run -- \
    python3 bench.py > $O/overlap_$arm/bench.log 2>&1
  cd $ROOT/tools
  python3 per_proof.py trace $O/prof_$arm/trace/run_kernel_trace.csv > $O/prof_$arm/tables_per_proof.txt
  python3 pmc_valu.py $O/pmc_$arm/valu/run_counter_collection.csv > $O/pmc_$arm/pmc_valu.txt
  python3 per_proof.py pmc $O/pmc_$arm/valu/run_counter_collection.csv > $O/pmc_$arm/pmc_per_proof.txt
  # a window of the timed steps: the last 0.8 s of the run but its last 0.2 s
  # (the 600 timed proofs take about 1 s), proofs counted by their k_expand
  T=$O/overlap_$arm/trace/run_kernel_trace.csv
  W=$(python3 -c "
import csv, sys
r = [(int(x['Start_Timestamp']), 'k_expand' in x['Kernel_Name']) for x in csv.DictReader(open(sys.argv[1]))]
t0, t1 = min(s for s, _ in r), max(s for s, _ in r)
a, b = t1 - 800e6, t1 - 200e6
print((a - t0) / 1e6, (b - t0) / 1e6, sum(1 for s, e in r if e and a <= s < b))" $T)
  python3 overlap.py $T $W > $O/overlap_$arm/overlap.txt
  rm -f $T $O/prof_$arm/trace/run_kernel_trace.csv
  cd $ROOT
done
for i in $(seq 1 $R); do
  want ab || break
  cd $PARENT
  timeout -k 10 200 python3 bench.py > $O/ab/parent_$i.json 2> $O/ab/parent_$i.err
  cd $ROOT
  timeout -k 10 200 python3 bench.py > $O/ab/new_$i.json 2> $O/ab/new_$i.err
  [ "$OFF" = none ] && continue
  env $OFF timeout -k 10 200 python3 bench.py > $O/ab/new_cache_off_$i.json 2> $O/ab/new_cache_off_$i.err
done
for i in $(seq 1 $RF); do
  want full || break
  cd $PARENT
  timeout -k 10 400 python3 bench.py --full --no-cpu-baseline --dump-outputs $O/full/dump_parent > $O/full/parent_$i.json 2> $O/full/parent_$i.err
  cd $ROOT
  timeout -k 10 400 python3 bench.py --full --no-cpu-baseline --dump-outputs $O/full/dump_new > $O/full/new_$i.json 2> $O/full/new_$i.err
done
if want full; then
  n=0
  for f in $O/full/dump_parent/*; do
    cmp $f $O/full/dump_new/$(basename $f)
    n=$((n + 1))
  done
  echo "dumped proofs identical: $n files" > $O/full/dumped_proofs_compare.txt
  python3 tools/dict_cache_report.py --full $O/full > $O/full/full_ab.txt
fi
if want ab; then python3 tools/dict_cache_report.py --off-label "$OFF" $O/ab > $O/ab/headline_ab.txt; fi
echo "dict_cache_ab done"
