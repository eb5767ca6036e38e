#!/bin/bash
# Runs on the GPU box (through gpurun): everything the r02_* files of profiles/ are built from.  Output under gpurun_out/r02/.
#   gpurun --timeout 2400 -- 'bash profiles/collect_r02.sh'        then here:  python profiles/summarise_r02.py
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/gpurun_out/r02
rm -rf $O; mkdir -p $O
cd $R
# 1. the driver's line: default workload (lineitem SF1, Zstandard), CPU baseline included
python bench.py --full > $O/bench_line.json 2> $O/bench_line.err
# 2. one bench line + one kernel table per workload / codec
cd /tmp && export TMPDIR=/tmp
run() {  # tag, bench args...
  tag=$1; shift
  ( cd $R && python bench.py --full "$@" --steps 10 --warmup 3 --no-cpu 2> $O/$tag.err | tail -1 > $O/line_$tag.json )
  ( cd $R && rocprofv3 --kernel-trace --stats --output-format csv -d $O/raw_$tag -- python3 bench.py --full "$@" --steps 5 --warmup 2 --no-cpu --skip-check > /dev/null 2> $O/prof_$tag.err )
  f=$(find $O/raw_$tag -name '*kernel_stats.csv' | head -1)
  [ -n "$f" ] && cp "$f" $O/kernel_stats_$tag.csv
  rm -rf $O/raw_$tag
}
for c in zstd snappy lz4 zlib none; do run lineitem_$c --workload lineitem --compression $c; done
run c2 --workload c2
run c2_adv --workload c2-adv --rows 24000000
run c2_rowgroup --workload c2-rowgroup
for c in none snappy zstd lz4 zlib; do run c3_$c --workload c3 --compression $c; done
run c5_lz4 --workload c5 --compression lz4
# 3. HBM traffic of the headline and of C3 / C2: FETCH_SIZE and WRITE_SIZE in passes of their own (no trace domains beside --kernel-trace)
pmc() {  # tag, counter, bench args...
  tag=$1; cnt=$2; shift; shift
  ( cd $R && rocprofv3 --kernel-trace --pmc $cnt --output-format csv -d $O/raw_pmc -- python3 bench.py --full "$@" --steps 2 --warmup 1 --no-cpu --skip-check > /dev/null 2> $O/pmc_${tag}_$cnt.err )
  f=$(find $O/raw_pmc -name '*counter_collection.csv' | head -1)
  [ -n "$f" ] && cp "$f" $O/pmc_${tag}_$cnt.csv
  rm -rf $O/raw_pmc
}
for cnt in FETCH_SIZE WRITE_SIZE; do
  pmc lineitem_zstd $cnt --workload lineitem --compression zstd
  pmc c3_none $cnt --workload c3 --compression none
  pmc c2 $cnt --workload c2
done
# the counter files are large (one row per dispatch): keep per-kernel averages only
python3 - $O <<'PY'
import csv, sys, glob, json, collections, os
O = sys.argv[1]
out = {}
for f in sorted(glob.glob(O + '/pmc_*_*.csv')):
    tag = os.path.basename(f)[4:-4]
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        acc[r['Kernel_Name'].split('(')[0]].append(float(r['Counter_Value']))
    out[tag] = {k: {"launches": len(v), "avg": sum(v) / len(v)} for k, v in acc.items()}
    os.remove(f)
json.dump(out, open(O + '/pmc_per_kernel.json', 'w'), indent=1)
PY
ls -la $O | head -60
