#!/bin/bash
# end-of-round evidence (run on the GPU machine: bash tools/final_profiles.sh), under ${OUT:-bench_out}/:
#   ${TAG:-r02_final}_bench.json                  the default bench line with --full (headline + sub-records)
#   ${TAG:-r02_final}_bench_<method>.json         one line per method (--full: with cpu_baseline)
#   ${TAG:-r02_final}_<method>_stats.txt          rocprofv3 --kernel-trace --stats of the headline-only command
#                                                 (tools/prof_stats.sh keeps the kernel_stats.csv tables)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
out=${OUT:-bench_out}
mkdir -p "$out"
timeout -k 10 400 python bench.py --full > $out/${TAG:-r02_final}_bench.json 2> $out/${TAG:-r02_final}_bench.err || exit 1
echo "default done"
for m in ${METHODS:-svb12_zd svb_zd slow5_svb_zd vbe21_zd hasgam_vbsse21_zdq shuffman_vbe21_zd zstd_svb_zd zstd_svb12_zd zstd_hasgam_vbsse21_zdq}; do
  extra="--method $m"
  timeout -k 10 300 python bench.py --full $extra > $out/${TAG:-r02_final}_bench_$m.json 2> $out/${TAG:-r02_final}_bench_$m.err || exit 1
  tools/prof_stats.sh ${TAG:-r02_final}_$m -- python3 bench.py --steps 5 --warmup 2 $extra > $out/${TAG:-r02_final}_${m}_stats.txt || exit 1
  echo "$m done"
done
for m in rc_vbe21_zd rcc_vbe21_zd rccm_vbbe21_zd; do # serial per read: seconds per step - bench line only, two steps
  timeout -k 10 500 python bench.py --full --method $m --steps 2 --warmup 1 > $out/${TAG:-r02_final}_bench_$m.json 2> $out/${TAG:-r02_final}_bench_$m.err || exit 1
  echo "$m done"
done
