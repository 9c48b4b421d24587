#!/bin/bash
# Per-kernel times and counters of the sampler in one matrix arithmetic (f32 | bf16x3 | bf16), on the GPU box:
#   tools/profile_math.sh <math> [tag] [outdir]   -> <outdir>/<tag>_<math>_kernel_stats.csv, <outdir>/<tag>_<math>_pmc.csv
# (outdir defaults to profile_out/, which git ignores)
# One lane, B = 256 (every kernel alone on the chip at the 512-sequence launch shape).  The kernel trace and every counter
# group are runs of their own (counters never together with a trace; FETCH_SIZE and WRITE_SIZE in separate passes).
set -o pipefail
math=${1:?usage: tools/profile_math.sh <f32|bf16x3|bf16> [tag] [outdir]}
tag=${2:-math}
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=${TMPDIR:-/tmp}
out=${3:-profile_out}
mkdir -p $out
d=$TMPDIR/prof_${tag}_${math}
rm -rf $d
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $d -- python3 tools/math_probe.py --one $math --one-steps 30 \
    > /dev/null 2> $out/${tag}_${math}_prof.err || { tail -5 $out/${tag}_${math}_prof.err; exit 1; }
cp $d/*/*kernel_stats.csv $out/${tag}_${math}_kernel_stats.csv
head -7 $out/${tag}_${math}_kernel_stats.csv
i=0
: > $out/${tag}_${math}_pmc.csv
for grp in "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA" "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU" "FETCH_SIZE" "WRITE_SIZE"; do
  i=$((i+1)); rm -rf $d.pmc$i
  timeout -k 10 200 rocprofv3 --pmc $grp --output-format csv -d $d.pmc$i -- python3 tools/math_probe.py --one $math --one-steps 3 \
      > /dev/null 2> $out/${tag}_${math}_pmc$i.err || { echo "pass failed: $grp"; tail -3 $out/${tag}_${math}_pmc$i.err; exit 1; }
  python3 - $d.pmc$i $out/${tag}_${math}_pmc.csv <<'PY'
import csv, glob, sys, collections
d, dst = sys.argv[1:3]
f = sorted(glob.glob(d + '/*/*counter_collection.csv'))[-1]
agg = collections.defaultdict(lambda: [0.0, 0])
for r in csv.DictReader(open(f)):
    if 'attn_fwd' in r['Kernel_Name'] or 'dit_rows' in r['Kernel_Name']:
        a = agg[(r['Kernel_Name'][:90], r['Counter_Name'])]; a[0] += float(r['Counter_Value']); a[1] += 1
with open(dst, 'a') as o:
    for (k, c), (v, n) in sorted(agg.items()):
        o.write('"%s",%s,%d,%.1f\n' % (k, c, n, v / n))
PY
done
cat $out/${tag}_${math}_pmc.csv
