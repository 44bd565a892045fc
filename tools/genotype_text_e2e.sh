#!/bin/bash
# The genotype text route measured end to end, on the GPU box from the repo root:
#   tools/genotype_text_e2e.sh <tag> <parent build directory or -> [genome_len 256000000] [variants 800000] [samples 3] [error k-mers per sample 560000000] [SVs per mille 10] [budget seconds 1000]
# One data set (tools/make_c2_dataset.cpp), makeBloom and `bayesTyper cluster` once, then `bayesTyper genotype` with BT_STAGE_TIMES=1 three times per setting:
# the parent build's executable (a directory holding its bayesTyper and libraries; "-" = none), this build with BT_GENOTYPE_TEXT_ON_DEVICE unset, and set — at
# -p <two threads per core of the quota> and at -p 1 (this build only: with the switch unset it runs the parent's code).  Then one run with BT_GIBBS_DEBUG (sizes,
# not-covered count) and one under rocprofv3 --kernel-trace --stats (the text kernels).  Every VCF body is compared with the first run's.  Runs that would start
# after the budget are skipped and listed.  Output: <BT_E2E_OUT, default build/e2e>/<tag>_genotype_text_e2e.txt (copy it to profiles/).
set -uo pipefail
root=$PWD
tag=$1; parent=$2; L=${3:-256000000}; NV=${4:-800000}; NS=${5:-3}; NE=${6:-560000000}; SV=${7:-10}; budget=${8:-1000}
T=$(python3 -c 'import sys; sys.path.insert(0, sys.argv[1]); from bayestyper_amd import hostinfo as h; print(h.baseline_threads(h.host_facts()))' "$root")
out=${BT_E2E_OUT:-$root/build/e2e}; mkdir -p $out
dst=$out/${tag}_genotype_text_e2e.txt
d=/tmp/gt_$tag; rm -rf $d; mkdir -p $d
exe=$root/bayestyper_amd/bayesTyper; tools_exe=$root/bayestyper_amd/bayesTyperTools
start=$(date +%s)
rows='Gibbs: sampling launch|genotypes on the device|VCF lines from|genotype text on the device|write VCF|wall since main|peak host memory|records route'
first_md5=""
genotype() {   # <label> <executable> <threads> [VAR=value ...]: one run, its stage rows, its VCF body against the first run's
  local label=$1 bin=$2 p=$3; shift 3
  if [ $(( $(date +%s) - start )) -gt $budget ]; then echo "## $label: SKIPPED (time budget)" >> $dst; return 0; fi
  echo "## $label" >> $dst
  rm -f $d/run.vcf
  env BT_STAGE_TIMES=1 "$@" timeout -k 10 600 $bin genotype -v $d/bt_unit_1/variant_clusters.bin -c $d/bt_cluster_data -s $d/samples.tsv -g $d/genome.fa -o $d/run -p $p -r 42 > $d/run.out 2> $d/run.err
  local rc=$?
  if [ $rc -ne 0 ]; then echo "rc $rc" >> $dst; tail -5 $d/run.err >> $dst; exit $rc; fi
  grep -E "$rows|^bt_gibbs_genotype" $d/run.err | cut -c1-400 >> $dst
  local md5=$(grep -v '^#' $d/run.vcf | md5sum | cut -d' ' -f1)
  [ -z "$first_md5" ] && first_md5=$md5
  [ "$md5" = "$first_md5" ] && echo "VCF body == first run ($(grep -vc '^#' $d/run.vcf) records)" >> $dst || echo "VCF BODY DIFFERS from the first run" >> $dst
}
echo "# genotype text e2e: genome $L nt, $NV candidate variants ($SV per mille long deletions with nested candidates), $NS sample(s), k=55, -p $T and -p 1; $(date -u)" > $dst
g++ -O2 -std=c++17 -fopenmp $root/tools/make_c2_dataset.cpp -o $d/make_c2_dataset || exit 1
$d/make_c2_dataset $d $L $NV $NS $NE $SV >> $dst 2>&1 || exit 1
( cd $d && for s in $(seq 1 $NS); do $tools_exe makeBloom -k sample$s -p $T > /dev/null 2>&1 || exit 1; done ) || exit 1
timeout -k 10 600 $exe cluster -v $d/candidates.vcf -s $d/samples.tsv -g $d/genome.fa -o $d/bt -p $T -r 42 > $d/cluster.out 2> $d/cluster.err || exit 1
echo "# data set, makeBloom and cluster took $(( $(date +%s) - start )) s" >> $dst
for rep in 1 2 3; do
  [ "$parent" != "-" ] && genotype "parent_p${T}_$rep" $parent/bayesTyper $T
  genotype "unset_p${T}_$rep" $exe $T
  genotype "text_p${T}_$rep" $exe $T BT_GENOTYPE_TEXT_ON_DEVICE=1
done
genotype "text_debug_p$T" $exe $T BT_GENOTYPE_TEXT_ON_DEVICE=1 BT_GIBBS_DEBUG=1
if [ $(( $(date +%s) - start )) -le $budget ]; then
  echo "## kernel trace (rocprofv3 --kernel-trace --stats), switch set: the text kernels and the genotype kernels" >> $dst
  TMPDIR=/tmp BT_GENOTYPE_TEXT_ON_DEVICE=1 timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $d/trace -- $exe genotype -v $d/bt_unit_1/variant_clusters.bin -c $d/bt_cluster_data \
    -s $d/samples.tsv -g $d/genome.fa -o $d/traced -p $T -r 42 > $d/trace.out 2> $d/trace.err || { echo "rc $?" >> $dst; exit 1; }
  python3 - "$(find $d/trace -name '*kernel_stats.csv' | head -1)" >> $dst <<'PY'
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0]
    if name.startswith(("text_", "geno_")):
        print(f'{name:28s} calls {r["Calls"]:>3s}  total {int(r["TotalDurationNs"]) / 1e6:8.3f} ms  average {float(r["AverageNs"]) / 1e6:8.3f} ms')
PY
fi
for rep in 1 2 3; do
  genotype "unset_p1_$rep" $exe 1
  genotype "text_p1_$rep" $exe 1 BT_GENOTYPE_TEXT_ON_DEVICE=1
done
echo "# total $(( $(date +%s) - start )) s" >> $dst
tail -n +1 $dst | cut -c1-300
rm -rf $d
