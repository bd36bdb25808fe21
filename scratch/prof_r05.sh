#!/bin/bash
# Round-5 profile collection (run on the GPU box through gpurun, from the repo root):
#     gpurun -- "GIT_HEAD=$(git rev-parse HEAD) bash scratch/prof_r05.sh"
# Summaries land in gpurun_out/r05/ together with r05_manifest.json = {lib_md5, git_head, ...}: the identity of the library every
# pass ran.  bench.py's pmc_traffic() refuses the PMC passes when that md5 is not the md5 of the library it has loaded.
# PMC passes are separate runs with --kernel-trace only (never combined with other trace domains).
cd /tmp && export TMPDIR=/tmp; cd "$GRAFT_REPO_ROOT"
O=gpurun_out/r05; mkdir -p $O
MD5=$(md5sum sparse-image-captioning_amd/libortk.so | cut -d' ' -f1)
B="python3 bench.py --full --no-extra-workloads --no-cpu-baseline --steps 3 --warmup 1"
stats() {   # name, extra args
  rocprofv3 --kernel-trace --stats --output-format csv -d $O/raw_$1 -o t -- $B $2 > $O/$1.log 2>&1
  cp $O/raw_$1/t_kernel_stats.csv $O/r05_$1_kernel_stats.csv
}
pmc() {     # name, counters..., then -- extra args
  local name=$1; shift; local ctr=(); while [ "$1" != "--" ]; do ctr+=("$1"); shift; done; shift
  rocprofv3 --kernel-trace --pmc "${ctr[@]}" --output-format csv -d $O/raw_$name -o t -- $B "$@" > $O/$name.log 2>&1
  python3 scratch/pmc_summary.py $O/raw_$name/t_counter_collection.csv > $O/r05_$name.csv
}
stats xe_b256_bf16 ""
stats decode_stack_b1024_beam5 "--workload decode"
stats sparse_decode_stack_b1024_beam5 "--workload sparse_decode"
stats scst_b256_ns5 "--workload scst"
stats sparse_xe_kernels "--workload sparse_xe --variant kernels"
stats decode_fp32_b1024_beam5 "--workload decode --variant fp32"
# the split fp32 GEMM: per-shape times / errors, and the counters of its instances
python3 scratch/f32x3_bench.py > $O/r05_f32_split_gemm.txt 2>&1
: > $O/r05_f32_split_pmc.txt
for ctr in "SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY" "SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_VALU SQ_INSTS_MFMA" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS" "GRBM_GUI_ACTIVE TCC_HIT_sum TCC_MISS_sum"; do
  rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $O/raw_x3 -o t -- python3 scratch/f32x3_one.py > $O/x3pmc.log 2>&1
  python3 scratch/pmc_kernels.py $O/raw_x3/t_counter_collection.csv gemm_f32 >> $O/r05_f32_split_pmc.txt 2>&1
  rm -rf $O/raw_x3
done
pmc xe_b256_pmc_fetch_size FETCH_SIZE --
pmc xe_b256_pmc_write_size WRITE_SIZE --
pmc decode_stack_pmc_fetch_size FETCH_SIZE -- --workload decode
pmc decode_stack_pmc_write_size WRITE_SIZE -- --workload decode
pmc sparse_decode_stack_pmc_fetch_size FETCH_SIZE -- --workload sparse_decode
pmc sparse_decode_stack_pmc_write_size WRITE_SIZE -- --workload sparse_decode
rm -rf $O/raw_*
python3 - <<PY
import json, time
json.dump({"lib_md5": "$MD5", "git_head": "${GIT_HEAD:-unknown}", "collected_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "command": "scratch/prof_r05.sh", "bench": "$B",
           "note": "every r05_*_kernel_stats.csv and r05_*_pmc_*.csv in this directory was produced by this library in this one gpurun call"},
          open("$O/r05_manifest.json", "w"), indent=1)
PY
cp $O/r05_manifest.json profiles/r05_manifest.json; cp $O/r05_*_pmc_*.csv profiles/     # (on the box: the bench line below reads them)
python3 bench.py --full --steps 50 --warmup 10 > $O/r05_default_bench_line.json 2> $O/bench.err
wc -c $O/r05_default_bench_line.json; tail -2 $O/bench.err
ls $O | head -40
