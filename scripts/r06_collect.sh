#!/bin/bash
# round 6: the records that go to profiles/ (run on the GPU box).  usage: OUT_DIR=<dir> scripts/r06_collect.sh
out=${OUT_DIR:?set OUT_DIR to the directory for the records}
mkdir -p $out
export PYTHONPATH=$PWD TMPDIR=/tmp
scripts/collect_profiles.sh r06 > $out/collect.log 2>&1
scripts/driver_form_profile.sh r06 > $out/driver_form_kernels.txt 2>&1
python bench.py --full > $out/bench.json 2> $out/bench.err
python bench.py --full --steps 20 --warmup 5 > $out/bench_driver_form.json 2> $out/bench_driver_form.err
python bench.py --full --width 1241 --height 376 --no-cpu-baseline --no-pmc > $out/bench_1241x376.json 2>/dev/null
scripts/driver_form_repeat.sh 5 > $out/driver_form_x5.json 2>/dev/null
quiet="--no-cpu-baseline --no-kernel-pass --no-full-leg --no-pmc --no-config-legs --no-session-leg"
python bench.py --session-loop --steps 20 --warmup 5 $quiet > $out/bench_session_loop_one_rank_rccl.json 2>/dev/null
python bench.py --session-loop --steps 300 --warmup 20 $quiet > $out/bench_session_loop_one_rank_rccl_300.json 2>/dev/null
DMS_BENCH_SESSION=1 DMS_BENCH_SHARE_GPU=1 DMS_BENCH_BACKEND=gloo timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29512 bench.py --full --gpus 2 --steps 20 --warmup 5 $quiet > $out/bench_two_gloo_ranks_one_gpu.json 2> $out/bench_two_gloo_ranks_one_gpu.err
rocprofv3 --kernel-trace --stats -d $out/kt_sess -o r -- python bench.py --session-loop --steps 100 --warmup 10 $quiet > /dev/null 2> $out/kt_sess.err
db=$(find $out/kt_sess -name "*results.db" | head -1)
python scripts/rocprof_summary.py $db 110 > $out/session_loop_kernel_stats.txt
rm -rf $out/kt_sess
tail -3 $out/collect.log; head -30 $out/driver_form_kernels.txt; cat $out/driver_form_x5.json; head -40 $out/session_loop_kernel_stats.txt
