# Round record (run at the end of a round; copy what is to be judged into profiles/rNN_*): full GPU suite, the full bench line, per-layer table, op-level table, rocprofv3 kernel stats, PMC traffic,
# the forced one-rank comm record and the two-ranks-on-one-GPU gloo run, as <output dir>/rec_*.
#   tools/round_record.sh <output dir>
mkdir -p "${1:?usage: tools/round_record.sh <output dir>}" && out=$(cd "$1" && pwd) || exit 1
cd $GRAFT_REPO_ROOT
root=$(pwd)
export TMPDIR=/tmp
( timeout 900 python -m pytest tests -m gpu -q 2>&1 | tail -8 ) > $out/rec_gpu_tests.txt
tail -2 $out/rec_gpu_tests.txt
( timeout 900 python bench.py --full > $out/rec_bench_line.json 2> $out/rec_bench.err )
cut -c1-300 $out/rec_bench_line.json
( timeout 300 python tools/per_layer_bench.py > $out/rec_per_layer.txt 2>&1 ); tail -1 $out/rec_per_layer.txt
( timeout 300 python tools/per_layer_bench.py --dtype f16 --batch 8 > $out/rec_per_layer_f16_b8.txt 2>&1 ); tail -1 $out/rec_per_layer_f16_b8.txt
( timeout 400 python bench_ops.py > $out/rec_bench_ops.jsonl 2>/dev/null ); wc -l $out/rec_bench_ops.jsonl
( cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/rec_prof -o b -- python $root/bench.py --steps 30 --warmup 6 --full --no-secondary --no-cpu-baseline --no-alt --no-parity > $out/rec_bench_under_rocprof.json 2> $out/rec_rocprof.err )
find $out/rec_prof -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $out/rec_bench_kernel_stats.csv
head -5 $out/rec_bench_kernel_stats.csv | cut -c1-160
PMC_TIMEOUT=150 bash tools/pmc_run.sh $out/rec_pmc "FETCH_SIZE" "WRITE_SIZE"
python tools/pmc_traffic.py $out/rec_pmc/pass1 $out/rec_pmc/pass2 > $out/rec_pmc_traffic.json 2> $out/rec_pmc_traffic.err; head -c 300 $out/rec_pmc_traffic.json; grep -A4 conv_family $out/rec_pmc_traffic.json
( RANK=0 WORLD_SIZE=1 LOCAL_RANK=0 MASTER_ADDR=127.0.0.1 MASTER_PORT=29519 UNFLOW_FORCE_REDUCER=1 timeout 600 python bench.py --gpus 1 --full --no-secondary --no-cpu-baseline --no-alt --no-parity --no-roofline > $out/rec_comm_record_forced_world1.json 2> $out/rec_comm.err )
# two ranks on the ONE GPU of the box, started by bench.py itself (no launcher around it: the command shape the driver uses);
# RCCL refuses two ranks on one device: gloo transport, same host code / streams / buckets
( UNFLOW_DIST_BACKEND=gloo timeout 600 python bench.py --gpus 2 --steps 10 --warmup 3 --full --no-secondary --no-cpu-baseline --no-alt --no-parity --no-roofline > $out/rec_2ranks.out 2> $out/rec_2ranks.err )
grep '^{"metric"' $out/rec_2ranks.out > $out/rec_bench_2ranks_gloo_one_gpu.json; tail -c 700 $out/rec_bench_2ranks_gloo_one_gpu.json
rm -rf $out/rec_prof $out/rec_pmc/pass*/ 2>/dev/null; ls $out | head -30
# round 6: the single-stream rocprof record (roofline_check reproduces the class time from the tracked CSV), the step timeline, the census VALU roofline
bash tools/serial_profile.sh rec > /dev/null 2>&1; tail -3 gpurun_out/rec_serial_roofline_check.txt
bash tools/step_trace.sh rec > /dev/null 2>&1; python tools/step_timeline.py gpurun_out/rec_step_trace.csv > gpurun_out/rec_step_timeline.txt 2>&1; head -2 gpurun_out/rec_step_timeline.txt
bash tools/census_valu.sh rec_census > /dev/null 2>&1
