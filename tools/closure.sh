# Round-end measurement pass (run from the repo root on the GPU box): full -m gpu suite, smoke, kernel trace of NORMAL decisions (+ per-pass
# table), PMC FETCH_SIZE pass of the SAME library build (its sha16 goes into profiles/<tag>_pmc_traffic.json), the bench line with its CPU
# leg (bench.py --full), the P1 line with its own kernel table, and the secondary configurations. Everything lands in closure_out/
# (git-ignored); copy what is to be judged into profiles/.
# Every GPU step runs under its own time limit and the pass stops at the first step that fails, faults or times out: nothing more is
# started on a card after a fault. Each step's stderr goes to its own log in closure_out/.
set -xeo pipefail
TAG=${1:-r06}
cd "$(dirname "$0")/.."
O=closure_out
SHA=$(sha256sum cover_vla_amd/libcover_hip.so | cut -c1-16)
mkdir -p $O
gpu() { local lim=$1; shift; timeout -k 10 "$lim" "$@"; }
gpu 1800 python -m pytest tests -m gpu -q > $O/${TAG}_gputests_full.txt 2>&1; tail -4 $O/${TAG}_gputests_full.txt > $O/${TAG}_gputests.txt; cat $O/${TAG}_gputests.txt
gpu 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/${TAG}_smoke.log 2>&1; tail -1 $O/${TAG}_smoke.log
gpu 600 rocprofv3 --kernel-trace --stats -d $O/${TAG} -o bench -- python3 bench.py --steps 5 --warmup 1 > $O/${TAG}_trace_stdout.log 2>&1
python tools/rocpd_stats.py $O/${TAG}/bench_results.db patchify_k > $O/${TAG}_bench_kernel_stats.txt 2>&1
python tools/timeline.py $O/${TAG}/bench_results.db > $O/${TAG}_timeline.txt 2>&1
gpu 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/${TAG}_pmc -o pmc -- python3 bench.py --steps 1 --warmup 0 > $O/${TAG}_pmc_stdout.log 2>&1
python tools/pmc_stats.py $O/${TAG}_pmc/pmc_results.db profiles/${TAG}_pmc_traffic.json $SHA > $O/${TAG}_pmc_fetch_size.txt 2>&1
cp profiles/${TAG}_pmc_traffic.json $O/${TAG}_pmc_traffic.json
tail -1 $O/${TAG}_pmc_fetch_size.txt
# matrix-pipe utilisation (own PMC pass, kernel trace only) through the COMMITTED tool
gpu 600 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE --kernel-trace -d $O/${TAG}_mf -o mf -- python3 bench.py --steps 1 --warmup 0 > $O/${TAG}_mf_stdout.log 2>&1
python tools/pmc_mfma.py $O/${TAG}_mf/mf_results.db > $O/${TAG}_pmc_mfma.txt 2>&1; head -12 $O/${TAG}_pmc_mfma.txt
gpu 900 python bench.py --full > $O/${TAG}_bench_line.json 2> $O/${TAG}_bench_stderr.log
cut -c1-400 $O/${TAG}_bench_line.json
gpu 300 python tools/phases.py > $O/${TAG}_phases.txt 2> $O/${TAG}_phases_stderr.log; cat $O/${TAG}_phases.txt
gpu 900 python bench.py --profile pi0 --full > $O/${TAG}_pi0_bench_line.json 2> $O/${TAG}_pi0_bench_stderr.log; cut -c1-300 $O/${TAG}_pi0_bench_line.json
gpu 600 rocprofv3 --kernel-trace --stats -d $O/${TAG}_pi0 -o pi0 -- python3 bench.py --profile pi0 --steps 3 --warmup 1 > $O/${TAG}_pi0_trace_stdout.log 2>&1
python tools/rocpd_stats.py $O/${TAG}_pi0/pi0_results.db patchify_k > $O/${TAG}_pi0_kernel_stats.txt 2>&1
gpu 600 python bench.py --full --config 3 --gpus 1 --steps 10 --warmup 2 --no-cpu-baseline > $O/${TAG}_config3_w1_line.json 2> $O/${TAG}_config3_w1_stderr.log
gpu 600 python bench.py --full --dtype fp8 --no-cpu-baseline > $O/${TAG}_fp8_n32_bench_line.json 2> $O/${TAG}_fp8_n32_stderr.log
gpu 900 python bench.py --full --dtype fp8 --samples 64 --horizon 8 --steps 3 --warmup 1 --no-cpu-baseline > $O/${TAG}_config5_fp8_n512_h8_bench_line.json 2> $O/${TAG}_config5_stderr.log
gpu 600 python bench.py --full --samples 2 --steps 10 --warmup 2 --no-cpu-baseline > $O/${TAG}_config2_n16_bench_line.json 2> $O/${TAG}_config2_stderr.log
gpu 600 python bench.py --full --samples 8 --cams 2 --members 2 --steps 10 --warmup 2 --no-cpu-baseline > $O/${TAG}_config4_2cam_n64_bench_line.json 2> $O/${TAG}_config4_stderr.log
gpu 900 python tools/bench_pi0fast.py > $O/${TAG}_pi0fast_stdout.log 2> $O/${TAG}_pi0fast_stderr.log; tail -1 $O/${TAG}_pi0fast_stdout.log > $O/${TAG}_pi0fast_line.json
for f in config3_w1_line fp8_n32_bench_line config5_fp8_n512_h8_bench_line config2_n16_bench_line config4_2cam_n64_bench_line pi0_bench_line; do python -c "import json,sys; d=json.load(open(sys.argv[2]+'/${TAG}_'+sys.argv[1]+'.json')); print(sys.argv[1], d['ms_per_step'], d['value'])" $f $O; done
cat $O/${TAG}_pi0fast_line.json
rm -rf $O/${TAG}_pmc/*.db $O/${TAG}/*.db $O/${TAG}_pi0/*.db $O/${TAG}_mf/*.db
