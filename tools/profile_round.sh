# Round profile set (run on the GPU box through gpurun): tests, bench lines, rocprofv3 kernel stats and the PMC passes the
# bench's roofline object cites.  usage: [OUT=dir] bash tools/profile_round.sh <tag> [a|b|all]     (e.g. r4b) -> $OUT/<tag>_* (default out/)
# Part a: GPU tests, the --full line, rocprofv3 --kernel-trace --stats of the same command.  Part b: the three PMC passes (FETCH_SIZE, WRITE_SIZE, matrix-pipe
# busy: separate runs, counters only), the other configurations (cfg2, cfg4, ref48 = the reference's shipped workload), --sample-calls, LSID, the 2-rank rehearsal.
# (a gpurun call is limited to 20 minutes: the two parts are two calls)
set -e
T=${1:-r5a}
PART=${2:-all}
cd /tmp && export TMPDIR=/tmp
R="${GRAFT_REPO_ROOT:?run through gpurun}"
cd "$R"
O=${OUT:-out}
mkdir -p "$O"
if [ "$PART" = a ] || [ "$PART" = all ]; then
[ -n "$SKIP_TESTS" ] || python -m pytest tests -m gpu -x -q > $O/${T}_pytest.log 2>&1 || { tail -30 $O/${T}_pytest.log; exit 1; }
python bench.py --full > $O/${T}_bench_default.jsonl 2> $O/${T}_bench_default.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$T -- python3 bench.py --steps 5 --warmup 1 --soak-s 0 --no-cpu --no-roofline --no-full-sample > $O/prof_$T.log 2>&1
cp $(ls $O/prof_$T/*/*kernel_stats.csv | head -1) $O/${T}_rocprofv3_kernel_stats_bench_steps5.csv
rm -rf $O/prof_$T
tail -2 $O/${T}_pytest.log
fi
if [ "$PART" = b ] || [ "$PART" = all ]; then
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 bench.py --steps 2 --warmup 1 --soak-s 0 --no-cpu --no-roofline --no-full-sample --eager > $O/pmc_fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 bench.py --steps 2 --warmup 1 --soak-s 0 --no-cpu --no-roofline --no-full-sample --eager > $O/pmc_write.log 2>&1
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_mfma -- python3 bench.py --steps 2 --warmup 1 --soak-s 0 --no-cpu --no-roofline --no-full-sample --eager > $O/pmc_mfma.log 2>&1
CMD="rocprofv3 --kernel-trace --pmc {COUNTERS} --output-format csv -- python3 bench.py --steps 2 --warmup 1 --soak-s 0 --no-cpu --no-roofline --no-full-sample --eager"
python tools/pmc_traffic.py $O/pmc_fetch $O/pmc_write $O/${T}_traffic.json "${CMD/\{COUNTERS\}/FETCH_SIZE | WRITE_SIZE (separate passes)}" > /dev/null
python tools/pmc_mfma.py $O/pmc_mfma $O/${T}_mfma_busy.json "${CMD/\{COUNTERS\}/SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE}"
rm -rf $O/pmc_fetch $O/pmc_write $O/pmc_mfma
python bench.py --full --config cfg2 --no-cpu > $O/${T}_bench_cfg2.jsonl 2>/dev/null
python bench.py --full --config cfg4 --no-cpu > $O/${T}_bench_cfg4.jsonl 2>/dev/null
python bench.py --full --config ref48 --steps 10 > $O/${T}_bench_ref48.jsonl 2>/dev/null
python bench.py --full --gpus 2 --one-device --backend gloo --no-cpu --steps 10 > $O/${T}_bench_2rank_selflaunch_one_device.jsonl 2>/dev/null
python bench.py --sample-calls --steps 1 --warmup 0 > $O/${T}_bench_sample_calls.jsonl 2>/dev/null
python tools/lsid_bench.py > $O/${T}_lsid.log 2>&1
for f in default cfg2 cfg4 ref48 sample_calls; do [ -f $O/${T}_bench_$f.jsonl ] && { echo "== $f"; python tools/bench_line.py < $O/${T}_bench_$f.jsonl; }; done
fi
