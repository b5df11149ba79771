# Full GPU check of the tree in ONE call, so every number of the round's evidence comes from the same box and tree
# (outputs under $OUT_DIR, default check_out/ in the repository root):
#  1. rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over the sweep -> profiles/trmm_pmc_traffic.json (read by bench.py
#     for roofline.traffic) and $OUT_DIR/trmm_pmc_traffic.json;
#  2. an MFMA-busy pass over the Cholesky launches -> $OUT_DIR/potrf_mfma.json (tools/pmc_potrf.py);
#  3. the -m gpu suite, smoke, bench --full (N=1, P=1 and P=4);
#  4. rocprofv3 --kernel-trace --stats of the bench.
# A failing test (pytest rc 1) does not stop the measurements; a crash, abort or time limit does.
set -o pipefail
R=$GRAFT_REPO_ROOT
O=${OUT_DIR:-$R/check_out}
mkdir -p $O/prof
cd /tmp && export TMPDIR=/tmp
timeout -s KILL 90 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/tools/sweep_only.py --m 131072 --reps 2 > $O/pmc_fetch.log 2>&1 &&
timeout -s KILL 90 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/tools/sweep_only.py --m 131072 --reps 2 > $O/pmc_write.log 2>&1 &&
timeout -s KILL 90 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F64 GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_potrf -- python3 $R/tools/fit_only.py --reps 3 > $O/pmc_potrf.log 2>&1 || exit $?
cd $R
python3 tools/pmc_traffic.py trmm_sumsq $O/pmc_fetch $O/pmc_write $O/trmm_pmc_traffic.json > $O/pmc_traffic.log 2>&1 &&
cp $O/trmm_pmc_traffic.json profiles/trmm_pmc_traffic.json &&
python3 tools/pmc_potrf.py $O/pmc_potrf 64 $O/potrf_mfma.json > $O/pmc_potrf_summary.log 2>&1 || exit $?
timeout -k 10 900 python -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread > $O/gpu_tests.log 2>&1
rc=$?
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "gpu tests ended with $rc"; exit $rc; fi
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 &&
timeout -k 10 400 python bench.py --full > $O/bench.json 2> $O/bench.err &&
timeout -k 10 300 python bench.py --full --problems-per-gpu 4 --steps 3 --warmup 1 --no-cpu-baseline > $O/bench_p4.json 2> $O/bench_p4.err &&
cd /tmp &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o bench --output-format csv -- python3 $R/bench.py --steps 3 --warmup 1 > $O/prof_bench.json 2> $O/prof_bench.err &&
exit $rc
