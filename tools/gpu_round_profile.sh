# Produces the rocprofv3 evidence committed under profiles/ (run on the GPU box). Raw output: $RAW_DIR/$ROUND (default
# build/profiles/rNN), read by tools/summarize_profiles.py with the same RAW_DIR.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
R=${ROUND:-r02}
O=${RAW_DIR:-build/profiles}/$R
rm -rf $O; mkdir -p $O
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -- python3 bench.py --steps 100 --warmup 10 --no-cpu-baseline --no-extra > $O/bench_under_rocprof.log 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 300 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/pmc_$c -- python3 bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-extra > $O/pmc_$c.log 2>&1
done
timeout 300 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES SQ_LDS_BANK_CONFLICT --output-format csv -d $O/pmc_SQ -- python3 bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-extra > $O/pmc_SQ.log 2>&1
# the bench with --full three times (G2P varies by a few us from process to process on one box): all lines are kept, the
# median by value becomes profiles/${R}_bench.json
: > $O/bench.json
for i in 1 2 3; do timeout 600 python3 bench.py --full >> $O/bench.json 2>> $O/bench.err; done
tail -1 $O/bench.json | cut -c1-300
