#!/bin/bash
# evidence run of a round (default r06): full bench line, driver-command line, rocprofv3 kernel stats + FETCH / WRITE PMC of the bench command, SQ counters of
# the lone pair's sweeps, batch profile + PMC + dynamic instruction counts; the bench lines, refresh_profiles.sh's files and every step's log land in
# $OUT/<R>_* (default bench_out/), the other scripts write where their headers say (copy what is to be judged into profiles/)
cd "$(dirname "$0")/../.."
R=${1:-r06}
export OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout 1500 python bench.py --full > $OUT/bench_full.log 2> $OUT/bench_full.err
grep '^{"metric"' $OUT/bench_full.log | tail -1 > $OUT/${R}_bench_full_line.json
timeout 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-extras > $OUT/bench_driver.log 2> $OUT/bench_driver.err
grep '^{"metric"' $OUT/bench_driver.log | tail -1 > $OUT/${R}_bench_driver_cmd_line.json
bash tests/micro/refresh_profiles.sh $R > $OUT/refresh_$R.log 2>&1
bash tests/micro/sweep_sq.sh $R > $OUT/sweep_sq_$R.log 2>&1
bash tests/micro/batch_profile.sh $R 9000 4000 1 > $OUT/batch_profile_$R.log 2>&1
bash tests/micro/batch_insts.sh > $OUT/${R}_batch_instruction_counts.txt 2> $OUT/batch_insts_$R.err
cut -c1-1500 $OUT/${R}_bench_full_line.json
cut -c1-300 $OUT/${R}_bench_driver_cmd_line.json
tail -5 $OUT/refresh_$R.log | cut -c1-300
tail -12 $OUT/sweep_sq_$R.log | cut -c1-200
tail -25 $OUT/batch_profile_$R.log | cut -c1-200
tail -22 $OUT/${R}_batch_instruction_counts.txt | cut -c1-200
tail -3 $OUT/bench_full.err
