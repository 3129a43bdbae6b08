R=${1:?usage: bash tools/final_r03.sh ROOT  -- ROOT is the folder tools/profile.sh and its siblings write their prof_<tag>/ folders into}
mkdir -p $R/fin
python bench.py --full 2> $R/fin/bench.err | tail -1 > $R/fin/r03_bench_n1_final.json
bash tools/profile.sh r03 > $R/fin/profile.log 2>&1
cp -r $R/prof_r03/summary $R/fin/summary; rm -rf $R/prof_r03
python -c "
import json; d=json.loads(open('$R/fin/r03_bench_n1_final.json').read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['wall_clock_per_video']['vae_decode_tiled_s'])"
head -8 $R/fin/summary/r03_kernel_stats.csv | cut -c1-120
