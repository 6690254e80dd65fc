# bench legs beside the headline line (one GPU session): whole epochs, N = 32 bank, directional, 2-rank rehearsals on one
# device over gloo (weak and strong).  Records go to $OUT (default: bench_checks/ in the checkout).
set -x
cd "$(dirname "${BASH_SOURCE[0]}")/.."
OUT=${OUT:-$PWD/bench_checks}
mkdir -p $OUT
true && \
timeout 300 python bench.py --epoch --steps 2 --warmup 1 > $OUT/b_epoch.json 2> $OUT/b_epoch.err && tail -c 900 $OUT/b_epoch.json && \
timeout 300 python bench.py --full --lines-per-group 8 --no-cpu-baseline > $OUT/b_n32.json 2> $OUT/b_n32.err && tail -c 400 $OUT/b_n32.json && \
timeout 300 python bench.py --distinct-t60 > $OUT/b_t60.json 2> $OUT/b_t60.err && tail -c 300 $OUT/b_t60.json && \
timeout 300 python bench.py --full --bands 1 --no-cpu-baseline > $OUT/b_band1.json 2> $OUT/b_band1.err && tail -c 300 $OUT/b_band1.json && \
timeout 300 python bench.py --full --config directional --no-cpu-baseline > $OUT/b_dir.json 2> $OUT/b_dir.err && tail -c 400 $OUT/b_dir.json && \
GFDN_BENCH_ONE_DEVICE=1 GFDN_BENCH_BACKEND=gloo timeout 300 python bench.py --full --gpus 2 --steps 30 --warmup 5 --no-cpu-baseline --extra-steps 10 > $OUT/b_w2.json 2> $OUT/b_w2.err && tail -c 600 $OUT/b_w2.json && \
GFDN_BENCH_ONE_DEVICE=1 GFDN_BENCH_BACKEND=gloo timeout 300 python bench.py --gpus 2 --steps 30 --warmup 5 --scaling weak > $OUT/b_w2s.json 2> $OUT/b_w2s.err && tail -c 600 $OUT/b_w2s.json
