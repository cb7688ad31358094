#!/bin/bash
# the bench lines kept under profiles/ per round (run on the GPU box from the repo root):  tools/bench_lines.sh [bdd|rest|all|driver] [r04]
# (every line with --full: the rooflines, kernel times and CPU baseline of a line are measured behind that option)
# (REFIND=1: MIOpen's exhaustive find into a scratch db -- ~9 GPU-minutes for the BDD100K pyramid; the default uses the
#  find-db that travels with the package, memotr_amd/tuning/miopen_db, which bench.py points MIOpen at)
R=${2:-r06}
mkdir -p gpurun_out/lines gpurun_out/miopen/db gpurun_out/miopen/cache
if [ "${REFIND:-0}" = "1" ]; then
  export MIOPEN_USER_DB_PATH=$PWD/gpurun_out/miopen/db
  export MIOPEN_CUSTOM_CACHE_DIR=$PWD/gpurun_out/miopen/cache
fi
run() { name=$1; shift; t0=$SECONDS; python bench.py "$@" 2> gpurun_out/lines/$name.err | tail -1 > gpurun_out/lines/$name.json; echo "$name: $((SECONDS - t0)) s wall"; cut -c1-160 gpurun_out/lines/$name.json; }
case "${1:-all}" in
  bdd|all)
    run ${R}_bench_config5_bdd100k_bf16 --full --config bdd100k --dtype bf16 --steps 10 --warmup 14 --no-cpu-baseline
    run ${R}_bench_config5_bdd100k_f32 --full --config bdd100k --dtype f32 --steps 10 --warmup 14 --no-cpu-baseline
    du -sh gpurun_out/miopen/db gpurun_out/miopen/cache ;;&
  rest|all)
    run ${R}_bench_config4_mot17_checkpoint --full --config mot17 --use-checkpoint --steps 8 --warmup 3 --no-cpu-baseline
    run ${R}_bench_train_bf16 --full --dtype bf16 --steps 10 --warmup 4 --no-cpu-baseline
    run ${R}_bench_train --full --steps 10 --warmup 4
    run ${R}_bench_infer --full --workload infer --no-cpu-baseline
    run ${R}_bench_msda --full --workload msda --no-cpu-baseline ;;
  driver)
    run ${R}_bench_default_driver_cmd --full --gpus 1 --steps 20 --warmup 5 ;;
esac
