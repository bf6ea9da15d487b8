#!/bin/bash
# Time flr_reduce beside fa_reduce over a 25 M transformer-like layout and config 2's 1 M (tools/lowrank_measure.py)
# and leave profiles/lowrank_measure.{log,json}.  Run from the repository root on a machine with an MI355X, with
# libfedagg.so already built (python -c "import __graft_entry__ as g; g.build()").  Every GPU step has its own time
# limit and the steps are chained: a step that fails or hangs ends the script, nothing is started after it.
set -o pipefail
export OMP_NUM_THREADS=${OMP_NUM_THREADS:-16}
mkdir -p profiles &&
timeout -k 10 120 python -c "from fedscale_amd import _native_lowrank as nl; nl.load(); print('fedlowrank ABI', nl.ABI_VERSION)" &&
timeout -k 10 900 python -u tools/lowrank_measure.py --configs t25,c2 --clients 100,1000 --ranks 4,8,32 --reps 20 \
    --pcie 100 --out profiles/lowrank_measure.json 2>&1 | tee profiles/lowrank_measure.log
