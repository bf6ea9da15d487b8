#!/bin/bash
# Time the geometric-median stages and both whole rounds beside fa_reduce at 100 x 1 M, 100 x 25 M and 1000 x 25 M
# (tools/geomed_measure.py) and leave profiles/geomed_measure.{log,json}.  Run from the repository root on a machine
# with an MI355X, with libfedagg.so already built (python -c "import __graft_entry__ as g; g.build()").  Every GPU
# step has its own time limit and the steps are chained: a step that fails or hangs ends the script, nothing is
# started after it.
set -o pipefail
export OMP_NUM_THREADS=${OMP_NUM_THREADS:-16}
mkdir -p profiles &&
timeout -k 10 120 python -c "from fedscale_amd import _native_geomed as ng; ng.load(); print('fedgeomed ABI', ng.ABI_VERSION)" &&
timeout -k 10 600 python -u tools/geomed_measure.py --configs c2,k100,head --reps 20 --round-reps 5 \
    --out profiles/geomed_measure.json 2>&1 | tee profiles/geomed_measure.log
