#!/bin/bash
# Time the trimmed-mean kernels beside fa_reduce at 1000 x 25 M and 100 x 1 M (tools/trim_reduce_measure.py) and
# leave profiles/trim_reduce_measure.{log,json}.  Run from the repository root on a machine with an MI355X, with
# libfedagg.so already built (python -c "import __graft_entry__ as g; g.build()").  Every GPU step has its own time
# limit and the steps are chained: a step that fails or hangs ends the script, nothing is started after it.
set -o pipefail
export OMP_NUM_THREADS=${OMP_NUM_THREADS:-16}
mkdir -p profiles &&
timeout -k 10 120 python -c "from fedscale_amd import _native_trim as nt; nt.load(); print('fedtrim ABI', nt.ABI_VERSION)" &&
timeout -k 10 420 python -u tools/trim_reduce_measure.py --configs head,c2 --reps 30 --round-reps 10 \
    --out profiles/trim_reduce_measure.json 2>&1 | tee profiles/trim_reduce_measure.log
