#!/bin/bash
# Time the secure-aggregation stages (modular reduce, mask sum at 10 / 100 / 1000 keys, finish) and the whole round
# beside fa_reduce and a plain round at 10 x 24,492, 100 x 1 M, 100 x 25 M and 1000 x 25 M (tools/secagg_measure.py)
# and leave profiles/secagg_measure.{log,json}.  Run from the repository root on a machine with an MI355X, with libfedagg.so
# already built (python -c "import __graft_entry__ as g; g.build()").  Every GPU step has its own time limit and the
# steps are chained: a step that fails or hangs ends the script, nothing is started after it.
set -o pipefail
export OMP_NUM_THREADS=${OMP_NUM_THREADS:-16}
mkdir -p profiles &&
timeout -k 10 120 python -c "from fedscale_amd import _native_secagg as ns; ns.load(); print('fedsecagg ABI', ns.ABI_VERSION)" &&
timeout -k 10 600 python -u tools/secagg_measure.py --configs c1,c2,k100,head --reps 20 --round-reps 5 \
    --out profiles/secagg_measure.json 2>&1 | tee profiles/secagg_measure.log
