#!/bin/bash
# Time fso_step for FedAdam, FedAdagrad and FedAvgM beside k_yogi_step at 1 M and 25 M parameters, non-temporal on and
# off, and the 1000 x 25 M round under fed-adam beside fed-yogi (tools/serveropt_measure.py), and leave
# profiles/serveropt_measure.{log,json}.  Run from the repository root on a machine with an MI355X, with
# libfedagg.so already built (python -c "import __graft_entry__ as g; g.build()").  Every GPU step has its own time
# limit and the steps are chained: a step that fails or hangs ends the script, nothing is started after it.
set -o pipefail
export OMP_NUM_THREADS=${OMP_NUM_THREADS:-16}
OUT=${1:-profiles}
mkdir -p "$OUT" &&
timeout -k 10 120 python -c "from fedscale_amd import _native_serveropt as ns; ns.load(); print('fedserveropt ABI', ns.ABI_VERSION)" &&
timeout -k 10 420 python -u tools/serveropt_measure.py --reps 30 --round-reps 5 \
    --out "$OUT/serveropt_measure.json" 2>&1 | tee "$OUT/serveropt_measure.log"
