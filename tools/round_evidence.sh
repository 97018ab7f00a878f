#!/bin/bash
# tools/round_evidence.sh TAG -- one visit's worth of round evidence, run from
# the repo root on the GPU box: the GPU tests, smoke(), the full bench line
# (bench.py --full: every phase beside the headline), then the rocprof kernel
# stats + PMC traffic of the warp (tools/profile_round.sh) and of the
# sequential hole-fill (tools/seq_pmc.sh).  Its own logs go to
# $OFD_EVIDENCE_DIR (default evidence_out/); the two profiling scripts write
# where they always did.
# Every GPU step has its own time limit; the first failure ends the script.
set -euo pipefail
TAG=${1:-r03}
R=$(pwd)
OUT=${OFD_EVIDENCE_DIR:-evidence_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/${TAG}_gputests.log" 2>&1
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/${TAG}_smoke.log" 2>&1
timeout -k 10 400 python bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"
bash tools/profile_round.sh ${TAG}
bash tools/seq_pmc.sh
tail -2 "$OUT/${TAG}_gputests.log"
tail -1 "$OUT/${TAG}_bench.json" | cut -c1-600
