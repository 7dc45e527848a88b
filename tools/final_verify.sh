#!/bin/bash
# GPU suite + smoke() + the full benchmark line (every leg) in one call, from the repository root; logs go to OUTDIR.
#   bash tools/final_verify.sh OUTDIR
# A step that aborts, crashes or runs out of time ends the script: nothing more is started on the GPU after it.
O=${1:?usage: tools/final_verify.sh OUTDIR}
mkdir -p "$O" && O=$(cd "$O" && pwd) || exit 1
cd "$(dirname "$0")/.." || exit 1
step() { "$@"; rc=$?; case $rc in 124|134|137|139) echo "stopped after exit status $rc: $*"; exit $rc;; esac; }
step timeout -k 10 1500 python -m pytest tests/ -m gpu -q > "$O/gputests.txt" 2>&1
tail -3 "$O/gputests.txt"
step timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.txt" 2>&1; tail -2 "$O/smoke.txt"
step timeout -k 10 1200 python bench.py --full > "$O/bench.txt" 2>&1; tail -c 600 "$O/bench.txt"
