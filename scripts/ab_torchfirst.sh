#!/bin/bash
# Bench with and without torch imported before the library: a torch-first
# process (every GPU test, bench.py at N > 1) compiles the scene kernels with
# torch's bundled hipRTC / comgr; jit.*_vgprs shows the build.
# (--full: the line's jit and roofline fields.)  Logs go to $GPU_OUT (default out/).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O="${GPU_OUT:-out}"
mkdir -p "$O"
for first in none torch none torch; do
  if [ $first = torch ]; then
    timeout -k 10 300 python -c "import torch, runpy, sys; sys.argv=['bench.py','--full','--steps','4','--warmup','1','--no-cpu-baseline']; runpy.run_path('bench.py', run_name='__main__')" > "$O/ab.tmp" 2>&1
  else
    timeout -k 10 300 python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline > "$O/ab.tmp" 2>&1
  fi
  rc=$?
  v=$(python -c "import json,sys;d=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1]);print(d['jit'])" "$O/ab.tmp" 2>/dev/null)
  echo "first=$first rc=$rc $(python scripts/parse_bench.py "$O/ab.tmp" 2>/dev/null | cut -c1-90) $v" | tee -a "$O/ab_torchfirst.log"
  [ $rc -eq 0 ] || { tail -20 "$O/ab.tmp"; exit $rc; }
done
