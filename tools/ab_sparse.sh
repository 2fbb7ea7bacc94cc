#!/bin/bash
# Same-box A/B of library builds on the fp32 W512 frame, per kernel (rocprofv3 kernel trace, a run of its own per build):
#   tools/ab_sparse.sh default f32enc2 f32noenc f32noappend f32noappend_noloads f32branch_noloads
# ("default" = the shipped library, anything else = build/variants/libsahs_<name>.so from `python tools/ablate.py build <name>`); prints the
# frame time and the field_forward_f32_kernel rows of the kernel statistics (calls, total ns, average ns, %, min, max, standard deviation)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT" || exit 1
export TMPDIR=${TMPDIR:-/tmp}
WORK=$(mktemp -d)
for V in "$@"; do
  if [ "$V" = default ]; then unset SAHS_NERF_LIB; else export SAHS_NERF_LIB=$ROOT/sahs-deformable-nerf_amd/build/variants/libsahs_$V.so; fi
  timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$WORK/$V" -o t -- python3 bench.py --steps 2 --warmup 1 > "$WORK/$V.json" 2> "$WORK/$V.err" || { echo "== $V failed"; tail -5 "$WORK/$V.err"; exit 1; }
  echo "== $V $(python3 -c "import json,sys;print(json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])['ms_per_step'])" "$WORK/$V.json") ms per frame (under the profiler)"
  grep -h field_forward_f32 $(find "$WORK/$V" -name "*kernel_stats.csv") | sed 's/"void sahs::field_forward_f32_kernel\(<[^>]*>\)([^"]*"/\1/'
done
rm -rf "$WORK"
