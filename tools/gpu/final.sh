#!/bin/bash
# Round-end evidence, in two GPU visits (each well under 20 minutes):
#   PART=1: the GPU suite, the full bench line (bench.py --full), the line profile (the same
#           command under rocprofv3 with a roctx range per entry, tools/profile_line.sh) and
#           the k2himport profile;
#   PART=2: the round profile of every bench config (timed window + PMC traffic / VALU).
#   OUT_ROOT=<dir> TAG=r06final PART=1 bash tools/gpu/final.sh   (then tools/summarize_line_profile.py,
#   tools/summarize_profiles.py and tools/summarize_import_profile.py on <dir>)
set -o pipefail
O=${OUT_ROOT:?set OUT_ROOT to the directory (relative to the repository root) the evidence goes to}
mkdir -p "$O"
T=${TAG:-final}
if [ "${PART:-1}" = 1 ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
    > "$O/${T}_pytest_gpu.txt" 2>&1 || { tail -30 "$O/${T}_pytest_gpu.txt"; exit 1; }
  tail -2 "$O/${T}_pytest_gpu.txt"
  timeout -k 10 400 python bench.py --full > "$O/${T}_bench.json" 2> "$O/${T}_bench.err" || { tail -20 "$O/${T}_bench.err"; exit 1; }
  OUT=$O/${T}_line bash tools/profile_line.sh || exit 1
  timeout -k 10 600 bash tools/gpu/import_prof.sh || exit 1
else
  OUT=$O/prof_${T} bash tools/profile_round.sh ${CONFIGS:-fixed32 csr fixed4096 fixed32_1g ralledata fixed32_index} || exit 1
fi
echo ${T}_PART${PART:-1}_OK
