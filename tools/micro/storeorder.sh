#!/bin/bash
# Runs the store-order study (tools/micro/storeorder.hip) in N fresh processes (default 3: where the buffers land
# physically differs between processes) and writes the record to OUT (default build/storeorder.txt) and to stdout.
# Builds build/storeorder first if it is not there (build it on a CPU box; the run itself needs the GPU).
#     tools/micro/storeorder.sh <git head> [N] [OUT]
set -o pipefail
cd "$(dirname "$0")/../.."
HEAD=${1:-unknown}; N=${2:-3}; OUT=${3:-build/storeorder.txt}
mkdir -p build "$(dirname "$OUT")"
[ -x build/storeorder ] || hipcc --offload-arch=gfx950 -O3 -o build/storeorder tools/micro/storeorder.hip || exit 1
echo "# tools/micro/storeorder.hip at $HEAD, $(date -u +%Y-%m-%dT%H:%MZ): store orders of the headline's write geometry, $N processes x three passes" > "$OUT"
for p in $(seq 1 $N); do
  echo "### process $p" >> "$OUT"
  timeout -k 10 300 build/storeorder >> "$OUT" 2>&1 || { echo "process $p failed: $?" >> "$OUT"; cat "$OUT"; exit 1; }
done
cat "$OUT"
