# Round-4 evidence at HEAD in one GPU call (run from the repo root on the box):
#   GPU suite, smoke, PMC traffic + kernel trace (profile_round.sh), SQ
#   counters (pmc_sq.sh), the isa_arithmetic peer, then the bench line on
#   this call's own counter files.  bash tools/refresh_r04.sh TAG
set -o pipefail
TAG=${1:-r04}
O=$(pwd)/gpurun_out/refresh_$TAG
mkdir -p $O
export TMPDIR=/tmp
T="timeout -k 10"
$T 600 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1 && \
$T 300 python3 -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 && \
bash tools/profile_round.sh $TAG && \
bash tools/pmc_sq.sh $TAG && \
python3 tools/pmc_summary.py gpurun_out/sq_$TAG > $O/sq_summary.txt 2>&1 && \
$T 120 ./storage-benchmarks_amd/bin/rs_arithmetic --vectors 8 16 32 --runs 3 > $O/arithmetic.log 2>&1 && \
$T 600 python3 bench.py --full --traffic $O/../prof_$TAG/traffic.json --sq-counters $O/sq_summary.txt --host-io 64 > $O/bench.log 2>&1
