#!/bin/bash
# On an MI355X: whole GPU test suite, the bench line of a --full run, and (unless NOPROF=1) the GBA-only profile passes.  usage: full_check.sh <tag> <log dir>
TAG=${1:-r02x}
LOGS=${2:?usage: full_check.sh <tag> <log dir>}
cd $GRAFT_REPO_ROOT
mkdir -p "$LOGS"
( time timeout 1500 python -m pytest tests -q -m gpu -x 2>&1 | tail -8 ) > "$LOGS/${TAG}_pytest.log" 2>&1
( time timeout 600 python bench.py --full ) > "$LOGS/${TAG}_bench.log" 2>&1
grep -h '^{"metric"' "$LOGS/${TAG}_bench.log" | tail -1 > "$LOGS/${TAG}_bench_line.json"
if [ -z "$NOPROF" ]; then bash scripts/profile.sh $TAG > "$LOGS/${TAG}_profile.log" 2>&1; fi
tail -5 "$LOGS/${TAG}_pytest.log"; tail -c 600 "$LOGS/${TAG}_bench_line.json"
