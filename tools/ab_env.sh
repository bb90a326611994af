# A/B of an environment switch on the end-to-end bench, interleaved in one GPU session
# (box-to-box spread is ~5 %).  usage: bash tools/ab_env.sh VAR "valA valB" [rounds] [utts]
# (results under $AB_OUT, default bench_out/ab)
set -eo pipefail
export TMPDIR=/tmp
V=$1; VALS=$2; R=${3:-2}; U=${4:-100}
O=${AB_OUT:-bench_out/ab}
mkdir -p $O
for r in $(seq 1 $R); do for v in $VALS; do
  env $V=$v timeout -k 10 300 python bench.py --full --utts $U --steps 3 --warmup 1 --cpu-seconds 0 > $O/$V-$v-$r.json 2> $O/$V-$v-$r.err
done; done
python - <<PY
import json,glob
for f in sorted(glob.glob("$O/$V-*.json")):
    d=json.loads(open(f).read().strip().splitlines()[-1]); print(f, d["value"], d.get("kinds_ms"))
PY
