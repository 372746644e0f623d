# A/B of the default liborbx.so against alternative builds (tools/diag/build_alt.sh), isolated stage times,
# two rounds in alternating order:  bash tools/diag/ab_multi.sh "DIR1 DIR2 ..." [bench args]
set -o pipefail
R=$GRAFT_REPO_ROOT
DIRS=$1; shift
cd $R
T=$(mktemp -d)
for i in 1 2; do
  for L in default $DIRS; do
    if [ $L = default ]; then unset ORBX_LIB; else export ORBX_LIB=$R/orb-slam-_amd/$L/liborbx.so; fi
    timeout -k 10 300 python bench.py --full --no-cpu --host-steps 0 --ingress-peers 0 --steps 20 --warmup 5 "$@" > $T/bench.json 2> $T/bench.err || exit 1
    python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print(sys.argv[2], d['value'], d['ms_per_step'], d['stage_ms_isolated'])" $T/bench.json $L
  done
done
