#!/usr/bin/env bash
# Same-GPU A/B of two builds of this repository: the tree this script is in ("new") against
# another built tree ("parent": bench.py, pathtracer-cpp_amd/{ptamd,lib,bin}), alternating, one
# bench.py --gpus 1 --steps 20 --warmup 5 line per run into bench_outputs/ab_builds/.
# usage: bash scripts/ab_builds.sh OTHER_TREE
set -u
R="$(cd "$(dirname "$0")/.." && pwd)"
P="$(cd "$1" && pwd)"
O="$R/bench_outputs/ab_builds"; mkdir -p "$O"
run() {  # build name [bench args...]
  local b=$1 n=$2; shift 2
  local dir=$R; [ "$b" = parent ] && dir=$P
  (cd "$dir" && timeout -k 10 240 python bench.py --gpus 1 --steps 20 --warmup 5 "$@" > "$O/${b}_$n.json" 2> "$O/${b}_$n.log")
  local rc=$?
  if [ $rc -ne 0 ]; then echo "bench $b $n rc=$rc"; tail -5 "$O/${b}_$n.log"; exit $rc; fi
  python -c "import json,sys; d=json.load(open(sys.argv[1])); print('%-8s %-10s %9.1f Mray/s  kernel %9.1f Mray/s  %s' % (sys.argv[2], sys.argv[3], d['value'], d['kernel_mrays'], d['roofline']['kernel']))" "$O/${b}_$n.json" "$b" "$n"
}
for i in 1 2 3; do
  for b in parent new; do run $b head$i; done
  for b in parent new; do run $b c256_$i --res 256 --spp 16 --depth 3; done
  for b in parent new; do run $b c4096_$i --res 4096 --depth 8 --spp 300; done
done
for b in parent new; do run $b sphere --scene sphere --spp 1000; done
for b in parent new; do run $b mc03 --scene mcornell --rough 0.3; done
(cd "$R" && PT_TEST_HOOKS=1 PT_EMIT_REJECT=0 timeout -k 10 240 python bench.py --gpus 1 --steps 20 --warmup 5 \
   > "$O/new_hookoff.json" 2> "$O/new_hookoff.log") || { echo "hook-off run failed"; tail -5 "$O/new_hookoff.log"; exit 1; }
python -c "import json,sys; d=json.load(open(sys.argv[1])); print('new, PT_EMIT_REJECT=0  %9.1f Mray/s  kernel %9.1f' % (d['value'], d['kernel_mrays']))" "$O/new_hookoff.json"
