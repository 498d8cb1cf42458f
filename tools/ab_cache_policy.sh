#!/bin/bash
# A/B of the stash cache policies on the GPU box:  bash tools/ab_cache_policy.sh [N rounds, default 3] ["<variant flags>" ...]
# The shipped sources carry the chosen policy of every call site as its only form (mlp_core.h: StashStore / StashLoad); the
# per-call-site selection macros live in archive/proto/stash_cache_policy.patch, which this script puts into the WORKING TREE
# (never commit that; `git checkout mpg_amd/csrc` drops it again):
#   -DMPG_AB_ST_FWD=<p>     H1 / H2 stash of the forward sweep          -DMPG_AB_ST_BWD=<p>   step-0 DZ1 / DZ2 of the reverse sweep
#   -DMPG_AB_ST_CRITIC=<p>  h1, h2, dz1, dz2 of the fused critic kernels  -DMPG_AB_ST_NET=<p>   k_forward / k_backward (large-batch path)
#   -DMPG_AB_LD_BWD=<q>     the reverse sweep's H1 / H2 reads             p: plain | write_through     q: plain | nontemporal
# Every variant is built once (split engine) into its own copy of the library, then the default bench form runs N rounds over
# baseline, variants..., and a last baseline: alternating on one box, baseline first and last (EXPERIMENTS.md section 4.14).
cd "$(dirname "$0")/.."
N=3
[[ "${1:-}" =~ ^[0-9]+$ ]] && { N=$1; shift; }
if ! grep -q "MPG_AB_ST_FWD" mpg_amd/csrc/mlp_core.h; then
    git apply archive/proto/stash_cache_policy.patch || { echo "archive/proto/stash_cache_policy.patch does not apply to this tree" >&2; exit 1; }
    echo "[ab_cache_policy] selection macros applied to the working tree (git checkout mpg_amd/csrc to drop them)" >&2
fi
if [ $# -eq 0 ]; then
    set -- "-DMPG_AB_ST_FWD=write_through" "-DMPG_AB_ST_CRITIC=write_through" "-DMPG_AB_ST_BWD=write_through" "-DMPG_AB_LD_BWD=nontemporal"
fi
LIBS=${TMPDIR:-/tmp}/ab_cache_policy.$$
mkdir -p $LIBS
build() {   # build <index> "<flags>"
    MPG_EXTRA_CFLAGS="$2" python3 -m mpg_amd.build --split-only > $LIBS/build.log 2>&1 || { echo "BUILD FAILED [$2]"; tail -5 $LIBS/build.log; exit 1; }
    cp mpg_amd/libmpg_hip.so $LIBS/lib$1.so
}
bench() {   # bench <index> <label>
    cp $LIBS/lib$1.so mpg_amd/libmpg_hip.so
    timeout -k 10 300 python3 bench.py --gpus 1 2>/dev/null | tail -1 | python3 -c "
import json,sys
print('%-60s ms/step %.4f' % (sys.argv[1], json.loads(sys.stdin.read())['ms_per_step']))" "$2" || exit 1
}
build 0 ""
i=0; for V in "$@"; do i=$((i + 1)); build $i "$V"; done
for r in $(seq $N); do
    bench 0 "[baseline]"
    i=0; for V in "$@"; do i=$((i + 1)); bench $i "[$V]"; done
done
bench 0 "[baseline]"
rm -rf $LIBS
python3 -m mpg_amd.build --split-only > /dev/null 2>&1      # leaves the tree built with the working tree's sources and no flags
