#!/bin/bash
# What does ranking cost inside k_smooth_xgb_h32?  A second library whose ranks<> is ONE conversion (-DGNX_RANK_ABLATE, gnx_rank.h:
# wrong ranks, the same loads and stores; it never enters the default library) against the default one, alternating, on the bench's
# shape: the difference of kernels.k_smooth_xgb.avg_ms is the ceiling of anything a better rank table can win.
#   bash scripts/dev/rank_ablate.sh build     (needs the default build's object files: make -C gnomix_amd/csrc first)
#   bash scripts/dev/rank_ablate.sh run       (on the GPU; REPS=3; BITS="10 12 14 16" also times forced table sizes, GNX_RK_BITS)
cd "$(dirname "$0")/../.." || exit 1   # the repository root
ABL=$PWD/gnomix_amd/libgnomix_hip_ablate.so
if [ "$1" = "build" ]; then
  cd gnomix_amd/csrc || exit 1
  HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}   # as gnomix_amd/csrc/Makefile
  TMPO=$(mktemp -d)/k_smooth_xgb_h32_ablate.obj
  FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -fno-fast-math -ffp-contract=off"
  $HIPCC $FLAGS -DGNX_RANK_ABLATE -c k_smooth_xgb_h32.hip -o $TMPO || exit 1
  OBJS=$(ls *.o */*.o | grep -v -e '^k_smooth_xgb_h32.o$')
  $HIPCC --offload-arch=gfx950 -shared -o $ABL $OBJS $TMPO -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined -lpthread -lz
  exit $?
fi
one() { "$@" timeout -k 10 120 python bench.py --steps 20 --warmup 5 | python -c "import json,sys; r=json.loads(sys.stdin.readlines()[-1]); print('smoother %.4f ms  base %.4f ms  value %.0f  checksum %s' % (r['kernels']['k_smooth_xgb']['avg_ms'], r['kernels']['k_base_logistic']['avg_ms'], r['value'], r['label_checksum']))"; }
for i in $(seq 1 ${REPS:-3}); do
  echo -n "default  : "; one env || exit 1
  echo -n "ablated  : "; one env GNX_LIBRARY=$ABL || exit 1
done
for b in $BITS; do echo -n "bits=$b  : "; one env GNX_RK_BITS=$b || exit 1; done
