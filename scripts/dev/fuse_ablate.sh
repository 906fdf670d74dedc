#!/bin/bash
# What can ranking in the base pass's flush win, and what does it cost?  Two more libraries whose gnx_infer_dev runs ONE half of the
# fused route each (-DGNX_FUSE_ABLATE, gnx_api.hip; they never enter the default library) against the float route
# (GNX_FUSE_RANKS=0), alternating, on the bench's shape:
#   a = k_smooth_xgb_h32 copies its strip from a rank image nobody wrote (WRONG outputs), the base pass writes B as before:
#       float route - a on kernels.k_smooth_xgb.avg_ms is the saving;
#   b = k_base_logistic_i8 writes the image beside B, the smoother ranks B as before (right outputs):
#       b - float route on kernels.k_base_logistic.avg_ms is the cost (an upper bound: the fused route no longer writes B).
#   bash scripts/dev/fuse_ablate.sh build     (needs the default build's object files: make -C gnomix_amd/csrc first)
#   bash scripts/dev/fuse_ablate.sh run       (on the GPU; REPS=3)
cd "$(dirname "$0")/../.." || exit 1   # the repository root
LIBA=$PWD/gnomix_amd/libgnomix_hip_fuse_a.so
LIBB=$PWD/gnomix_amd/libgnomix_hip_fuse_b.so
if [ "$1" = "build" ]; then
  cd gnomix_amd/csrc || exit 1
  HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}   # as gnomix_amd/csrc/Makefile
  TMPD=$(mktemp -d)
  FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -fno-fast-math -ffp-contract=off"
  OBJS=$(ls *.o */*.o | grep -v -e '^gnx_api.o$')
  for v in 1 2; do
    $HIPCC $FLAGS -DGNX_FUSE_ABLATE=$v -c gnx_api.hip -o $TMPD/gnx_api_$v.obj || exit 1
    if [ $v = 1 ]; then OUT=$LIBA; else OUT=$LIBB; fi
    $HIPCC --offload-arch=gfx950 -shared -o $OUT $OBJS $TMPD/gnx_api_$v.obj -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined -lpthread -lz || exit 1
  done
  exit 0
fi
one() { "$@" timeout -k 10 120 python bench.py --steps 20 --warmup 5 | python -c "import json,sys; r=json.loads(sys.stdin.readlines()[-1]); print('smoother %.4f ms  base %.4f ms  pass %.4f ms  value %.0f  checksum %s' % (r['kernels']['k_smooth_xgb']['avg_ms'], r['kernels']['k_base_logistic']['avg_ms'], r['ms_per_pass'], r['value'], r['label_checksum']))"; }
for i in $(seq 1 ${REPS:-3}); do
  echo -n "float    : "; one env GNX_FUSE_RANKS=0 || exit 1
  echo -n "a (copy) : "; one env GNX_LIBRARY=$LIBA || exit 1
  echo -n "b (rank) : "; one env GNX_LIBRARY=$LIBB || exit 1
  echo -n "fused    : "; one env || exit 1
done
