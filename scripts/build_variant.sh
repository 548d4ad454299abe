#!/bin/bash
# development aid: build a variant of libcvo_hip.so into tmp_libs/  usage: build_variant.sh <name> [extra hipcc -D flags...]
# (the sources and the four builds of cvo_kernels.hip are those of cvo_slam_amd/csrc/Makefile; the objects go to a directory of their own)
set -e
name=$1; shift
cd "$(dirname "$0")/../cvo_slam_amd/csrc"
out=${TMPDIR:-/tmp}/variant_$name; mkdir -p $out ../../tmp_libs
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wno-unused-function $*"
for f in cvo_kernels cvo_score_kernels cvo_support_kernels cvo_match_kernels cvo_hypothesis_kernels cvo_pose_model_kernels cvo_pcd_kernels cvo_reduce_kernels cvo_fuse_kernels cvo_selftest cvo_track_kernels cvo_capi; do
  hipcc $F -DCVO_BLOCK_MAX=512 -c $f.hip -o $out/$f.o &
done
hipcc $F -DCVO_KNS=cvohip_w3 -DCVO_BLOCK_MAX=768 -c cvo_kernels.hip -o $out/cvo_kernels_w3.o &
hipcc $F -DCVO_KNS=cvohip_e337 -DCVO_ARITH_MODES -DCVO_BLOCK_MAX=512 -c cvo_kernels.hip -o $out/cvo_kernels_e337.o &
hipcc $F -DCVO_KNS=cvohip_e337_w3 -DCVO_ARITH_MODES -DCVO_BLOCK_MAX=768 -c cvo_kernels.hip -o $out/cvo_kernels_e337_w3.o &
wait
hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tmp_libs/libcvo_hip_$name.so $out/*.o
echo built tmp_libs/libcvo_hip_$name.so
