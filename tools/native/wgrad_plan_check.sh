#!/bin/bash
# tools/native/wgrad_plan_check.sh: the weight-gradient launchers' host side (api.cpp's family choice, every family's choose(), the plan and
# workspace queries) under -fsanitize=address,undefined on the host side (-Xarch_host), driven by wgrad_plan_check.cpp.  Nothing is launched and no
# HIP call is made, so it runs on a machine without a GPU.  Exit status 0 = every expectation held and the sanitizers are silent.
set -e
cd "$(dirname "$0")"
mkdir -p bin/plan_check
C=../../osvos-pytorch_amd/csrc
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O1 -g -std=c++17 --offload-arch=gfx950 -Wno-unused-function -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
# api.cpp names every op-level launcher: their translation units come along (host side only)
SRCS="api.cpp errors.cpp wgrad_f32.hip wgrad_f32x3.hip wgrad_bf16.hip wgrad_small_f32.hip conv3x3_f32.hip conv3x3_f32x3.hip conv3x3_bf16.hip conv3x3_bf16_dma.hip conv3x3_bf16_p64.hip pack.hip pool.hip head.hip dgrad_c3.hip"
for f in $SRCS; do $HIPCC $FLAGS -x hip -c $C/$f -o bin/plan_check/${f%.*}.o & done
$HIPCC $FLAGS -x hip -c wgrad_plan_check.cpp -o bin/plan_check/main.o
wait
$HIPCC -fsanitize=address,undefined -o bin/wgrad_plan_check bin/plan_check/*.o -ldl
env -u OSVOS_WGRAD_VARIANT -u OSVOS_WGRAD_PW -u OSVOS_WGRAD_BLOCKS -u OSVOS_WGRAD_GENERIC -u OSVOS_WGRAD_REDUCE_T -u OSVOS_WGRAD_MAP -u OSVOS_WGRAD_FORM \
    -u OSVOS_WGRAD_X3_OLDADDR bin/wgrad_plan_check
