#!/usr/bin/env bash
# Builds hcunet_amd/libhcunet.so for gfx950 (hipcc cross-compiles without a GPU).
# Usage: ./build.sh [extra hipcc flags]
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${OUT:-hcunet_amd/libhcunet.so}   # (OUT / BDIR: a variant build for A/B runs)
BDIR=${BDIR:-build}
SRC="hcunet_amd/csrc/timing.cpp hcunet_amd/csrc/families.cpp hcunet_amd/csrc/gconv.hip hcunet_amd/csrc/conv2.hip hcunet_amd/csrc/conv8.hip hcunet_amd/csrc/wgrad.hip hcunet_amd/csrc/wgrad8.hip hcunet_amd/csrc/wgrad3.hip hcunet_amd/csrc/pointwise.hip hcunet_amd/csrc/loss_adam.hip hcunet_amd/csrc/loss_ext.hip hcunet_amd/csrc/prep_all.hip hcunet_amd/csrc/bconv.hip hcunet_amd/csrc/bconv_f32.hip hcunet_amd/csrc/bconv_f32_cv1.hip hcunet_amd/csrc/bconv_f32_cv2.hip hcunet_amd/csrc/bconv_f32_cv4.hip hcunet_amd/csrc/bconv_bf16_cv1.hip hcunet_amd/csrc/bconv_bf16_cv2.hip hcunet_amd/csrc/bconv_bf16_cv4.hip hcunet_amd/csrc/bwgrad.hip hcunet_amd/csrc/segment.hip hcunet_amd/csrc/ingest.hip hcunet_amd/csrc/augment.hip hcunet_amd/csrc/targets.hip hcunet_amd/csrc/instances.hip hcunet_amd/csrc/cells.hip hcunet_amd/csrc/layout.hip hcunet_amd/csrc/pwconv.hip hcunet_amd/csrc/error.cpp hcunet_amd/csrc/layers.cpp hcunet_amd/csrc/exec.cpp hcunet_amd/csrc/unet.cpp hcunet_amd/csrc/chain.cpp hcunet_amd/csrc/ops.cpp"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Iinclude $*"
mkdir -p "$BDIR"
objs=()
pids=()
for s in $SRC; do
  o=$BDIR/$(basename "$s").o
  stale=0
  if [ ! -f "$o" ]; then stale=1; fi
  for dep in "$s" hcunet_amd/csrc/*.h include/hcunet.h build.sh; do   # (any internal header: no list to keep)
    if [ "$dep" -nt "$o" ]; then stale=1; fi
  done
  if [ $stale -eq 1 ]; then
    lang=""
    case "$s" in *.cpp) lang="-x hip";; esac
    $HIPCC $lang $FLAGS -c "$s" -o "$o.tmp" && mv "$o.tmp" "$o" &
    pids+=($!)
  fi
  objs+=("$o")
done
status=0
for p in "${pids[@]:-}"; do
  [ -z "$p" ] && continue
  wait "$p" || status=1
done
if [ $status -ne 0 ]; then echo "build failed" >&2; exit 1; fi
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT.tmp" "${objs[@]}"
mv "$OUT.tmp" "$OUT"
echo "built $OUT"
