#!/usr/bin/env bash
# AddressSanitizer + UBSan run of hcu_ingest_jobs' host-side validation: a
# stand-alone host program (tools/ingest_validate_main.cpp) linked with
# csrc/augment.hip and csrc/timing.cpp, host code instrumented.  No device is
# used: every job is rejected before anything is enqueued.
set -euo pipefail
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${OUT:-build/ingest_validate_asan}
mkdir -p "$(dirname "$OUT")"
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Ihcunet_amd/csrc \
  -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
  hcunet_amd/csrc/augment.hip -x hip hcunet_amd/csrc/timing.cpp -x hip tools/ingest_validate_main.cpp \
  -fsanitize=address,undefined -o "$OUT"
"$OUT"
