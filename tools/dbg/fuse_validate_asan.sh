#!/bin/bash
# Builds tools/dbg/fuse_validate.hip with orbfe_fuse.hip, host code under AddressSanitizer and UBSan, and runs it on
# the CPU: every call of orbfe_fuse_search, orbfe_scw_search, orbfe_sim3_search and orbfe_fkf_search returns from the
# argument validation, before any device call.
set -euo pipefail
cd "$(dirname "$0")/../.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
$HIPCC -O1 -g -std=c++17 --offload-arch=${ARCH:-gfx950} -ffp-contract=off -fno-fast-math \
    -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
    -o tools/dbg/fuse_validate tools/dbg/fuse_validate.hip pyorbslam_amd/csrc/orbfe_fuse.hip
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 tools/dbg/fuse_validate
