#!/bin/bash
# The whole GPU suite under every diagnostic / A-B switch (each must pass: the switches select other kernels, not other answers).
set -u
cd ${GRAFT_REPO_ROOT:-/root/repo}
O=gpurun_out/switch_matrix; rm -rf $O; mkdir -p $O
run() { name=$1; shift; (env "$@" timeout 1200 python -m pytest tests -m gpu -q 2>&1 | tail -3) > $O/$name.log; echo "$name: $(tail -1 $O/$name.log | cut -c1-120)"; }
run default LSR_NOP=1
run ndt_quad0 LSR_NDT_QUAD=0
run wait_sleep LSR_WAIT_MODE=sleep
run wait_yield LSR_WAIT_MODE=yield
run table_dense LSR_NDT_TABLE_MODE=0
run ndt_lane512 LSR_NDT_QUAD=0 LSR_NDT_WORKGROUP=512
