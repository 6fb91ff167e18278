#!/bin/bash
# The frame-stacking measurement of profiles/framestack/README.md: the library's fingerprint, then tools/framestack_bench.py -- each GPU
# step under a time limit of its own, chained with &&, so that a fault ends the run.  usage: tools/framestack_bench.sh [out-dir] [bench args]
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
out=${1:-profiles/framestack}
shift
mkdir -p "$out" &&
sha256sum gym_auv_amd/csrc/libauv_hip.so | tee "$out/lib_sha256.txt" &&
timeout -k 10 420 python tools/framestack_bench.py "$@" | tee "$out/framestack_bench.jsonl"
