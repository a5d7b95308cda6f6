#!/bin/bash
# tools/build_all.sh: the library (csrc/libivfadc_hip.so).
# Fails loudly: a compile error ends the script with hipcc's status and leaves the previous library untouched.
set -euo pipefail
cd "$(dirname "$0")/../ivfadc.jl_amd/csrc"
FL="--offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -fPIC -shared -std=c++17"
build() {   # $1 = output
  local out="$1"
  rm -f "$out.tmp"
  if ! /opt/rocm/bin/hipcc $FL -o "$out.tmp" ivfadc_hip.hip 2>build.log; then
    grep -E "error" -A4 build.log || cat build.log
    rm -f "$out.tmp"
    echo "build_all.sh: hipcc failed for $out (previous library left in place)" >&2
    exit 1
  fi
  mv "$out.tmp" "$out"
}
build libivfadc_hip.so
ls -la --time-style=+%T libivfadc_hip.so
