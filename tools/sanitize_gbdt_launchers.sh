#!/usr/bin/env bash
# Host-side sanitizer run of the GBDT launchers' argument checks (gbdt.hip launch_gbdt_bin /
# launch_gbdt_split / launch_gbdt_leaf / launch_gbdt_predict, quantile.hip launch_quantile_select; old
# and new call forms, the monotone masks and bounds, the interaction groups and path and reg_alpha /
# max_delta_step among them):
# csrc/kernels/gbdt_args_selftest.cpp, a stand-alone program whose host code is built under
# ASan + UBSan while the device code is built as usual.  Needs hipcc and no GPU; nothing sanitised is
# loaded into Python.  Kept apart from sanitize_host.sh: it compiles gbdt.hip, a minute or two.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/fdx_sanitize}"
mkdir -p "$OUT"
HIPCC="$(command -v hipcc || echo /opt/rocm/bin/hipcc)"
K="$ROOT/fraud_detection_amd/csrc/kernels"
"$HIPCC" -std=c++17 -O1 -g --offload-arch="${FDX_ARCH:-gfx950}" -Xarch_host -fsanitize=address,undefined \
  -Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer -I"$K" \
  "$K/gbdt.hip" "$K/quantile.hip" -x hip "$K/gbdt_args_selftest.cpp" -o "$OUT/gbdt_args_selftest_asan"
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 "$OUT/gbdt_args_selftest_asan"
echo "sanitize_gbdt_launchers: ASan+UBSan clean"
