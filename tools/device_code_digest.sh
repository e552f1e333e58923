#!/usr/bin/env bash
# usage: bash tools/device_code_digest.sh [unit.hip ...] > profiles/device_code_digest.txt   (no GPU needed: hipcc cross-compiles gfx950)
# One line per translation unit (default: every csrc/*.hip):   unit  device-sha256  host-sha256
# Each is the sha256 of the assembly the unit compiles to with build.sh's flags (-S --cuda-device-only, -S --cuda-host-only),
# with the one hash of the source text replaced by a fixed word: the compilation unit's id, which names the symbol
# __hip_cuid_<hex> on both sides and __hip_fatbin_<hex> / __hip_gpubin_handle_<hex> on the host side.  A source-only refactor
# leaves every digest as it was: diff this tool's output against the committed record before and after.  The compiler runs
# from the tree root on relative paths, so two checkouts of the same sources give the same file names in the assembly.
# DIGEST_JOBS (default 8, at most 16) units compile at a time.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
JOBS="${DIGEST_JOBS:-8}"; (( JOBS > 16 )) && JOBS=16
cd "$HERE"
CSRC=python-wlsqm_amd/csrc
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fopenmp -Iinclude -I"$CSRC" -Wall -Wno-unused-function)
FILES=("$@")
if (( ${#FILES[@]} == 0 )); then for src in "$CSRC"/*.hip; do FILES+=("$(basename "$src")"); done; fi
TMP="$(mktemp -d /tmp/digest_XXXX)"
trap 'rm -rf "$TMP"' EXIT

digest() {   # digest <unit.hip> <device|host>: the masked assembly's sha256 into $TMP/<unit>.<side>
  "$HIPCC" "${FLAGS[@]}" -S "--cuda-$2-only" -o "$TMP/$1.$2.s" "$CSRC/$1" 2>/dev/null ||
    { echo "device_code_digest: $1 ($2 side) does not compile" >&2; return 1; }
  sed -E 's/__hip_(cuid|fatbin|gpubin_handle)_[0-9a-f]+/__hip_\1_MASKED/g' "$TMP/$1.$2.s" | sha256sum | cut -d' ' -f1 > "$TMP/$1.$2"
  rm -f "$TMP/$1.$2.s"
}

# the same stamp as isa_stats.sh: the lines of libwlsqm_hip.manifest, hashed
echo "# sources sha256: $(cd "$HERE/python-wlsqm_amd" && export LC_ALL=C && sha256sum csrc/*.hip csrc/*.hpp ../include/*.h | sed 's#\.\./include#include#' | sha256sum | cut -d' ' -f1)"
pids=()
for f in "${FILES[@]}"; do
  for side in device host; do
    while (( $(jobs -rp | wc -l) >= JOBS )); do wait -n; done
    digest "$f" "$side" &
    pids+=($!)
  done
done
for p in "${pids[@]}"; do wait "$p"; done
for f in "${FILES[@]}"; do
  printf '%-22s %s  %s\n' "$f" "$(cat "$TMP/$f.device")" "$(cat "$TMP/$f.host")"
done
