#!/bin/bash
# device assembly of every translation unit, BASE_TREE (a checkout of another commit, _abtmp/base by convention) against the
# working tree: differing lines per file, comments / directives / the per-build __hip_cuid_ symbol left out; exit 1 if any differ
# usage (repo root, no GPU needed): bash tools/isa_diff.sh [BASE_TREE]
set -euo pipefail
BASE=$(cd "${1:-_abtmp/base}" && pwd)
HERE=$(cd "$(dirname "$0")/.." && pwd)
MK=$HERE/srrg2_proslam_amd/csrc/Makefile   # one Makefile for both trees: the base may predate the asm target
for t in "$BASE" "$HERE"; do
  make -s -C "$t/srrg2_proslam_amd/csrc" -f "$MK" -j"${JOBS:-8}" asm
done
strip() { grep -v -e '^[[:space:]]*[;.]' -e '__hip_cuid_' "$1" || true; }
rc=0
for s in "$HERE"/srrg2_proslam_amd/csrc/build/*.s; do
  f=$(basename "$s")
  n=$(diff <(strip "$BASE/srrg2_proslam_amd/csrc/build/$f") <(strip "$s") | grep -c '^[<>]' || true)
  printf '%-24s %d\n' "$f" "$n"
  [ "$n" -eq 0 ] || rc=1
done
exit $rc
