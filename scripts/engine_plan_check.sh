#!/bin/bash
# Builds the engine planner's stand-alone check (csrc/native/engine_plan_check.cpp) under AddressSanitizer and
# UndefinedBehaviorSanitizer and runs it.  Host code only: a CPU program with its own main, not a Python module.
#   scripts/engine_plan_check.sh [build dir]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$ROOT/build/san_address}"
mkdir -p "$OUT"
"${CXX:-g++}" -O1 -g -fno-omit-frame-pointer -std=c++17 -march=x86-64-v3 -pthread -Wall \
  -fsanitize=address,undefined -fno-sanitize-recover=undefined -I"$ROOT/csrc/native" \
  "$ROOT/csrc/native/engine_plan.cpp" "$ROOT/csrc/native/engine_plan_check.cpp" -o "$OUT/engine_plan_check"
"$OUT/engine_plan_check"
