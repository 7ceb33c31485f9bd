#!/bin/bash
# Builds the host side of ppde_api.hip (no device code) + the mock runtime + one driver of this directory with AddressSanitizer
# and runs it: bash tests/hostcheck/build_and_run.sh NAME [sweep], NAME one of abi, reversible, tempering, recorder, pairs,
# archive, stats, anneal, anneal_adaptive, recombine. Output: tests/hostcheck/_build/NAME/ (git-ignored; one directory per driver,
# so two drivers can be built at the same time). HIPMOCK_TRACE=FILE in the environment: the mock's call trace (hipmock.cpp).
set -e
NAME=${1:?usage: build_and_run.sh NAME [sweep]}; shift
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); B=$HERE/_build/$NAME
[ -f "$HERE/$NAME.cpp" ] || { echo "no driver $HERE/$NAME.cpp" >&2; exit 2; }
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$B"
FLAGS="-O1 -g -std=c++17 -fPIC -fno-omit-frame-pointer -fsanitize=address -w"
$HIPCC $FLAGS --cuda-host-only -c "$ROOT/ppde_amd/csrc/ppde_api.hip" -o "$B/api.o"
# the host object refers to the embedded device image by a hashed name: give it an empty one
SYM=$(nm "$B/api.o" | awk '/ U __hip_fatbin/ {print $2; exit}')
echo "const char ${SYM:-__hip_fatbin_unused}[64] = {0};" > "$B/fatbin_stub.c"
$HIPCC $FLAGS --cuda-host-only -x hip -c "$HERE/hipmock.cpp" -o "$B/hipmock.o"
g++ -O1 -g -std=c++17 -fno-omit-frame-pointer -I "$ROOT/include" -c "$HERE/$NAME.cpp" -o "$B/driver.o"
gcc -c "$B/fatbin_stub.c" -o "$B/fatbin_stub.o"
if [ "$NAME" = abi ]; then
    # the split-precision helpers of cnn.h (scales, two-term fp16 split, cross-term error bound): host-only, no runtime calls
    $HIPCC -O1 -std=c++17 -w --cuda-host-only -x hip "$HERE/splitcheck.cpp" -o "$B/splitcheck" -L/opt/rocm/lib -lamdhip64
    "$B/splitcheck"
fi
/opt/rocm/lib/llvm/bin/clang++ -fsanitize=address "$B/api.o" "$B/hipmock.o" "$B/driver.o" "$B/fatbin_stub.o" -o "$B/hostcheck_$NAME" -lpthread -ldl
ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 "$B/hostcheck_$NAME" "$@"
