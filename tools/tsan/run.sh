#!/bin/bash
# Host ThreadSanitizer run of the rule compiler under concurrent compiles
# (tools/tsan/tsan_main.cpp).  CPU only: no GPU code is built or run.
# usage: tools/tsan/run.sh   (or: make -C vpp_amd/csrc tsan)
set -e -o pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
OUT=${TMPDIR:-/tmp}/contivcls_tsan
mkdir -p $OUT
python3 $ROOT/tools/asan/dump_acls.py $OUT/acls.txt
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# .cpp units: hipcc compiles them as host C++ (no device side to sanitize)
SAN="-O1 -g -std=c++17 -fsanitize=thread -fno-omit-frame-pointer"
OBJS=
PIDS=
for src in tools/tsan/tsan_main.cpp vpp_amd/csrc/compile.cpp vpp_amd/csrc/options.cpp; do
    o=$OUT/$(basename $src).o
    $HIPCC $SAN -I$ROOT/include -c -o $o $ROOT/$src &
    PIDS="$PIDS $!"
    OBJS="$OBJS $o"
done
for p in $PIDS; do wait $p; done
$HIPCC -fsanitize=thread -o $OUT/tsan_main $OBJS
# a report ends the run with status 1, like a difference
TSAN_OPTIONS=exitcode=1:halt_on_error=0:second_deadlock_stack=1 $OUT/tsan_main $OUT/acls.txt 2>&1 | tee $OUT/run.log | tail -40
