#!/bin/bash
# A host twin's stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer: the host library's sources - the build
# entry's HOST_SRCS, with its exact-arithmetic flags: the one list there is - and tools/sanitize_NAME.c (a program with its own
# main) built with -fsanitize=address,undefined into one executable, which is run from the repository root on the monkey bust.
# CPU only; nothing is loaded into python. tools/sanitize_{box,obox,capsule,frustum,point}_query.sh and tools/sanitize_pose.sh call it.
#   tools/sanitize_standalone.sh NAME
set -e
NAME=$1
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build/san
cd $R
SRCS=$(python3 -c 'import __graft_entry__ as ge; print(*ge.HOST_SRCS)')
EXACT=$(python3 -c 'import __graft_entry__ as ge; print(*ge.EXACT_FLAGS)')
SAN="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
gcc -std=c11 $SAN -Wall -I $R/include -c -o $R/build/san/sanitize_$NAME.o $R/tools/sanitize_$NAME.c
g++ -std=c++17 $SAN $EXACT -Wall -o $R/build/san/sanitize_$NAME $R/build/san/sanitize_$NAME.o $SRCS -ldl -lm
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 $R/build/san/sanitize_$NAME $R/assets/monkey_bust.glb
