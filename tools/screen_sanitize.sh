#!/bin/bash
# Builds the library's host layer (stm_runtime, stm_api, stm_stream, stm_dropin) with AddressSanitizer + UndefinedBehaviorSanitizer
# on the HOST side only (-Xarch_host: device code is compiled as always and never runs here) into tools/build/, links
# tools/screen_sanitize.cpp against them and the product build's kernel objects, and runs it: the argument screens' varargs
# helper, its buffer and the name lists of the null-pointer rule under the sanitizers.  Needs no GPU and loads nothing into
# Python.  Any sanitizer report or unexpected answer fails the run.
set -e
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SRC=stereo-to-multiview-cuda_amd/csrc
OUT=tools/build/screen_sanitize
FLAGS="--offload-arch=gfx950 -O3 -g -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -DSTM_BUILD"
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer"
make -s -j"${JOBS:-8}" -C $SRC all   # the kernel objects, as the product has them
mkdir -p $OUT
for f in stm_runtime stm_api stm_stream stm_dropin; do $HIPCC $FLAGS $SAN -c $SRC/$f.hip -o $OUT/$f.o & done
$HIPCC $FLAGS $SAN -x hip -c tools/screen_sanitize.cpp -o $OUT/main.o &
wait
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined $OUT/*.o $SRC/build/stm_kernels_*.o $SRC/build/stm_bmp.o -o $OUT/screen_sanitize
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $OUT/screen_sanitize
