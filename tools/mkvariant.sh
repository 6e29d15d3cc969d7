#!/bin/bash
# build a variant of libnae_gpu.so for A/B timing:  tools/mkvariant.sh TAG [extra stft flags...]
# e.g. tools/mkvariant.sh slp  (re-enables SLP)   tools/mkvariant.sh x -DNAE_FOO=1
# The translation units and their flags are the Makefile's (SRC, HIPFLAGS, NOSLP).  The extra flags (+slp: drop -fno-slp-vectorize) apply to
# the STFT, transposer, pipeline and spectrum TUs; SRC_STFT / SRC_PVPIPE: a patched copy in place of kernels_stft.hip / kernels_pvpipe.hip (tools/experiments).
set -e
TAG=$1; shift
D=$(cd "$(dirname "$0")/../nodey-audio-editor_amd" && pwd)
mk() { make -s --no-print-directory -C "$D" "print-$1"; }
HIPCC=$(mk HIPCC); ARCH=$(mk ARCH); HIPFLAGS=$(mk HIPFLAGS); NOSLP=" $(mk NOSLP) "
STFT="-fno-slp-vectorize"
for a in "$@"; do
  if [ "$a" == "+slp" ]; then STFT=""; else STFT="$STFT $a"; fi
done
O=$(mktemp -d); trap 'rm -rf "$O"' EXIT
pids=(); objs=()
for f in $(mk SRC); do
  n=$(basename "$f" .hip); src=$D/$f
  case $n in
    kernels_stft)   src=${SRC_STFT:-$src};   fl="$STFT -I$D/csrc" ;;
    kernels_pvpipe) src=${SRC_PVPIPE:-$src}; fl="$STFT -I$D/csrc" ;;
    kernels_spectrum|kernels_resample) fl="$STFT" ;;
    *) if [[ "$NOSLP" == *" $f "* ]]; then fl="-fno-slp-vectorize"; else fl="$NODEFLAGS"; fi ;;
  esac
  $HIPCC $HIPFLAGS $fl -c "$src" -o "$O/$n.o" &
  pids+=($!); objs+=("$O/$n.o")
done
for p in "${pids[@]}"; do wait "$p"; done   # (set -e: a TU that fails to compile ends the script)
mkdir -p "$D/variants"
$HIPCC --offload-arch=$ARCH -shared -fPIC -o "$D/variants/libnae_gpu_$TAG.so" "${objs[@]}"
echo built $D/variants/libnae_gpu_$TAG.so
