#!/bin/bash
# Build libvitmi.so from a modified copy of csrc/ for A/B kernel timing (load it with VITMI_LIB):
#   [VARIANT_FLAGS=-D...] tools/build_variant.sh NAME SRC_DIR   -> transformer-stm_amd/variants/NAME.so
# SRC_DIR must sit two levels below a directory holding include/ (mirror of the repo layout).
# The source list and the per-file flags are the Makefile's.
set -e
name=$1; src=$(cd "$2" && pwd)
pkg=$(cd "$(dirname "$0")/../transformer-stm_amd" && pwd)
mkdir -p "$pkg/variants"
make -C "$pkg" -j16 CSRC="$src" BUILD="build-exp/$name" LIB="variants/$name.so" VARIANT_FLAGS="$VARIANT_FLAGS"
echo built "$pkg/variants/$name.so"
