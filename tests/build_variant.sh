#!/bin/bash
# builds a variant of the library for A/B runs on one box:  tests/build_variant.sh NAME -DFLAG...   -> nlzm_amd/libnlzm_hip_NAME.so
# (the product's own build -- every object, the Makefile's flags -- under another name, from objects in a directory of its own)
set -e
name=$1; shift
cd "$(dirname "$0")/../nlzm_amd/csrc"
d=$(mktemp -d); trap 'rm -rf "$d"' EXIT
make -j8 OBJDIR="$d" LIB="libnlzm_hip_$name.so" EXTRA="$*" "../libnlzm_hip_$name.so"
