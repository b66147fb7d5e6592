#!/bin/bash
# tools/mkvariant.sh NAME [extra hipcc flags...] -- build libvrhip with extra -D flags into
# volumerenderercl_amd/_variants/libvrhip_NAME.so (git-ignored; travels to the GPU box) for
# A/B runs with tools/ab.sh / VRHIP_LIB_PATH.  The units and the flags are the Makefile's.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
make -C "$ROOT/volumerenderercl_amd/csrc" -j8 EXTRA="$*" OBJDIR="_obj/var_$NAME" OUT="../_variants/libvrhip_$NAME.so"
echo "built _variants/libvrhip_$NAME.so"
