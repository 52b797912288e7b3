#!/bin/bash
# A/B builds of libpcops: tools/build_variant.sh NAME "-DFLAG=1 ..."  ->  scanobjectnn_amd/libpcops_NAME.so
# (run a benchmark against it with PCOPS_LIB=$PWD/scanobjectnn_amd/libpcops_NAME.so; *.so is git-ignored).  The default
# library is untouched.  The recipe is csrc/Makefile's -- the product's sources and translation units -- with the flags
# added and the objects kept in a directory of the variant's own; changed flags rebuild everything.
set -e
NAME=$1; shift
EXTRA="$*"
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OBJ=/tmp/pcops_variant_$NAME
mkdir -p $OBJ
echo "$EXTRA" > $OBJ/flags.new
if ! cmp -s $OBJ/flags.new $OBJ/flags 2>/dev/null; then rm -f $OBJ/*.o; cp $OBJ/flags.new $OBJ/flags; fi
make -C $ROOT/scanobjectnn_amd/csrc -j"${MAX_JOBS:-8}" EXTRA="$EXTRA" OBJDIR=$OBJ LIB=../libpcops_$NAME.so
echo built $ROOT/scanobjectnn_amd/libpcops_$NAME.so
