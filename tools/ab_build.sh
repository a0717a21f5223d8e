#!/bin/bash
# A/B builds of the library with extra macros for ONE source file:
#   tools/ab_build.sh <tag> <source.hip> [-DNAME=VALUE ...]   ->  exblas_amd/lib/ab/libexblas_<tag>.so
# Sources and flags are those of exblas_amd/build.py.  The other objects are compiled once into /tmp/exblas_ab_objs
# and reused.  Load with EXBLAS_AMD_LIB=<path>.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TAG=$1; SRC=$2; shift 2
CFG=$(cd "$ROOT/exblas_amd" && python3 -c 'import build; print(" ".join(build.SOURCES)); print(" ".join(build.FLAGS))')
SOURCES=$(echo "$CFG" | sed -n 1p); FLAGS=$(echo "$CFG" | sed -n 2p)
case " $SOURCES " in *" $SRC "*) ;; *) echo "ab_build.sh: $SRC is not one of: $SOURCES" >&2; exit 2 ;; esac
OBJ=/tmp/exblas_ab_objs; mkdir -p $OBJ $ROOT/exblas_amd/lib/ab
for s in $SOURCES; do
  o=$OBJ/${s//./_}.o
  if [ "$s" != "$SRC" ] && { [ ! -f $o ] || [ $ROOT/exblas_amd/csrc/$s -nt $o ]; }; then
    hipcc $FLAGS -x hip -c $ROOT/exblas_amd/csrc/$s -o $o &
  fi
done
hipcc $FLAGS "$@" -x hip -c $ROOT/exblas_amd/csrc/$SRC -o $OBJ/${SRC//./_}.$TAG.o
wait
objs=""
for s in $SOURCES; do
  if [ "$s" = "$SRC" ]; then objs="$objs $OBJ/${s//./_}.$TAG.o"; else objs="$objs $OBJ/${s//./_}.o"; fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/exblas_amd/lib/ab/libexblas_$TAG.so $objs
echo $ROOT/exblas_amd/lib/ab/libexblas_$TAG.so
