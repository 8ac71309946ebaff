#!/bin/bash
# A/B build of libisls_hip.so with extra compiler flags into ab/<name>/ (git-ignored; select with ISLS_HIP_LIB).  The sources,
# families and flags are the Makefile's (csrc/Makefile, OUT= and EXTRA_CXXFLAGS=):
#     tools/ab_build.sh diag -DISLS_DIAG                       everything rebuilt with the flags
#     ISLS_AB_ONLY="riccati" tools/ab_build.sh g1 -DFOO=1      only riccati.hip rebuilt, the other objects taken from the in-tree build
#                                                              ("rollout_f": the rollout family objects)
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/ilqr-admm_amd/csrc
out=$root/ab/$name
mkdir -p "$out"
if [[ -n "$ISLS_AB_ONLY" ]]; then
  cp -p "$csrc"/*.o "$out"/                    # with their times: make keeps what is up to date ...
  for s in $ISLS_AB_ONLY; do rm -f "$out/$s.o" "$out/$s"_[0-9]*.o; done      # ... and rebuilds what is named
  make -C "$csrc" -j5 OUT="$out" EXTRA_CXXFLAGS="$*"
else
  make -C "$csrc" -j5 -B OUT="$out" EXTRA_CXXFLAGS="$*"
fi
echo "$out/libisls_hip.so"
