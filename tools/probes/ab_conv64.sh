#!/bin/bash
# tools/probes/ab_conv64.sh <unit> "<-D flags>" ...: rebuild ONLY salsa_amd/csrc/<unit>.hip -- conv_mfma, conv_stem, conv_c64_wrw or
# conv_stem_wrw -- per flag set (other objects prebuilt under salsa_amd/lib/obj: tools/dev_build.sh), run the wrw probe (PROBE=<another>)
UNIT=$(basename "$1" .hip); shift
for FLAGS in "$@"; do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $FLAGS -c -o /tmp/$UNIT.o salsa_amd/csrc/$UNIT.hip 2>/dev/null || { echo BUILD FAIL; exit 1; }
  hipcc --offload-arch=gfx950 -shared -fPIC -o salsa_amd/lib/libsalsa_hip.so /tmp/$UNIT.o $(ls salsa_amd/lib/obj/*.o | grep -v /$UNIT.o) || { echo LINK FAIL; exit 1; }
  echo "== $FLAGS"; python tools/probes/${PROBE:-wrw64_probe.py} 2>&1 | grep -E "wrw64|conv64"
done
