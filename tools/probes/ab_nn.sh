#!/bin/bash
# tools/probes/ab_nn.sh <unit> "<-D flags>" ...: for each flag set rebuild ONLY salsa_amd/csrc/<unit>.hip -- nn_batchnorm, nn_pool,
# nn_reduce, nn_loss or nn_optim -- (the other objects are prebuilt under salsa_amd/lib/obj: tools/dev_build.sh), link, run the
# CRNN training bench
UNIT=$(basename "$1" .hip); shift
for FLAGS in "$@"; do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $FLAGS -c -o /tmp/$UNIT.o salsa_amd/csrc/$UNIT.hip 2>/dev/null || { echo BUILD FAIL; exit 1; }
  hipcc --offload-arch=gfx950 -shared -fPIC -o salsa_amd/lib/libsalsa_hip.so /tmp/$UNIT.o $(ls salsa_amd/lib/obj/*.o | grep -v /$UNIT.o) || { echo LINK FAIL; exit 1; }
  python bench_crnn.py --steps 20 --warmup 5 2>/dev/null | tail -1 | python -c "
import sys,json; d=json.loads(sys.stdin.read()); print('$FLAGS', '|', d['value'], 'chunks/s', d['ms_per_step'], 'ms')"
done
