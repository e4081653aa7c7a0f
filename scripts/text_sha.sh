#!/bin/bash
# usage: scripts/text_sha.sh <build dir>  -- per unit: sha256 (16 hex) and bytes of the .text of its gfx950 code object.  A host-only
# change leaves every line as it was (the whole code object is not comparable: it changes with the output path; .text does not).
B=/opt/rocm/lib/llvm/bin
for o in "$1"/*.o; do
  u=$(basename "$o" .o); [ "$u" = abi ] && continue
  T=$(mktemp -d)
  $B/llvm-objcopy --dump-section .hip_fatbin=$T/fat.bin "$o" 2>/dev/null
  $B/clang-offload-bundler --unbundle --type=o --input=$T/fat.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/k.co 2>/dev/null
  $B/llvm-objcopy -O binary --only-section=.text $T/k.co $T/text.bin
  echo "$u $(sha256sum $T/text.bin | cut -c1-16) $(stat -c %s $T/text.bin)"
  rm -rf $T
done
