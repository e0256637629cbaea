#!/bin/bash
# Compares the gfx950 device code of two builds of the library (two csrc/build directories of objects), unit by unit: the disassembly
# of every kernel and its resource notes (vgpr_count, sgpr_count, spill counts, private_segment_fixed_size, group_segment_fixed_size).
# Prints, per unit, `same` or the mangled names of the kernels that differ; exit status 1 if any does.  How a refactoring of the
# kernel sources shows that it moved no instance's code (no GPU needed).   tools/isa_diff.sh <build dir A> <build dir B>
B=/opt/rocm/lib/llvm/bin
[ -d "$1" ] && [ -d "$2" ] || { echo "usage: $0 <build dir A> <build dir B>" >&2; exit 2; }
T=$(mktemp -d)
# one line per kernel: name, checksum of its instructions (addresses dropped, encodings kept), its resource notes
sig() {
  $B/llvm-objcopy --dump-section .hip_fatbin=$T/x.fat "$1" 2>/dev/null || return 1
  $B/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$T/x.fat --output=$T/x.elf 2>/dev/null || return 1
  $B/llvm-objdump -d $T/x.elf | sed -E 's#// [0-9A-F]+:#//#' | awk -v dir=$T/k '
    /^[0-9a-f]+ <.*>:$/ { if (f) close(f); name = $2; gsub(/[<>:]/, "", name); f = dir "/" (++n); print name > (dir "/names"); next }
    f && !/^[ \t]*(\.\.\.)?$/ { print > f }'   # (without the "..." that stands for the padding behind the last kernel of a unit: the kernels may come in another order)
  n=0
  while read -r name; do n=$((n + 1)); echo "$name code $(md5sum < $T/k/$n | cut -d" " -f1)"; done < $T/k/names
  $B/llvm-readelf --notes $T/x.elf | awk '
    /^  - \./ { if (name) print name, "notes", r; name = ""; r = "" }
    /^ +(- )?\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):/ { r = r " " $(NF - 1) $NF }
    /^ +\.name:/ { name = $2 }
    END { if (name) print name, "notes", r }'
}
rc=0
for a in "$1"/*.o; do
  u=$(basename "$a" .o)
  [ -f "$2/$u.o" ] || { echo "$u: only in $1"; rc=1; continue; }
  rm -rf $T/k; mkdir $T/k; sig "$a" | sort > $T/a.sig; ok=$?
  rm -rf $T/k; mkdir $T/k; sig "$2/$u.o" | sort > $T/b.sig
  if [ ! -s $T/a.sig ] && [ ! -s $T/b.sig ]; then echo "$u: same (no gfx950 code)"; continue; fi
  d=$(diff $T/a.sig $T/b.sig | awk '/^[<>]/ { print $2 }' | sort -u)
  if [ -z "$d" ]; then echo "$u: same ($(grep -c " code " $T/a.sig) kernels)"; else echo "$u: DIFFERS"; echo "$d" | sed 's/^/    /'; rc=1; fi
done
for b in "$2"/*.o; do [ -f "$1/$(basename "$b")" ] || { echo "$(basename "$b" .o): only in $2"; rc=1; }; done
rm -rf $T
exit $rc
