#!/bin/bash
# Are the gfx950 kernels of two builds of libaggmg_hip.so the same kernels?  (a host-side refactor must leave them alone)
#   tools/compare_kernels.sh old/libaggmg_hip.so new/libaggmg_hip.so
# Compares, per kernel symbol, the disassembled instruction stream and the metadata note (VGPR, SGPR, scratch, LDS, ...);
# prints one line and exits 0 when the symbol sets and all of that are identical.
set -e
LLVM=/opt/rocm/lib/llvm/bin
tmp=$(mktemp -d /tmp/kcmp.XXXXXX)
trap 'rm -rf $tmp' EXIT
dump() {   # $1 library, $2 output directory: one code object per translation unit -> sorted per-symbol text
  mkdir -p $2
  $LLVM/llvm-objcopy --dump-section .hip_fatbin=$2/fat.bin $1
  python3 - $2/fat.bin $2 <<'PY'
import sys
data = open(sys.argv[1], "rb").read()
magic = b"__CLANG_OFFLOAD_BUNDLE__"
at = [i for i in range(len(data)) if data.startswith(magic, i)]
for n, i in enumerate(at):
    open(f"{sys.argv[2]}/bundle{n}", "wb").write(data[i:at[n + 1] if n + 1 < len(at) else len(data)])
PY
  for b in $2/bundle*; do
    $LLVM/clang-offload-bundler --unbundle --type=o --input=$b --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$b.co
    $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr $b.co | grep -v "file format" >> $2/isa.raw
    $LLVM/llvm-readelf --notes $b.co >> $2/notes.raw
  done
  python3 - $2 <<'PY'
import re, sys
d = sys.argv[1]
# instruction streams keyed by symbol, branch targets kept as the disassembler prints them (symbol + offset)
syms, cur = {}, None
for line in open(f"{d}/isa.raw"):
    m = re.match(r"^<(\S+)>:", line)
    if m:
        cur = m.group(1)
        syms[cur] = []
    elif cur and line.strip():
        syms[cur].append(line.strip())
with open(f"{d}/isa.txt", "w") as f:
    for k in sorted(syms):
        f.write(f"== {k}\n" + "\n".join(syms[k]) + "\n")
# metadata: one block per kernel (from ".name:" of a kernel entry), sorted by symbol
txt = open(f"{d}/notes.raw").read()
blocks = re.split(r"\n(?=\s+- \.agpr_count:|\s+- \.args:)", txt)
kern = {}
for b in blocks:
    m = re.search(r"\.symbol:\s+(\S+)", b)
    if m:
        kern[m.group(1)] = re.sub(r"amdhsa\.target:.*|amdhsa\.version:.*(\n\s+- \d+)*|\.\.\.|---|Displaying notes.*|\s+Owner.*|\s+AMDGPU.*|\s+AMDGPU Metadata.*", "", b).rstrip()
with open(f"{d}/meta.txt", "w") as f:
    for k in sorted(kern):
        f.write(f"== {k}\n{kern[k]}\n")
with open(f"{d}/symbols.txt", "w") as f:
    f.write("\n".join(sorted(kern)) + "\n")
PY
}
dump $1 $tmp/a
dump $2 $tmp/b
rc=0
cmp -s $tmp/a/symbols.txt $tmp/b/symbols.txt || { echo "kernel symbol sets differ"; diff $tmp/a/symbols.txt $tmp/b/symbols.txt | head -20; rc=1; }
cmp -s $tmp/a/isa.txt $tmp/b/isa.txt || { echo "instruction streams differ"; diff $tmp/a/isa.txt $tmp/b/isa.txt | grep "^[<>] ==" | head -20; rc=1; }
cmp -s $tmp/a/meta.txt $tmp/b/meta.txt || { echo "kernel metadata differs"; diff $tmp/a/meta.txt $tmp/b/meta.txt | head -20; rc=1; }
[ $rc = 0 ] && echo "identical: $(wc -l < $tmp/a/symbols.txt) kernels, $(grep -vc '^==' $tmp/a/isa.txt) instructions, metadata (VGPR, SGPR, scratch, LDS) equal"
exit $rc
