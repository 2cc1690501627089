#!/bin/bash
# Are the gfx950 kernels of two builds of libaggmg_hip.so the same kernels?  (a host-side refactor must leave them alone)
#   tools/compare_kernels.sh old/libaggmg_hip.so new/libaggmg_hip.so
# Compares, per kernel symbol and translation unit, the disassembled instruction stream (without the addresses the
# disassembler prints beside it: they move when a kernel is added in front) and the metadata note (VGPR, SGPR, scratch,
# LDS, ...); prints one line and exits 0 when every kernel of the old build is in the new one with all of that identical.
# Kernels only the new build has are additions: counted, not an error.
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
# (a static kernel of a shared header has one copy per translation unit that launches it: #0, #1, ... in file order)
syms, cur, seen = {}, None, {}
for line in open(f"{d}/isa.raw"):
    m = re.match(r"^<(\S+)>:", line)
    if m:
        k = seen.get(m.group(1), 0)
        seen[m.group(1)] = k + 1
        cur = f"{m.group(1)}#{k}"
        syms[cur] = []
    elif cur and line.strip() and line.strip() != "..." and not line.startswith("Disassembly of section"):
        # (the disassembler's own lines between two code objects are not the last kernel's instructions)
        syms[cur].append(re.sub(r"// [0-9A-Fa-f]+:", "//", line.strip()))
with open(f"{d}/isa.txt", "w") as f:
    for k in sorted(syms):
        f.write(f"== {k}\n" + "\n".join(syms[k]) + "\n")
# metadata: one block per kernel (from ".name:" of a kernel entry), sorted by symbol
txt = open(f"{d}/notes.raw").read()
blocks = re.split(r"\n(?=\s+- \.agpr_count:|\s+- \.args:)", txt)
kern, seen = {}, {}
for b in blocks:
    m = re.search(r"\.symbol:\s+(\S+)", b)
    if m:
        k = seen.get(m.group(1), 0)
        seen[m.group(1)] = k + 1
        # (without the note's own header and trailer, which land in the first / last kernel's block of a code object)
        b = re.sub(r"amdhsa\.kernels:|amdhsa\.target:.*|amdhsa\.version:.*(\n\s+- \d+)*|\.\.\.|---|Displaying notes.*|\s+Owner.*|\s+AMDGPU.*|\s+AMDGPU Metadata.*", "", b)
        kern[f"{m.group(1)}#{k}"] = "\n".join(l for l in b.splitlines() if l.strip())
with open(f"{d}/meta.txt", "w") as f:
    for k in sorted(kern):
        f.write(f"== {k}\n{kern[k]}\n")
with open(f"{d}/symbols.txt", "w") as f:
    f.write("\n".join(sorted(kern)) + "\n")
PY
}
dump $1 $tmp/a
dump $2 $tmp/b
python3 - $tmp/a $tmp/b <<'PY'
import sys
def load(p):
    d, cur = {}, None
    for line in open(p):
        if line.startswith("== "):
            cur = line[3:].strip()
            d[cur] = []
        else:
            d[cur].append(line)
    return d
a, b = sys.argv[1], sys.argv[2]
rc = 0
ia, ib, ma, mb = load(f"{a}/isa.txt"), load(f"{b}/isa.txt"), load(f"{a}/meta.txt"), load(f"{b}/meta.txt")
gone = sorted(k for k in ia if k not in ib)
if gone:
    print(f"{len(gone)} kernels of the old build are missing from the new one:", *gone[:20], sep="\n  ")
    rc = 1
for what, x, y in (("instruction streams differ", ia, ib), ("kernel metadata differs", ma, mb)):
    bad = sorted(k for k in x if k in y and x[k] != y[k])
    if bad:
        print(f"{what} in {len(bad)} kernels:", *bad[:20], sep="\n  ")
        rc = 1
added = sorted(k for k in ib if k not in ia)
if rc == 0:
    print(f"identical: {len(ia)} kernels, {sum(map(len, ia.values()))} instructions, metadata (VGPR, SGPR, scratch, LDS) equal"
          + (f"; {len(added)} kernels added" if added else ""))
    for k in added:
        print("  +", k)
sys.exit(rc)
PY
