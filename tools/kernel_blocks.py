#!/usr/bin/env python3
"""Basic blocks of one gfx950 kernel with their instruction counts by class, for counting the instructions on a path by
hand (profiles/r26_element_threads.md was made this way).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -c -o k.bundle aggmg_hip.hip
    clang-offload-bundler --unbundle --type=o --input=k.bundle --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=k.co
    llvm-objdump -d k.co > k.s          (with the raw encodings: the comment carries each address)
    tools/kernel_blocks.py k.s SYMBOL_SUBSTRING [--path B0,B2,B5x3,...]

Prints one line per block: name, address, instructions, VALU (v_*), of them fp64 arithmetic (v_fma/fmac/mul/add_f64), memory
(global / ds), SALU, and where it goes (fall-through and branch target).  --path sums the listed blocks (BnxK: K times)."""
import re
import sys


def blocks(path, sym):
    ins = []   # (address, text, branch target or None)
    on, base = False, 0
    for line in open(path):
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            if on:
                break
            on, base = sym in m.group(2), int(m.group(1), 16)
            continue
        if on:
            # "\tinsn operands   // 0000000A1470: BF8704FE <symbol+0x146c>" (the target of a branch, as the disassembler resolves it)
            m = re.match(r"^\s+(\S.*?)\s+// ([0-9A-Fa-f]+):[0-9A-Fa-f ]*(?:<\S+\+0x([0-9a-f]+)>)?\s*$", line)
            if m:
                ins.append((int(m.group(2), 16), m.group(1), base + int(m.group(3), 16) if m.group(3) else None))
    if not ins:
        sys.exit(f"no kernel matching {sym}")
    addr = [a for a, _, _ in ins]
    target = {a: to for a, t, to in ins if to is not None and re.match(r"^s_c?branch", t)}
    ins = [(a, t) for a, t, _ in ins]
    leaders = {addr[0]} | set(target.values())
    for k, (a, t) in enumerate(ins):
        if (a in target or t.startswith("s_endpgm")) and k + 1 < len(ins):
            leaders.add(addr[k + 1])
    out, cur = [], None
    for a, t in ins:
        if a in leaders:
            cur = dict(addr=a, ins=[], to=None, fall=True)
            out.append(cur)
        cur["ins"].append(t)
        if a in target:
            cur["to"] = target[a]
            cur["fall"] = not t.startswith("s_branch")
        if t.startswith("s_endpgm"):
            cur["fall"] = False
    return out


def classify(b):
    v = [t for t in b["ins"] if t.startswith("v_")]
    return dict(total=len(b["ins"]), valu=len(v),
                f64=sum(1 for t in v if re.match(r"v_(fmac?|mul|add)_f64", t)),
                mem=sum(1 for t in b["ins"] if t.startswith(("global_", "ds_", "buffer_", "flat_", "scratch_"))),
                salu=sum(1 for t in b["ins"] if t.startswith("s_")),
                bar=sum(1 for t in b["ins"] if t.startswith("s_barrier")))


def main():
    bl = blocks(sys.argv[1], sys.argv[2])
    name = {b["addr"]: f"B{k}" for k, b in enumerate(bl)}
    tot = {}
    for k, b in enumerate(bl):
        c = classify(b)
        tot[f"B{k}"] = c
        nxt = name.get(bl[k + 1]["addr"]) if b["fall"] and k + 1 < len(bl) else None
        print(f"B{k:<3d} {b['addr']:6x} total {c['total']:4d} valu {c['valu']:4d} f64 {c['f64']:3d} mem {c['mem']:3d} "
              f"salu {c['salu']:3d} bar {c['bar']}  -> {nxt or '-'} / {name.get(b['to'], '-') if b['to'] is not None else '-'}"
              f"   [{b['ins'][-1]}]")
    print("static:", {k: sum(c[k] for c in tot.values()) for k in ("total", "valu", "f64", "mem", "salu")})
    if "--path" in sys.argv:
        s = dict(total=0, valu=0, f64=0, mem=0, salu=0)
        for item in sys.argv[sys.argv.index("--path") + 1].split(","):
            n, _, k = item.partition("x")
            for key in s:
                s[key] += tot[n][key] * int(k or 1)
        print("path:", s)


if __name__ == "__main__":
    main()
