#!/usr/bin/env python3
"""Dev tool: compare every gfx950 kernel of TWO builds of libasq_hip.so (a refactor's check that the device code did not move).

usage: python tools/kernel_diff.py parent/libasq_hip.so head/libasq_hip.so [--all] > table.txt

Per kernel (matched by code object and mangled name): the resource figures of the ELF notes (VGPR, AGPR, SGPR, scratch, VGPR / SGPR spills, static LDS), parent next to head,
and the disassembly (llvm-objdump -d, text left of the address comment):
  code    "same"  the instruction stream is identical
          "tail"  it is identical up to and including the last matrix instruction (branch targets aside) and differs behind it
          "LOOP"  it differs before the last matrix instruction (kernels without one: anywhere)
  tail    instructions behind the last matrix instruction, parent / head
Without --all only kernels whose figures or code differ are listed; then one line per kernel family (the function template's name) with the sums of
those figures and instruction counts over its kernels, parent | head, and a last line that counts all kernels.  Exit status 1 if any kernel is missing on one side,
differs in its figures or is marked LOOP."""
import os, re, shutil, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIGS = ["vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size"]
BRANCH = re.compile(r"^(s_branch|s_cbranch_\w+|s_call_b64\s+\S+,)\s+\S+")


def kernels(path):
    """{(code object index, mangled name): (figures, [instructions])}"""
    td = tempfile.mkdtemp()
    out = {}
    try:
        so = os.path.join(td, "lib.so")
        shutil.copy(path, so)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", so], check=True, capture_output=True, cwd=td)
        for idx, o in enumerate(sorted(p for p in os.listdir(td) if "gfx950" in p)):
            co = os.path.join(td, o)
            figs = {}
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                cur = {"agpr_count": blk.split("\n", 1)[0].strip()}
                for line in blk.splitlines():
                    m = re.match(r"\s*\.(\w+):\s+(\S+)", line)
                    if m and m.group(1) not in cur:
                        cur[m.group(1)] = m.group(2)
                if cur.get("name") and cur.get("vgpr_count"):
                    figs[cur["name"]] = tuple(cur.get(f, "0") for f in FIGS)
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
            name = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    name = m.group(1)
                    if name in figs:
                        out[(idx, name)] = (figs[name], [])
                    continue
                if name in figs and line.startswith(("\t", " ")):
                    ins = line.split("//")[0].strip()
                    if ins:
                        out[(idx, name)][1].append(ins)
    finally:
        shutil.rmtree(td, ignore_errors=True)
    return out


def last_mfma(code):
    for i in range(len(code) - 1, -1, -1):
        if code[i].startswith(("v_mfma", "v_smfma")):
            return i
    return -1


def main():
    args = [a for a in sys.argv[1:] if a != "--all"]
    show_all = "--all" in sys.argv
    a, b = kernels(args[0]), kernels(args[1])
    names = sorted(set(a) | set(b), key=lambda k: (k[0], k[1]))
    demangled = dict(zip([n for _, n in names], subprocess.run(["c++filt"], input="\n".join(n for _, n in names), capture_output=True, text=True).stdout.splitlines()))
    print("figures: vgpr agpr sgpr scratch vgpr-spill sgpr-spill lds   (parent | head)")
    count = {"same": 0, "tail": 0, "LOOP": 0, "figures": 0, "missing": 0}
    fam = {}   # family -> [kernels, same, tail, LOOP, figure sums parent, figure sums head, tail sum parent, tail sum head]
    for key in names:
        dem = demangled.get(key[1], key[1])[:150]
        if key not in a or key not in b:
            count["missing"] += 1
            print(f"MISSING in {'parent' if key not in a else 'head'}: [{key[0]}] {dem}")
            continue
        (fa, ca), (fb, cb) = a[key], b[key]
        la, lb = last_mfma(ca), last_mfma(cb)
        if ca == cb:
            code = "same"
        elif la >= 0 and la == lb and [BRANCH.sub(r"\1 L", i) for i in ca[:la + 1]] == [BRANCH.sub(r"\1 L", i) for i in cb[:lb + 1]]:
            code = "tail"
        else:
            code = "LOOP"
        count[code] += 1
        if fa != fb:
            count["figures"] += 1
        f = fam.setdefault(re.split(r"[<(]", dem.replace("void ", ""))[0], [0, 0, 0, 0, [0] * len(FIGS), [0] * len(FIGS), 0, 0])
        f[0] += 1
        f[1 + ["same", "tail", "LOOP"].index(code)] += 1
        f[4], f[5] = [x + int(y) for x, y in zip(f[4], fa)], [x + int(y) for x, y in zip(f[5], fb)]
        f[6], f[7] = f[6] + len(ca) - la - 1, f[7] + len(cb) - lb - 1
        if show_all or code != "same" or fa != fb:
            print(f"{' '.join(fa):>26} | {' '.join(fb):>26} {'' if fa == fb else 'FIGURES'} code {code}  tail {len(ca) - la - 1:5d} / {len(cb) - lb - 1:5d}  [{key[0]}] {dem}")
    print("per family: kernels same/tail/LOOP | sums over the family: figures parent | figures head | instructions behind the last matrix instruction parent / head")
    for name, f in sorted(fam.items()):
        print(f"{name:34s} {f[0]:4d} {f[1]:4d}/{f[2]}/{f[3]} | {' '.join(map(str, f[4])):>34} | {' '.join(map(str, f[5])):>34} | {f[6]:8d} / {f[7]:8d}")
    print(f"{len(names)} kernels: {count['same']} identical, {count['tail']} differ behind the last matrix instruction only, {count['LOOP']} differ before it, "
          f"{count['figures']} differ in their figures, {count['missing']} present on one side only")
    return 1 if count["LOOP"] or count["figures"] or count["missing"] else 0


if __name__ == "__main__":
    sys.exit(main())
