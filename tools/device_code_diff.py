"""Device code of two libalipmpc.so builds, function by function: the gfx950 code objects embedded in each library (one
per translation unit) are unbundled and disassembled, and every function of the first build is compared with the
second's as instruction text (alignment padding behind a function left out).  Classes: equal; 'pc-relative only' (the
differing instructions are the literals that follow an s_getpc_b64: the address of a called, not inlined device
function, which moves when a unit gains code); 'id only' (a differing s_mov_b32 literal, e.g. a dynamic-LDS table
index); differ; missing.  No GPU needed.

  python tools/device_code_diff.py PARENT/libalipmpc.so HEAD/libalipmpc.so WORKDIR > profiles/<pr>/device_code_vs_parent.txt
"""
import collections
import os
import re
import subprocess
import sys

LLVM = os.environ.get("ALIPMPC_LLVM_BIN", "/opt/rocm/llvm/bin")
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
OBJCOPY = os.path.join(LLVM, "llvm-objcopy")
BUNDLER = os.path.join(LLVM, "clang-offload-bundler")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, work):
    os.makedirs(work, exist_ok=True)
    fat = os.path.join(work, "fatbin")
    subprocess.check_call([OBJCOPY, "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    outs = []
    for i, s in enumerate(starts):
        e = starts[i + 1] if i + 1 < len(starts) else len(data)
        b = os.path.join(work, f"bundle{i}")
        open(b, "wb").write(data[s:e])
        co = os.path.join(work, f"co{i}.elf")
        subprocess.check_call([BUNDLER, "--unbundle", "--type=o", f"--input={b}", f"--output={co}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        outs.append(co)
    return outs


def functions(co):
    """{symbol: [instruction text]} of a code object"""
    txt = subprocess.check_output([OBJDUMP, "-d", "--no-show-raw-insn", co], text=True)
    fn, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            fn[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        ins = re.sub(r"\s*//.*$", "", line).strip()
        if ins:
            fn[cur].append(ins)
    for k in fn:   # alignment padding behind a function's last instruction belongs to the layout, not to the function
        while fn[k] and fn[k][-1] in ("s_nop 0", "..."):
            fn[k].pop()
    # prologue<N, WT> became prologue<N, MAP, WT>: both builds' prologue<N[, false], WT> under one name
    return {re.sub(r"^(_ZN4alip8prologueILi\d+E)(Lb0E)?(NS_3WSS.*?)RKT[01]_(.*?)(Pj)?$", r"\1\3RKT_\4", k): v
            for k, v in fn.items()}


def diff_kind(a, b):
    if a == b:
        return "equal", 0
    if len(a) != len(b):
        return "differ", abs(len(a) - len(b))
    d = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    # pc-relative address of a called (not inlined) device function: s_getpc_b64 then s_add_u32 / s_addc_u32 literals
    def pcrel(i):
        return any(a[j].startswith("s_getpc_b64") for j in range(max(0, i - 3), i)) and \
            re.match(r"s_addc?_u32 ", a[i]) and re.match(r"s_addc?_u32 ", b[i])
    if all(pcrel(i) for i, _, _ in d):
        return "pc-relative only", len(d)
    if all(re.match(r"s_mov_b32 s\d+, (0x[0-9a-f]+|\d+)$", x) and re.match(r"s_mov_b32 s\d+, (0x[0-9a-f]+|\d+)$", y)
           and x.split(",")[0] == y.split(",")[0] for _, x, y in d if not pcrel(_)):
        return "id only", len(d)
    return "differ", len(d)


def main(parent, head, work):
    P = [functions(c) for c in code_objects(parent, os.path.join(work, "parent"))]
    Hd = [functions(c) for c in code_objects(head, os.path.join(work, "head"))]
    assert len(P) == len(Hd), (len(P), len(Hd))
    for k, (p, h) in enumerate(zip(P, Hd)):
        kinds = collections.defaultdict(list)
        for name, ins in p.items():
            if name not in h:
                kinds["missing"].append((name, 0))
            else:
                kd, n = diff_kind(ins, h[name])
                kinds[kd].append((name, n))
        new = sorted(set(h) - set(p))
        print(f"code object {k}: {len(p)} functions in the parent: {len(kinds['equal'])} equal, "
              f"{len(kinds['pc-relative only'])} pc-relative only, {len(kinds['id only'])} id only, "
              f"{len(kinds['differ'])} differ, {len(kinds['missing'])} missing; {len(new)} new")
        for kd in ("pc-relative only", "id only", "differ", "missing"):
            for name, n in sorted(kinds[kd]):
                print(f"  {kd} ({n}): {name}")
        kn = collections.Counter(re.sub(r"I.*", "", n) for n in new)
        for n, c in sorted(kn.items()):
            print(f"  new: {c} x {n}")


if __name__ == "__main__":
    main(*sys.argv[1:4])
