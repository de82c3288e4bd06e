#!/usr/bin/env python3
"""Static instruction classes of the solve kernels in a device-only assembly listing.

    hipcc --offload-arch=gfx950 <build flags> -DALIP_PART=3 -DALIP_DEV_ONLY_KSM=10 --cuda-device-only -S -o part3.s csrc/alipmpc.hip
    python tools/isa_classes.py part3.s [kernel-name-substring ...]

For every matching kernel: the code-object figures (VGPRs, scratch, code bytes are in the metadata; here the
instruction count stands in for size) and the instruction classes of the whole kernel and of its largest loop (the
widest backward branch span — the interior-point loop of a one-instance-per-wave build).  No GPU involved.
"""
import re
import sys
from collections import Counter

FP = ("v_fma_f64", "v_fmac_f64", "v_add_f64", "v_mul_f64", "v_max_f64", "v_min_f64", "v_rcp_f64", "v_rsq_f64",
      "v_sqrt_f64", "v_ldexp_f64", "v_frexp", "v_cvt", "v_rndne_f64", "v_div_", "v_trig_preop")


def classify(op):
    if op.endswith("_dpp") or op.startswith("v_mov_b64_dpp"):
        return "dpp"
    if op.startswith(("v_readlane", "v_readfirstlane")):
        return "readlane"
    if op.startswith("v_permlane"):
        return "permlane"
    if op.startswith(("v_mov", "v_accvgpr", "v_swap")):
        return "v_mov"
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith(("v_mfma", "v_smfma")):
        return "mfma"
    if op.startswith(FP):
        return "fp64/cvt"
    if op.startswith("v_cmp"):
        return "v_cmp"
    if op.startswith("v_"):
        return "valu other"
    if op in ("s_nop",):
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith(("global_", "flat_", "buffer_")):
        return "vmem"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu/smem"
    return "other"


def kernels(path):
    name, body, meta = None, [], {}
    out = {}
    fn = re.compile(r"^(_Z\w+):")
    for line in open(path):
        m = fn.match(line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = line.strip()
        if s.startswith(".amdhsa_kernel"):
            meta = {}
        elif s.startswith(".amdhsa_next_free_vgpr"):
            meta["vgpr"] = int(s.split()[1])
        elif s.startswith(".amdhsa_accum_offset"):
            meta["accum_offset"] = int(s.split()[1])
        elif s.startswith(".amdhsa_private_segment_fixed_size"):
            meta["scratch"] = int(s.split()[1])
        elif s.startswith(".end_amdhsa_kernel"):
            out[name] = (body, meta)
            name = None
        elif s.startswith(".L") and s.endswith(":"):
            body.append(("label", s[:-1]))
        elif s and not s.startswith((".", ";")):
            op = s.split()[0]
            if op.startswith(("s_", "v_", "ds_", "global_", "scratch_", "flat_", "buffer_")):
                tgt = s.split()[1] if op.startswith(("s_cbranch", "s_branch")) else None
                body.append((op, tgt, "dpp" in s or "row_newbcast" in s))
    return out


def count(ins):
    c = Counter()
    for i in ins:
        if i[0] == "label":
            continue
        c["dpp" if i[2] and i[0].startswith("v_") else classify(i[0])] += 1
    return c


def widest_loop(body):
    pos = {i[1]: k for k, i in enumerate(body) if i[0] == "label"}
    best = (0, 0)
    for k, i in enumerate(body):
        if i[0] != "label" and i[1] in pos and pos[i[1]] < k and k - pos[i[1]] > best[1] - best[0]:
            best = (pos[i[1]], k)
    return body[best[0]:best[1] + 1]


def main():
    ks = kernels(sys.argv[1])
    pats = sys.argv[2:] or ["solve_kernel"]
    for name, (body, meta) in ks.items():
        if not any(p in name for p in pats):
            continue
        whole, loop = count(body), count(widest_loop(body))
        print(f"{name}: {meta}")
        print(f"  {'class':<12} {'kernel':>8} {'loop':>8}")
        for c in sorted(set(whole) | set(loop), key=lambda c: -whole[c]):
            print(f"  {c:<12} {whole[c]:>8} {loop[c]:>8}")
        print(f"  {'total':<12} {sum(whole.values()):>8} {sum(loop.values()):>8}")


if __name__ == "__main__":
    main()
