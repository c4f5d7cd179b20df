#!/usr/bin/env python3
"""Static resource and instruction table of the tower kernels in csrc/clip_ops.hip (no GPU needed: hipcc, device only, to ISA).

    tools/clip_ops_isa_table.py [COMMIT]      clip_ops.hip of COMMIT (default: the working tree) with the tree's headers

One row per GEMM instance and per layernorm / vit_tokens / gather_rows kernel: registers, LDS, scratch and spills from the
code object's metadata, and per-kernel counts of the instruction classes an epilogue or load/store change would move.
profiles/r16a_clip_ops_fold.txt holds this table at the parent and after the fold."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tise_toolbox_amd", "csrc")
KERNELS = re.compile(r"gemm(16)?_f16(_big)?_kernel|layernorm|vit_tokens|gather_rows")
CLASSES = [("mfma", r"v_mfma"), ("ldsdma", r"global_load_lds"), ("ds_rd", r"ds_read"), ("ds_wr", r"ds_write"),
           ("g_ld", r"global_load_(?!lds)"), ("g_st", r"global_store"), ("cvt", r"v_cvt"), ("exp", r"v_exp"), ("rcp", r"v_rcp")]
META = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
        ("scratch", ".private_segment_fixed_size"), ("vspill", ".vgpr_spill_count"), ("sspill", ".sgpr_spill_count")]


def short_name(mangled):
    """gemm16_f16_kernel<1,0> from _ZN12_GLOBAL__N_117gemm16_f16_kernelILb1ELi0EEEv...: the kernels' template arguments are
    integers, booleans, _Float16 and float only."""
    n, rest = re.match(r"_ZN12_GLOBAL__N_1(\d+)(.*)", mangled).groups()
    name, rest = rest[:int(n)], rest[int(n):]
    args = []
    if rest.startswith("I"):
        rest = rest[1:]
        while not rest.startswith("E"):
            m = re.match(r"L[ib](\d+)E|(DF16_)|(f)", rest)
            args.append(m.group(1) or ("_Float16" if m.group(2) else "float"))
            rest = rest[m.end():]
    return name + ("<" + ",".join(args) + ">" if args else "")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(CSRC, "clip_ops.hip")
        if len(sys.argv) > 1:
            src = os.path.join(tmp, "clip_ops.hip")
            with open(src, "wb") as f:
                f.write(subprocess.check_output(["git", "-C", ROOT, "show", sys.argv[1] + ":tise_toolbox_amd/csrc/clip_ops.hip"]))
        asm = os.path.join(tmp, "clip_ops.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-std=c++17",
                               "-Wno-unused-value", "-I", CSRC, "--cuda-device-only", "-S", src, "-o", asm])
        text = open(asm).read()
    rows = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s+s_endpgm", text, re.S | re.M):
        if KERNELS.search(m.group(1)):
            ops = re.findall(r"^\s+([a-z]\w+)", m.group(2), re.M)
            rows[m.group(1)] = {k: sum(1 for o in ops if re.match(p, o)) for k, p in CLASSES}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.S | re.M):
        name = re.search(r"^\s+\.name:\s+(\S+)", m.group(0), re.M).group(1)
        if name in rows:
            for k, key in META:
                rows[name][k] = int(re.search(r"^[\s-]+\%s:\s+(\d+)" % key, m.group(0), re.M).group(1))
    cols = [k for k, _ in META] + [k for k, _ in CLASSES]
    print("%-34s" % "kernel" + "".join("%8s" % c for c in cols))
    for name, d in sorted((short_name(n), rows[n]) for n in rows):
        print("%-34s" % name + "".join("%8d" % d[c] for c in cols))


if __name__ == "__main__":
    main()
