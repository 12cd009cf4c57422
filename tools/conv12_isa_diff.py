#!/usr/bin/env python3
"""Compare the gfx950 assembly of every kernel of srcnn_kernels.hip between two trees (profiles/conv12_fold_isa.txt).

    python tools/conv12_isa_diff.py PARENT_TREE RESULT_TREE [SOURCE]     (or two .s files made with the command below)

SOURCE: another file of csrc (srcnn_delta.hip: profiles/delta_frame_isa.txt).  Then every kernel gets a line, which also says
whether the .amdhsa_ block and the multiset of opcodes are the same on both sides.

Each tree's csrc/srcnn_kernels.hip is compiled device-only to assembly with the Makefile's HIPFLAGS.  A kernel's text runs from
its label to the end of its .amdhsa_kernel block, so register counts, scratch, LDS and kernarg size are compared too.  Comments
go, the kernel's own symbol becomes K and block labels lose their function number.  k_conv12_tiers and k_conv12_mfma<R, LD>
are compared with the k_conv12_mfma<R, LD, TIERS> that replaced them, k_conv3_sparse and k_conv3<STRICT, OFF64, X64, SDMA> with
the k_conv3<STRICT, OFF64, X64, SDMA, SKIP> that replaced them (profiles/conv3_fold_isa.txt).  Needs hipcc; no GPU."""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ("--offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -fvisibility=hidden -Wall -Wno-unused-result "
         "-Wno-unused-value -Wno-ignored-attributes -D__HIP_PLATFORM_AMD__ --cuda-device-only -S -x hip").split()


def assembly(path, source="srcnn_kernels.hip"):
    if os.path.isfile(path):
        return open(path).read()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS +
                       [os.path.join(path, "libsrcnn_amd", "csrc", source), "-o", out], check=True)
        return open(out).read()


def key(sym):
    """one name for a kernel on both sides of the fold"""
    if "k_conv12_tiers" in sym:
        return "k_conv12_mfma<0,1,1>"
    m = re.search(r"k_conv12_mfmaILi(\d)ELb(\d)E(?:Lb(\d)E)?EEv", sym)
    if m:
        return "k_conv12_mfma<%s,%s,%s>" % (m.group(1), m.group(2), m.group(3) or "0")
    if "k_conv3_sparse" in sym:
        return "k_conv3<1,0,0,1,1>"
    m = re.search(r"k_conv3ILb(\d)ELb(\d)ELb(\d)ELb(\d)E(?:Lb(\d)E)?EEv", sym)
    return "k_conv3<%s,%s,%s,%s,%s>" % (m.group(1), m.group(2), m.group(3), m.group(4), m.group(5) or "0") if m else sym


def kernels(asm):
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?\.amdhsa_kernel \1\n.*?\.end_amdhsa_kernel)", asm, re.M | re.S):
        lines = [re.sub(r"\s*;.*", "", l).rstrip() for l in m.group(2).replace(m.group(1), "K").split("\n")]
        out[key(m.group(1))] = [re.sub(r"\.L(BB|func_end|tmp)\d+", r".L\1", l) for l in lines if l.strip()]
    return out


def resources_and_opcodes(lines):
    """the .amdhsa_ directives in order, and how often each opcode occurs"""
    code = [l.split()[0] for l in lines if l[:1] in " \t" and not l.strip().startswith(".")]
    return [l.strip() for l in lines if l.strip().startswith(".amdhsa_")], collections.Counter(code)


def main(a, b, source=None):
    ka, kb = kernels(assembly(a, source or "srcnn_kernels.hip")), kernels(assembly(b, source or "srcnn_kernels.hip"))
    print("kernels: %d / %d; only in one tree: %s" % (len(ka), len(kb), sorted(set(ka) ^ set(kb)) or "none"))
    same = 0
    for k in sorted(set(ka) & set(kb)):
        d = [l for l in difflib.unified_diff(ka[k], kb[k], lineterm="", n=0) if l[0] in "+-" and l[:3] not in ("+++", "---")]
        if source:
            (ra, oa), (rb, ob) = resources_and_opcodes(ka[k]), resources_and_opcodes(kb[k])
            print("%-60s %5d / %5d lines, %d differ; .amdhsa_ block %s, opcode multiset %s (%d)" % (
                k[:60], len(ka[k]), len(kb[k]), len(d), "same" if ra == rb else "DIFFERS", "same" if oa == ob else "DIFFERS", sum(oa.values())))
            same += not d
        elif d or "k_conv12" in k or "k_conv3<" in k:
            print("%-60s %5d / %5d lines, %d differ" % (k[:60], len(ka[k]), len(kb[k]), len(d)))
            for l in d[:20]:
                print("    " + l)
        else:
            same += 1
    print(("kernels without a differing line: %d" if source else "every other kernel (%d): 0 lines differ") % same)


if __name__ == "__main__":
    main(*sys.argv[1:4])
