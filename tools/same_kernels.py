#!/usr/bin/env python3
"""tools/same_kernels.py A.so B.so: do two builds of the library hold the same gfx950 machine code?  For a refactor that moves kernel text between files.

Unbundles the gfx950 code object of each library (as tools/kernel_resources.sh and tools/disasm_kernel.sh do) and compares, function by function, the resource
notes of the kernels (registers, spills, LDS, scratch) and the instruction text with the addresses stripped.  Prints per function `identical`, `differs only in
pc-relative literals` (the constant behind s_getpc_b64: a table or a callee moved in the image) or the first differing lines; the exit status is 1 if a
function differs otherwise or is missing on one side."""
import difflib
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
NOTES = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size",
         "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")
PCREL = re.compile(r"(s_addc?_u32 s\d+, s\d+, )0x[0-9a-f]+$")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def load(so, tmp, tag):
    """{symbol: (resource notes or None, instructions, instructions with the pc-relative literals masked)} of the gfx950 code object of `so`"""
    fb, co = "%s/%s.fb" % (tmp, tag), "%s/%s.co" % (tmp, tag)
    run(LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, so, co)   # (with an output file: llvm-objcopy would otherwise rewrite `so` in place)
    run(LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co)
    notes = {}
    for blk in run(LLVM + "llvm-readelf", "--notes", co).split("  - .agpr_count")[1:]:
        blk = ".agpr_count" + blk
        get = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "?"])[1]
        notes[get("name")] = tuple((k, get(k)) for k in NOTES)
    out, sym = {}, None
    for line in run(LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(.*)>:$", line)
        if m:
            sym = m.group(1)
            out[sym] = (notes.get(sym), [], [])
            continue
        ins = line.split("//")[0].strip()
        if sym is None or not ins or ins == "...":   # (...: zero padding the disassembler elides)
            continue
        _, text, masked = out[sym]
        near_getpc = any(t.startswith("s_getpc_b64") for t in text[-2:])   # s_getpc_b64, s_add_u32 lo, s_addc_u32 hi
        text.append(ins)
        masked.append(PCREL.sub(r"\1<pcrel>", ins) if near_getpc else ins)
    bare = [s for s in out if re.match(r"_Z\d+k_", s) and s not in notes]
    if not notes or bare:   # (a toolchain that lays the notes out differently must not pass as "resources equal")
        sys.exit("%s: no resource notes found for %s" % (so, ", ".join(bare[:3]) or "any kernel"))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        A, B = load(sys.argv[1], tmp, "a"), load(sys.argv[2], tmp, "b")
    tally = {"identical": 0, "differs only in pc-relative literals": 0, "DIFFERS": 0, "MISSING": 0}
    kernels = 0
    for sym in sorted(set(A) | set(B)):
        a, b = A.get(sym), B.get(sym)
        detail = []
        if a is None or b is None:
            verdict = "MISSING"
            detail = ["only in " + sys.argv[2 if a is None else 1]]
        elif a[0] != b[0]:
            verdict = "DIFFERS"
            detail = ["resources: %s | %s" % (" ".join("%s=%s" % kv for kv in a[0] or ()), " ".join("%s=%s" % kv for kv in b[0] or ()))]
        elif a[1] == b[1]:
            verdict = "identical"
        elif a[2] == b[2]:
            verdict = "differs only in pc-relative literals"
        else:
            verdict = "DIFFERS"
            detail = [l for l in difflib.unified_diff(a[2], b[2], "A", "B", n=1, lineterm="")][:12]
        kernels += (a or b)[0] is not None
        tally[verdict] += 1
        print("%-44s %s" % (sym if len(sym) <= 44 else sym[:41] + "...", verdict))
        for l in detail:
            print("    " + l)
    print("%d functions (%d kernels): " % (len(set(A) | set(B)), kernels) + ", ".join("%d %s" % (n, k) for k, n in tally.items()))
    sys.exit(1 if tally["DIFFERS"] or tally["MISSING"] else 0)


if __name__ == "__main__":
    main()
