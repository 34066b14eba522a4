#!/usr/bin/env python3
"""Code-object metadata and instruction counts of the kernels of two builds of the library, side by side (needs no GPU):

    python tools/kernel_meta_diff.py parent/libtrajopt_mi355x.so trajopt_amd/_build/libtrajopt_mi355x.so [kernel substring ...]

Per kernel: VGPRs, AGPRs, SGPRs, VGPR / SGPR spills, private segment (from the msgpack notes of every gfx950 code object of the
library) and the number of instructions of the kernel's own symbol (llvm-objdump -d).  The last column says whether the two builds
agree on every figure.  Exit code 1 if a kernel named on the command line differs."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exec0_scan as xs  # noqa: E402  (the code objects of a library, the disassembly)

KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def kernels(lib):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in xs.code_objects(lib, tmp):
            cur = {}
            for line in subprocess.check_output([f"{xs.LLVM}/llvm-readelf", "--notes", co], text=True).split("\n"):
                m = re.match(r"\.?(\w[\w.]*):\s*(.*)$", line.strip().lstrip("- "))
                if not m:
                    continue
                k, v = m.group(1), m.group(2).strip()
                if k == "name" or k in KEYS:
                    cur[k] = v
                if k == "vgpr_spill_count":  # (the last key of a kernel's record)
                    if "name" in cur:
                        out[cur["name"]] = {q: int(cur.get(q, -1)) for q in KEYS}
                    cur = {}
            name, n = None, 0
            for line in xs.disasm(co) + ["0 <end>:"]:
                f = xs.FUNC.match(line)
                if f:
                    if name in out:
                        out[name]["instructions"] = n
                    name, n = f.group(2), 0
                elif xs.INS.match(line):
                    n += 1
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pats = sys.argv[3:]
    cols = KEYS + ("instructions",)
    print(f"{'kernel':44s} " + " ".join(f"{c.replace('_count', '').replace('_fixed_size', ''):>16s}" for c in cols) + "  (first build -> second build)")
    bad = 0
    for name in sorted(set(a) | set(b)):
        if pats and not any(p in name for p in pats):
            continue
        ra, rb = a.get(name, {}), b.get(name, {})
        same = ra == rb
        cells = " ".join(f"{(str(ra.get(c, '-')) if ra.get(c) == rb.get(c) else str(ra.get(c, '-')) + ' -> ' + str(rb.get(c, '-'))):>16s}" for c in cols)
        print(f"{name[:44]:44s} {cells}  {'same' if same else 'DIFFERENT'}")
        bad += 0 if same else 1
    return 1 if (pats and bad) else 0


if __name__ == "__main__":
    sys.exit(main())
