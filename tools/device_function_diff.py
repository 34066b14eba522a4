#!/usr/bin/env python3
"""Every function symbol (kernels and out-of-line device functions) of the gfx950 code objects of two builds of the library:
instruction count and whether the instruction text is identical (needs no GPU).  Ignored: addresses, branch-target annotations, the
s_nop padding behind a function, and the 32-bit literal of the s_add_u32 that follows an s_getpc_b64 (a PC-relative offset to a
callee or a constant: it moves with the code layout, not with the function).

    python tools/device_function_diff.py parent/libtrajopt_mi355x.so trajopt_amd/_build/libtrajopt_mi355x.so"""
import sys, subprocess, tempfile, re
import os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exec0_scan as xs
def funcs(lib):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in xs.code_objects(lib, tmp):
            txt = subprocess.check_output([f"{xs.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
            cur = None
            for l in txt.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", l)
                if m:
                    cur = m.group(1); out[cur] = []; continue
                if cur is None or not l.strip():
                    continue
                ins = re.sub(r"//.*", "", l).strip()
                ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
                ins = re.sub(r"<[^>]*>", "", ins).strip()
                if ins.startswith("s_add_u32") and out[cur] and out[cur][-1].startswith("s_getpc_b64"):
                    ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)
                if ins:
                    out[cur].append(ins)
    for k in out:
        while out[k] and out[k][-1].startswith("s_nop"):
            out[k].pop()
    return out
a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
for k in sorted(set(a) | set(b)):
    if re.search(r"\.(kd)$", k): continue
    na, nb = len(a.get(k, [])), len(b.get(k, []))
    if k not in a: st = "new"
    elif k not in b: st = "gone"
    else: st = "identical" if a[k] == b[k] else "DIFFERENT"
    print(f"{k[:78]:78s} {na if k in a else '-':>7} -> {nb if k in b else '-':>7}  {st}")
