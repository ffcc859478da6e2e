#!/usr/bin/env python3
"""Compare the gfx950 code of two builds of libnvsr_hip.so kernel by kernel, modulo symbol names (the procedure behind
profiles/colour_order_split_isa.txt, render_route_host_isa.txt and deterministic_isa.txt).

    python tools/isa_compare.py PARENT_LIB THIS_LIB [--alias 'new demangled name=parent demangled name' ...] [--list SUBSTRING ...]

Every code object of a library is unbundled (llvm-objdump --offloading, on a copy in a temporary directory) and disassembled
(llvm-objdump -d); per kernel symbol the instruction stream is mnemonic + operands, without address, encoding and the disassembler's
comments, so two kernels compare equal when they differ in their symbol names only.  Register / spill / scratch / LDS figures come from
tools/kernel_resources.py.  Kernels are matched by demangled name; --alias maps a kernel of THIS_LIB whose name changed (a new defaulted
template parameter) onto the parent's.  Exit status 1 when a kernel present in both differs."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import _tool, kernel_table  # noqa: E402


def streams(lib):
    """{mangled kernel name: [instruction text]} for every function symbol of every gfx950 code object"""
    objdump = _tool("llvm-objdump")
    out = {}
    with tempfile.TemporaryDirectory(prefix="nvsr_isa_") as tmp:
        copy = os.path.join(tmp, "lib.so")
        shutil.copyfile(os.path.abspath(lib), copy)
        subprocess.run([objdump, "--offloading", copy], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            text = subprocess.run([objdump, "-d", "--no-show-raw-insn", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                    continue
                if cur is None or not line.startswith("\t") and not line.startswith(" "):
                    continue
                ins = line.split("//")[0].strip()
                ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
                if ins:
                    cur.append(ins)
    # what follows a kernel's last instruction is padding up to the next symbol's alignment (s_nop 0, s_code_end, zeros printed as "..."):
    # it depends on where the linker placed the kernel, not on the kernel
    for ins in out.values():
        while ins and (ins[-1] in ("s_nop 0", "...") or ins[-1].startswith("s_code_end")):
            ins.pop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--alias", action="append", default=[], help="'new demangled name=parent demangled name'")
    ap.add_argument("--list", action="append", default=[], help="print one line per kernel whose demangled name contains this")
    ap.add_argument("--diff", type=int, default=0, help="print up to this many lines of a unified diff per differing kernel")
    a = ap.parse_args()
    alias = dict(x.split("=", 1) for x in a.alias)
    res = {}
    for side, lib in (("parent", a.parent), ("this", a.this)):
        st = streams(lib)
        for k in kernel_table(lib):
            name = k["name"] if side == "parent" else alias.get(k["name"], k["name"])
            fig = tuple(k[f] for f in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds"))
            res.setdefault(name, {})[side] = (st.get(k["mangled"], []), fig, k["name"])
    both = sorted(n for n, v in res.items() if len(v) == 2)
    same = [n for n in both if res[n]["parent"][:2] == res[n]["this"][:2]]
    differ = [n for n in both if n not in same]
    only_parent = sorted(n for n, v in res.items() if "this" not in v)
    only_this = sorted(n for n, v in res.items() if "parent" not in v)
    print("%d kernels in both libraries; %d identical (instruction stream and vgpr / agpr / sgpr / spills / scratch / LDS), %d differ" %
          (len(both), len(same), len(differ)))
    for n in differ:
        p, t = res[n]["parent"], res[n]["this"]
        print("  DIFFERS  %d -> %d instr  %s -> %s  %s" % (len(p[0]), len(t[0]), p[1], t[1], n))
        if a.diff:
            import difflib
            for line in list(difflib.unified_diff(p[0], t[0], "parent", "this", n=2, lineterm=""))[:a.diff]:
                print("      " + line)
    print("%d kernels only in the parent:" % len(only_parent))
    for n in only_parent:
        print("  ", n)
    print("%d kernels only in this tree (vgpr agpr sgpr vgpr_spill sgpr_spill scratch lds):" % len(only_this))
    stubs = [n for n in only_this if len(res[n]["this"][0]) <= 2]       # (a library template's instantiations for other targets: s_endpgm)
    for n in only_this:
        t = res[n]["this"]
        if n not in stubs:
            print("   %6d instr  %-32s %s" % (len(t[0]), " ".join(str(x) for x in t[1]), t[2][:200]))
    if stubs:
        print("   + %d empty kernels of at most 2 instructions (instantiations for other targets)" % len(stubs))
    if alias:
        print("renamed (a new defaulted template parameter), compared under the parent's name:")
        for new, old in sorted(alias.items()):
            print("   %s  <-  %s" % (old, new))
    for sub in a.list:
        for n in both:
            if sub in n:
                t = res[n]["this"]
                print("  %s %6d instr  vgpr=%d agpr=%d sgpr=%d vgpr_spill=%d sgpr_spill=%d scratch=%d lds=%d  %s" %
                      ((("same  " if n in same else "DIFFER"), len(t[0])) + t[1] + (n[:140],)))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
