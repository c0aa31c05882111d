#!/usr/bin/env python3
"""Static instruction counts of a unit's kernels and of their inner loops, from the gfx950 assembly.

    python tools/lean_isa_counts.py                                   # swd_lean.hip, swd_lean_kernel<16, false, true>
    python tools/lean_isa_counts.py swd_group_fa.hip -k swd_group_kernel
    python tools/lean_isa_counts.py --src OTHER_TREE/bayhunter_amd/csrc -k 'swd_lean_kernel<16, false, true>'

The unit is compiled to assembly with the flags the Makefile builds its object with (the command is taken from
`make -n UNIT.o`, so a per-file EXTRA is honoured), device side only; no GPU is needed.  For every kernel whose demangled name
contains one of the -k strings the tool prints one row for the whole kernel and one per INNER loop (a backward branch to a label,
with no other loop of --min-loop instructions or more inside), in the order of the listing: static instructions, VALU, SALU, LDS,
v_mov_b*, v_cndmask*, conditional branches (s_cbranch*) and lane moves (v_readlane*, v_readfirstlane*, v_writelane*).  A loop that
holds listed inner loops gets a row too, `round L - inner`: what of it lies OUTSIDE those inner loops -- in the lean kernel the
round loop without the layer loops of the secular evaluations, i.e. the search's bookkeeping (trial velocities, round decision).

It counts by instruction-class prefix only (v_ / s_ / ds_), names no opcode beyond the move / select / branch / lane prefixes, and knows
nothing of trip counts: a row is what the loop body holds, not what a launch issues.  The loops of the lean kernel, by size: the
Rayleigh layer steps are the largest ones (~400 instructions), the Love layer step the next (~160).
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "bayhunter_amd", "csrc")

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\w+)")


def compile_command(src, unit):
    """the Makefile's command for UNIT.o, turned into one that writes the device assembly"""
    obj = os.path.splitext(unit)[0] + ".o"
    out = subprocess.check_output(["make", "-n", "-B", "-C", src, obj], text=True)
    lines = [l for l in out.splitlines() if " -c " in l and l.rstrip().endswith("-o " + obj)]
    if not lines:
        sys.exit("no compile command for %s in `make -n %s`" % (unit, obj))
    cmd = shlex.split(lines[-1])
    cmd = cmd[:cmd.index("-c")]  # drop `-c UNIT -o UNIT.o`
    return cmd


def assembly(src, unit):
    cmd = compile_command(src, unit)
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "unit.s")
        subprocess.check_call(cmd + ["--cuda-device-only", "-S", unit, "-o", s], cwd=src)
        with open(s) as f:
            return f.read().splitlines()


def demangle(names):
    try:
        out = subprocess.check_output(["c++filt"] + names, text=True).splitlines()
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def functions(lines):
    """{symbol: (first line, last line)} of the functions of the listing"""
    start, out = {}, {}
    for i, l in enumerate(lines):
        m = re.match(r"^\s*\.type\s+([\w.$]+),@function", l)
        if m:
            start[m.group(1)] = i
        m = re.match(r"^\s*\.size\s+([\w.$]+),", l)
        if m and m.group(1) in start:
            out[m.group(1)] = (start[m.group(1)], i)
    return out


def classify(body):
    n = dict(instr=0, valu=0, salu=0, lds=0, mov=0, cnd=0, cbr=0, lane=0)
    for l in body:
        if LABEL.match(l):
            continue
        m = INSTR.match(l)
        if not m:
            continue
        op = m.group(1)
        n["instr"] += 1
        if op.startswith("v_"):
            n["valu"] += 1
            if op.startswith("v_mov_b"):
                n["mov"] += 1
            elif op.startswith("v_cndmask"):
                n["cnd"] += 1
            elif op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
                n["lane"] += 1
        elif op.startswith("s_"):
            n["salu"] += 1
            if op.startswith("s_cbranch"):
                n["cbr"] += 1
        elif op.startswith("ds_"):
            n["lds"] += 1
    return n


def loops(body, min_loop):
    """([(label, first, last)] inner, [(label, first, last, [inner inside])] outer): the loops (a backward branch to a label) of at
    least min_loop instructions that hold no other such loop, and the outermost loops that hold some of those"""
    at = {}
    for i, l in enumerate(body):
        m = LABEL.match(l)
        if m:
            at[m.group(1)] = i
    spans = []
    for i, l in enumerate(body):
        m = BRANCH.match(l)
        if m and m.group(1) in at and at[m.group(1)] <= i:
            spans.append((m.group(1), at[m.group(1)], i))
    best = {}
    for lab, a, b in spans:  # several back edges to one header: the widest
        if lab not in best or b > best[lab][2]:
            best[lab] = (lab, a, b)
    # (loops below the size asked for do not count as loops: the layer steps hold waterfall loops of ten instructions)
    spans = sorted((s for s in best.values() if classify(body[s[1]:s[2] + 1])["instr"] >= min_loop), key=lambda s: s[1])
    inner = [s for s in spans if not any(o is not s and s[1] <= o[1] and o[2] <= s[2] for o in spans)]
    outer = []
    for s in spans:
        held = [i for i in inner if i is not s and s[1] <= i[1] and i[2] <= s[2]]
        if held and not any(o is not s and o[1] <= s[1] and s[2] <= o[2] for o in spans):
            outer.append(s + (held,))
    return inner, outer


def report(lines, wanted, min_loop):
    fn = functions(lines)
    names = demangle(sorted(fn))
    rows = []
    for sym in sorted(fn, key=lambda s: fn[s][0]):
        dn = names[sym]
        if not any(w in dn for w in wanted):
            continue
        a, b = fn[sym]
        body = lines[a:b]
        rows.append((dn, "whole kernel", classify(body)))
        inner, outer = loops(body, min_loop)
        for lab, la, lb in inner:
            rows.append((dn, "loop %s" % lab, classify(body[la:lb + 1])))
        for lab, la, lb, held in outer:  # the outer loop without its listed inner loops
            rest = [l for i, l in enumerate(body[la:lb + 1], la) if not any(a_ <= i <= b_ for _, a_, b_ in held)]
            rows.append((dn, "round %s - inner" % lab, classify(rest)))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("unit", nargs="?", default="swd_lean.hip")
    ap.add_argument("-k", "--kernel", action="append", help="substring of the demangled kernel name (repeatable)")
    ap.add_argument("--src", default=CSRC, help="the csrc directory to compile in (default: this tree's)")
    ap.add_argument("--min-loop", type=int, default=40, help="loops shorter than this many instructions are not loops")
    a = ap.parse_args()
    wanted = a.kernel or ["swd_lean_kernel<16, false, true>"]
    rows = report(assembly(a.src, a.unit), wanted, a.min_loop)
    if not rows:
        sys.exit("no kernel of %s matches %s" % (a.unit, wanted))
    print("%-24s %6s %6s %6s %5s %8s %10s %10s %10s   %s" % ("part", "instr", "VALU", "SALU", "LDS", "v_mov_b*", "v_cndmask*", "s_cbranch*", "lane moves", "kernel"))
    for dn, part, n in rows:
        print("%-24s %6d %6d %6d %5d %8d %10d %10d %10d   %s" % (part, n["instr"], n["valu"], n["salu"], n["lds"], n["mov"], n["cnd"], n["cbr"], n["lane"],
                                                                  re.sub(r"^void \(anonymous namespace\)::|\(.*$", "", dn)))


if __name__ == "__main__":
    main()
