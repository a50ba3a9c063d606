#!/usr/bin/env python3
"""Counts what the parser's pass update costs in the compiled persistent kernels.

    python tests/isa_pass.py [--json] [--extra=-DFLAG ...]

The update is the part of a parser pass behind the workgroup barrier (Parser::parse_segment's pass loop, nlzm_v2.h): every wave of the stage
computes it identically and it is a chain of dependent operations, so its length is on the stream's critical path (DESIGN.md sections 7, 30).
This tool compiles nlzm_kernels.hip to device assembly through the Makefile's `isa-asm` target, as tests/isa_spills.py does, and reports for
each inlined copy of the update in pipeline2_kernel and pipeline2_multi_kernel (the parser stage's and the helper parsers'):

  * instructions in all, `s_waitcnt` that wait for lgkmcnt, `ds_*` instructions, exec-mask instructions (`*saveexec*`, `s_cbranch_exec*`,
    `s_or_b64 exec`), `s_nop`;
  * dependent LDS round trips: groups of DS instructions that return a value, each closed by the first lgkmcnt wait that brings one of
    its values back (a wait that lets the group's operations stay on their way closes nothing).

  * The update's source lines lie between `// pass-update: begin` and `// pass-update: end` in nlzm_v2.h; an instruction is the update's when
    a frame of its line entry's inlining chain lies between the two.
  * A copy in the assembly runs from the pass loop's `s_barrier` (an `s_barrier` whose line entry names the line of the `xw::block_sync()`
    in front of the begin marker; it is counted) to the loop's back edge (the first branch behind it to a label in front of it; counted
    too).  The tool checks the two against each other: at least 85 % of the instructions of such a span must be the update's by their
    lines, or it refuses to report (the compiler has laid the loop out in a way this tool does not understand).  Instructions of the
    update's lines that lie outside every span are reported as a count of their own.

No GPU is needed.
"""
from __future__ import annotations

import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import isa_spills  # noqa: E402

KERNELS = isa_spills.KERNELS
SOURCE = os.path.join(isa_spills.CSRC, "nlzm_v2.h")
BEGIN, END = "// pass-update: begin", "// pass-update: end"
FIGURES = ("instructions", "lgkm_waits", "ds_instructions", "exec_mask", "s_nop", "lds_round_trips")
MIN_SHARE = 0.85

_FRAME = re.compile(r"(?:^|[\s/])nlzm_v2\.h:(\d+)")
_LABEL = re.compile(r"^(\.?\w+):")
_BRANCH = re.compile(r"^s_c?branch\w*\s+(\.?\w+)")
_EXEC = re.compile(r"saveexec|^s_cbranch_exec|^s_or_b64\s+exec\b")
_LGKM = re.compile(r"lgkmcnt\((\d+)\)")
_DS_VALUE =re.compile(r"^ds_(read|load|bpermute|permute|swizzle|consume|append|\w+_rtn)")


def update_lines() -> tuple:
    """(the barrier's line, first line of the update, last line of it)"""
    with open(SOURCE, encoding="utf-8") as f:
        text = f.read().splitlines()
    begin = [n for n, t in enumerate(text, 1) if t.strip() == BEGIN]
    end = [n for n, t in enumerate(text, 1) if t.strip() == END]
    if len(begin) != 1 or len(end) != 1 or begin[0] >= end[0]:
        raise SystemExit("isa_pass: nlzm_v2.h needs one '// pass-update: begin' in front of one '// pass-update: end'")
    barrier = next((n for n in range(begin[0], 0, -1) if "xw::block_sync()" in text[n - 1]), None)
    if barrier is None:
        raise SystemExit("isa_pass: no xw::block_sync() in front of the update")
    return barrier, begin[0] + 1, end[0] - 1


def instructions(lines: list, lo: int, hi: int, barrier: int) -> tuple:
    """-> ([(text, is the update's, is the pass barrier)], label -> index of the instruction it stands in front of)"""
    out, labels, frames = [], {}, []
    for line in lines:
        s = line.strip()
        if s.startswith(".loc"):
            got = [int(m.group(1)) for m in _FRAME.finditer(s.split(";", 1)[1] if ";" in s else "")]
            frames = [n for n in got if n > 0] or frames
            continue
        if (m := _LABEL.match(s)) and not line[:1].isspace():
            labels[m.group(1)] = len(out)
            continue
        if not s or s[0] in ".;" or not line[:1].isspace():
            continue
        s = s.split(";", 1)[0].strip()
        out.append((s, any(lo <= n <= hi for n in frames), s.startswith("s_barrier") and barrier in frames))
    return out, labels


def copies(ins: list, labels: dict) -> list:
    """the spans [barrier, back edge] of the update's inlined copies"""
    spans = []
    for at, (_, _, is_barrier) in enumerate(ins):
        if not is_barrier:
            continue
        edge = None
        for j in range(at + 1, len(ins)):
            if ins[j][0].startswith("s_barrier"):
                break
            if (m := _BRANCH.match(ins[j][0])) and labels.get(m.group(1), len(ins)) <= at:
                edge = j
                break
        if edge is None:
            raise SystemExit("isa_pass: no back edge behind the pass loop's barrier")
        inside = ins[at + 1:edge]
        share = sum(1 for x in inside if x[1]) / max(1, len(inside))
        if share < MIN_SHARE:
            raise SystemExit(f"isa_pass: only {100 * share:.0f} % of the span between barrier and back edge is the update by its lines")
        spans.append((at, edge))
    return spans


def figures(span: list) -> dict:
    f = dict.fromkeys(FIGURES, 0)
    f["instructions"] = len(span)
    # DS operations come back in order: lgkmcnt(n) waits until at most n are out.  A group is the values asked for since the last wait that
    # brought one back; it is closed, and counts as a round trip, by the first wait that brings one of ITS values back.
    out, group, closed = [], 0, set()                   # out: the group of every DS operation on its way (None: it returns nothing)
    for s, _, _ in span:
        if s.startswith("s_waitcnt") and (m := _LGKM.search(s)):
            f["lgkm_waits"] += 1
            back, out = out[:max(0, len(out) - int(m.group(1)))], out[max(0, len(out) - int(m.group(1))):]
            for g in back:
                if g is not None and g not in closed:
                    closed.add(g)
                    f["lds_round_trips"] += 1
            if any(g is not None for g in back):
                group += 1
        elif s.startswith("ds_"):
            f["ds_instructions"] += 1
            out.append(group if _DS_VALUE.match(s) else None)
        elif _EXEC.search(s):
            f["exec_mask"] += 1
        elif s.startswith("s_nop"):
            f["s_nop"] += 1
    return f


def measure(extra: str = "") -> dict:
    asm, remarks = isa_spills.compile_asm(extra)
    barrier, lo, hi = update_lines()
    bodies, res = isa_spills.kernel_bodies(asm), isa_spills.resources(remarks)
    out = {}
    for k in KERNELS:
        if k not in bodies or k not in res:
            raise SystemExit(f"isa_pass: {k} is not in the compiler's output")
        ins, labels = instructions(bodies[k], lo, hi, barrier)
        spans = copies(ins, labels)
        if not spans:
            raise SystemExit(f"isa_pass: {k}: the pass loop's barrier is not in the assembly")
        # (instructions of the update's lines that the compiler has put somewhere else: in front of the barrier, behind the loop)
        inside = set()
        for at, edge in spans:
            inside.update(range(at, edge + 1))
        elsewhere = sum(1 for n, x in enumerate(ins) if x[1] and n not in inside)
        out[k] = {"copies": [figures(ins[at:edge + 1]) for at, edge in spans], "update_lines_elsewhere": elsewhere, "resources": res[k]}
    return out


def report(result: dict) -> str:
    text = []
    for k in KERNELS:
        r = result[k]
        text.append(f"{k}: {len(r['copies'])} copies of the update; {r['update_lines_elsewhere']} instructions of its lines outside them")
        text.append("  " + "; ".join(f"{key} {val}" for key, val in r["resources"].items()))
        text.append("  " + f"{'copy':<6}" + "".join(f"{name:>17}" for name in FIGURES))
        for n, f in enumerate(r["copies"]):
            text.append("  " + f"{n:<6}" + "".join(f"{f[name]:>17}" for name in FIGURES))
    return "\n".join(text)


def main(argv: list) -> int:
    extra = " ".join(a[len("--extra="):] for a in argv if a.startswith("--extra="))
    result = measure(extra)
    print(json.dumps(result, indent=1) if "--json" in argv else report(result))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
