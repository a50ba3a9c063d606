#!/usr/bin/env python3
"""Counts the scalar-register spill moves of the persistent kernels, by region of the source.

    python tests/isa_spills.py [--json] [--extra=-DFLAG ...]

Compiles nlzm_kernels.hip to device assembly through the Makefile's `isa-asm` target (the product's own flags plus line
tables and the resource-usage remarks) and prints, for pipeline2_kernel and pipeline2_multi_kernel, instructions, spill
stores and spill reloads per region, and what the compiler reports for the kernel (registers, occupancy, scratch, LDS).

  * A spill VGPR is one that `v_writelane_b32 vX, sN, <immediate>` writes eight times or more; a spill store is such a
    write, a spill reload a `v_readlane_b32 sN, vX, <immediate>` of such a register.
  * A region starts at a line `// isa-region: NAME` of nlzm_v2.h or nlzm_kernels.hip and ends at the file's next such
    line (a name may stand more than once); lines in front of a file's first marker are "kernel entry".  An instruction
    belongs to the region of the innermost frame of its line entry's inlining chain that lies in a marked region of the
    two files (a shared helper counts for the role that called it); with frames in the two files but none in a marked
    region, to "kernel entry"; with no frame in the two files, to the region of the instruction before it.

No GPU is needed.
"""
from __future__ import annotations

import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlzm_amd", "csrc")
FILES = ("nlzm_v2.h", "nlzm_kernels.hip")
KERNELS = ("pipeline2_kernel", "pipeline2_multi_kernel")
ENTRY = "kernel entry"
REGIONS = ("finder block", "finder chunk loop", "table stage", "parser and helper parsers", "hot-bin wave", "worker lanes", ENTRY)
SINGLE_WAVE = ("finder block", "table stage", "parser and helper parsers", "hot-bin wave")     # the regions whose loops bound the stream

_MARK = re.compile(r"//\s*isa-region:\s*(.+?)\s*$")
_FRAME = re.compile(r"(?:^|[\s/])(nlzm_v2\.h|nlzm_kernels\.hip):(\d+)")
_WRITE = re.compile(r"^\s*v_writelane_b32\s+(v\d+),\s*s\d+,\s*\d+\b")
_READ = re.compile(r"^\s*v_readlane_b32\s+s\d+,\s*(v\d+),\s*\d+\b")
_REMARK = re.compile(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]):\s*(\S+)")


def markers() -> dict:
    """file name -> [(line, region)] in line order"""
    out = {}
    for name in FILES:
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            out[name] = [(no, m.group(1)) for no, text in enumerate(f, 1) if (m := _MARK.search(text))]
        for _, region in out[name]:
            if region not in REGIONS:
                raise SystemExit(f"isa_spills: {name}: unknown region '{region}'")
    return out


def region_of(marks: dict, name: str, line: int) -> str:
    region = ENTRY
    for no, r in marks[name]:
        if no > line:
            break
        region = r
    return region


def compile_asm(extra: str = "") -> tuple:
    """(assembly text, remarks text)"""
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "kernels.s")
        cmd = ["make", "-s", "-C", CSRC, "isa-asm", f"ASM={asm}"] + ([f"EXTRA={extra}"] if extra else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("isa_spills: the compile failed:\n" + r.stdout + r.stderr)
        with open(asm, encoding="utf-8") as f:
            return f.read(), r.stderr


def kernel_bodies(asm: str) -> dict:
    """kernel name -> the lines between its label and the end of the function"""
    out, cur = {}, None
    for line in asm.splitlines():
        if cur is None:
            for k in KERNELS:
                if re.match(rf"^_ZN4nlzm{len(k)}{k}E\w*:", line):
                    cur = k
                    out[k] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        else:
            out[cur].append(line)
    return out


def count(lines: list, marks: dict) -> dict:
    writes = {}
    for line in lines:
        if (m := _WRITE.match(line)):
            writes[m.group(1)] = writes.get(m.group(1), 0) + 1
    spill = {v for v, n in writes.items() if n >= 8}
    table = {r: {"instructions": 0, "spill_stores": 0, "spill_reloads": 0} for r in REGIONS}
    region = ENTRY
    for line in lines:
        s = line.strip()
        if s.startswith(".loc"):
            # innermost frame first: "; file:line:col @[ file:line:col @[ ... ] ]"
            frames = [region_of(marks, m.group(1), int(m.group(2))) for m in _FRAME.finditer(s.split(";", 1)[1] if ";" in s else "")
                      if int(m.group(2)) > 0]         # (line 0: code the compiler made, of no line)
            if frames:
                region = next((r for r in frames if r != ENTRY), ENTRY)
            continue
        if not s or s[0] in ".;" or s.endswith(":") or not line[:1].isspace():
            continue
        row = table[region]
        row["instructions"] += 1
        if (m := _WRITE.match(line)) and m.group(1) in spill:
            row["spill_stores"] += 1
        elif (m := _READ.match(line)) and m.group(1) in spill:
            row["spill_reloads"] += 1
    return {"spill_vgprs": sorted(spill), "regions": table}


def resources(remarks: str) -> dict:
    out, cur = {}, None
    for m in _REMARK.finditer(remarks):
        key, val = m.group(1), m.group(2)
        if key == "Function Name":
            cur = next((k for k in KERNELS if re.match(rf"^_ZN4nlzm{len(k)}{k}E", val)), None)
            if cur:
                out[cur] = {}
        elif cur:
            out[cur][key] = int(val)
    return out


def measure(extra: str = "") -> dict:
    asm, remarks = compile_asm(extra)
    marks = markers()
    bodies, res = kernel_bodies(asm), resources(remarks)
    out = {}
    for k in KERNELS:
        if k not in bodies or k not in res:
            raise SystemExit(f"isa_spills: {k} is not in the compiler's output")
        out[k] = count(bodies[k], marks)
        out[k]["resources"] = res[k]
    return out


def report(result: dict) -> str:
    text = []
    for k in KERNELS:
        r, res = result[k], result[k]["resources"]
        total = sum(row["instructions"] for row in r["regions"].values())
        text.append(f"{k}: {total} instructions; spill VGPRs {', '.join(r['spill_vgprs']) or 'none'}")
        text.append("  " + "; ".join(f"{key} {val}" for key, val in res.items()))
        text.append(f"  {'region':<28}{'instructions':>13}{'spill stores':>14}{'spill reloads':>15}{'share':>8}")
        for name in REGIONS:
            row = r["regions"][name]
            share = 100.0 * (row["spill_stores"] + row["spill_reloads"]) / row["instructions"] if row["instructions"] else 0.0
            text.append(f"  {name:<28}{row['instructions']:>13}{row['spill_stores']:>14}{row['spill_reloads']:>15}{share:>7.1f}%")
        text.append(f"  {'all':<28}{total:>13}{sum(x['spill_stores'] for x in r['regions'].values()):>14}{sum(x['spill_reloads'] for x in r['regions'].values()):>15}")
    return "\n".join(text)


def main(argv: list) -> int:
    extra = " ".join(a[len("--extra="):] for a in argv if a.startswith("--extra="))
    result = measure(extra)
    print(json.dumps(result, indent=1) if "--json" in argv else report(result))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
