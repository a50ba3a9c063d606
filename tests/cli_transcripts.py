"""What the command line prints, returns and leaves behind, case by case: tests/test_cli_transcripts.py replays the cases against the
transcripts under tests/golden/, which the command line of the commit BEFORE a change to nlzm_cli.cpp wrote:

    python -m tests.cli_transcripts cpu PATH_TO_nlzm tests/golden/cli_transcripts.json                  (no device needed)
    python -m tests.cli_transcripts nodevice PATH_TO_nlzm tests/golden/cli_nodevice_transcripts.json    (on a machine without a GPU)
    python -m tests.cli_transcripts gpu PATH_TO_nlzm tests/golden/cli_gpu_transcripts.json              (on a GPU)

A case is a directory of input files and a list of invocations run there one after another, with relative names.  Its transcript is every
invocation's stdout (two-decimal numbers are timings and read #.##) and exit status, and every file in the directory afterwards by its SHA-256
-- so a file that is missing, or there where it should not be, shows as well as one whose bytes moved.  The streams are the oracle's, the
indexes are written here, the CRCs are zlib's."""
import functools
import hashlib
import json
import os
import re
import subprocess
import sys
import zlib

import numpy as np

from nlzm_amd import corpus
from tests import cli_tools, oracle_py, planes_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [60_000, 45_001, 0, 70_003, 30_000]          # five blocks, the third of raw length 0
M = 1 << 64
GPU_FORMS = ("c alone", "c -crc", "c -blocks:3", "c -blocks:3 -verify", "c -cdc:10 -dedup", "c -elem:4 -blocks:2", "c -cdc:10 -elem:2")


def index_text(*args, **kw):
    return cli_tools.index_text(*args, **kw).encode()


@functools.lru_cache(maxsize=None)
def inputs():
    raw = corpus.mixed(sum(SIZES), corpus.SEED + 51).tobytes()
    st = [sum(SIZES[:i]) for i in range(len(SIZES) + 1)]
    blocks = [raw[st[i]:st[i + 1]] for i in range(len(SIZES))]
    streams = [oracle_py.compress(np.frombuffer(b, dtype=np.uint8), 17) for b in blocks]
    text = corpus.syn_text(120_000).tobytes()
    rng = np.random.default_rng(corpus.SEED + 170)
    tblocks = [((rng.standard_normal(3000) * 0.02).astype("<f4").view("<u4") >> 16).astype("<u2").tobytes(),
               (np.arange(2500) * 3 + 1000).astype("<i4").tobytes(),
               (np.arange(700) * 7).astype("<i8").tobytes() + b"tail"]
    telems = [2, 4, 8]
    return {"raw": raw, "st": st, "streams": streams, "lens": [len(s) for s in streams], "crcs": [zlib.crc32(b) for b in blocks], "whole": zlib.crc32(raw),
            "text": text, "one": oracle_py.compress(np.frombuffer(text, dtype=np.uint8), 17),
            "tblocks": tblocks, "telems": telems, "tstreams": [oracle_py.compress(planes_model.forward(b, e), 17) for b, e in zip(tblocks, telems)]}


def cpu_cases():
    """(name, {file: bytes}, [argv, ...]) for every host-only case; the `-gpu` forms are in nodevice_cases()"""
    i = inputs()
    blob, lens, st, total = b"".join(i["streams"]), i["lens"], i["st"], sum(SIZES)
    idx = lambda **kw: index_text(lens, SIZES, kw.pop("crcs", i["crcs"]), kw.pop("whole", i["whole"]), **kw)
    dt = [["t", "c.nlzm"], ["d", "c.nlzm", "o.bin"]]
    cases = [("no arguments", {}, [[]]), ("a command that is none", {}, [["q", "a"], ["c", "a"], ["x", "a", "b"]])]
    bad = ["-cdc:", "-cdc:9", "-cdc:31", "-cdc:12x", "-cdc:+12", "-cdc: 12", "-cdc:99999999999", "-cdc:010",
           "-elem:", "-elem:0", "-elem:1", "-elem:3", "-elem:16", "-elem:4x",
           "-steps:", "-steps:0", "-steps:4294967296", "-steps:2x", "-steps:-1", "-steps:99999999999999999999999",
           "-range:5", "-range:5:", "-range::5", "-range:5:6x", "-range:-1:2", "-range:1:-2", "-range: 1:2", "-range:+1:2", "-range:18446744073709551616:1",
           "-range:1:99999999999999999999", "-nosuch", "-Window:3", "--BLOCKS:0", "-gpus:99", "-window:99"]
    cases.append(("flags that are ill-formed or not known", {"a": b"abc"}, [[f, "h", "a"] for f in bad]))
    cases.append(("flags that do not go together", {"a": b"abc"},
                  [["-cdc:12", "-blocks:2", "c", "a", "b"], ["-cdc:12", "-gpus:1", "c", "a", "b"], ["-dedup", "c", "a", "b"], ["-elem:4", "-gpus:1", "c", "a", "b"],
                   ["-gpus:2", "-blocks:2", "-elem:8", "c", "a", "b"], ["-gpus:2", "-blocks:100", "h", "a"], ["-steps:2", "t", "a"], ["-steps:2", "-gpu", "h", "a"],
                   ["-gpu", "-steps:2", "d", "a"], ["-steps:4294967295", "-cdc:30", "-elem:8", "-range:0:0", "h", "a"], ["-elem:4", "h", "a"]]))
    cases.append(("h", {"a": i["text"], "e": b""}, [["h", "a"], ["h", "e"], ["h", "missing"], ["H", "a"]]))
    cases.append(("files that exist or do not", {"c.nlzm": i["one"], "o.bin": b"keep"},
                  [["d", "c.nlzm", "o.bin"], ["d", "missing", "p.bin"], ["t", "missing"], ["c", "c.nlzm", "o.bin"], ["d", "c.nlzm", "nodir/p.bin"],
                   ["-range:0:1", "x", "c.nlzm", "o.bin"], ["-range:0:1", "x", "missing", "p.bin"], ["-range:0:1", "x", "c.nlzm", "nodir/p.bin"]]))
    cases.append(("one stream", {"c.nlzm": i["one"]}, dt))
    one_crc = zlib.crc32(i["text"])
    cases.append(("one stream with an index", {"c.nlzm": i["one"], "c.nlzm.idx": index_text([len(i["one"])], [len(i["text"])], [one_crc], one_crc)}, dt))
    cases.append(("one stream with an index of a wrong CRC", {"c.nlzm": i["one"], "c.nlzm.idx": index_text([len(i["one"])], [len(i["text"])], [one_crc ^ 0x80], one_crc ^ 0x80)}, dt))
    cases.append(("one stream with an index of a wrong raw length", {"c.nlzm": i["one"], "c.nlzm.idx": index_text([len(i["one"])], [len(i["text"]) + 1], [one_crc], one_crc)}, dt))
    cases.append(("five blocks, no index", {"c.nlzm": blob}, dt))
    for v in (1, 2):
        cases.append((f"five blocks, index version {v}", {"c.nlzm": blob, "c.nlzm.idx": idx(version=v)}, dt))
    cases.append(("index with fields behind the last block", {"c.nlzm": blob, "c.nlzm.idx": idx() + b"7\n"}, dt + [["-range:5:6", "x", "c.nlzm", "p.bin"]]))
    cases.append(("lying index: lengths that do not add up", {"c.nlzm": blob, "c.nlzm.idx": idx(n_in=total + 1)}, dt))
    cases.append(("lying index: n_out larger than the file", {"c.nlzm": blob, "c.nlzm.idx": idx(n_out=len(blob) + 1)}, dt))
    cases.append(("lying index: a gap between two blocks", {"c.nlzm": blob, "c.nlzm.idx": idx(offs=[0, lens[0], lens[0] + lens[1] + 1, sum(lens[:3]), sum(lens[:4])])}, dt))
    other = [SIZES[0] - 5, SIZES[1] + 5] + SIZES[2:]
    cases.append(("lying index: raw lengths of another partition", {"c.nlzm": blob, "c.nlzm.idx": index_text(lens, other, i["crcs"], i["whole"])}, dt))
    cases.append(("lying index: raw lengths of another partition, version 1", {"c.nlzm": blob, "c.nlzm.idx": index_text(lens, other, version=1)}, dt))
    wrong = list(i["crcs"]); wrong[3] ^= 0x00010000
    cases.append(("lying index: a wrong block CRC", {"c.nlzm": blob, "c.nlzm.idx": idx(crcs=wrong)},
                  dt + [[f"-range:{st[3] + 100}:{SIZES[3] - 100}", "x", "c.nlzm", "p.bin"], [f"-range:{st[3] + 100}:{SIZES[3] - 101}", f"-range:{st[4]}:{SIZES[4]}", "x", "c.nlzm", "q.bin"]]))
    cases.append(("lying index: a wrong whole CRC", {"c.nlzm": blob, "c.nlzm.idx": idx(whole=i["whole"] ^ 1)}, dt + [["-range:0:10", "x", "c.nlzm", "p.bin"]]))
    cases.append(("lying index: a block length that wraps", {"c.nlzm": blob, "c.nlzm.idx": index_text([lens[0], M - lens[0] + 16] + lens[2:], SIZES, version=1)}, dt + [["-range:0:10", "x", "c.nlzm", "p.bin"]]))
    cases.append(("lying index: a number beyond 64 bits", {"c.nlzm": blob, "c.nlzm.idx": index_text(lens, SIZES, version=1, n_in=M + total)}, [["t", "c.nlzm"], ["-range:0:1", "x", "c.nlzm", "p.bin"]]))
    cases.append(("lying index: a signed number, a hexadecimal prefix", {"c.nlzm": blob, "c.nlzm.idx": idx().replace(b"\n0 ", b"\n+0 ", 1).replace(b" " + b"%08X" % i["crcs"][0], b" 0x%08X" % i["crcs"][0])},
                  [["t", "c.nlzm"], ["-range:0:1", "x", "c.nlzm", "p.bin"]]))
    cases.append(("lying index: a block count of 0", {"c.nlzm": blob, "c.nlzm.idx": f"NLZMIDX 1 0 0 0\n".encode()}, [["t", "c.nlzm"], ["-range:0:1", "x", "c.nlzm", "p.bin"]]))
    empty = bytes.fromhex("000a000e00000000")            # (a stream of no bytes)
    for k in (4096, 4097):                                # (the container cut off inside block 2: one stream to decode, not a thread for each of k)
        cases.append((f"index of {k} blocks: d and t read 4096 at most, x 65536", {"c.nlzm": empty + empty[:4], "c.nlzm.idx": index_text([8] * k, [0] * k, version=1)},
                      [["t", "c.nlzm"], ["-range:0:0", "x", "c.nlzm", "p.bin"]]))
    cases.append(("index of version 4, and one that is no index", {"c.nlzm": blob, "c.nlzm.idx": idx().replace(b"NLZMIDX 2", b"NLZMIDX 4"), "n.nlzm": blob, "n.nlzm.idx": b"hello\n"},
                  [["t", "c.nlzm"], ["-range:0:1", "x", "c.nlzm", "p.bin"], ["t", "n.nlzm"], ["-range:0:1", "x", "n.nlzm", "q.bin"]]))
    cut = sum(lens[:2]) + 3
    for v, what in ((2, "with an index"), (0, "without one")):
        files = {"c.nlzm": blob[:cut]}
        if v:
            files["c.nlzm.idx"] = idx()
        cases.append((f"container cut inside block 3, {what}", files, dt + [[f"-range:{st[1] - 50}:100", f"-range:{st[2] - 1}:1", "x", "c.nlzm", "p.bin"], [f"-range:{st[3]}:10", "x", "c.nlzm", "q.bin"]]))
    cases.append(("container cut inside block 4's frames", {"c.nlzm": blob[:sum(lens[:3]) + 100], "c.nlzm.idx": idx()}, dt))
    cases.append(("container cut inside block 4's frames, no index", {"c.nlzm": blob[:sum(lens[:3]) + 100]}, dt))
    cases.append(("trailing junk", {"c.nlzm": blob + b"junk behind", "c.nlzm.idx": idx()}, dt + [["-range:0:10", "x", "c.nlzm", "p.bin"]]))
    cases.append(("trailing junk, no index", {"c.nlzm": blob + b"junk behind"}, dt + [["-range:0:10", "x", "c.nlzm", "p.bin"]]))
    cases.append(("a malformed first stream", {"c.nlzm": b"\x01\x02\x03 not a stream at all", "e.nlzm": b"", "h.nlzm": i["one"][:200]},
                  dt + [["t", "e.nlzm"], ["d", "e.nlzm", "p.bin"], ["t", "h.nlzm"], ["d", "h.nlzm", "q.bin"], ["-range:0:1", "x", "c.nlzm", "r.bin"], ["-range:0:1", "x", "h.nlzm", "s.bin"]]))
    damaged = bytearray(blob); damaged[lens[0] + 40:lens[0] + 60] = bytes(20)
    cases.append(("a block damaged inside", {"c.nlzm": bytes(damaged), "c.nlzm.idx": idx()}, dt + [[f"-range:{st[1]}:10", "x", "c.nlzm", "p.bin"], ["-range:0:10", "x", "c.nlzm", "q.bin"]]))
    ranges = {"inside one block": [(1000, 4096), (st[3] + 5, 77)], "across three blocks": [(st[1] + 40_000, 5001 + 70_003 + 10)], "empty ranges": [(0, 0), (total, 0), (st[2], 0), (777, 0)],
              "the last byte": [(total - 1, 1)], "whole, repeat, overlap, out of order": [(0, total), (st[4], 100), (st[4], 100), (50, 100), (10, 100)],
              "over the end": [(total, 1)], "over the end by one": [(total - 1, 2)], "wraps": [(M - 1, 2)]}
    xs = [[f"-range:{o}:{n}" for o, n in r] + ["x", "c.nlzm", f"x{j}.bin"] for j, r in enumerate(ranges.values())]
    for v in (2, 1, 0):
        files = {"c.nlzm": blob}
        if v:
            files["c.nlzm.idx"] = idx(version=v)
        cases.append((f"x, index version {v}" if v else "x without an index", files, xs))
    tblob, tlens, traws = b"".join(i["tstreams"]), [len(s) for s in i["tstreams"]], [len(b) for b in i["tblocks"]]
    tcrcs, twhole = [zlib.crc32(b) for b in i["tblocks"]], zlib.crc32(b"".join(i["tblocks"]))
    tidx = lambda **kw: index_text(tlens, traws, tcrcs, twhole, version=3, elems=kw.pop("elems", i["telems"]), **kw)
    cases.append(("typed blocks on the host path", {"c.nlzm": tblob, "c.nlzm.idx": tidx()}, dt + [["-range:0:10", "x", "c.nlzm", "p.bin"]]))
    cases.append(("typed blocks, one of them alone", {"c.nlzm": i["tstreams"][2], "c.nlzm.idx": index_text(tlens[2:], traws[2:], tcrcs[2:], tcrcs[2], version=3, elems=[8])}, dt))
    cases.append(("typed blocks, a flipped element size", {"c.nlzm": tblob, "c.nlzm.idx": tidx(elems=[2, 8, 8])}, dt))
    cases.append(("typed blocks, an element size of 3", {"c.nlzm": tblob, "c.nlzm.idx": tidx(elems=[2, 3, 8])}, dt))
    cases.append(("typed blocks, an index that does not fit", {"c.nlzm": tblob, "c.nlzm.idx": tidx(n_out=sum(tlens) + 1)}, dt))
    cases.append(("typed blocks, an index without the element sizes", {"c.nlzm": tblob, "c.nlzm.idx": tidx().replace(b"NLZMIDX 3", b"NLZMIDX 2")}, dt))
    cases.append(("typed blocks, raw lengths of another partition", {"c.nlzm": tblob, "c.nlzm.idx": index_text(tlens, [traws[0] - 4, traws[1] + 4, traws[2]], tcrcs, twhole, version=3, elems=i["telems"])}, dt))
    return cases


def nodevice_cases():
    """the forms that ask for a device, on a machine without one: each says so and leaves nothing behind"""
    i = inputs()
    files = {"c.nlzm": b"".join(i["streams"]), "c.nlzm.idx": index_text(i["lens"], SIZES, i["crcs"], i["whole"]), "a": i["text"][:5000]}
    runs = [["-gpu", "t", "c.nlzm"], ["-gpu", "d", "c.nlzm", "o.bin"], ["-gpu", "-steps:1", "t", "c.nlzm"], ["-gpu", "-steps:1", "d", "c.nlzm", "o.bin"],
            ["-gpu", "-range:0:10", "x", "c.nlzm", "p.bin"], ["-gpu", "h", "a"], ["c", "a", "a.nlzm"], ["-crc", "c", "a", "a.nlzm"], ["-blocks:3", "-verify", "c", "a", "a.nlzm"],
            ["-cdc:10", "-dedup", "c", "a", "a.nlzm"], ["-elem:4", "-blocks:2", "c", "a", "a.nlzm"], ["-gpus:2", "c", "a", "a.nlzm"], ["c", "missing", "a.nlzm"], ["-blocks:2", "c", "missing", "a.nlzm"]]
    return [("no device", files, runs)]


def gpu_cases():
    """well-formed small inputs through `c` in each of its forms, and every reader over each container written"""
    text = corpus.syn_text(100_003).tobytes()
    rep = corpus.mixed(24_000, corpus.SEED + 7).tobytes()
    repeated = rep + corpus.syn_text(8_000).tobytes() + rep + corpus.syn_text(8_001).tobytes()      # (about 64 KB, a region twice)
    typed = (np.arange(12_500) * 3 + 1000).astype("<i4").tobytes() + b"xyz"                      # (no multiple of 4)
    data_of = {"c alone": text[:50_000], "c -crc": text[:50_000], "c -blocks:3": text, "c -blocks:3 -verify": text, "c -cdc:10 -dedup": repeated,
               "c -elem:4 -blocks:2": typed, "c -cdc:10 -elem:2": typed}
    forms = {name: ([w for w in name.split() if w.startswith("-")], data_of[name]) for name in GPU_FORMS}
    cases = []
    for name, (flags, data) in forms.items():
        n = len(data)
        cases.append((name, {"a": data}, [flags + ["c", "a", "c.nlzm"], ["-gpu", "t", "c.nlzm"], ["-gpu", "d", "c.nlzm", "o.bin"], ["-gpu", "-steps:1", "t", "c.nlzm"],
                                          ["-gpu", "-steps:1", "d", "c.nlzm", "s.bin"], ["-gpu", "-range:5:1000", f"-range:{n - 7}:7", f"-range:{n // 2}:0", "x", "c.nlzm", "x.bin"],
                                          ["-gpu", "h", "a"], ["t", "c.nlzm"]]))
    return cases


SETS = {"cpu": (cpu_cases, "cli_transcripts.json"), "nodevice": (nodevice_cases, "cli_nodevice_transcripts.json"), "gpu": (gpu_cases, "cli_gpu_transcripts.json")}


def normalise(out):
    """timings read #.##; so does what c's progress line (the one a carriage return ends) says is written so far, which is the pipeline's pace"""
    return re.sub(r"(Working\.\.\. \d+ -> )\d+\r", r"\1#\r", re.sub(r"\d+\.\d\d\b", "#.##", out))


def run_case(cli_path, workdir, files, runs, timeout=60):
    """the case's transcript: run in `workdir`, which is made for it and holds `files`"""
    os.makedirs(workdir)
    for name, data in files.items():
        with open(os.path.join(workdir, name), "wb") as f:
            f.write(data)
    steps = []
    for argv in runs:
        r = subprocess.run([cli_path] + argv, cwd=workdir, capture_output=True, timeout=timeout)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):      # (killed, or aborted: nothing more is started)
            raise RuntimeError(f"{argv}: status {r.returncode}\n{r.stdout.decode('latin-1')}{r.stderr.decode('latin-1')}")
        out = r.stdout.decode("latin-1") + (("\n[stderr]\n" + r.stderr.decode("latin-1")) if r.stderr else "")
        steps.append({"argv": argv, "status": r.returncode, "stdout": normalise(out)})
    left = {}
    for name in sorted(os.listdir(workdir)):
        with open(os.path.join(workdir, name), "rb") as f:
            data = f.read()
        left[name] = f"{len(data)} {hashlib.sha256(data).hexdigest()}"
    return {"steps": steps, "files": left}


def record(which, cli_path, workdir):
    return {name: run_case(cli_path, os.path.join(workdir, f"{which}{n}"), files, runs) for n, (name, files, runs) in enumerate(SETS[which][0]())}


if __name__ == "__main__":
    import tempfile
    which, cli_path, dest = sys.argv[1:4]
    with tempfile.TemporaryDirectory() as tmp:
        got = record(which, os.path.abspath(cli_path), tmp)
    with open(dest, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases, {sum(len(c['steps']) for c in got.values())} invocations -> {dest}")
