"""CPU suite: the sidecar index's one parser, two validators and one writer (nlzm_amd/csrc/nlzm_index.h), which the command line runs.  The header is
plain C++ with no device in it; the harness (tests/host_sim/index_sim.cpp) is a program of its own under AddressSanitizer and UBSan and includes the
header the command line includes.

The round trip (in the harness): the three layouts and the one-stream form word for word, and writer -> parser for 1, 5 and 300 blocks.  Here: the
malformed indexes that tests/test_range_abi.py::test_read_index and tests/test_planes_abi.py::test_read_index_typed give nlzm_amd.read_index*, each
through both validators, as x takes an index (versions 1 and 2, 65,536 blocks, nothing behind the last entry, the container not looked at) and as
d / t take one (versions 1 to 3, 4096 blocks, fields behind the last entry let pass, against the container's bytes).  What is expected below is what
these readers have done since they were written, scanf's reading of a number included: it takes a sign, and a number too large saturates (a field
beyond 64 bits reads as 2^64 - 1, a CRC beyond 32 bits loses its upper bits), where nlzm_amd.read_index* refuses both."""
import os
import re

import pytest

from tests import simkit
from tests.cli_tools import index_text

M = 1 << 64


@pytest.fixture(scope="module")
def sim():
    sim, = simkit.build("index_sim_san")
    assert "-fsanitize=address,undefined" in simkit.compiled_with("index_sim_san")
    assert "nlzm_amd/csrc/nlzm_index.h" in simkit.compiled_from("index_sim_san")
    return sim


def run(sim, *args):
    r = simkit.sh([sim, *args], 120)
    assert r.returncode == 0 and "index_sim: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def judge(sim, tmp_path, text, size):
    """((x structural, x fits_file blocks), (d structural, d fits_file blocks, d cut_tail)), and the parser's line"""
    p = tmp_path / "c.idx"
    p.write_text(text)
    out = run(sim, "judge", p, size)
    v = {who: tuple(map(int, re.search(rf"^{who}: structural=(\d) fits_file=(\d+) cut_tail=(\d+)$", out, re.M).groups())) for who in "xd"}
    return (v["x"][:2], v["d"]), re.search(r"^parsed (.*)$", out, re.M).group(1)


def test_round_trip(sim):
    assert re.search(r"roundtrip: cases=9", run(sim, "roundtrip"))


def test_command_line_and_harness_read_one_header():
    csrc = os.path.join(simkit.ROOT, "nlzm_amd", "csrc")
    cli = open(os.path.join(csrc, "nlzm_cli.cpp")).read()
    assert '#include "nlzm_index.h"' in cli and "index::structural(" in cli and "index::fits_file(" in cli and "index::write(" in cli
    assert "fscanf" not in cli and "NLZMIDX %u" not in cli              # (no reader or writer of its own left)
    assert "kExtractTakes{ 2, nlzm::container::kMaxBlocks, false }" in cli and "kDecodeTakes{ 3, 4096, true }" in cli      # (what index_sim.cpp restates)
    sim = open(os.path.join(simkit.SIMDIR, "index_sim.cpp")).read()
    assert "kX{ 2, 65536, false }, kD{ 3, 4096, true }" in sim and "nlzm_index.h" in sim


LENS, RAWS, CRCS = [12, 8, 30], [10, 0, 20], [1, 2, 3]
N_OUT, N_IN = sum(LENS), sum(RAWS)
NO = ((0, 0), (0, 0, 0))


def test_well_formed_indexes(sim, tmp_path):
    for version in (1, 2, 3):
        text = index_text(LENS, RAWS, CRCS, 0xABCD, version=version, elems=[2, 4, 8])
        got, parsed = judge(sim, tmp_path, text, N_OUT)
        x = (lambda blocks: (1, blocks)) if version <= 2 else (lambda blocks: (0, 0))      # (x does not read typed blocks)
        assert got == (x(3), (1, 3, 0)) and parsed == f"version={version} header=1 k=3 entries=3 trailing=0", (version, got, parsed)
        # the container cut off inside block 3, and inside block 1: the index still agrees with itself, which is all x asks; against the file it
        # gives the blocks in front of the cut, if there is one
        assert judge(sim, tmp_path, text, LENS[0] + LENS[1] + 5)[0] == (x(2), (1, 2, 5)), version
        assert judge(sim, tmp_path, text, 5)[0] == (x(0), (1, 0, 0)), version
        # a container with bytes behind the last block does not fit
        assert judge(sim, tmp_path, text, N_OUT + 1)[0] == (x(0), (1, 0, 0)), version


def test_block_caps(sim, tmp_path):
    for k, d in ((4096, (1, 4096, 0)), (4097, (0, 0, 0)), (65536, (0, 0, 0))):
        assert judge(sim, tmp_path, index_text([8] * k, [0] * k, version=1), 8 * k)[0] == ((1, k), d), k
    assert judge(sim, tmp_path, index_text([8] * 65537, [0] * 65537, version=1), 8 * 65537)[0] == NO


def test_malformed_indexes(sim, tmp_path):
    """(text, container size, x's verdicts, d's): the lists of test_read_index and test_read_index_typed"""
    cases = {
        "raw lengths over n_in": (index_text(LENS, RAWS, version=1, n_in=N_IN - 1), N_OUT, NO),
        "raw lengths under n_in": (index_text(LENS, RAWS, version=1, n_in=N_IN + 1), N_OUT, NO),
        "block lengths under n_out": (index_text(LENS, RAWS, version=1, n_out=N_OUT + 1), N_OUT, NO),
        "a gap between two blocks": (index_text(LENS, RAWS, version=1, offs=[0, 12, 21]), N_OUT, NO),
        # d / t read a block that claims more bytes than the file has left as "the file is cut inside it": block 1 is decoded
        "an off + len that wraps": (f"NLZMIDX 1 2 100 {M - 1}\n0 50 60\n50 {M - 40} 40\n", 100, ((0, 1), (0, 1, 50))),
        "an off + len that wraps, typed": (f"NLZMIDX 3 2 100 {M - 1} 00000000\n0 50 60 00000000 2\n50 {M - 40} 40 00000000 2\n", 100, ((0, 0), (0, 1, 50))),
        "raw lengths whose sum wraps": (f"NLZMIDX 1 2 {M - 1} 100\n0 50 {M - 5}\n50 50 10\n", 100, NO),
        "raw lengths whose sum wraps, typed": (f"NLZMIDX 3 2 {M - 1} 100 00000000\n0 50 {M - 5} 00000000 2\n50 50 10 00000000 2\n", 100, NO),
        # scanf saturates: n_out and the block's length both read 2^64 - 1, and the index agrees with itself; no file is that long
        "a field beyond 64 bits": (f"NLZMIDX 1 1 10 {M + 8}\n0 {M + 8} 10\n", 100, ((1, 0), (1, 0, 0))),
        "a field beyond 64 bits, typed": (f"NLZMIDX 3 1 10 {M + 8} 00000000\n0 {M + 8} 10 00000000 2\n", 100, ((0, 0), (1, 0, 0))),
        "a CRC32 beyond 32 bits": ("NLZMIDX 2 1 10 8 100000000\n0 8 10 00000000\n", 8, ((1, 1), (1, 1, 0))),
        "a CRC32 beyond 32 bits, typed": ("NLZMIDX 3 1 10 8 100000000\n0 8 10 00000000 2\n", 8, ((0, 0), (1, 1, 0))),
        "no element size": ("NLZMIDX 3 1 10 8 00000000\n0 8 10 00000000\n", 8, NO),
        "an element size that is none": ("NLZMIDX 3 1 10 8 00000000\n0 8 10 00000000 3\n", 8, NO),
        "no CRC32 of the whole file": ("NLZMIDX 3 1 10 8\n0 8 10 00000000 2\n", 8, NO),
        "no CRC32 of the whole file, version 2": ("NLZMIDX 2 1 10 8\n0 8 10 00000000\n", 8, NO),
        "a field too few": ("NLZMIDX 1 2 30 20\n0 12 10\n12 8\n", 20, NO),
        # x refuses fields behind the last block, d / t let them pass
        "a field too many": ("NLZMIDX 2 1 10 8 00000000\n0 8 10 00000000 7\n", 8, ((0, 0), (1, 1, 0))),
        "a field too many, typed": ("NLZMIDX 3 1 10 8 00000000\n0 8 10 00000000 2 7\n", 8, ((0, 0), (1, 1, 0))),
        "version 4": ("NLZMIDX 4 1 10 8 00000000\n0 8 10 00000000 2\n", 8, NO),
        "no index at all": ("hello\n", 8, NO),
    }
    for what, (text, size, want) in cases.items():
        got, parsed = judge(sim, tmp_path, text, size)
        assert got == want, (what, got, parsed)
    # the version is known as soon as the header word is read, whatever follows: d and x word their errors from it
    assert judge(sim, tmp_path, "NLZMIDX 3 junk\n", 8)[1].startswith("version=3 header=0 ")
    assert judge(sim, tmp_path, "NLZMIDX 4 1 10 8\n", 8)[1].startswith("version=4 header=0 ")
