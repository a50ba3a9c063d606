"""CPU suite: the kit under the host simulators itself.  The guarded buffer (tests/host_sim/sim_kit.h) is what every out-of-bounds claim of the CPU
suite rests on, and the dependency files the compiler writes (tests/host_sim/Makefile) are what keeps a built program from outliving a header
it was compiled from: both are held to their promises here."""
import os
import re

from tests import simkit


def test_guarded_buffer_keeps_its_promises():
    """A buffer in each of the three places: its address, its fill, intact(), and intact() turning false after one byte written just outside it
    (kit_sim.cpp, under AddressSanitizer and UBSan).  Asked to, the program reads the first byte of the PROT_NONE page behind a kBack buffer and
    must end with SIGSEGV: host code in a child process, which is where faults belong.  (AddressSanitizer would catch the signal, print a
    report and leave with status 1; handle_segv=0 leaves the signal to the system, as in the UBSan builds of the simulators.)"""
    sim, = simkit.build("kit_sim_san")
    assert "-fsanitize=address,undefined" in simkit.compiled_with("kit_sim_san")
    r = simkit.sh([sim], 60)
    assert r.returncode == 0 and "kit_sim: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = simkit.sh([sim, "behind"], 60, {"ASAN_OPTIONS": "handle_segv=0"})
    assert r.returncode == -11 and "OK" not in r.stdout and "FAIL" not in r.stdout, (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])


def included(source):
    """the files a source of tests/host_sim includes by name, as paths from the repository's root"""
    text = open(os.path.join(simkit.SIMDIR, source)).read()
    return {os.path.relpath(os.path.realpath(os.path.join(simkit.SIMDIR, h)), simkit.ROOT) for h in re.findall(r'^#include "([^"]+)"', text, re.M)}


def test_a_program_depends_on_what_it_was_compiled_from():
    """Two programs with fibers (two sources on one compile line would leave the first one's headers out of the dependency file): each one's file
    names its own source, the fiber runtime, the kit and every header the source includes, and not the header only the other one reads."""
    programs = {"crc_sim_san": ("crc_sim.cpp", "nlzm_amd/csrc/nlzm_crc.h"), "cut_sim_san": ("cut_sim.cpp", "nlzm_amd/csrc/nlzm_cut.h")}
    simkit.build(*programs, jobs=2)
    for program, (source, own) in programs.items():
        line, deps = simkit.compiled_with(program).split(), simkit.compiled_from(program)
        assert [w for w in line if w.endswith((".cpp", ".o"))] == [source], line      # (one translation unit: one dependency file covers the program)
        direct = included(source)
        assert {own, "tests/host_sim/xw_sim.cpp", "tests/host_sim/sim_kit.h"} <= direct, direct      # (what this test counts on)
        assert {"tests/host_sim/" + source, own, "nlzm_amd/csrc/xw.h"} | direct <= deps, sorted(direct - deps)
        other = next(o for p, (_, o) in programs.items() if p != program)
        assert other not in deps, (program, other)
