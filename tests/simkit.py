"""What the CPU suites of tests/host_sim share: building the programs a module asks for (tests/host_sim/Makefile), what a program was
compiled with and from, running them, and the runs a module starts together."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMDIR = os.path.join(ROOT, "tests", "host_sim")


def sh(cmd, timeout=600, env=None):
    return subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env) if env else None)


def build(*programs, jobs=4):
    """make exactly these programs (what is up to date stays); returns their paths"""
    assert programs
    r = subprocess.run(["make", f"-j{min(jobs, 16)}", "-C", SIMDIR] + list(programs), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [os.path.join(SIMDIR, p) for p in programs]


def compiled_with(program):
    """the compile line make runs for this program"""
    r = subprocess.run(["make", "-n", "-B", "-C", SIMDIR, program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if f" -o {program} " in l + " "]
    assert len(lines) == 1, r.stdout
    return lines[0]


def compiled_from(program):
    """the files the program, built now if it is not up to date, was compiled from (the dependency file its compile line wrote), as paths
    from the repository's root"""
    build(program)
    words = open(os.path.join(SIMDIR, program + ".d")).read().replace("\\\n", " ").split("\n")[0].split()
    assert words[0] == program + ":", words[:2]
    return {os.path.relpath(os.path.realpath(os.path.join(SIMDIR, w)), ROOT) for w in words[1:]}


class Runs:
    """Runs of a module (one process each) that are started together, a few beside each other in the order they are submitted; every
    test takes the result of its own."""

    def __init__(self, workers):
        self.pool = ThreadPoolExecutor(workers)
        self.futs = {}

    def submit(self, key, cmd, env=None, timeout=600):
        assert key not in self.futs
        self.futs[key] = self.pool.submit(sh, cmd, timeout, env)

    def ok(self, key, marker):
        """the finished run, which ended with status 0 and printed the marker (3 / 4: the simulator's own checks and its watchdog; -11: an
        access left a guarded buffer)"""
        r = self.futs[key].result()
        assert r.returncode == 0 and marker in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        return r

    def close(self):
        self.pool.shutdown(wait=False, cancel_futures=True)
