"""bench.py's input: stand_in makes syn_text's text blocks in worker processes and must give exactly corpus.syn_text's bytes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("size, seed_off, workers", [
    (3 * (8 << 20) + 12_345, 0, 3),      # two blocks made by workers (one worker idle), a short last one made in place
    (60_000_000, 7, 4),                  # five blocks on four workers (one makes two), another seed
    (5_000_000, 0, 4),                   # one block: syn_text itself
])
def test_stand_in_is_syn_text(size, seed_off, workers):
    # (in a process of its own: stand_in forks, and this one may have the GPU open already)
    code = ("import numpy as np, bench; from nlzm_amd import corpus; s = corpus.SEED + %d; "
            "assert np.array_equal(bench.stand_in(%d, s, %d), corpus.syn_text(%d, s)); "
            "assert corpus._text_block.__name__ == '_text_block'" % (seed_off, size, workers, size))
    r = subprocess.run([sys.executable, "-s", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
