"""The command line against its own earlier output: every case of tests/cli_transcripts.py run again and compared with the transcript under
tests/golden/ -- stdout (timings aside), exit status, and every file left behind, by presence and by bytes.  A change to nlzm_cli.cpp or
nlzm_index.h that moves a message, a status, an output file or an index byte fails here; one that means to records the transcripts anew (the
module's docstring says how) and says so."""
import json
import os

import pytest

import nlzm_amd
from tests import cli_transcripts


@pytest.fixture(scope="module")
def cli_path():
    nlzm_amd.build()
    return nlzm_amd.CLI_PATH


def golden(which):
    with open(os.path.join(cli_transcripts.GOLDEN, cli_transcripts.SETS[which][1])) as f:
        return json.load(f)


def replay(which, cli_path, tmp_path_factory, only=None):
    want = golden(which)
    cases = cli_transcripts.SETS[which][0]()
    assert sorted(want) == sorted(name for name, _, _ in cases)
    for n, (name, files, runs) in enumerate(cases):
        if only is not None and name != only:
            continue
        got = cli_transcripts.run_case(cli_path, str(tmp_path_factory.mktemp(which) / f"case{n}"), files, runs)
        for g, w in zip(got["steps"], want[name]["steps"]):
            assert g == w, (name, g["argv"])
        assert got == want[name], name


def test_host_only_transcripts(cli_path, tmp_path_factory):
    replay("cpu", cli_path, tmp_path_factory)


def test_device_forms_without_a_device(cli_path, tmp_path_factory):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    replay("nodevice", cli_path, tmp_path_factory)


@pytest.mark.gpu
@pytest.mark.parametrize("form", cli_transcripts.GPU_FORMS)
def test_gpu_transcripts(form, tmp_path_factory):
    """`c` in the form named, then t, d, d in steps, x and h on the device over what it wrote: the container and the index byte for byte too"""
    replay("gpu", nlzm_amd.CLI_PATH, tmp_path_factory, only=form)
