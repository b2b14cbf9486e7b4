"""CPU: the front-end's --sam-seq switch against the test double of the device half (tests/stub_abi.cpp; reader and writer are the real host
code, built as in tests/test_cli_frontend_cpu.py): the .sam carries a SEQ column of the length its CIGAR implies, made of the read's and the
genome's bases; the output does not depend on --block-reads or --gpus; -ss itself is still refused."""
import os
import subprocess

import pytest

from tests import writer_seq_cases as sc
from tests.test_cli_frontend_cpu import BUILD, CSRC, ROOT, run, write_inputs


@pytest.fixture(scope="module")
def cli():
    os.makedirs(BUILD, exist_ok=True)
    so, exe = os.path.join(BUILD, "libstub_linear_amd_seq.so"), os.path.join(BUILD, "linear_filter_stub_seq")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "stub_abi.cpp"), os.path.join(CSRC, "lnr_reader.cpp"),
                           os.path.join(CSRC, "lnr_output.cpp"), "-o", so, "-lz", "-lpthread"])
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", exe, so, "-Wl,-rpath," + BUILD, "-lpthread"])
    return exe


def test_sam_seq_switch(cli, tmp_path):
    reads, ref = write_inputs(tmp_path)
    outs = {}
    for tag, extra in {"plain": [], "seq": ["--sam-seq"], "seq_b7": ["--sam-seq", "--block-reads", "7"], "seq_g3": ["--sam-seq", "--gpus", "3", "--block-reads", "5"]}.items():
        p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / tag), "-g", "0"] + extra, tmp_path)
        assert p.returncode == 0, p.stderr.decode()
        outs[tag] = (open(tmp_path / (tag + ".sam"), "rb").read(), open(tmp_path / (tag + ".apf"), "rb").read())
    assert outs["seq_b7"][0] == outs["seq"][0] and outs["seq_g3"][0] == outs["seq"][0]      # (the .apf's blank lines follow the blocks, with or without the switch)
    assert outs["seq"][1] == outs["plain"][1]                                 # .apf is not affected
    assert sc.star_seq(outs["seq"][0]) == outs["plain"][0] and outs["seq"][0] != outs["plain"][0]
    text = {l.split(b" ")[0][1:]: s for l, s in zip(*[iter(open(reads[0], "rb").read().split(b"\n"))] * 2)}
    recs = [l.split(b"\t") for l in outs["seq"][0].split(b"\n") if l and not l.startswith(b"@")]
    assert len(recs) > 200
    for f in recs:
        assert len(f[9]) == sc.seq_len_of_cigar(f[5]) > 0 and set(f[9]) <= set(b"ACGTN")
        read = text[f[0].split(b" ")[0]]
        lead = int(f[5].split(b"S")[0]) if b"S" in f[5].split(b"=")[0] else 0
        assert f[9][:lead] == read[:lead]                                    # the leading clip prints the read (the double's cords are forward)
    # the usage text names the switch next to -ss
    assert b"--sam-seq" in run(cli, ["-h", "x", "y"], tmp_path).stderr


def test_ss_is_still_refused(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=5)
    for args in (["-ss"], ["-ss", "1"], ["--sam-seq", "-ss"]):
        p = run(cli, ["filter", reads[0], ref] + args, tmp_path)
        assert p.returncode == 1 and b"not built" in p.stderr, args
