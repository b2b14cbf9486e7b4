"""CPU: the front-end's --gpu-genome switch against the test double of the device half (tests/stub_abi.cpp + the real reader and writer): the
double has no genome loader (lnr_genome_*: linear_amd/csrc/lnr_genome.cpp is not part of it) and the front-end refers to those entry points
weakly, so it still links; the switch is refused with exit code 1 and a message that names it, before any output file exists.  The usage
text lists the switch; --gpu-gunzip still needs one of --gpu-reader / --gpu-genome; without the switch nothing changes and the load time is
printed."""
import os
import subprocess

import pytest

from tests.test_cli_frontend_cpu import write_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CSRC = os.path.join(ROOT, "linear_amd", "csrc")


@pytest.fixture(scope="module")
def cli():
    os.makedirs(BUILD, exist_ok=True)
    so, exe = os.path.join(BUILD, "libstub_gpug_linear_amd.so"), os.path.join(BUILD, "linear_filter_stub_gpug")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "stub_abi.cpp"), os.path.join(CSRC, "lnr_reader.cpp"),
                           os.path.join(CSRC, "lnr_output.cpp"), "-o", so, "-lz", "-lpthread"])
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", exe, so, "-Wl,-rpath," + BUILD, "-lpthread"])
    return exe


def run(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_gpu_genome_switch_without_a_loader(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    common = ["filter", reads[0], ref, "-t", "2", "-ot", "3", "--block-reads", "7"]
    base = run(cli, common + ["-o", str(tmp_path / "plain")], tmp_path)
    assert base.returncode == 0, base.stderr.decode()
    assert b"Genome loaded in" in base.stderr and b"End creating index" in base.stderr
    for extra in (["--gpu-genome"], ["--gpu-genome", "--gpu-gunzip"], ["--gpu-genome", "-g", "0", "--sam-seq"]):
        p = run(cli, common + ["-o", str(tmp_path / "gg")] + extra, tmp_path)
        assert p.returncode == 1, p.stderr.decode()
        assert b"--gpu-genome" in p.stderr and b"no genome loader" in p.stderr
        assert not os.path.exists(tmp_path / "gg.sam") and not os.path.exists(tmp_path / "gg.apf")      # nothing half written
    # the switch takes no value: what follows it is still read as an argument
    p = run(cli, ["filter", "--gpu-genome", reads[0], ref, "-ot", "2", "-o", str(tmp_path / "gg2")], tmp_path)
    assert p.returncode == 1 and b"--gpu-genome" in p.stderr and not os.path.exists(tmp_path / "gg2.sam")
    # without it: the same run gives the same files again
    again = run(cli, common + ["-o", str(tmp_path / "plain2")], tmp_path)
    assert again.returncode == 0
    for ext in (".sam", ".apf"):
        a, b = open(tmp_path / ("plain" + ext), "rb").read(), open(tmp_path / ("plain2" + ext), "rb").read()
        assert a == b and len(a) > 500


def test_usage_lists_the_switch(cli, tmp_path):
    p = run(cli, ["filter", "-h", "x", "y"], tmp_path)
    tail = p.stderr.split(b"MI355X front-end")[1]
    assert p.returncode == 0 and tail.count(b"    --gpu-genome ") == 1
    assert tail.index(b"    --gpu-gunzip ") < tail.index(b"    --gpu-genome ") < tail.index(b"    --sam-seq ")


def test_gpu_gunzip_alone_is_still_refused(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=10)
    p = run(cli, ["filter", reads[0], ref, "-ot", "2", "-o", str(tmp_path / "gz"), "--gpu-gunzip"], tmp_path)
    assert p.returncode == 1 and b"--gpu-gunzip" in p.stderr and b"--gpu-reader" in p.stderr and b"--gpu-genome" in p.stderr
    assert not os.path.exists(tmp_path / "gz.sam")
