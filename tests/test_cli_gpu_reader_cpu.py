"""CPU: the front-end's --gpu-reader switch against the test double of the device half (tests/stub_abi.cpp + the real reader and writer): the
double has neither the device form of the filter nor the reader's GPU side, and the front-end refers to both weakly, so it still links; the
switch is refused with exit code 1 and a message that names it, before any output file exists.  Without the switch nothing changes."""
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
    so, exe = os.path.join(BUILD, "libstub_gpur_linear_amd.so"), os.path.join(BUILD, "linear_filter_stub_gpur")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "stub_abi.cpp"), os.path.join(CSRC, "lnr_reader.cpp"),
                           os.path.join(CSRC, "lnr_output.cpp"), "-o", so, "-lz", "-lpthread"])
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", exe, so, "-Wl,-rpath," + BUILD, "-lpthread"])
    return exe


def run(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_gpu_reader_switch_without_a_gpu_side(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    common = ["filter", reads[0], ref, "-t", "2", "-ot", "3", "--block-reads", "7"]
    base = run(cli, common + ["-o", str(tmp_path / "plain")], tmp_path)
    assert base.returncode == 0, base.stderr.decode()
    for extra in (["--gpu-reader"], ["--gpu-reader", "--gpu-writer"], ["--gpu-reader", "-g", "0"]):
        p = run(cli, common + ["-o", str(tmp_path / "gr")] + extra, tmp_path)
        assert p.returncode == 1, p.stderr.decode()
        assert b"--gpu-reader" in p.stderr or b"--gpu-writer" in p.stderr
        if "--gpu-writer" not in extra:
            assert b"--gpu-reader" in p.stderr and b"no usable device" in p.stderr
        assert not os.path.exists(tmp_path / "gr.sam") and not os.path.exists(tmp_path / "gr.apf")      # nothing half written
    # the switch takes no value: what follows it is still read as an argument
    p = run(cli, ["filter", "--gpu-reader", reads[0], ref, "-ot", "2", "-o", str(tmp_path / "gr2")], tmp_path)
    assert p.returncode == 1 and b"--gpu-reader" in p.stderr and not os.path.exists(tmp_path / "gr2.sam")
    # without it: the same run gives the same files again
    again = run(cli, common + ["-o", str(tmp_path / "plain2")], tmp_path)
    assert again.returncode == 0
    for ext in (".sam", ".apf"):
        a, b = open(tmp_path / ("plain" + ext), "rb").read(), open(tmp_path / ("plain2" + ext), "rb").read()
        assert a == b and len(a) > 500


def test_usage_lists_the_switch(cli, tmp_path):
    p = run(cli, ["filter", "-h", "x", "y"], tmp_path)
    tail = p.stderr.split(b"MI355X front-end")[1]
    assert p.returncode == 0 and b"--gpu-reader" in tail and tail.index(b"--gpu-writer") < tail.index(b"--gpu-reader") < tail.index(b"--sam-seq")
