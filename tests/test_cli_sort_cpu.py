"""CPU: the front-end's --sort switch against the test double of the device half (tests/stub_abi.cpp + the real reader and writer): without
--gpu-writer, and without -ot 4 / 8, the run is refused with a message that names what is missing and no file is created; with both the
double has no GPU side, so the run is refused for the missing device; the usage text lists the switch."""
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
    so, exe = os.path.join(BUILD, "libstub_sort_linear_amd.so"), os.path.join(BUILD, "linear_filter_stub_sort")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "stub_abi.cpp"), os.path.join(CSRC, "lnr_reader.cpp"),
                           os.path.join(CSRC, "lnr_output.cpp"), "-o", so, "-lz", "-lpthread"])
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", exe, so, "-Wl,-rpath," + BUILD, "-lpthread"])
    return exe


def run(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def outputs(tmp_path, prefix):
    return sorted(f for f in os.listdir(tmp_path) if f.startswith(prefix + ".") or f.startswith(prefix + "_"))


def test_sort_needs_the_gpu_writer(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    for pos in (0, 1):                                    # the switch takes no value, in any position
        args = ["filter", reads[0], ref, "-t", "2", "-ot", "6", "-o", str(tmp_path / "so"), "--block-reads", "7"]
        args.insert(1 if pos else len(args), "--sort")
        p = run(cli, args, tmp_path)
        assert p.returncode == 1, p.stderr.decode()
        assert b"--sort" in p.stderr and b"--gpu-writer" in p.stderr
        assert outputs(tmp_path, "so") == []


@pytest.mark.parametrize("ot", ["1", "2", "3"])
def test_sort_needs_bam_output(cli, tmp_path, ot):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", ot, "-o", str(tmp_path / "so"), "--sort", "--gpu-writer"], tmp_path)
    assert p.returncode == 1, p.stderr.decode()
    assert b"--sort" in p.stderr and b"-ot" in p.stderr and b"4" in p.stderr and b"8" in p.stderr and b"no usable device" not in p.stderr
    assert outputs(tmp_path, "so") == []


def test_sort_with_everything_and_no_device(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "12", "-o", str(tmp_path / "so"), "--sort", "--gpu-writer"], tmp_path)
    assert p.returncode == 1 and b"no usable device" in p.stderr, p.stderr.decode()
    assert outputs(tmp_path, "so") == []


def test_usage_lists_the_switch(cli, tmp_path):
    p = run(cli, ["filter", "-h", "x", "y"], tmp_path)
    assert p.returncode == 0 and b"MI355X front-end" in p.stderr
    tail = p.stderr.split(b"MI355X front-end")[1]
    assert b"--sort" in tail and b".bam.bai" in tail and b"GPU memory" in tail
