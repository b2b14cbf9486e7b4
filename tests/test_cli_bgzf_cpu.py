"""CPU: the front-end's --bgzf switch against the test double of the device half (tests/stub_abi.cpp + the real reader and writer): without
--gpu-writer the run is refused with a message that names both switches; with it the double has no GPU side, so the run is refused for the
missing device; no .gz file (nor any other output) is left behind either way; the usage text lists the switch; a run without it gives the
files it gave before."""
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
    so, exe = os.path.join(BUILD, "libstub_bgzf_linear_amd.so"), os.path.join(BUILD, "linear_filter_stub_bgzf")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "stub_abi.cpp"), os.path.join(CSRC, "lnr_reader.cpp"),
                           os.path.join(CSRC, "lnr_output.cpp"), "-o", so, "-lz", "-lpthread"])
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", exe, so, "-Wl,-rpath," + BUILD, "-lpthread"])
    return exe


def run(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def outputs(tmp_path, prefix):
    return sorted(f for f in os.listdir(tmp_path) if f.startswith(prefix + "."))


def test_bgzf_needs_the_gpu_writer(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    for pos in (0, 1):                                    # the switch takes no value, in any position
        args = ["filter", reads[0], ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / "bz"), "--block-reads", "7"]
        args.insert(1 if pos else len(args), "--bgzf")
        p = run(cli, args, tmp_path)
        assert p.returncode == 1, p.stderr.decode()
        assert b"--bgzf" in p.stderr and b"--gpu-writer" in p.stderr
        assert outputs(tmp_path, "bz") == []


def test_bgzf_with_the_gpu_writer_and_no_device(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / "bz"), "--block-reads", "7", "--bgzf", "--gpu-writer"], tmp_path)
    assert p.returncode == 1 and b"no usable device" in p.stderr, p.stderr.decode()
    assert outputs(tmp_path, "bz") == []


def test_usage_lists_the_switch(cli, tmp_path):
    p = run(cli, ["filter", "-h", "x", "y"], tmp_path)
    assert p.returncode == 0 and b"MI355X front-end" in p.stderr
    tail = p.stderr.split(b"MI355X front-end")[1]
    assert b"--bgzf" in tail and b".sam.gz" in tail


def test_without_the_switch_nothing_changes(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    for tag in ("a", "b"):
        p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / tag), "--block-reads", "7"], tmp_path)
        assert p.returncode == 0, p.stderr.decode()
        assert outputs(tmp_path, tag) == [tag + ".apf", tag + ".sam"]
    for ext in (".sam", ".apf"):
        a, b = open(tmp_path / ("a" + ext), "rb").read(), open(tmp_path / ("b" + ext), "rb").read()
        assert a == b and len(a) > 500 and not a.startswith(b"\x1f\x8b")
