"""CPU: the front-end's BAM output (-ot 4 / 8) against the test double of the device half (tests/stub_abi.cpp + the real reader and writer):
without --gpu-writer the run is refused with a message that names the switch, before any file is opened; with it the double has no GPU
side, so the run is refused for the missing device; the usage text lists the formats; -ot 2 gives the file it gave before."""
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
    so, exe = os.path.join(BUILD, "libstub_bam_linear_amd.so"), os.path.join(BUILD, "linear_filter_stub_bam")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "stub_abi.cpp"), os.path.join(CSRC, "lnr_reader.cpp"),
                           os.path.join(CSRC, "lnr_output.cpp"), "-o", so, "-lz", "-lpthread"])
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", exe, so, "-Wl,-rpath," + BUILD, "-lpthread"])
    return exe


def run(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def outputs(tmp_path, prefix):
    return sorted(f for f in os.listdir(tmp_path) if f.startswith(prefix + ".") or f.startswith(prefix + "_"))


@pytest.mark.parametrize("ot", ["4", "8", "6", "15"])
def test_bam_needs_the_gpu_writer(cli, tmp_path, ot):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", ot, "-o", str(tmp_path / "bm"), "--block-reads", "7"], tmp_path)
    assert p.returncode == 1, p.stderr.decode()
    assert b"BAM" in p.stderr and b"--gpu-writer" in p.stderr and b"not built" in p.stderr
    assert outputs(tmp_path, "bm") == []


@pytest.mark.parametrize("extra", [[], ["--sam-seq"], ["--bgzf"]])
def test_bam_with_the_gpu_writer_and_no_device(cli, tmp_path, extra):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "4", "-o", str(tmp_path / "bm"), "--block-reads", "7", "--gpu-writer"] + extra, tmp_path)
    assert p.returncode == 1 and b"no usable device" in p.stderr, p.stderr.decode()
    assert outputs(tmp_path, "bm") == []


def test_usage_lists_the_formats(cli, tmp_path):
    p = run(cli, ["filter", "-h", "x", "y"], tmp_path)
    assert p.returncode == 0 and b"4 .bam" in p.stderr and b"8 _pbsv.bam" in p.stderr and b"BAM needs --gpu-writer" in p.stderr


def test_ot_without_any_format_is_refused(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=20)
    p = run(cli, ["filter", reads[0], ref, "-ot", "16", "-o", str(tmp_path / "z")], tmp_path)
    assert p.returncode == 1 and b"not built" in p.stderr and outputs(tmp_path, "z") == []


def test_ot_2_is_unchanged(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    for tag in ("a", "b"):
        p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "2", "-o", str(tmp_path / tag), "--block-reads", "7"], tmp_path)
        assert p.returncode == 0, p.stderr.decode()
        assert outputs(tmp_path, tag) == [tag + ".sam"]
    a, b = open(tmp_path / "a.sam", "rb").read(), open(tmp_path / "b.sam", "rb").read()
    assert a == b and len(a) > 500 and a.startswith(b"@SQ\tSN:chrA\tLN:6000\n")
