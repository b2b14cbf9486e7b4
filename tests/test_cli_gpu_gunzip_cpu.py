"""CPU: the front-end's --gpu-gunzip switch against the test double of the device half (tests/stub_abi.cpp + the real reader and writer):
without --gpu-reader the run is refused with a message that names both switches; with it the double has no device chain, so the run is
refused for the missing device; no output is left behind either way; the usage text lists the switch; a run without it reads a plain
.gz file through gzread and gives the files it gives for the plain text.  Against the same double, lnr_gunzip_gpu and the reader's switch
answer "no device" and "not before lnr_reader_gpu_open"."""
import ctypes as C
import gzip
import os
import subprocess

import pytest

from tests.test_cli_frontend_cpu import write_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CSRC = os.path.join(ROOT, "linear_amd", "csrc")
SO = os.path.join(BUILD, "libstub_gunzip_linear_amd.so")


@pytest.fixture(scope="module")
def cli():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "linear_filter_stub_gunzip")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "stub_abi.cpp"), os.path.join(CSRC, "lnr_reader.cpp"),
                           os.path.join(CSRC, "lnr_output.cpp"), "-o", SO, "-lz", "-lpthread"])
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", exe, SO, "-Wl,-rpath," + BUILD, "-lpthread"])
    return exe


def run(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def outputs(tmp_path, prefix):
    return sorted(f for f in os.listdir(tmp_path) if f.startswith(prefix + "."))


def test_gpu_gunzip_needs_the_gpu_reader(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    for pos in (0, 1):                                    # the switch takes no value, in any position
        args = ["filter", reads[0], ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / "gz"), "--block-reads", "7"]
        args.insert(1 if pos else len(args), "--gpu-gunzip")
        p = run(cli, args, tmp_path)
        assert p.returncode == 1, p.stderr.decode()
        assert b"--gpu-gunzip" in p.stderr and b"--gpu-reader" in p.stderr
        assert outputs(tmp_path, "gz") == []


def test_gpu_gunzip_with_the_gpu_reader_and_no_device(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / "gz"), "--block-reads", "7", "--gpu-gunzip", "--gpu-reader"], tmp_path)
    assert p.returncode == 1 and b"no usable device" in p.stderr, p.stderr.decode()
    assert outputs(tmp_path, "gz") == []


def test_usage_lists_the_switch(cli, tmp_path):
    p = run(cli, ["filter", "-h", "x", "y"], tmp_path)
    assert p.returncode == 0 and b"MI355X front-end" in p.stderr
    tail = p.stderr.split(b"MI355X front-end")[1]
    assert b"--gpu-gunzip" in tail and b"plain gzip" in tail and b"needs --gpu-reader" in tail


def test_without_the_switch_a_gz_file_is_read_through_gzread(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    zp = str(tmp_path / "reads_z.fa.gz")
    with open(zp, "wb") as f:
        f.write(gzip.compress(open(reads[0], "rb").read()))
    for tag, path in (("a", reads[0]), ("b", zp)):
        p = run(cli, ["filter", path, ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / tag), "--block-reads", "7"], tmp_path)
        assert p.returncode == 0, p.stderr.decode()
        assert outputs(tmp_path, tag) == [tag + ".apf", tag + ".sam"]
    for ext in (".sam", ".apf"):
        a, b = open(tmp_path / ("a" + ext), "rb").read(), open(tmp_path / ("b" + ext), "rb").read()
        assert a == b and len(a) > 500


def test_abi_without_the_device_half(cli, tmp_path):
    lib = C.CDLL(SO)
    lib.lnr_gunzip_gpu.argtypes = [C.c_int32, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_char_p, C.c_size_t]
    raw = gzip.compress(b">r\nACGT\n")
    out, err, n = C.create_string_buffer(64), C.create_string_buffer(256), C.c_uint64(7)
    assert lib.lnr_gunzip_gpu(0, raw, len(raw), out, 64, C.byref(n), None, err, 256) == -2 and n.value == 0 and b"device" in err.value
    assert lib.lnr_gunzip_gpu(0, raw, len(raw), out, 64, None, None, err, 256) == -1
    p = str(tmp_path / "r.fa.gz")
    with open(p, "wb") as f:
        f.write(raw)
    lib.lnr_reader_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.lnr_reader_gpu_gzip.argtypes = [C.c_void_p, C.c_int]
    lib.lnr_reader_close.argtypes = [C.c_void_p]
    lib.lnr_reader_error.argtypes = [C.c_void_p]
    lib.lnr_reader_error.restype = C.c_char_p
    r = C.c_void_p()
    assert lib.lnr_reader_open(p.encode(), C.byref(r)) == 0
    assert lib.lnr_reader_gpu_gzip(r, 1) == -1 and b"lnr_reader_gpu_open" in lib.lnr_reader_error(r)
    lib.lnr_reader_close(r)
