"""CPU: the front-end's --paf switch against the test double of the device half (tests/stub_abi.cpp + the real reader and writer, built as in
tests/test_cli_frontend_cpu.py): the usage text lists the switch; against a library without the PAF entry points (the same double with
the three symbols kept local by a linker version script) the run is refused with a message before any output file is opened; a run without
the switch leaves no .paf and the files it left before; with it, on the host path, the .paf is the Python derivation (tests/paf_cases.py) of
the same run's .sam -- per read file without -o, in one file with it --, and the .sam and .apf are those of the run without it."""
import os
import subprocess

import pytest

from tests import paf_cases as pc
from tests.test_cli_frontend_cpu import BUILD, CSRC, ROOT, run, write_inputs

PAF_SYMBOLS = ("lnr_writer_format_paf", "lnr_writer_format_paf_gpu", "lnr_writer_format_paf_dev")


def build_double(tag, link_extra=()):
    os.makedirs(BUILD, exist_ok=True)
    so, exe = os.path.join(BUILD, f"libstub_{tag}_linear_amd.so"), os.path.join(BUILD, f"linear_filter_stub_{tag}")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "stub_abi.cpp"), os.path.join(CSRC, "lnr_reader.cpp"),
                           os.path.join(CSRC, "lnr_output.cpp"), "-o", so, "-lz", "-lpthread"] + list(link_extra))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", exe, so, "-Wl,-rpath," + BUILD, "-lpthread"])
    return so, exe


@pytest.fixture(scope="module")
def cli():
    return build_double("paf")[1]


@pytest.fixture(scope="module")
def cli_without_paf():
    """the double as a library of before: the three entry points are not exported"""
    script = os.path.join(BUILD, "no_paf.map")
    os.makedirs(BUILD, exist_ok=True)
    with open(script, "w") as f:
        f.write("{ local: " + " ".join(s + ";" for s in PAF_SYMBOLS) + " };\n")
    so, exe = build_double("nopaf", ["-Wl,--version-script=" + script])
    exported = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    assert "lnr_writer_format_gpu" in exported and not any(s + "\n" in exported for s in PAF_SYMBOLS)
    return exe


def outputs(tmp_path, prefix):
    return sorted(f for f in os.listdir(tmp_path) if f.startswith(prefix + "."))


def lengths_and_genome(reads_paths, ref):
    L, G = {}, {}
    for p in reads_paths:
        lines = open(p, "rb").read().split(b"\n")
        for h, s in zip(lines[0::2], lines[1::2]):
            L[h[1:]] = len(s)                                 # the QNAME is the whole header line
    name = None
    for l in open(ref, "rb").read().split(b"\n"):
        if l.startswith(b">"):
            name = l[1:].split(b" ")[0]                        # the genome's ids are cut at the first blank
        elif l:
            G[name] = G.get(name, 0) + len(l)
    return L, G


def test_usage_lists_the_switch(cli, tmp_path):
    p = run(cli, ["filter", "-h", "x", "y"], tmp_path)
    assert p.returncode == 0 and b"MI355X front-end" in p.stderr
    tail = p.stderr.split(b"MI355X front-end")[1]
    assert b"--paf" in tail and b"PREFIX.paf" in tail


def test_refused_without_the_entry_points(cli_without_paf, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    for pos in (0, 1):                                        # the switch takes no value, in any position
        args = ["filter", reads[0], ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / "np"), "--block-reads", "7"]
        args.insert(1 if pos else len(args), "--paf")
        p = run(cli_without_paf, args, tmp_path)
        assert p.returncode == 1, p.stderr.decode()
        assert b"--paf" in p.stderr and b"no PAF form of the writer" in p.stderr
        assert outputs(tmp_path, "np") == []
    # the same library serves every run that does not ask for PAF
    p = run(cli_without_paf, ["filter", reads[0], ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / "ok"), "--block-reads", "7"], tmp_path)
    assert p.returncode == 0 and outputs(tmp_path, "ok") == ["ok.apf", "ok.sam"], p.stderr.decode()


def test_without_the_switch_no_paf_and_with_it_the_derivation_of_the_sam(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    L, G = lengths_and_genome(reads, ref)
    common = ["filter", reads[0], ref, "-t", "2", "-ot", "3", "--block-reads", "7", "-g", "50"]
    p = run(cli, common + ["-o", str(tmp_path / "a")], tmp_path)
    assert p.returncode == 0 and outputs(tmp_path, "a") == ["a.apf", "a.sam"], p.stderr.decode()
    p = run(cli, common + ["-o", str(tmp_path / "b"), "--paf"], tmp_path)
    assert p.returncode == 0 and outputs(tmp_path, "b") == ["b.apf", "b.paf", "b.sam"], p.stderr.decode()
    rd = lambda f: open(tmp_path / f, "rb").read()
    assert rd("b.sam") == rd("a.sam") and rd("b.apf") == rd("a.apf")
    paf = rd("b.paf")
    assert paf == pc.paf_of_sam(rd("a.sam"), L, G) and paf.count(b"\n") > 40 and not paf.startswith(b"@")
    pc.check_valid(paf, pc.sam_records(rd("a.sam")))
    # -ot 1 alone: the .paf stands next to whatever -ot asks for
    p = run(cli, ["filter", reads[0], ref, "-t", "2", "-ot", "1", "--block-reads", "7", "-g", "50", "-o", str(tmp_path / "c"), "--paf"], tmp_path)
    assert p.returncode == 0 and outputs(tmp_path, "c") == ["c.apf", "c.paf"] and rd("c.paf") == paf, p.stderr.decode()


def test_one_paf_per_read_file_as_the_sam(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_files=2, n_reads=40)
    L, G = lengths_and_genome(reads, ref)
    p = run(cli, ["filter"] + reads + ["x", ref, "-t", "2", "--block-reads", "7", "--paf"], tmp_path)
    assert p.returncode == 0, p.stderr.decode()
    for k in (0, 1):
        assert outputs(tmp_path, f"reads{k}") == [f"reads{k}.paf", f"reads{k}.part.fa", f"reads{k}.sam"]
        paf, sam = open(tmp_path / f"reads{k}.paf", "rb").read(), open(tmp_path / f"reads{k}.sam", "rb").read()
        assert paf == pc.paf_of_sam(sam, L, G) and paf.count(b"\n") > 20 and all(l.startswith(b"r%d_" % k) for l in paf.split(b"\n")[:-1])


def test_ot_16_stays_refused_with_the_switch(cli, tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=20)
    p = run(cli, ["filter", reads[0], ref, "-ot", "16", "-o", str(tmp_path / "z"), "--paf"], tmp_path)
    assert p.returncode == 1 and outputs(tmp_path, "z") == []
