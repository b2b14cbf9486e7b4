"""CPU: a BAM read file through the front-end, against the test double of the device half (tests/stub_abi.cpp + the real reader and writer):
the default host reader finds the BAM by its content (under a name that says nothing), the .sam / .apf equal those of the same reads as
FASTA, output naming is unchanged, an invalid record ends the run with its ordinal and offset, a BAM genome is refused, and the usage
text says so."""
import os
import subprocess

import pytest

from tests import bgzf_cases as bc, ubam_cases as ub
from tests.test_cli_frontend_cpu import write_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CSRC = os.path.join(ROOT, "linear_amd", "csrc")
CODE = {"A": 1, "C": 2, "G": 4, "T": 8}


@pytest.fixture(scope="module")
def cli():
    os.makedirs(BUILD, exist_ok=True)
    so, exe = os.path.join(BUILD, "libstub_bamin_linear_amd.so"), os.path.join(BUILD, "linear_filter_stub_bamin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "stub_abi.cpp"), os.path.join(CSRC, "lnr_reader.cpp"),
                           os.path.join(CSRC, "lnr_output.cpp"), "-o", so, "-lz", "-lpthread"])
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", exe, so, "-Wl,-rpath," + BUILD, "-lpthread"])
    return exe


def run(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def fasta_records(path):
    out = []
    for chunk in open(path, "rb").read().decode().split(">")[1:]:
        head, _, body = chunk.partition("\n")
        out.append((head.split()[0], "".join(body.split()).upper()))
    return out


@pytest.fixture()
def inputs(tmp_path):
    reads, ref = write_inputs(tmp_path, n_reads=60)
    recs = fasta_records(reads[0])
    fa, bam = str(tmp_path / "same.fa"), str(tmp_path / "same.reads")          # (the BAM's name says nothing: it is found by content)
    with open(fa, "w") as f:
        f.write("".join(">%s\n%s\n" % r for r in recs))
    stream = ub.header() + b"".join(ub.record(name.encode(), [CODE.get(c, 15) for c in seq], aux=b"rqf\0\0\x80\x3f") for name, seq in recs)
    with open(bam, "wb") as f:
        f.write(bc.bgzf(stream, payload=3000))
    return fa, bam, ref, stream, recs


def test_bam_reads_give_the_fasta_outputs(cli, inputs, tmp_path):
    fa, bam, ref, _, _ = inputs
    for tag, reads in (("fa", fa), ("bam", bam)):
        p = run(cli, ["filter", reads, ref, "-t", "2", "-ot", "3", "-o", str(tmp_path / tag), "--block-reads", "7"], tmp_path)
        assert p.returncode == 0, p.stderr.decode()
    for ext in (".sam", ".apf"):
        a, b = open(tmp_path / ("fa" + ext), "rb").read(), open(tmp_path / ("bam" + ext), "rb").read()
        assert a == b and len(a) > 500, ext
    p = run(cli, ["filter", bam, ref, "-t", "2", "--block-reads", "7"], tmp_path)      # without -o: named by the read file's name up to its first '.'
    assert p.returncode == 0 and os.path.exists(tmp_path / "same.sam"), p.stderr.decode()


def test_invalid_record_ends_the_run(cli, inputs, tmp_path):
    _, _, ref, stream, recs = inputs
    hdr, _, parsed = ub.parse(stream)
    at = parsed[10][0]
    bad = str(tmp_path / "bad.bam")
    with open(bad, "wb") as f:
        f.write(bc.bgzf(stream[:at] + ub.record(b"bad", [1] * 10, block_size=8) + stream[at:]))
    p = run(cli, ["filter", bad, ref, "-t", "2", "-o", str(tmp_path / "o"), "--block-reads", "7"], tmp_path)
    assert p.returncode != 0 and ("BAM record 10 at offset %d " % at).encode() in p.stderr, p.stderr.decode()


def test_bam_genome_is_refused_and_usage(cli, inputs, tmp_path):
    fa, bam, _, _, _ = inputs
    p = run(cli, ["filter", fa, bam, "-t", "2", "-o", str(tmp_path / "g")], tmp_path)
    assert p.returncode == 1 and b"BAM" in p.stderr and b"genome" in p.stderr, p.stderr.decode()
    p = run(cli, ["filter", "-h", "x", "y"], tmp_path)
    assert b"BAM" in p.stderr and b"samtools fastq" in p.stderr
