"""GPU: BAM input of the reader's GPU twin (k_bam_find / k_bam_stitch / k_bam_meta / k_bam_emit / k_rd_gather in
linear_amd/csrc/lnr_reader_kernels.hip behind lnr_reader_next_dev): on every fixture of tests/ubam_cases.py the blocks of lnr_reader_next --
the same n per call, offsets, ordinals, ids -- through the device inflate and through gzread (LNR_READER_BGZF=0); the counts of
lnr_reader_gpu_bam_stats against the Python decoder; windows of one BGZF block and of less than a record; the decoy and the long record
make the stitch walk tiles again; invalid records are refused with the host reader's ordinal and offset; lnr_reader_next mixed in; the
device-resident chain and the front-end on a BAM file."""
import os
import subprocess

import numpy as np
import pytest

from tests import reader_gpu_cases as rg, ubam_cases as ub
from tests.test_gpu_reader import d2h, same_blocks
from tests.test_gpu_writer import diff

pytestmark = pytest.mark.gpu
LIMITS = [(1 << 22, 100000), (5000, 7), (1000, 1)]


def dev_run(path, dst_cap, max_reads):
    """([(off, bases, ids)] per block of next_dev, total BAM stats, total inflate stats, True when the run ended in LNR_ERR_LIMIT)"""
    from linear_amd.api import LnrError, Reader
    r = Reader(path)
    r.gpu_open(0, 2)
    out, limit = [], False
    while True:
        try:
            n, dr, dof, off, ids = r.next_dev(dst_cap, max_reads)
        except LnrError as e:
            if e.status != -6:
                raise
            limit = True
            break
        if n == 0:
            break
        assert np.array_equal(d2h(dof, 8 * (n + 1), np.uint64), off)
        out.append((off, d2h(dr, int(off[n])), ids))
    bst, ist = r.gpu_bam_stats()["total"], r.gpu_inflate_stats()["total"]
    r.close()
    return out, bst, ist, limit


@pytest.fixture(scope="module")
def lib():
    from linear_amd import build as lb
    lb.build()
    return lb


@pytest.fixture(scope="module")
def files(lib, tmp_path_factory):
    from linear_amd.api import Reader
    tile = Reader.gpu_bam_tile()
    assert tile > 0
    paths = ub.write(str(tmp_path_factory.mktemp("gpu_bam")), tile)
    counts = {name: ub.reads_of(ub.stream_of(p))[2] for name, p in paths.items()}      # the decoder reads the written files
    return paths, counts, {}


def host_blocks(files, name, cap, mr):
    paths, _, want = files
    if (name, cap, mr) not in want:
        want[(name, cap, mr)] = rg.serial_blocks(paths[name], cap, mr, serial=False)
    return want[(name, cap, mr)]


@pytest.mark.parametrize("cap,mr", LIMITS)
def test_blocks_and_stats_device_inflate(files, cap, mr):
    paths, counts, _ = files
    for name, p in paths.items():
        got, bst, ist, limit = dev_run(p, cap, mr)
        same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
        assert ist["gzread_bytes"] == 0, (name, ist)
        if not limit:
            assert {k: bst[k] for k in ("records", "skipped", "reverse")} == counts[name], (name, bst)
            if counts[name]["records"]:
                assert ist["blocks"] > 0 and bst["tiles"] > 0 and bst["find_ms"] > 0 and bst["stitch_ms"] > 0


@pytest.mark.parametrize("cap,mr", LIMITS)
def test_blocks_through_gzread(files, cap, mr, monkeypatch):
    paths, counts, _ = files
    monkeypatch.setenv("LNR_READER_BGZF", "0")
    for name, p in paths.items():
        got, bst, ist, limit = dev_run(p, cap, mr)
        same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
        assert ist["blocks"] == 0 and ist["gzread_bytes"] > 0
        if not limit:
            assert {k: bst[k] for k in ("records", "skipped", "reverse")} == counts[name], (name, bst)


@pytest.mark.parametrize("window", [65536, 16])
def test_small_windows(files, window, monkeypatch):
    """a window of one BGZF block; a window smaller than a record (it is doubled): records and the long header straddle blocks and windows"""
    paths, counts, _ = files
    monkeypatch.setenv("LNR_READER_GPU_WINDOW", str(window))
    for name, p in paths.items():
        for cap, mr in ((1 << 22, 100000), (5000, 7)):
            got, bst, ist, limit = dev_run(p, cap, mr)
            same_blocks(got, host_blocks(files, name, cap, mr), (name, window, cap, mr))
            assert ist["gzread_bytes"] == 0
            if not limit:
                assert {k: bst[k] for k in ("records", "skipped", "reverse")} == counts[name], (name, bst)


def test_repair(files):
    """the decoy's false first guess (tests/test_reader_bam_cpu.py shows it on the CPU) and the tiles inside the 300 kb record"""
    paths, _, _ = files
    for name in ("9_decoy", "7_long"):
        got, bst, _, _ = dev_run(paths[name], 1 << 22, 100000)
        same_blocks(got, host_blocks(files, name, 1 << 22, 100000), name)
        assert bst["repaired_tiles"] >= 1, (name, bst)


def test_bad_files(lib, files, tmp_path, monkeypatch):
    from linear_amd.api import LnrError, Reader
    paths, _, _ = files
    for name, (p, ordinal, off, why) in ub.write_bad(str(tmp_path)).items():
        r = Reader(p)
        with pytest.raises(LnrError) as eh:
            r.next(np.zeros(1 << 20, np.uint8), 100000)
        r.close()
        r = Reader(p)
        r.gpu_open(0, 2)
        with pytest.raises(LnrError) as e:
            r.next_dev(1 << 22, 100000)                       # one window holds the whole file: the failing call delivers no block
        assert e.value.status == -1 and str(e.value) == str(eh.value) and ("BAM record %d at offset %d " % (ordinal, off)) in str(e.value), (name, str(e.value), str(eh.value))
        r.close()
    got, _, _, _ = dev_run(paths["2_names"], 1 << 22, 100000)  # a reader opened afterwards works
    same_blocks(got, host_blocks(files, "2_names", 1 << 22, 100000), "after the bad files")


def test_mixing_next_and_next_dev(files):
    from linear_amd.api import Reader
    paths, _, _ = files
    name = "1_rnd200"
    want = host_blocks(files, name, 5000, 7)
    r = Reader(paths[name])
    r.gpu_open(0, 2)
    dst = np.zeros(5000, np.uint8)
    got = []
    for k in range(len(want) + 1):
        if k % 3 == 1:
            n, off, ids = r.next(dst, 7)
            blk = (off, dst[: int(off[n])].copy(), ids)
        else:
            n, dr, dof, off, ids = r.next_dev(5000, 7)
            blk = (off, d2h(dr, int(off[n])), ids)
        if n == 0:
            break
        got.append(blk)
    st = r.gpu_inflate_stats()["total"]
    r.close()
    same_blocks(got, want, name)
    assert st["blocks"] > 0                                  # the first call inflated on the device; lnr_reader_next then took the stream over


def test_chain_and_front_end(lib, case_inputs, tmp_path):
    from linear_amd import Filter
    from linear_amd.api import Reader, Writer
    from tests import bgzf_cases as bc, cases
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    _, gid = cases.text_ids(n, len(refs))
    _, gp, _, _ = cases.write_fasta_case(tmp_path, refs, reads, off)
    rid = ["read_%d" % i for i in range(n)]                  # no blanks: a BAM name and a FASTA header line agree
    abc = np.frombuffer(b"ACGTN", np.uint8)
    code = np.array([1, 2, 4, 8, 15], np.uint8)
    rp, bp = str(tmp_path / "reads_noblank.fa"), str(tmp_path / "reads.bam")
    with open(rp, "wb") as f:
        for i in range(n):
            f.write(b">" + rid[i].encode() + b"\n" + abc[reads[int(off[i]):int(off[i + 1])]].tobytes() + b"\n")
    with open(bp, "wb") as f:
        f.write(bc.bgzf(ub.header() + b"".join(ub.record(rid[i].encode(), code[reads[int(off[i]):int(off[i + 1])]].tolist()) for i in range(n))))
    flt = Filter(device=0)
    flt.build_index(refs, 3)
    host = rg.serial_blocks(rp, 1 << 24, 100000, serial=False)
    want = flt.filter_batch(host[0][1], host[0][0])
    w = Writer(gid, [x.size for x in refs])
    w.gpu_open(0)
    w.set_genome(refs)
    ref_sam = w.format_seq(*want, reads, off, host[0][2])
    r = Reader(bp)
    r.gpu_open(0, 2)
    k, dr, dof, hoff, ids = r.next_dev(1 << 24, 100000)
    st, bst = r.gpu_inflate_stats()["last"], r.gpu_bam_stats()["last"]
    assert k == n and ids == host[0][2] and st["blocks"] > 0 and st["gzread_bytes"] == 0 and bst["records"] == n
    dev = flt.filter_batch_dev(dr, dof, k)
    sam = w.format_seq_dev(dev, dr, dof, ids)
    assert sam == ref_sam and len(sam) > 300_000, diff(ref_sam, sam)
    w.close(); r.close(); flt.close()
    outs = {}
    for tag, reads_path, extra in (("fa", rp, []), ("bam", bp, []), ("bam_gpu", bp, ["--gpu-reader"])):
        p = subprocess.run(["timeout", "-k", "10", "240", lib.CLI, "filter", reads_path, gp, "-t", "1", "-g", "0", "-o", str(tmp_path / tag), "--block-reads", "23"] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        outs[tag] = open(str(tmp_path / tag) + ".sam", "rb").read()
    assert len(outs["fa"]) > 1000
    for tag in ("bam", "bam_gpu"):
        assert outs[tag] == outs["fa"], (tag, diff(outs["fa"], outs[tag]))
    p = subprocess.run(["timeout", "-k", "10", "240", lib.CLI, "filter", rp, bp, "-t", "1", "-g", "0", "-o", str(tmp_path / "bad")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"BAM" in p.stderr           # a genome file that is a BAM is refused
