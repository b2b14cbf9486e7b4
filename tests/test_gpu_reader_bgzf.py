"""GPU: BGZF input of the reader's GPU twin (k_bgzf_inflate / k_rd_gather in linear_amd/csrc/lnr_reader_kernels.hip behind
lnr_reader_next_dev): on every fixture of tests/bgzf_cases.py the blocks of lnr_reader_next -- the same n per call, offsets, ordinals, ids --
and lnr_reader_gpu_inflate_stats says that the device did the inflate; windows of one block and of less than a record; the switch; the
hand-overs to the gzread stream; lnr_reader_next mixed in; corrupt blocks; the device-resident chain and the front-end on a BGZF file.

The stats conditions: on a file that is BGZF from its first to its last member and is read to its end, blocks inflated == the file's
non-empty blocks and no text byte came through gzread.  A run that ends in LNR_ERR_LIMIT (a record longer than dst_cap, as
lnr_reader_next ends there too) has not read the file to its end: there gzread bytes == 0 and no block was inflated twice.  The three
files of bgzf_cases.HANDOVER (multi-line FASTQ, a plain gzip member in the middle, a plain .gz) have their own conditions below."""
import os
import subprocess

import numpy as np
import pytest

from tests import bgzf_cases as bc, cases, reader_gpu_cases as rg
from tests.test_gpu_reader import d2h, same_blocks
from tests.test_gpu_writer import diff
from tests.test_inflate_hd_cpu import clean_corrupt_cases

pytestmark = pytest.mark.gpu
LIMITS = [(1 << 22, 100000), (5000, 7), (1000, 1)]


def dev_run(path, dst_cap, max_reads):
    """([(off, bases, ids)] per block of next_dev, total stats, True when the run ended in LNR_ERR_LIMIT)"""
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
    st = r.gpu_inflate_stats()["total"]
    r.close()
    return out, st, limit


@pytest.fixture(scope="module")
def lib():
    from linear_amd import build as lb
    lb.build()
    return lb


@pytest.fixture(scope="module")
def files(lib, tmp_path_factory):
    paths = bc.write_files(str(tmp_path_factory.mktemp("gpu_bgzf")))
    nonempty = {name: sum(1 for b in bc.walk(open(p, "rb").read()) if b[2]) for name, p in paths.items()}
    want = {}                                             # the yardstick, once per (file, limits)
    return paths, nonempty, want


def host_blocks(files, name, cap, mr):
    paths, _, want = files
    if (name, cap, mr) not in want:
        want[(name, cap, mr)] = rg.serial_blocks(paths[name], cap, mr, serial=False)
    return want[(name, cap, mr)]


@pytest.mark.parametrize("cap,mr", LIMITS)
def test_blocks_and_stats(files, cap, mr):
    paths, nonempty, _ = files
    for name, p in paths.items():
        if name in bc.HANDOVER:
            continue
        want = host_blocks(files, name, cap, mr)
        got, st, limit = dev_run(p, cap, mr)
        same_blocks(got, want, (name, cap, mr))
        assert st["gzread_bytes"] == 0, (name, st)
        if limit:
            assert 0 < st["blocks"] <= nonempty[name], (name, st)
        else:
            assert st["blocks"] == nonempty[name] and st["text_bytes"] == len(rg.plain_text(p)) and 0 < st["compressed_bytes"] <= os.path.getsize(p), (name, st)
            assert st["inflate_ms"] > 0 and st["gather_ms"] > 0


@pytest.mark.parametrize("window", [65536, 16])
def test_small_windows(files, window, monkeypatch):
    """a window of one block; a window smaller than a record (it is doubled): records, header lines and quality lines straddle blocks and windows"""
    paths, nonempty, _ = files
    monkeypatch.setenv("LNR_READER_GPU_WINDOW", str(window))
    for name in ("rnd200.fa.gz", "pay4096.fq.gz", "crlf.fasta.gz", "pay7.fa.gz", "a_run.fa.gz", "empty_mid_eof.fa.gz", "rnd.fastq_multiline.gz"):
        for cap, mr in ((1 << 22, 100000), (5000, 7)):
            got, st, limit = dev_run(paths[name], cap, mr)
            same_blocks(got, host_blocks(files, name, cap, mr), (name, window, cap, mr))
            if name not in bc.HANDOVER:
                assert st["gzread_bytes"] == 0 and (limit or st["blocks"] == nonempty[name]), (name, st)


def test_switch_off(files, monkeypatch):
    paths, _, _ = files
    monkeypatch.setenv("LNR_READER_BGZF", "0")
    for name in ("rnd200.fa.gz", "pay4096.fq.gz"):
        got, st, _ = dev_run(paths[name], 1 << 22, 100000)
        same_blocks(got, host_blocks(files, name, 1 << 22, 100000), name)
        assert st["blocks"] == 0 and st["gzread_bytes"] == len(rg.plain_text(paths[name]))


@pytest.mark.parametrize("cap,mr", LIMITS)
def test_hand_overs(files, cap, mr):
    paths, nonempty, _ = files
    # multi-line FASTQ: the device inflates up to the hand-over, the serial parser reads the rest through gzread
    name = "rnd.fastq_multiline.gz"
    got, st, limit = dev_run(paths[name], cap, mr)
    same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
    assert limit or (0 < st["blocks"] <= nonempty[name] and 0 < st["gzread_bytes"] < len(rg.plain_text(paths[name])))
    # a plain gzip member after two BGZF blocks: those two on the device, the rest through gzread
    name = "plain_member.fa.gz"
    got, st, limit = dev_run(paths[name], cap, mr)
    same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
    assert st["blocks"] == 2 and (limit or st["gzread_bytes"] >= len(rg.plain_text(paths[name])) - 10000)
    name = "plain_control.fa.gz"
    got, st, limit = dev_run(paths[name], cap, mr)
    same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
    assert st["blocks"] == 0 and st["gzread_bytes"] > 0


def test_mixing_next_and_next_dev(files):
    from linear_amd.api import Reader
    paths, _, _ = files
    for name in ("rnd200.fa.gz", "pay4096.fq.gz"):
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
        assert st["blocks"] > 0                          # the first call inflated on the device; lnr_reader_next then took the stream over


def test_corrupt_blocks(lib, files, tmp_path):
    from linear_amd.api import LnrError, Reader
    bad = bc.corrupt_files(str(tmp_path))
    assert sorted(bad) == clean_corrupt_cases()           # only cases the CPU test has shown to be clean on the host
    paths, nonempty, _ = files
    for name, (p, off) in bad.items():
        r = Reader(p)
        r.gpu_open(0, 2)
        with pytest.raises(LnrError) as e:
            r.next_dev(1 << 22, 100000)                   # one window holds the whole file: the failing call delivers no block
        assert e.value.status == -1 and ("offset %d:" % off) in str(e.value), (name, str(e.value))
        r.close()
        got, st, _ = dev_run(paths["rnd200.fa.gz"], 1 << 22, 100000)      # a reader opened afterwards works
        same_blocks(got, host_blocks(files, "rnd200.fa.gz", 1 << 22, 100000), name)
        assert st["blocks"] == nonempty["rnd200.fa.gz"]


def test_chain_and_front_end(lib, case_inputs, tmp_path):
    from linear_amd import Filter
    from linear_amd.api import Reader, Writer
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    rid, gid = cases.text_ids(n, len(refs))
    rp, gp, _, _ = cases.write_fasta_case(tmp_path, refs, reads, off)
    zp = str(tmp_path / "reads.fa.gz")
    with open(zp, "wb") as f:
        f.write(bc.bgzf(open(rp, "rb").read()))
    flt = Filter(device=0)
    flt.build_index(refs, 3)
    host = rg.serial_blocks(rp, 1 << 24, 100000, serial=False)
    want = flt.filter_batch(host[0][1], host[0][0])
    w = Writer(gid, [x.size for x in refs])
    w.gpu_open(0)
    w.set_genome(refs)
    ref_sam = w.format_seq(*want, reads, off, host[0][2])
    r = Reader(zp)
    r.gpu_open(0, 2)
    k, dr, dof, hoff, ids = r.next_dev(1 << 24, 100000)
    st = r.gpu_inflate_stats()["last"]
    assert k == n and ids == host[0][2] and st["blocks"] > 0 and st["gzread_bytes"] == 0
    dev = flt.filter_batch_dev(dr, dof, k)
    sam = w.format_seq_dev(dev, dr, dof, ids)
    assert sam == ref_sam and len(sam) > 300_000, diff(ref_sam, sam)
    w.close(); r.close(); flt.close()
    outs = {}
    for tag, reads_path in (("plain", rp), ("bgzf", zp)):
        p = subprocess.run(["timeout", "-k", "10", "240", lib.CLI, "filter", reads_path, gp, "--gpu-reader", "--gpu-writer", "--sam-seq", "-t", "1", "-g", "0", "-ot", "3",
                            "-o", str(tmp_path / tag), "--block-reads", "23"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        outs[tag] = {e: open(tmp_path / (tag + e), "rb").read() for e in (".sam", ".apf")}
    for e in (".sam", ".apf"):
        assert outs["plain"][e] == outs["bgzf"][e] and len(outs["plain"][e]) > 1000, (e, diff(outs["plain"][e], outs["bgzf"][e]))
