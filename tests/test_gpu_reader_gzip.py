"""GPU: plain gzip inflated on the device, in parallel from DEFLATE block starts (the k_gz_* kernels of linear_amd/csrc/lnr_reader_kernels.hip
behind lnr_gunzip_gpu and, with lnr_reader_gpu_gzip, behind lnr_reader_next_dev).  lnr_gunzip_gpu equals zlib on every fixture of
tests/gzip_cases.py at four chunk sizes and in rounds of 8 KiB; on the level-6 FASTQ at 32 KiB chunks at least three quarters of the
chunks start a true piece (a serial fallback would not); the statistics are consistent.  Through the reader with the switch on: the blocks
of lnr_reader_next -- n per call, offsets, ordinals, ids -- at the limits of the BGZF test, at a window of 16 bytes, in rounds of 8 KiB, on
files of several members, with no text byte through gzread; the hand-overs (multi-line FASTQ, lnr_reader_next mixed in); the switch off;
a plain member inside a BGZF file; corrupt files; the device chain and the front-end.

The yardstick is zlib's inflate (gzip.decompress) and lnr_reader_next, never the code under test."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import bgzf_cases as bc, cases, gzip_cases as gc, reader_gpu_cases as rg
from tests.test_gpu_reader import d2h, same_blocks
from tests.test_gpu_writer import diff

pytestmark = pytest.mark.gpu
LIMITS = [(1 << 22, 100000), (5000, 7), (1000, 1)]
# (the names are listed here so that collecting the tests does not build the fixtures)
ALL = ["fq_l1.fq.gz", "fq_l6.fq.gz", "fq_l9.fq.gz", "fa_l1.fa.gz", "fa_l6.fa.gz", "fa_l9.fa.gz", "fq_m4.fq.gz", "fq_m1.fq.gz", "fq_fixed.fq.gz", "fq_huffman.fq.gz",
       "fq_rle.fq.gz", "fq_l0.fq.gz", "fq_sync.fq.gz", "fq_full.fq.gz", "a_run.fa.gz", "far.fa.gz", "len0.fa.gz", "len1.fa.gz", "len30000.fa.gz",
       "two_members.fq.gz", "three_members.fq.gz", "header_fields.fq.gz", "crlf.fa.gz", "multiline.fq.gz", "false_a.gz", "false_b.gz"]
READER = ["fq_l6.fq.gz", "fa_l9.fa.gz", "fq_m1.fq.gz", "fq_l0.fq.gz", "fq_sync.fq.gz", "far.fa.gz", "len0.fa.gz", "len1.fa.gz", "len30000.fa.gz", "two_members.fq.gz",
          "three_members.fq.gz", "header_fields.fq.gz", "crlf.fa.gz"]


@pytest.fixture(scope="module")
def lib():
    from linear_amd import build as lb
    lb.build()
    return lb


@pytest.fixture(scope="module")
def files(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_gzip")
    allf = gc.all_files()
    assert sorted(allf) == sorted(ALL)
    paths = {}
    allf.update(gc.small_files())
    for name in READER + ["multiline.fq.gz"] + sorted(gc.small_files()):
        paths[name] = str(d / name)
        with open(paths[name], "wb") as f:
            f.write(allf[name][0])
    bgzf = bc.write_files(str(d / "bgzf"))                 # (some of its names are names of gzip_cases too)
    for name in ("plain_member.fa.gz", "plain_control.fa.gz", "rnd200.fa.gz"):
        paths[name] = bgzf[name]
    return paths, {}


def host_blocks(files, name, cap, mr):
    paths, want = files
    if (name, cap, mr) not in want:
        want[(name, cap, mr)] = rg.serial_blocks(paths[name], cap, mr, serial=False)
    return want[(name, cap, mr)]


def consistent(st, text_len, name):
    assert st["true_pieces"] + st["false_candidates"] == st["candidates"] + st["rounds"], (name, st)
    assert st["text_bytes"] == text_len and st["rounds"] >= st["members"] >= 1 and st["deflate_blocks"] >= st["true_pieces"], (name, st)


@pytest.mark.parametrize("chunk", [1024, 4096, 32768, 0])
@pytest.mark.parametrize("name", ALL)
def test_gunzip_equals_zlib(lib, name, chunk, monkeypatch):
    from linear_amd.api import gunzip_gpu
    raw, text = gc.all_files()[name]
    if chunk:
        monkeypatch.setenv("LNR_READER_GZ_CHUNK", str(chunk))
    got, st = gunzip_gpu(raw, len(text))
    assert got == text, (name, chunk, len(got), len(text))
    consistent(st["total"], len(text), name)
    if name.startswith("false_") and chunk:
        assert st["total"]["false_candidates"] > 0, (name, st)
    if name.startswith(("fq_l", "fa_l", "fq_m")):
        assert st["total"]["false_candidates"] == 0, (name, st)
    if name == "fq_l6.fq.gz" and chunk == 32768:          # no serial fallback: the chunks start true pieces (shown on the host driver by the CPU test)
        t = st["total"]
        assert 4 * t["true_pieces"] >= 3 * t["chunks"] and t["chunks"] > 20, t
    if name == "fq_m1.fq.gz" and chunk == 1024:           # every window spans many pieces: what the chain pass exists for
        assert st["total"]["true_pieces"] * 32768 > 8 * len(text) and st["total"]["window_symbols"] > 0, st      # more than 8 pieces per 32 KiB of text


@pytest.mark.parametrize("chunk", [1024, 131072])
def test_gunzip_in_rounds_of_8k(lib, chunk, monkeypatch):
    from linear_amd.api import gunzip_gpu
    monkeypatch.setenv("LNR_READER_GZ_ROUND", "8192")
    monkeypatch.setenv("LNR_READER_GZ_CHUNK", str(chunk))
    grown = 0
    for name, (raw, text) in gc.small_files().items():
        got, st = gunzip_gpu(raw, len(text))
        assert got == text, (name, chunk)
        consistent(st["total"], len(text), name)
        assert st["total"]["rounds"] > len(raw) // 65536 + 1, (name, st)      # (a round is 8 KiB, or a few times that where it had to grow)
        grown += st["total"]["grown_rounds"]
    assert grown > 0                                      # level-6 blocks are longer than 8 KiB: such a round is run again with twice the bytes


def test_gunzip_errors(lib):
    from linear_amd.api import LnrError, gunzip_gpu
    raw, text = gc.fixtures()["fq_l6.fq.gz"]
    for bad, where in ((raw[:len(raw) // 2], None), (raw[:-8] + struct.pack("<I", zlib.crc32(text) ^ 4) + raw[-4:], len(raw) - 8), (b"\x1f\x8c" + raw[2:], 0)):
        with pytest.raises(LnrError) as e:
            gunzip_gpu(bad, len(text))
        assert e.value.status == -1 and "file offset" in str(e.value) and text.startswith(e.value.text), str(e.value)
        if where is not None:
            assert ("file offset %d:" % where) in str(e.value)
    with pytest.raises(LnrError) as e:
        gunzip_gpu(raw, len(text) - 1)
    assert e.value.status == -1 and "does not fit" in str(e.value)
    assert gunzip_gpu(raw + b"\0" * 100, len(text))[0] == text          # bytes that start no member are passed over, as gzread does


def test_files_that_end_behind_a_header(lib, tmp_path):
    """no DEFLATE byte behind a member's header (a round without a byte): an error with the file's end as offset, no launch on nothing"""
    from linear_amd.api import LnrError, gunzip_gpu
    for name, (raw, text, where) in gc.cut_behind_header_files().items():
        with pytest.raises(LnrError) as e:
            gunzip_gpu(raw, len(text) + 200)
        assert e.value.status == -1 and ("file offset %d:" % where) in str(e.value) and e.value.text == text, (name, str(e.value))
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(raw)
        with pytest.raises(LnrError) as e:
            gz_run(p, 1 << 22, 100000)
        assert e.value.status == -1 and ("gzip data at file offset %d:" % where) in str(e.value), (name, str(e.value))
    raw, text = gc.fixtures()["len30000.fa.gz"]
    assert gunzip_gpu(raw, len(text))[0] == text          # and the device goes on working


def gz_run(path, dst_cap, max_reads, switch=True):
    """([(off, bases, ids)] per block of next_dev, gzip stats, inflate stats, True when the run ended in LNR_ERR_LIMIT)"""
    from linear_amd.api import LnrError, Reader
    r = Reader(path)
    r.gpu_open(0, 2)
    if switch:
        r.gpu_gzip()
    out, limit = [], False
    while True:
        try:
            n, dr, dof, off, ids = r.next_dev(dst_cap, max_reads)
        except LnrError as e:
            if e.status != -6:
                r.close()
                raise
            limit = True
            break
        if n == 0:
            break
        assert np.array_equal(d2h(dof, 8 * (n + 1), np.uint64), off)
        out.append((off, d2h(dr, int(off[n])), ids))
    st, ist = r.gpu_gzip_stats()["total"], r.gpu_inflate_stats()["total"]
    r.close()
    return out, st, ist, limit


@pytest.mark.parametrize("cap,mr", LIMITS)
def test_reader_blocks_and_stats(files, cap, mr):
    paths, _ = files
    for name in READER:
        text = gc.all_files()[name][1]
        got, st, ist, limit = gz_run(paths[name], cap, mr)
        same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
        assert st["gzread_bytes"] == 0 and ist["gzread_bytes"] == 0 and ist["blocks"] == 0, (name, st, ist)
        if not limit:
            consistent(st, len(text), name)
            assert st["members"] == (3 if name.startswith("three") else 2 if name.startswith("two") else 1), (name, st)


def test_reader_small_window(files, monkeypatch):
    paths, _ = files
    monkeypatch.setenv("LNR_READER_GPU_WINDOW", "16")
    for name in ("fq_l6.fq.gz", "crlf.fa.gz", "three_members.fq.gz", "len30000.fa.gz"):
        for cap, mr in ((1 << 22, 100000), (5000, 7)):
            got, st, _, limit = gz_run(paths[name], cap, mr)
            same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
            assert st["gzread_bytes"] == 0


def test_reader_rounds_of_8k(files, monkeypatch):
    paths, _ = files
    monkeypatch.setenv("LNR_READER_GZ_ROUND", "8192")
    monkeypatch.setenv("LNR_READER_GZ_CHUNK", "1024")
    for name in ("small_l6.fq.gz", "small_m1.fq.gz", "crlf.fa.gz", "small_three.fq.gz", "small_far.fa.gz"):
        for cap, mr in ((1 << 22, 100000), (20000, 7)):
            got, st, _, limit = gz_run(paths[name], cap, mr)
            same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
            assert st["gzread_bytes"] == 0 and (limit or st["rounds"] > os.path.getsize(paths[name]) // 65536 + 1), (name, st)


@pytest.mark.parametrize("cap,mr", LIMITS)
def test_hand_overs(files, cap, mr):
    paths, _ = files
    name = "multiline.fq.gz"                              # the device reads up to the hand-over, the serial parser the rest through a fresh gzread stream
    got, st, _, limit = gz_run(paths[name], cap, mr)
    same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
    assert limit or (st["rounds"] > 0 and 0 < st["gzread_bytes"] < len(gc.all_files()[name][1])), st
    name = "plain_member.fa.gz"                           # two BGZF blocks through the BGZF path, the rest through the gzip rounds
    got, st, ist, limit = gz_run(paths[name], cap, mr)
    same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
    assert ist["blocks"] == 2 and st["gzread_bytes"] == 0 and ist["gzread_bytes"] == 0 and (limit or st["members"] >= 2), (st, ist)
    name = "rnd200.fa.gz"                                 # BGZF keeps precedence
    got, st, ist, limit = gz_run(paths[name], cap, mr)
    same_blocks(got, host_blocks(files, name, cap, mr), (name, cap, mr))
    assert ist["blocks"] > 0 and st["rounds"] == 0 and st["gzread_bytes"] == 0


def test_switch_off(files, monkeypatch):
    paths, _ = files
    for name in ("fq_l6.fq.gz", "plain_control.fa.gz"):
        got, st, ist, _ = gz_run(paths[name], 1 << 22, 100000, switch=False)
        same_blocks(got, host_blocks(files, name, 1 << 22, 100000), name)
        assert st["rounds"] == 0 and ist["blocks"] == 0 and ist["gzread_bytes"] == len(rg.plain_text(paths[name]))
    monkeypatch.setenv("LNR_READER_BGZF", "0")
    for name in ("fq_l6.fq.gz", "rnd200.fa.gz"):
        got, st, ist, _ = gz_run(paths[name], 1 << 22, 100000)
        same_blocks(got, host_blocks(files, name, 1 << 22, 100000), name)
        assert st["rounds"] == 0 and ist["blocks"] == 0 and ist["gzread_bytes"] == len(rg.plain_text(paths[name]))


def test_switch_order(files):
    from linear_amd.api import LnrError, Reader
    paths, _ = files
    r = Reader(paths["fq_l6.fq.gz"])
    with pytest.raises(LnrError) as e:
        r.gpu_gzip()                                      # before gpu_open
    assert e.value.status == -1
    r.gpu_open(0, 2)
    r.next_dev(1 << 20, 10)
    with pytest.raises(LnrError) as e:
        r.gpu_gzip()                                      # after the first read
    assert e.value.status == -1
    r.close()


def test_mixing_next_and_next_dev(files):
    from linear_amd.api import Reader
    paths, _ = files
    for name in ("crlf.fa.gz", "multiline.fq.gz"):
        want = host_blocks(files, name, 5000, 7)
        r = Reader(paths[name])
        r.gpu_open(0, 2)
        r.gpu_gzip()
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
        st = r.gpu_gzip_stats()["total"]
        r.close()
        same_blocks(got, want, name)
        assert st["rounds"] > 0 and st["gzread_bytes"] > 0, st      # the first call inflated on the device; lnr_reader_next then took the stream over


def test_corrupt_files(files, tmp_path):
    from linear_amd.api import LnrError
    paths, _ = files
    raw, text = gc.fixtures()["fq_l6.fq.gz"]
    clean = gc.flips_clean_on_host(step=20)               # only flips the host driver has just taken without a fault, with zlib's verdict
    assert len(clean) == 10
    bad = [(name, b, ztext, None) for name, b, ztext in clean]
    bad.append(("cut", raw[:len(raw) // 2], None, None))
    bad.append(("trailer_crc", raw[:-8] + struct.pack("<I", zlib.crc32(text) ^ 4) + raw[-4:], None, len(raw) - 8))
    errors = 0
    for name, b, ztext, where in bad:
        p = str(tmp_path / (name + ".fq.gz"))
        with open(p, "wb") as f:
            f.write(b)
        if ztext is None:
            with pytest.raises(LnrError) as e:
                gz_run(p, 1 << 24, 100000)
            msg = str(e.value)
            assert e.value.status == -1 and "gzip data at file offset " in msg, (name, msg)
            at = int(msg.split("file offset ")[1].split(":")[0])
            assert 0 < at <= len(b) and (where is None or at == where), (name, msg)
            errors += 1
        else:
            got, st, _, _ = gz_run(p, 1 << 24, 100000)
            same_blocks(got, rg.serial_blocks(p, 1 << 24, 100000, serial=False), name)
    assert errors >= 6
    got, st, _, _ = gz_run(paths["fq_l6.fq.gz"], 1 << 22, 100000)         # a reader opened afterwards works
    same_blocks(got, host_blocks(files, "fq_l6.fq.gz", 1 << 22, 100000), "afterwards")


def test_chain_and_front_end(lib, case_inputs, tmp_path):
    from linear_amd import Filter
    from linear_amd.api import Reader, Writer
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    rid, gid = cases.text_ids(n, len(refs))
    rp, gp, _, _ = cases.write_fasta_case(tmp_path, refs, reads, off)
    zp = str(tmp_path / "reads.fa.gz")
    with open(zp, "wb") as f:
        f.write(gc.gz(open(rp, "rb").read()))
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
    r.gpu_gzip()
    k, dr, dof, hoff, ids = r.next_dev(1 << 24, 100000)
    st = r.gpu_gzip_stats()["last"]
    assert k == n and ids == host[0][2] and st["rounds"] > 0 and st["gzread_bytes"] == 0
    dev = flt.filter_batch_dev(dr, dof, k)
    sam = w.format_seq_dev(dev, dr, dof, ids)
    assert sam == ref_sam and len(sam) > 300_000, diff(ref_sam, sam)
    w.close(); r.close(); flt.close()
    outs = {}
    for tag, reads_path, more in (("plain", rp, []), ("gzip", zp, ["--gpu-gunzip"])):
        p = subprocess.run(["timeout", "-k", "10", "240", lib.CLI, "filter", reads_path, gp, "--gpu-reader", "--gpu-writer", "--sam-seq", "-t", "1", "-g", "0", "-ot", "3",
                            "-o", str(tmp_path / tag), "--block-reads", "23"] + more, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        outs[tag] = {e: open(tmp_path / (tag + e), "rb").read() for e in (".sam", ".apf")}
    for e in (".sam", ".apf"):
        assert outs["plain"][e] == outs["gzip"][e] and len(outs["plain"][e]) > 1000, (e, diff(outs["plain"][e], outs["gzip"][e]))
