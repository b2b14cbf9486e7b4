"""GPU: BGZF output of the writer's GPU side (lnr_writer_set_bgzf / lnr_writer_bgzf_bytes_gpu, k_bgzf_deflate / k_bgzf_pack in
linear_amd/csrc/lnr_output_kernels.hip).  The kernel's bytes EQUAL those of lnr_deflate_hd.h on the host (tests/test_deflate_hd_cpu.py pins
those to zlib, the project's own inflate and the sanitizers) on every text of tests/deflate_cases.py; every format call with the switch
on inflates to the text it gives with the switch off; buffer reuse; the stats; a round trip through the reader's device inflate; the
front-end's --bgzf."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import bgzf_cases as bc, cases, deflate_cases as dc, reader_gpu_cases as rg, writer_cases as wc, writer_seq_cases as sc
from tests.test_gpu_reader import d2h, same_blocks
from tests.test_gpu_writer import diff

pytestmark = pytest.mark.gpu
BLOCK = dc.BLOCK
TIMES = {"upload_ms", "measure_ms", "scan_ms", "emit_ms", "download_ms"}


@pytest.fixture(scope="module")
def writers():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    made = []

    def make(seq=False):
        w = Writer(sc.GIDS, sc.GLEN) if seq else Writer(wc.GIDS, wc.GLEN)
        if seq:
            w.set_genome(sc.genome())
        w.gpu_open(0)
        made.append(w)
        return w
    yield make
    for w in made:
        w.close()


@pytest.fixture(scope="module")
def host():
    return dc.host_bgzf()


def plain_of(raw, eof):
    return gzip.decompress(raw + eof) if raw else b""


def test_hd_texts_on_the_device_equal_the_host_build(writers, host):
    w = writers()
    sam = w.format(*wc.synthetic(), "sam")
    texts = dc.texts(sam)
    texts["apf"] = w.format(*wc.synthetic(), "apf")
    for name, text in texts.items():
        got = w.bgzf_bytes_gpu(text)
        want, stored = host(text)
        assert got == want, (name, len(got), len(want), [i for i, (a, b) in enumerate(zip(bc.walk(got), bc.walk(want))) if a != b][:3])
        st = w.bgzf_stats()
        assert st["blocks"] == (len(text) + BLOCK - 1) // BLOCK and st["stored_blocks"] == stored, (name, st)
        assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(got), (name, st)
    assert w.bgzf_bytes_gpu(b"") == b""
    assert w.bgzf_eof() == bc.EOF_BLOCK


@pytest.mark.parametrize("name,dup", wc.GAP_SETS)
def test_format_calls_on_gap_cords(writers, name, dup):
    w = writers()
    batch = wc.gap_set(name, dup)
    for k in ("sam", "apf"):
        w.set_bgzf(False)
        want = w.format_gpu(*batch, k)
        w.set_bgzf(True)
        got = w.format_gpu(*batch, k)
        assert plain_of(got, w.bgzf_eof()) == want, (k, len(got))


def test_format_calls_on_synthetic_cords_and_stats(writers):
    w = writers()
    eof = w.bgzf_eof()
    for batch in (wc.synthetic(), wc.one_read(), wc.empty()):
        for k in ("sam", "apf"):
            w.set_bgzf(False)
            want = w.format_gpu(*batch, k)
            w.set_bgzf(True)
            got = w.format_gpu(*batch, k)
            assert plain_of(got, eof) == want, (k, len(got))
            st, t = w.bgzf_stats(), w.gpu_times()
            assert set(t) == TIMES
            assert st["blocks"] == (len(want) + BLOCK - 1) // BLOCK and st["text_bytes"] == len(want) and st["compressed_bytes"] == len(got), st
            assert st["stored_blocks"] == 0, st                    # SAM / APF text never needs the stored form
            if want:
                assert len(bc.walk(got)) == st["blocks"] and st["deflate_ms"] > 0 and st["pack_ms"] > 0, st
    assert w.format_gpu(*wc.empty(), "sam") == b"" and w.format_gpu(*wc.empty(), "apf") == b""
    w.set_bgzf(False)
    w.format_gpu(*wc.one_read(), "sam")
    assert w.bgzf_stats()["blocks"] == 0                           # the stats are those of the last GPU call


def test_seq(writers):
    w = writers(seq=True)
    for batch in (sc.synthetic(), sc.one_read(), sc.empty()):
        w.set_bgzf(False)
        want = w.format_seq_gpu(*batch)
        w.set_bgzf(True)
        got = w.format_seq_gpu(*batch)
        assert plain_of(got, w.bgzf_eof()) == want, len(got)
        assert w.bgzf_stats()["text_bytes"] == len(want)


def test_device_form(case_inputs):
    """behind a Filter result: format_dev and format_seq_dev with the switch on inflate to their text with it off"""
    import torch
    from linear_amd import Filter
    from linear_amd.api import Writer
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    rid, gid = cases.text_ids(n, len(refs))
    flt = Filter(device=0)
    flt.build_index(refs, 3)
    d_reads = torch.from_numpy(np.ascontiguousarray(reads, dtype=np.uint8)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = flt.filter_batch_dev(d_reads.data_ptr(), d_off.data_ptr(), n)
    w = Writer(gid, [r.size for r in refs])
    w.gpu_open(0)
    w.set_genome(refs)
    calls = {"sam": lambda: w.format_dev(dev, d_off.data_ptr(), rid, "sam"), "apf": lambda: w.format_dev(dev, d_off.data_ptr(), rid, "apf"),
             "seq": lambda: w.format_seq_dev(dev, d_reads.data_ptr(), d_off.data_ptr(), rid)}
    for k, call in calls.items():
        w.set_bgzf(False)
        want = call()
        w.set_bgzf(True)
        got = call()
        assert len(want) > 10_000 and plain_of(got, w.bgzf_eof()) == want, k
        assert w.bgzf_stats()["stored_blocks"] == 0
    w.close(); flt.close()


def test_buffer_reuse(writers):
    """large then small, SAM after APF, switch on / off / on: what a fresh writer gives; a returned run stays intact until the next call"""
    big, small = wc.synthetic(), wc.one_read()
    fresh = {}
    for b in (big, small):
        for k in ("sam", "apf"):
            f = writers()
            plain = f.format_gpu(*b, k)
            f.set_bgzf(True)
            fresh[(id(b), k, True)] = f.format_gpu(*b, k)
            fresh[(id(b), k, False)] = plain
    w = writers()
    for b, k, on in ((big, "apf", True), (small, "apf", True), (small, "sam", True), (big, "sam", True), (big, "sam", False), (small, "apf", False),
                     (big, "apf", True), (small, "sam", False), (small, "sam", True)):
        w.set_bgzf(on)
        assert w.format_gpu(*b, k) == fresh[(id(b), k, on)], (k, on)
    w.set_bgzf(True)
    addr, size = w.format_gpu(*small, "apf", copy=False)
    assert ctypes.string_at(addr, size) == fresh[(id(small), "apf", True)]
    assert w.bgzf_stats()["compressed_bytes"] == size            # (no GPU call in between)
    assert ctypes.string_at(addr, size) == fresh[(id(small), "apf", True)]


def test_needs_gpu_open():
    from linear_amd.api import LnrError, Writer
    w = Writer(wc.GIDS, wc.GLEN)
    for call in (lambda: w.set_bgzf(True), lambda: w.bgzf_bytes_gpu(b"abc"), lambda: w.bgzf_stats()):
        with pytest.raises(LnrError) as e:
            call()
        assert e.value.status == -1
    assert w.bgzf_eof() == bc.EOF_BLOCK                            # a host constant
    w.close()


def test_round_trip_through_the_reader(writers, tmp_path):
    """random_fasta() -> bgzf_bytes_gpu + bgzf_eof -> a file -> Reader.next_dev: the blocks of Reader.next on the plain text, inflated on the device"""
    from linear_amd.api import Reader
    text = bc.random_fasta()
    w = writers()
    raw = w.bgzf_bytes_gpu(text) + w.bgzf_eof()
    pz, pp = str(tmp_path / "rt.fa.gz"), str(tmp_path / "rt.fa")
    open(pz, "wb").write(raw)
    open(pp, "wb").write(text)
    want = rg.serial_blocks(pp, 1 << 22, 100000, serial=False)
    r = Reader(pz)
    r.gpu_open(0, 2)
    got = []
    while True:
        n, dr, dof, off, ids = r.next_dev(1 << 22, 100000)
        if n == 0:
            break
        got.append((off, d2h(dr, int(off[n])), ids))
    st = r.gpu_inflate_stats()["total"]
    r.close()
    same_blocks(got, want, "round trip")
    assert st["blocks"] == (len(text) + BLOCK - 1) // BLOCK and st["gzread_bytes"] == 0 and st["text_bytes"] == len(text), st


@pytest.mark.parametrize("seq", [False, True])
def test_front_end_switch(case_inputs, tmp_path, seq):
    """linear_filter --gpu-writer --bgzf: every .gz inflates to the file of the same run without --bgzf and ends with the EOF marker"""
    from linear_amd import build as lb
    lb.build()
    refs, reads, off = case_inputs("edge")
    rp, gp, _, _ = cases.write_fasta_case(tmp_path, refs, reads, off)
    base = ["timeout", "-k", "10", "240", lb.CLI, "filter", rp, gp, "-t", "3", "-g", "0", "-ot", "3", "--block-reads", "17", "--gpu-writer"] + (["--sam-seq"] if seq else [])
    for tag, extra in (("plain", []), ("bz", ["--bgzf"])):
        p = subprocess.run(base + ["-o", str(tmp_path / tag)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
    assert not os.path.exists(tmp_path / "bz.sam") and not os.path.exists(tmp_path / "bz.apf")
    for ext in (".sam", ".apf"):
        want, raw = open(tmp_path / ("plain" + ext), "rb").read(), open(tmp_path / ("bz" + ext + ".gz"), "rb").read()
        assert raw.endswith(bc.EOF_BLOCK) and len(raw) < len(want) // 2
        got = gzip.decompress(raw)
        assert got == want, diff(want, got)
        assert all(isize <= BLOCK for _, _, isize, _ in bc.walk(raw))
