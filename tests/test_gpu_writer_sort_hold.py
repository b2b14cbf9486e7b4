"""GPU: what the sort mode of the GPU writer holds and where (lnr_writer_sort_spill, lnr_writer_sort_hold_info_get; k_sort_keep and the
three-range k_sort_gather in linear_amd/csrc/lnr_output_kernels.hip).  On the cases of tests/sort_cases.py: the compact hold (the bytes held
are the records without their l_seq quality bytes, the pieces are the full sorted stream); every batch in pinned host memory; one batch on
the device and the rest on the host, with the index; the host budget to the byte; the call order and a round after a spilled one; the device
form; the front-end's --sort-device-mem / --sort-host-mem."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_cases as bmc, bgzf_cases as bc, cases, sort_cases as stc, writer_cases as wc, writer_seq_cases as sc
from tests.test_cli_golden_cpu import sam_by_read
from tests.test_output_bam_cpu import first_diff

pytestmark = pytest.mark.gpu
BLOCK = stc.BLOCK
EOF = bc.EOF_BLOCK
HOST = 64 << 20


@pytest.fixture(scope="module")
def writers():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    made = {}

    def get(seq):
        if seq not in made:
            w = Writer(sc.GIDS, sc.GLEN) if seq else Writer(wc.GIDS, wc.GLEN)
            if seq:
                w.set_genome(sc.genome())
            w.gpu_open(0)
            made[seq] = w
        return made[seq]
    yield get
    for w in made.values():
        w.close()


def bam_call(w, batch, seq):
    if seq:
        coff, cs, ce, reads, off, ids = batch
        return w.format_bam_gpu(coff, cs, ce, None, ids, reads=reads, read_off=off)
    return w.format_bam_gpu(*batch)


@pytest.fixture(scope="module")
def raws(writers):
    """the unsorted record stream of every batch of a case, encoded once with the mode off"""
    memo = {}

    def get(name, batches, seq, index_only=False):
        if (name, index_only) not in memo:
            w = writers(seq)
            w.set_bgzf(False)
            memo[name, index_only] = [bam_call(w, b, seq) for b in batches]
        return memo[name, index_only]
    return get


def inflate(pieces):
    return gzip.decompress(b"".join(pieces) + EOF) if pieces else b""


def held_size(raw):
    """the bytes of a record stream without the quality spans: l_seq at byte 20 of each record"""
    return len(raw) - sum(struct.unpack_from("<i", raw, s + 20)[0] for s, *_ in stc.records(raw))


def run(w, batches, seq, cap=0, host=None, piece=0):
    """a round up to its last piece: (pieces, sort info, hold info); the mode stays on"""
    w.sort_begin(cap)
    if host is not None:
        w.sort_spill(host)
    for b in batches:
        assert bam_call(w, b, seq) == b""
    hold = w.sort_hold_info()
    info = w.sort_finish(piece)
    return list(w.sort_pieces()), info, hold


def case(name, seq=False, index_only=False):
    return next(b for n, b in (stc.seq_cases if seq else stc.plain_cases)(index_only) if n == name)


def test_compact_hold_on_the_device(writers, raws):
    for name, batches, seq in [(n, b, False) for n, b in stc.plain_cases()] + [(n, b, True) for n, b in stc.seq_cases()]:
        w = writers(seq)
        raw = b"".join(raws(name, batches, seq))
        pieces, info, hold = run(w, batches, seq)
        got, want = inflate(pieces), stc.sorted_stream(raw)
        assert got == want, (name, first_diff(want, got))
        assert got == w.sort_host(raw), name
        assert hold["held_device_bytes"] == held_size(raw) and hold["stream_bytes"] == len(raw) == info["record_bytes"] and hold["held_host_bytes"] == 0, (name, hold)
        assert hold["host_batches"] == 0 and hold["device_batches"] == sum(1 for r in raws(name, batches, seq) if r), (name, hold)
        if name == "seq_three_calls":
            assert len(raw) - held_size(raw) > 0 and hold["keep_ms"] > 0              # sum of l_seq: the compaction is exercised
        assert w.sort_hold_info() == hold                       # readable until sort_end
        w.sort_end()


@pytest.mark.parametrize("name,seq", [("every_batch", False), ("tie", False), ("seq_three_calls", True)])
def test_everything_on_the_host(writers, raws, name, seq):
    w = writers(seq)
    batches = case(name, seq)
    per = raws(name, batches, seq)
    raw = b"".join(per)
    plain = b"".join(run(w, batches, seq)[0])
    w.sort_end()
    files = {}
    for piece in (1, 3, 0):
        pieces, info, hold = run(w, batches, seq, cap=1, host=HOST, piece=piece)
        w.sort_end()
        files[piece] = b"".join(pieces)
        assert hold["held_device_bytes"] == 0 and hold["device_batches"] == 0 and hold["host_batches"] == sum(1 for r in per if r), hold
        assert hold["held_host_bytes"] == held_size(raw) and hold["stream_bytes"] == len(raw) and hold["spill_ms"] > 0, hold
    got, want = inflate([files[0]]), stc.sorted_stream(raw)
    assert got == want, first_diff(want, got)
    assert files[1] == files[3] == files[0] == plain


@pytest.mark.parametrize("name,seq", [("every_batch", False), ("tie", False), ("seq_three_calls", True)])
def test_mixed_tiers(writers, raws, name, seq):
    w = writers(seq)
    batches = case(name, seq, index_only=True)
    per = raws(name, batches, seq, True)
    raw = b"".join(per)
    assert per[0] and sum(1 for r in per if r) >= 2
    pieces, info, hold = run(w, batches, seq, cap=held_size(per[0]), host=HOST, piece=2)
    assert hold["device_batches"] == 1 and hold["held_device_bytes"] == held_size(per[0]), hold
    assert hold["host_batches"] == sum(1 for r in per[1:] if r) and hold["held_host_bytes"] == held_size(raw) - held_size(per[0]), hold
    moff, srt = stc.parse_bgzf(b"".join(pieces))
    want = stc.sorted_stream(raw)
    assert srt == want, first_diff(want, srt)
    assert srt == w.sort_host(raw)
    for first in (0, 70_001):
        got, host, ref = w.sort_bai(first), w.bai_host(srt, first, moff), stc.bai_of(srt, first, moff, 3)
        assert host == ref and got == ref, (first, first_diff(ref, got))
    w.sort_end()


def test_host_budget(writers, raws):
    from linear_amd.api import LnrError
    w = writers(True)
    batches = [b for b in case("seq_three_calls", True)]
    per = raws("seq_three_calls", batches, True)
    first, second = batches[0], batches[1]
    h1, h2 = held_size(per[0]), held_size(per[1])
    assert h1 and h2
    w.sort_begin(1)
    w.sort_spill(h1 + h2 - 1)
    assert bam_call(w, first, True) == b""
    with pytest.raises(LnrError) as e:
        bam_call(w, second, True)
    assert e.value.status == -4 and " 0 record bytes held on the device" in str(e.value) and f"{h1} in host memory" in str(e.value) and str(h2) in str(e.value), str(e.value)
    hold = w.sort_hold_info()
    assert hold["held_host_bytes"] == h1 and hold["host_batches"] == 1 and hold["stream_bytes"] == len(per[0])       # nothing of the state changed
    info = w.sort_finish()
    assert inflate(list(w.sort_pieces())) == stc.sorted_stream(per[0]) and info["record_bytes"] == len(per[0])
    w.sort_end()
    w.sort_begin(1)
    w.sort_spill(h1 + h2)                                       # exactly enough
    assert bam_call(w, first, True) == b"" and bam_call(w, second, True) == b""
    w.sort_finish()
    assert inflate(list(w.sort_pieces())) == stc.sorted_stream(per[0] + per[1])
    w.sort_end()


def test_call_order_and_rounds(writers, raws):
    from linear_amd.api import LnrError, Writer
    w = writers(False)
    batches = stc.tie_batches()
    per = raws("tie", batches, False)
    raw = b"".join(per)

    def refused(call):
        with pytest.raises(LnrError) as e:
            call()
        assert e.value.status == -1 and "sort" in str(e.value)
    refused(lambda: w.sort_spill(HOST))                         # before sort_begin
    fresh = Writer(wc.GIDS, wc.GLEN)                            # before gpu_open
    with pytest.raises(LnrError) as e:
        fresh.sort_spill(HOST)
    assert e.value.status == -1 and "sort" in str(e.value)
    with pytest.raises(LnrError) as e:
        fresh.sort_hold_info()
    assert e.value.status == -1
    fresh.close()
    files = []
    for _ in range(2):                                           # two spilled rounds on one writer: the same bytes
        pieces, _, hold = run(w, batches, False, cap=1, host=HOST)
        assert hold["host_batches"] == 2
        refused(lambda: w.sort_spill(HOST))                      # after sort_finish
        files.append(b"".join(pieces))
        w.sort_end()
    assert files[0] == files[1] and inflate([files[0]]) == stc.sorted_stream(raw)
    w.sort_begin(len(raw) - 1)                                  # a round without sort_spill behaves as before: the cap gives -4
    assert w.format_bam_gpu(*batches[0]) == b""
    with pytest.raises(LnrError) as e:
        w.format_bam_gpu(*batches[1])
    assert e.value.status == -4 and str(len(per[0])) in str(e.value) and str(len(per[1])) in str(e.value) and "host" not in str(e.value)
    w.sort_end()
    w.sort_begin(1)                                             # switched on and off again inside a round
    w.sort_spill(HOST)
    w.sort_spill(0)
    with pytest.raises(LnrError) as e:
        w.format_bam_gpu(*batches[0])
    assert e.value.status == -4
    w.sort_end()


def test_device_form(case_inputs):
    """behind a Filter result, on device cords and device reads, with SEQ: everything spilled and nothing spilled"""
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
    coff, cs, ce = flt.cords_to_host()
    w = Writer(gid, [r.size for r in refs])
    w.gpu_open(0)
    w.set_genome(refs)
    host = w.format_bam(coff, cs, ce, None, rid, reads=reads, read_off=off)
    want = stc.sorted_stream(host + host)
    assert len(host) > 10_000 and want == w.sort_host(host + host)
    for spill in (True, False):
        w.sort_begin(1 if spill else 0)
        if spill:
            w.sort_spill(HOST)
        for _ in range(2):
            assert w.format_bam_dev(dev, d_off.data_ptr(), rid, d_reads.data_ptr()) == b""
        hold = w.sort_hold_info()
        assert (hold["host_batches"], hold["device_batches"]) == ((2, 0) if spill else (0, 2)) and hold["held_host_bytes"] + hold["held_device_bytes"] == held_size(host + host)
        w.sort_finish(2)
        got = inflate(list(w.sort_pieces()))
        assert got == want, (spill, first_diff(want, got))
        w.sort_end()
    w.close(); flt.close()


@pytest.mark.parametrize("reader", [False, True])
def test_front_end(case_inputs, tmp_path, reader):
    """linear_filter -ot 14 --sam-seq --block-reads 23 --gpu-writer --sort, plain and with --sort-device-mem 1 --sort-host-mem 64M: the same
    .bam, _pbsv.bam and indexes byte for byte, and the records are the sorted records of the run's .sam (the golden .sam)"""
    from linear_amd import build as lb
    lb.build()
    refs, reads, off = case_inputs("edge")
    gss = np.load(os.path.join(os.path.dirname(__file__), "golden", "cli_ss_edge.npz"))
    rp, gp, _, gid = cases.write_fasta_case(tmp_path, refs, reads, off)
    out = {}
    for tag, more in (("plain", []), ("spill", ["--sort-device-mem", "1", "--sort-host-mem", "64M"])):
        pre = str(tmp_path / tag)
        p = subprocess.run(["timeout", "-k", "10", "240", lb.CLI, "filter", rp, gp, "-t", "1", "-ot", "14", "-o", pre, "--gpu-writer", "--sort", "--sam-seq", "--block-reads", "23"] +
                           cases.CLI_MODES["g0"] + more + (["--gpu-reader"] if reader else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        out[tag] = [open(pre + ext, "rb").read() for ext in (".bam", "_pbsv.bam", ".bam.bai", "_pbsv.bam.bai", ".sam")]
    assert out["plain"] == out["spill"]
    sam = out["spill"][4]
    assert sam_by_read(sam) == sam_by_read(gss["sam_g0"].tobytes())
    want = stc.sorted_stream(bmc.bam_of_sam(sam, gid))
    for raw in out["spill"][:2]:
        assert raw.endswith(EOF)
        _, plain = stc.parse_bgzf(raw[:-len(EOF)])
        recs = bmc.split_bam(plain)[2]
        assert recs == want and len(stc.records(recs)) > 20, first_diff(want, recs)
