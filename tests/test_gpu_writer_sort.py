"""GPU: coordinate-sorted BAM with a BAI index from the GPU writer (lnr_writer_sort_*; k_sort_index, the rocPRIM sort, k_sort_gather in
linear_amd/csrc/lnr_output_kernels.hip).  On the cases of tests/sort_cases.py, without and with SEQ: the inflated pieces == sort_host of the
records the same calls return with the mode off == the plain-Python order; the device form behind a Filter result; piece_members 1, 3 and
default give the same file bytes, members of exactly 0xff00 bytes; sort_bai == bai_host == bai_of with two first_offset values and the query
test on the real members; the @HD line; the mode on and off, twice; the memory cap; the call order; the front-end's --sort on the CLI golden
cases, with host cords and under --gpu-reader."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import bam_cases as bmc, bgzf_cases as bc, cases, sort_cases as stc, writer_cases as wc, writer_seq_cases as sc
from tests.test_cli_golden_cpu import sam_by_read
from tests.test_output_bam_cpu import first_diff

pytestmark = pytest.mark.gpu
BLOCK = stc.BLOCK
GOLD = os.path.join(os.path.dirname(__file__), "golden")
EOF = bc.EOF_BLOCK


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


def unsorted(w, batches, seq):
    w.set_bgzf(False)
    return b"".join(bam_call(w, b, seq) for b in batches)


def sort_run(w, batches, seq, piece=0):
    """begin, the BAM calls, finish, every piece: (pieces, info); the mode stays on for sort_bai"""
    w.sort_begin()
    for b in batches:
        assert bam_call(w, b, seq) == b""
    info = w.sort_finish(piece)
    return list(w.sort_pieces()), info


def inflate(pieces):
    return gzip.decompress(b"".join(pieces) + EOF) if pieces else b""


def all_cases(index_only=False):
    return [(n, b, False) for n, b in stc.plain_cases(index_only)] + [(n, b, True) for n, b in stc.seq_cases(index_only)]


@pytest.fixture(scope="module")
def raw_of(writers):
    """the unsorted record stream of a case, encoded once"""
    memo = {}

    def get(name, batches, seq, index_only=False):
        if (name, index_only) not in memo:
            memo[name, index_only] = unsorted(writers(seq), batches, seq)
        return memo[name, index_only]
    return get


def test_sorted_stream(writers, raw_of):
    for name, batches, seq in all_cases():
        w = writers(seq)
        raw = raw_of(name, batches, seq)
        pieces, info = sort_run(w, batches, seq)
        got, host, want = inflate(pieces), w.sort_host(raw), stc.sorted_stream(raw)
        assert host == want, (name, first_diff(want, host))
        assert got == want, (name, first_diff(want, got))
        assert info["records"] == len(stc.records(raw)) and info["record_bytes"] == len(raw) and info["members"] == (len(raw) + BLOCK - 1) // BLOCK, (name, info)
        if raw:
            after = w.sort_info()
            assert info["device_bytes"] >= len(raw) and info["index_ms"] > 0 and info["sort_ms"] > 0 and after["gather_ms"] > 0 and after["deflate_ms"] > 0, (name, info, after)
        else:
            assert pieces == []
        w.sort_end()


def test_device_form(case_inputs):
    """behind a Filter result, on device cords and device reads, without and with SEQ"""
    import torch
    from linear_amd import Filter
    from linear_amd.api import Writer
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    rid, gid = cases.text_ids(n, len(refs))
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
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
    for seq in (False, True):
        host = w.format_bam(coff, cs, ce, None, rid, reads=reads, read_off=off) if seq else w.format_bam(coff, cs, ce, rl, rid)
        w.sort_begin()
        for _ in range(2):                                       # the batch twice: ties across batches
            assert w.format_bam_dev(dev, d_off.data_ptr(), rid, d_reads.data_ptr() if seq else None) == b""
        w.sort_finish(2)
        got = inflate(list(w.sort_pieces()))
        want = stc.sorted_stream(host + host)
        assert len(host) > 10_000 and got == want == w.sort_host(host + host), (seq, first_diff(want, got))
        w.sort_end()
    w.close(); flt.close()


@pytest.mark.parametrize("seq", [False, True])
def test_piece_size_does_not_change_the_file(writers, seq):
    w = writers(seq)
    name, batches = (stc.seq_cases() if seq else stc.plain_cases())[1 - seq]      # every_batch / seq_three_calls
    files = {}
    for piece in (1, 3, 0):
        pieces, info = sort_run(w, batches, seq, piece)
        w.sort_end()
        files[piece] = b"".join(pieces)
        assert len(pieces) == (info["members"] + (piece or 4096) - 1) // (piece or 4096)
        for p in pieces:                                         # every piece is whole members
            assert stc.parse_bgzf(p)[0][-1] == len(p)
    assert files[1] == files[3] == files[0] and len(files[0]) > 0
    members = bc.walk(files[0])
    assert len(members) > (4 if seq else 1) and all(isize == BLOCK for _, _, isize, _ in members[:-1]) and 0 < members[-1][2] <= BLOCK
    if seq:                                                      # a record that covers five members: split across pieces, pieces smaller than it
        assert max(r[1] for r in stc.records(inflate([files[0]]))) > 4 * BLOCK


def test_index(writers):
    for name, batches, seq in all_cases(index_only=True):
        w = writers(seq)
        pieces, info = sort_run(w, batches, seq, 2)
        moff, srt = stc.parse_bgzf(b"".join(pieces))
        assert len(moff) == info["members"] + 1
        for first in (0, 70_001):
            got, host, want = w.sort_bai(first), w.bai_host(srt, first, moff), stc.bai_of(srt, first, moff, 3)
            assert host == want, (name, first, first_diff(want, host))
            assert got == want, (name, first, first_diff(want, got))
        hits, empty = stc.check_queries(got, srt, first, moff, wc.GLEN)
        if len(stc.records(srt)) > 5:
            assert hits > 20 and empty > 20, (name, hits, empty)
        if not srt:
            assert pieces == [] and stc.bai_parse(got) == ([({}, None, [])] * 3, 0)
        w.sort_end()


def test_what_cannot_be_indexed(writers):
    from linear_amd.api import LnrError
    w = writers(False)
    pieces, _ = sort_run(w, [wc.synthetic()], False)
    srt = inflate(pieces)
    bad = next(i for i, r in enumerate(stc.records(srt)) if r[2] >= 0 and r[5] > 1 << 29)
    with pytest.raises(LnrError) as e:
        w.sort_bai(0)
    assert e.value.status == -7 and f"record {bad} " in str(e.value)
    assert srt == stc.sorted_stream(unsorted_after_end(w, [wc.synthetic()]))                # the sorted BAM itself is whole


def unsorted_after_end(w, batches):
    w.sort_end()
    return unsorted(w, batches, False)


def test_header_and_mode_on_off(writers):
    from linear_amd.api import LnrError
    w = writers(False)
    batches = stc.tie_batches() + [wc.one_read()]
    head, head8 = w.bam_header("cl", False), w.bam_header("cl", True)
    before, sam = unsorted(w, batches, False), w.format_gpu(*batches[0], "sam")
    files = []
    for _ in range(2):                                           # a second round on the same writer: the same bytes
        w.sort_begin()
        text, refs, rest = bmc.split_bam(w.bam_header("cl", False))
        plain = bmc.split_bam(head)
        assert text == stc.HD + plain[0] and refs == plain[1] and rest == b""
        assert bmc.split_bam(w.bam_header("cl", True))[0] == stc.HD + bmc.split_bam(head8)[0]
        for b in batches:
            assert w.format_bam_gpu(*b) == b""
            assert w.format_gpu(*batches[0], "sam") == sam       # every other call is unchanged while the mode is on
        w.sort_finish()
        files.append(b"".join(w.sort_pieces()))
        assert w.sort_bai(0)[:4] == b"BAI\1"
        w.sort_end()
        assert w.bam_header("cl", False) == head and w.bam_header("cl", True) == head8
        assert unsorted(w, batches, False) == before
    assert files[0] == files[1] and inflate([files[0]]) == stc.sorted_stream(before)
    # the call order
    for call in (lambda: w.sort_finish(), lambda: list(w.sort_pieces()), lambda: w.sort_bai(0)):
        with pytest.raises(LnrError) as e:
            call()
        assert e.value.status == -1 and "sort" in str(e.value)
    w.sort_begin()
    for call in (lambda: w.sort_begin(), lambda: list(w.sort_pieces()), lambda: w.sort_bai(0)):
        with pytest.raises(LnrError) as e:
            call()
        assert e.value.status == -1 and "sort" in str(e.value)
    w.format_bam_gpu(*batches[2])
    w.sort_finish(1)
    with pytest.raises(LnrError) as e:                           # the index needs the members' offsets: after the last piece
        w.sort_bai(0)
    assert e.value.status == -1
    with pytest.raises(LnrError) as e:                           # no BAM call between finish and end
        w.format_bam_gpu(*batches[2])
    assert e.value.status == -1 and "sort_end" in str(e.value)
    assert inflate(list(w.sort_pieces())) == stc.sorted_stream(w.format_bam(*batches[2]))
    w.sort_end()
    w.sort_end()                                                 # leaving twice is harmless


def test_memory_cap(writers):
    from linear_amd.api import LnrError
    w = writers(False)
    first, second = wc.gap_set(*wc.GAP_SETS[0]), wc.synthetic()
    raw1, raw2 = unsorted(w, [first], False), unsorted(w, [second], False)
    w.sort_begin(len(raw1) + len(raw2) - 1)
    assert w.format_bam_gpu(*first) == b""
    with pytest.raises(LnrError) as e:
        w.format_bam_gpu(*second)
    assert e.value.status == -4 and str(len(raw1)) in str(e.value) and str(len(raw2)) in str(e.value)
    info = w.sort_finish()                                       # the batch added before is intact: exactly it, sorted
    got = inflate(list(w.sort_pieces()))
    assert got == stc.sorted_stream(raw1) and info["record_bytes"] == len(raw1)
    w.sort_end()
    w.sort_begin(len(raw1) + len(raw2))                          # exactly enough
    assert w.format_bam_gpu(*first) == b"" and w.format_bam_gpu(*second) == b""
    w.sort_finish()
    assert inflate(list(w.sort_pieces())) == stc.sorted_stream(raw1 + raw2)
    w.sort_end()


FRONT_MODE = {"edge": "g0", "chim": "g50dup1"}                   # a mode per case whose `-ss 1` .sam is a golden and that has no excluded read


@pytest.mark.parametrize("reader", [False, True])
@pytest.mark.parametrize("name", ["edge", "chim"])
def test_front_end(case_inputs, tmp_path, name, reader):
    """linear_filter --gpu-writer --sort with -ot 4, and with -ot 14 --sam-seq --block-reads 23: every .bam inflates to the golden header behind
    an @HD line + the records of the unsorted golden .bam (with SEQ: of the run's own .sam, which is the golden .sam) in sorted_stream order;
    the .bai next to it is bai_of of that file; members of 0xff00 bytes"""
    from linear_amd import build as lb
    lb.build()
    refs, reads, off = case_inputs(name)
    mode = FRONT_MODE[name]
    g, gss = (np.load(os.path.join(GOLD, f"{k}_{name}.npz")) for k in ("cli_bam", "cli_ss"))
    rp, gp, _, gid = cases.write_fasta_case(tmp_path, refs, reads, off)
    for ot, more in (("4", []), ("14", ["--sam-seq", "--block-reads", "23"])):
        pre = str(tmp_path / f"s{ot}")
        p = subprocess.run(["timeout", "-k", "10", "240", lb.CLI, "filter", rp, gp, "-t", "1", "-ot", ot, "-o", pre, "--gpu-writer", "--sort"] + cases.CLI_MODES[mode] + more +
                           (["--gpu-reader"] if reader else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        if ot == "14":
            sam = open(pre + ".sam", "rb").read()
            (head, got_r), (whead, want_r) = sam_by_read(sam), sam_by_read(gss[f"sam_{mode}"].tobytes())
            assert head == whead and got_r == want_r             # the .sam stays in read order, without @HD
            want = bmc.bam_of_sam(sam, gid)
        else:
            assert not os.path.exists(pre + ".sam")
            want = g[f"recs_{mode}"].tobytes()
        want = stc.sorted_stream(want)
        for path, key in [(pre + ".bam", f"header_{mode}")] + ([(pre + "_pbsv.bam", "header_pbsv")] if ot == "14" else []):
            raw = open(path, "rb").read()
            assert raw.endswith(EOF) and raw.count(EOF) == 1
            moff, plain = stc.parse_bgzf(raw[:-len(EOF)])
            text, ref_list, recs = bmc.split_bam(plain)
            assert text == stc.HD + g[key].tobytes() and ref_list == [(i.encode(), r.size) for i, r in zip(gid, refs)]
            assert recs == want and len(stc.records(recs)) > 20 and recs != g[f"recs_{mode}"].tobytes(), first_diff(want, recs)
            n_head = (len(plain) - len(recs) + BLOCK - 1) // BLOCK      # the header's members, then one per 0xff00 bytes of records
            assert len(moff) - 1 - n_head == (len(recs) + BLOCK - 1) // BLOCK
            first = moff[n_head]
            bai = open(path + ".bai", "rb").read()
            assert bai == stc.bai_of(recs, first, [m - first for m in moff[n_head:]], len(refs))
            stc.check_queries(bai, recs, first, [m - first for m in moff[n_head:]], [r.size for r in refs])


@pytest.mark.parametrize("reader", [False, True])
def test_front_end_one_output_per_read_file(case_inputs, tmp_path, reader):
    """two read files without -o: a sort round per output file (under --gpu-reader the calculator waits at the fence until the writer thread has
    finished the first file); both files are the single file's sorted records with their own index"""
    import shutil
    from linear_amd import build as lb
    lb.build()
    refs, reads, off = case_inputs("edge")
    g = np.load(os.path.join(GOLD, "cli_bam_edge.npz"))
    rp, gp, _, gid = cases.write_fasta_case(tmp_path, refs, reads, off)
    for name in ("one.fa", "two.fa"):
        shutil.copy(rp, str(tmp_path / name))
    p = subprocess.run(["timeout", "-k", "10", "240", lb.CLI, "filter", "one.fa", "two.fa", "x", gp, "-t", "1", "-ot", "4", "-g", "0", "--gpu-writer", "--sort", "--block-reads", "23"] +
                       (["--gpu-reader"] if reader else []), cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-1000:]
    raw = [open(str(tmp_path / f"{n}.bam"), "rb").read() for n in ("one", "two")]
    bai = [open(str(tmp_path / f"{n}.bam.bai"), "rb").read() for n in ("one", "two")]
    assert raw[0] == raw[1] and bai[0] == bai[1] and raw[0].endswith(EOF) and raw[0].count(EOF) == 1
    moff, plain = stc.parse_bgzf(raw[0][:-len(EOF)])
    text, _, recs = bmc.split_bam(plain)
    assert text.startswith(stc.HD) and recs == stc.sorted_stream(g["recs_g0"].tobytes())
    n_head = (len(plain) - len(recs) + BLOCK - 1) // BLOCK
    assert bai[0] == stc.bai_of(recs, moff[n_head], [m - moff[n_head] for m in moff[n_head:]], len(refs))
