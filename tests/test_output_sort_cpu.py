"""CPU: the host forms of the coordinate sort and the BAI index (lnr_writer_sort_host / lnr_writer_bai_host, linear_amd/csrc/lnr_output.cpp)
against the plain-Python yardstick of tests/sort_cases.py, on the record streams lnr_writer_format_bam gives for its cases:
  - sort_host(raw) == sorted_stream(raw), and sorting twice changes nothing;
  - bai_host == bai_of with made-up member offsets and two first_offset values, with a record that ends exactly on a member boundary and a
    stream that ends on one;
  - the query test: every record that overlaps a region by brute force lies inside the chunks the index gives for it;
  - a record with end > 2^29: LNR_ERR_UNSUPPORTED naming it; a stream cut short: LNR_ERR_ARG; the GPU entry points before gpu_open: LNR_ERR_ARG;
  - the key extraction header as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_cases as bmc, sort_cases as stc, writer_cases as wc, writer_seq_cases as sc
from tests.test_output_bam_cpu import first_diff

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = stc.BLOCK


@pytest.fixture(scope="module")
def writers():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    w, ws = Writer(wc.GIDS, wc.GLEN), Writer(sc.GIDS, sc.GLEN)
    ws.set_genome(sc.genome())
    yield w, ws
    w.close(); ws.close()


def stream_of(w, batches, seq):
    if seq:
        return b"".join(w.format_bam(coff, cs, ce, None, ids, reads=reads, read_off=off) for coff, cs, ce, reads, off, ids in batches)
    return b"".join(w.format_bam(*b) for b in batches)


@pytest.fixture(scope="module")
def streams(writers):
    """(name, raw stream, writer) of every case, and of what a BAI can hold of it -- formatted once"""
    w, ws = writers
    out = {}
    for index_only in (False, True):
        out[index_only] = [(name, stream_of(w, b, False), w) for name, b in stc.plain_cases(index_only)] + [(name, stream_of(ws, b, True), ws) for name, b in stc.seq_cases(index_only)]
    return out


def made_up_offsets(n_bytes, seed):
    rng = np.random.default_rng(seed)
    n = (n_bytes + BLOCK - 1) // BLOCK
    return np.concatenate([[0], np.cumsum(rng.integers(28, 65536, n))]).astype(np.uint64)


def test_sort_host_equals_the_rule(streams):
    seen = 0
    for name, raw, w in streams[False]:
        want, got = stc.sorted_stream(raw), w.sort_host(raw)
        assert got == want, (name, first_diff(want, got))
        assert w.sort_host(got) == got and stc.is_sorted(got) and len(got) == len(raw), name
        seen += got != raw
    assert seen >= 4                                             # the cases are not sorted as they come


def test_the_shapes_are_in_there(streams):
    by = {name: raw for name, raw, _ in streams[False]}
    recs = stc.records(by["every_batch"])
    assert any(r[2] == -1 for r in recs) and any(r[5] > 1 << 29 for r in recs) and len(recs) > 300
    keys = [(r[2], r[3]) for r in stc.records(by["tie"])]
    ties = [k for k in set(keys) if keys.count(k) > 1]
    flags = {k: {r[4] & 16 for r in stc.records(by["tie"]) if (r[2], r[3]) == k} for k in ties}
    assert len(ties) >= 2 and all(v == {0, 16} for v in flags.values())          # equal and different strand bits on one (refID, pos)
    assert max(r[1] for r in stc.records(by["seq_three_calls"])) > 4 * BLOCK       # a record that covers five members
    assert by["empty_only"] == b"" and by["no_batch"] == b"" and len(stc.records(by["one_record"])) == 1
    assert {r[0] % 4 for r in recs} == {0, 1, 2, 3}                                 # records at every alignment


def test_bai_host_equals_the_rule(streams):
    for name, raw, w in streams[True]:
        srt = w.sort_host(raw)
        for first, seed in ((0, 1), (123_457, 2)):
            moff = made_up_offsets(len(srt), seed)
            want, got = stc.bai_of(srt, first, moff, 3), w.bai_host(srt, first, moff)
            assert got == want, (name, first, first_diff(want, got))
        refs, no_coor = stc.bai_parse(got)
        recs = stc.records(srt)
        assert no_coor == sum(r[2] < 0 for r in recs) and len(refs) == 3
        for ref, (bins, pseudo, lin) in enumerate(refs):
            mine = [r for r in recs if r[2] == ref]
            if not mine:
                assert not bins and pseudo is None and not lin, name
            else:
                assert pseudo[1] == (sum(not r[4] & 4 for r in mine), sum(bool(r[4] & 4) for r in mine)) and len(lin) == 1 + max((r[5] - 1) >> 14 for r in mine)
    for name in ("empty_only", "no_batch"):
        raw, w = next((r, w) for n, r, w in streams[True] if n == name)
        assert w.bai_host(raw, 77, np.zeros(1, np.uint64)) == b"BAI\1" + struct.pack("<i", 3) + struct.pack("<II", 0, 0) * 3 + struct.pack("<Q", 0)


def test_bai_host_on_member_boundaries(streams):
    raw, w = next((r, w) for n, r, w in streams[True] if n == "every_batch")
    padded, first_member = stc.pad_to_boundary(w.sort_host(raw))
    for srt in (padded, first_member):                           # a record that ends exactly where member 1 starts; a stream that ends on the boundary
        moff = made_up_offsets(len(srt), 3)
        want, got = stc.bai_of(srt, 4321, moff, 3), w.bai_host(srt, 4321, moff)
        assert got == want, first_diff(want, got)
    ends = {stc.voffset(s + z, 4321, moff) for s, z, *_ in stc.records(first_member)}
    assert (4321 + int(moff[1])) << 16 in ends                 # the end of the last record points at what follows the last member


def test_queries(streams):
    for name, raw, w in streams[True]:
        srt = w.sort_host(raw)
        moff = made_up_offsets(len(srt), 4)
        hits, empty = stc.check_queries(w.bai_host(srt, 999, moff), srt, 999, moff, wc.GLEN)
        if len(stc.records(srt)) > 5:
            assert hits > 20 and empty > 20, (name, hits, empty)


def test_what_cannot_be_indexed(streams, writers):
    from linear_amd.api import LnrError
    raw, w = next((r, w) for n, r, w in streams[False] if n == "every_batch")
    srt = w.sort_host(raw)
    bad = next(i for i, r in enumerate(stc.records(srt)) if r[2] >= 0 and r[5] > 1 << 29)
    with pytest.raises(stc.Unindexable):
        stc.bai_of(srt, 0, made_up_offsets(len(srt), 1), 3)
    with pytest.raises(LnrError) as e:
        w.bai_host(srt, 0, made_up_offsets(len(srt), 1))
    assert e.value.status == -7 and f"record {bad} " in str(e.value)
    with pytest.raises(LnrError) as e:                           # a stream that ends inside a record
        w.sort_host(srt[:-3])
    assert e.value.status == -1 and "block_size" in str(e.value)
    with pytest.raises(LnrError) as e:
        w.bai_host(srt[:BLOCK], 0, made_up_offsets(BLOCK, 1))
    assert e.value.status == -1


def test_gpu_entry_points_before_gpu_open(writers):
    from linear_amd.api import LnrError
    w, _ = writers
    for call in (lambda: w.sort_begin(), lambda: w.sort_finish(), lambda: list(w.sort_pieces()), lambda: w.sort_bai(0), lambda: w.sort_end()):
        with pytest.raises(LnrError) as e:
            call()
        assert e.value.status == -1 and "gpu_open" in str(e.value)
    assert not w.bam_header("", False)[12:].startswith(b"@HD")


def test_key_extraction_under_sanitizers(streams, tmp_path):
    """host code with its own main: every record of the big cases at the four alignments, in a heap block of exactly its size"""
    exe = str(tmp_path / "sort_key_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "sort_key_main.cpp")])
    for name, raw, _ in streams[False]:
        if name not in ("every_batch", "tie", "seq_three_calls", "one_record"):
            continue
        path = str(tmp_path / f"{name}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<Q", len(raw)) + raw)
            for s, z, ref, pos, flag, end in stc.records(raw):
                f.write(struct.pack("<5q", ref, pos, flag, z - 4, end))
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0 and p.stdout.startswith(b"ok"), (name, p.stderr.decode()[-2000:])
