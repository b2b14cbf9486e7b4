"""CPU: the quality span of a raw BAM record (bam_qual_span, linear_amd/csrc/lnr_output_hd.h: what the sort mode of the GPU writer does not
hold and its gather writes again) through a small host shim, on every record of the sort cases: the span is the one
tests/bam_cases.walk_records finds, it holds 0xff alone, and dropping it and putting l_seq bytes of 0xff back at qoff gives the record
again; a span that does not fit its record is no span; the same function as a stand-alone program (tests/qual_span_main.cpp) under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_cases as bmc, sort_cases as stc, writer_cases as wc, writer_seq_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libqual_span_shim.so")


@pytest.fixture(scope="module")
def span():
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    srcs = [os.path.join(HERE, "qual_span_shim.cpp"), os.path.join(HERE, "..", "linear_amd", "csrc", "lnr_output_hd.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", SO, srcs[0]])
    lib = C.CDLL(SO)
    lib.qs_span.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.qs_span.restype = None

    def get(rec: bytes):
        out = (C.c_uint32 * 2)()
        lib.qs_span(rec, len(rec), out)                          # (a bytes object of exactly the record's size)
        return int(out[0]), int(out[1])
    return get


@pytest.fixture(scope="module")
def streams():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    w, ws = Writer(wc.GIDS, wc.GLEN), Writer(sc.GIDS, sc.GLEN)
    ws.set_genome(sc.genome())
    out = [(name, b"".join(w.format_bam(*b) for b in batches)) for name, batches in stc.plain_cases()]
    out += [(name, b"".join(ws.format_bam(coff, cs, ce, None, ids, reads=reads, read_off=off) for coff, cs, ce, reads, off, ids in batches)) for name, batches in stc.seq_cases()]
    w.close(); ws.close()
    return out


def test_span_of_every_record(span, streams):
    with_seq = 0
    for name, raw in streams:
        p = 0
        for r in bmc.walk_records(raw):
            size = 4 + struct.unpack_from("<i", raw, p)[0]
            rec = raw[p:p + size]
            qoff, l_seq = span(rec)
            if r["l_seq"] == 0:
                assert (qoff, l_seq) == (0, 0), (name, p)
            else:
                want = 36 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + (r["l_seq"] + 1) // 2
                assert (qoff, l_seq) == (want, r["l_seq"]), (name, p)
                assert rec[qoff:qoff + l_seq] == r["qual"] == b"\xff" * l_seq, (name, p)
                held = rec[:qoff] + rec[qoff + l_seq:]
                assert len(held) == size - l_seq and held[:qoff] + b"\xff" * l_seq + held[qoff:] == rec, (name, p)
                with_seq += 1
            p += size
        assert p == len(raw)
    assert with_seq > 50


def test_span_under_sanitizers(streams, tmp_path):
    """host code with its own main: every record of the big cases at the four alignments, in a heap block of exactly its size"""
    exe = str(tmp_path / "qual_span_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "qual_span_main.cpp")])
    for name, raw in streams:
        if name not in ("every_batch", "tie", "seq_three_calls", "one_record"):
            continue
        path = str(tmp_path / f"{name}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<Q", len(raw)) + raw)
            for r in bmc.walk_records(raw):
                qoff = 36 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + (r["l_seq"] + 1) // 2 if r["l_seq"] else 0
                f.write(struct.pack("<2q", qoff, r["l_seq"]))
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0 and p.stdout.startswith(b"ok"), (name, p.stderr.decode()[-2000:])


def test_a_span_that_does_not_fit(span, streams):
    raw = dict(streams)["seq_three_calls"]
    p = next(s for s, z, *_ in stc.records(raw) if struct.unpack_from("<i", raw, s + 20)[0] > 8)
    size = 4 + struct.unpack_from("<i", raw, p)[0]
    rec = bytearray(raw[p:p + size])
    qoff, l_seq = span(bytes(rec))
    assert l_seq > 8
    tail = size - qoff - l_seq                                   # the bytes behind the span (a tag, or none)
    struct.pack_into("<i", rec, 20, l_seq + 2 * tail + 2)        # packed SEQ grows by tail + 1, the span by 2 tail + 2: it ends past the record
    assert span(bytes(rec)) == (0, 0)
    struct.pack_into("<i", rec, 20, -1)                          # a negative l_seq
    assert span(bytes(rec)) == (0, 0)
    cut = bytes(raw[p:p + qoff + l_seq - 1])                     # the record cut short inside its span
    assert span(cut) == (0, 0)
    assert span(bytes(raw[p:p + qoff + l_seq])) == (qoff, l_seq)    # a record that ends with its span
