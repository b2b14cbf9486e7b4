"""Shared by the PAF tests (tests/test_output_paf_cpu.py, tests/test_cli_paf_cpu.py, tests/test_gpu_writer_paf.py): the PAF line derived in
Python from a SAM line -- flag, RNAME, POS and CIGAR* -- plus the read's length and the genome's lengths (the definition of the line:
include/linear_amd.h), the validity of a line, and small batches of cord words for the shapes the kernels' read skeleton can get wrong."""
import re

import numpy as np

from tests import writer_cases as wc

ELEMENT = re.compile(rb"(\d+)([SID=X])")


def paf_of_sam_line(line: bytes, L: int, glen: dict, clips=None) -> bytes:
    """glen: target name -> length.  clips: (lead, trail) where the CIGAR* cannot say them: one single S element is either of the two."""
    f = line.split(b"\t")
    qname, flag, rname, pos, cigar = f[0], int(f[1]), f[2], int(f[3]), f[5]
    els = [(int(c), o) for c, o in ELEMENT.findall(cigar)] if cigar != b"*" else []
    assert b"".join(b"%d%s" % e for e in els) == (cigar if cigar != b"*" else b""), cigar
    if clips is None:
        assert not (len(els) == 1 and els[0][1] == b"S"), "a CIGAR* of one S element: lead and trail cannot be told apart from the text"
        lead = els[0][0] if els and els[0][1] == b"S" else 0
        trail = els[-1][0] if len(els) > 1 and els[-1][1] == b"S" else 0
    else:
        lead, trail = clips
    core = [(c, o) for c, o in els if o != b"S"]
    assert len(core) >= len(els) - 2
    rev = bool(flag & 16)
    qs, qe = (trail, L - lead) if rev else (lead, L - trail)
    ts = pos - 1
    te = ts + sum(c for c, o in core if o in b"=XD")
    cols = [qname, b"%d" % L, b"%d" % qs, b"%d" % qe, b"-" if rev else b"+", rname, b"%d" % (glen[rname] if rname != b"*" else 0), b"%d" % ts, b"%d" % te,
            b"%d" % sum(c for c, o in core if o == b"="), b"%d" % sum(c for c, o in core), b"255"]
    if core:
        cols.append(b"cg:Z:" + b"".join(b"%d%s" % e for e in core))
    return b"\t".join(cols) + b"\n"


def paf_of_sam(sam: bytes, read_len: dict, glen: dict) -> bytes:
    """The PAF of a SAM text (header lines skipped).  read_len: QNAME -> bases."""
    return b"".join(paf_of_sam_line(l, read_len[l.split(b"\t")[0]], glen) for l in sam.split(b"\n") if l and not l.startswith(b"@"))


def check_valid(paf: bytes, n_records: int) -> None:
    """0 <= qstart <= qend <= qlen, tstart <= tend, matches <= block, twelve columns and at most the cg tag, as many lines as SAM records."""
    lines = paf.split(b"\n")
    assert lines[-1] == b"" and len(lines) - 1 == n_records
    for l in lines[:-1]:
        f = l.split(b"\t")
        assert len(f) in (12, 13) and f[4] in (b"+", b"-") and f[11] == b"255", l
        ql, qs, qe, tl, ts, te, m, bl = (int(f[i]) for i in (1, 2, 3, 6, 7, 8, 9, 10))
        assert 0 <= qs <= qe <= ql and ts <= te and m <= bl, l
        assert f[5] != b"*" or tl == 0, l
        if len(f) == 13:
            assert f[12].startswith(b"cg:Z:") and ELEMENT.sub(b"", f[12][5:]) == b"" and b"S" not in f[12][5:], l
        else:
            assert bl == 0, l


def sam_records(sam: bytes) -> int:
    return sum(1 for l in sam.split(b"\n") if l and not l.startswith(b"@"))


# ---- batches for the GPU twin: every read starts with the dummy cord, as the pipeline emits it
def strands_and_clips():
    """One-cord reads on both strands: lead and trail clips of zero and of a positive number; L below the last cord's end (the trail clamps to 0)."""
    B = wc.Batch()
    for strand in (0, 1):
        for y in (0, 17):
            for extra in (0, 23):
                B.read([(5000, y, strand, 0, True, 96)], L=y + 96 + extra)
        B.read([(5000, 17, strand, 0, True, 96)], L=100)             # L < 17 + 96
    return B.arrays()


def tile_edges():
    """Reads of 64, 65, 128 and 129 cords (with the dummy): in one record, and with a record per cord, so a tile boundary falls inside and between records."""
    B = wc.Batch()
    for n in (64, 65, 128, 129):
        B.read(wc.run(n - 1))
        B.read(wc.many_records(n - 1))
    return B.arrays()


def window_lines():
    """One line longer than the kernels' LDS window (8192 bytes), and a line that straddles a window edge.  A line grows with its cg tag -- a
    record of cords that alternate between two diagonals has some nine bytes of it per cord -- and with its QNAME; the lines of one tile of 64
    cords share windows that start at the tile's first byte, so the edge falls into the third and the sixth of six lines of 3 kB whose records start in one tile."""
    B = wc.Batch()
    B.read([(10_000 + 200 * i + (7 if i & 1 else 0), 5 + 200 * i, 0, 0, False, 96) for i in range(1500)])
    B.read(wc.many_records(6), rid="W" * 3000)
    B.read(wc.run(2))
    return B.arrays()


def misaligned():
    """Consecutive reads whose texts have lengths = 1, 2, 3 mod 4 (the QNAME grows by one character): every destination misalignment."""
    B = wc.Batch()
    for k in range(8):
        B.read(wc.run(2), rid="q" * (k + 1))
    return B.arrays()


def target_fields():
    """An id beyond nseq ('*', length 0) and the sequence with the 10-digit length."""
    B = wc.Batch()
    B.read(wc.run(2, gid=5))
    B.read(wc.run(2, gid=0))
    B.read(wc.run(2, gid=2, strand=1))
    return B.arrays()
