"""Inputs for the reader's GPU twin (tests/test_reader_hd_cpu.py on the host logic, tests/test_gpu_reader.py on the device): the seeded
random file of tests/test_reader_cpu.py::test_parallel_and_serial_parsers_agree as a function, the tile / window edge files, and the
serial reader as the yardstick."""
import gzip
import os

import numpy as np


def random_file(path, fmt, n=1500, seed=17):
    """CRLF, blanks inside FASTA lines, empty records, '>' / '@' inside headers and qualities; fmt 'fastq_multiline' leaves the four-line
    form from record 701 on.  Returns the byte offset of the first record that is not in four-line form (None: none)."""
    rng = np.random.default_rng(seed)
    abc = np.frombuffer(b"ACGTacgtNnRYKMU", np.uint8)
    handover = None
    with open(path, "wb") as f:
        for i in range(n):
            L = int(rng.integers(0, 900)) if i % 97 else 0
            s = abc[rng.integers(0, abc.size, L)].tobytes()
            eol = b"\r\n" if i % 5 == 0 else b"\n"
            if fmt == "fasta":
                w = int(rng.integers(20, 200))
                body = eol.join(s[k:k + w] for k in range(0, max(L, 1), w)) if i % 3 else s
                if i % 11 == 0:
                    body = body.replace(b"A", b"A ", 1)
                f.write(b">rd%d > x @ y" % i + eol + body + eol + (eol if i % 7 == 0 else b""))
            else:
                q = bytes(rng.integers(33, 74, L, dtype=np.uint8).tolist())        # '@' (64) and '>' (62) occur in qualities
                if fmt == "fastq_multiline" and i > 700 and L > 50:
                    if handover is None:
                        handover = f.tell()
                    f.write(b"@rd%d" % i + eol + s[:30] + eol + s[30:] + eol + b"+" + eol + q[:40] + eol + q[40:] + eol)
                else:
                    f.write(b"@rd%d desc" % i + eol + s + eol + b"+" + (b"rd%d" % i if i % 2 else b"") + eol + q + eol)
    return handover


def plain_text(path):
    """the text of a fixture, inflated where it is gzip"""
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def serial_blocks(path, dst_cap, max_reads, serial=True):
    """[(off, bases, ids)] per block of lnr_reader_next (with LNR_READER_SERIAL=1: the byte-wise parser that SeqAn's reader pins)"""
    from linear_amd.api import Reader
    old = os.environ.get("LNR_READER_SERIAL")
    if serial:
        os.environ["LNR_READER_SERIAL"] = "1"
    try:
        r = Reader(path)
    finally:
        if serial:
            if old is None:
                del os.environ["LNR_READER_SERIAL"]
            else:
                os.environ["LNR_READER_SERIAL"] = old
    dst = np.zeros(max(dst_cap, 1), np.uint8)
    out = []
    from linear_amd.api import LnrError
    while True:
        try:
            n, off, ids = r.next(dst, max_reads)
        except LnrError as e:                 # a record longer than the block: the blocks before it stand
            if e.status != -6:
                raise
            break
        if n == 0:
            break
        out.append((off.copy(), dst[: int(off[n])].copy(), ids))
    r.close()
    return out


def edge_files(d, T):
    """FASTA / FASTQ files of 1 to 5 records whose record starts, header ends, CR / LF of a CRLF and '+' lines land at T-1, T, T+1 and the
    same around 2T; a header longer than 2T, a sequence line longer than 3T, an empty last record, a last record without '\\n', one record."""
    os.makedirs(d, exist_ok=True)
    out = {}

    def put(name, data):
        p = os.path.join(d, name)
        with open(p, "wb") as f:
            f.write(data)
        out[name] = p

    def seq(n, k=0):
        return bytes(b"ACGTNacgtRY"[(i * 7 + k) % 11] for i in range(n))
    for base in (T, 2 * T):
        for d_ in (-1, 0, 1):
            at = base + d_
            tag = "%d%+d" % (base // T, d_)
            # FASTA: record 2 starts at `at`
            h = b">r1 first\n"
            put(f"fa_start_{tag}.fa", h + seq(at - len(h) - 1) + b"\n>r2 second\n" + seq(300, 1) + b"\n>r3\n" + seq(70, 2) + b"\n")
            # the header's '\n' at `at`
            put(f"fa_hdrnl_{tag}.fa", b">" + b"h" * (at - 1) + b"\n" + seq(200) + b"\n>r2\n" + seq(50, 3) + b"\n>r3 x\n" + seq(9) + b"\n")
            # CRLF: '\r' at `at` (so '\n' at at + 1), and '\n' at `at`
            put(f"fa_cr_{tag}.fa", b">r1\r\n" + seq(at - 5) + b"\r\n" + seq(100, 1) + b"\r\n>r2 y\r\n" + seq(80, 2) + b"\r\n>r3\r\n" + seq(8) + b"\r\n")
            put(f"fa_lf_{tag}.fa", b">r1\r\n" + seq(at - 6) + b"\r\n" + seq(100, 1) + b"\r\n>r2 y\r\n" + seq(80, 2) + b"\r\n>r3\r\n\r\n")
            # FASTQ: record 2 starts at `at`; the '+' line at `at`; CR / LF of the sequence line
            L1 = (at - len(b"@q1 a\n") - len(b"\n+\n") - 1) // 2
            pad = at - (len(b"@q1 a\n") + 2 * L1 + len(b"\n+\n") + 1)
            put(f"fq_start_{tag}.fq", b"@q1 a" + b"x" * pad + b"\n" + seq(L1) + b"\n+\n" + b"I" * L1 + b"\n@q2 b\n" + seq(200, 1) + b"\n+q2\n" + b"@" * 200 + b"\n@q3\n" + seq(5) + b"\n+\n" + b">>>>>\n")
            L2 = at - len(b"@q1 a\n") - 1
            put(f"fq_plus_{tag}.fq", b"@q1 a\n" + seq(L2) + b"\n+\n" + b"J" * L2 + b"\n@q2\n" + seq(33, 2) + b"\n+\n" + b"K" * 33 + b"\n@q3\n\n+\n\n")
            L3 = at - len(b"@q1\r\n")
            put(f"fq_cr_{tag}.fq", b"@q1\r\n" + seq(L3) + b"\r\n+\r\n" + b"J" * L3 + b"\r\n@q2\r\n" + seq(40) + b"\r\n+\r\n" + b"K" * 40 + b"\r\n@q3\r\n" + seq(7) + b"\r\n+\r\n" + b"L" * 7)
            put(f"fq_lf_{tag}.fq", b"@q1\r\n" + seq(L3 - 1) + b"\r\n+\r\n" + b"J" * (L3 - 1) + b"\r\n@q2\r\n" + seq(40) + b"\r\n+\r\n" + b"K" * 40 + b"\r\n@q3\r\n" + seq(7) + b"\r\n+\r\n" + b"L" * 7 + b"\r\n")
    put("fa_long_header.fa", b">" + b"H" * (2 * T + 37) + b"\n" + seq(100) + b"\n>r2\n" + seq(10) + b"\n>r3\n" + seq(20, 1) + b"\n")
    put("fa_long_line.fa", b">r1\n" + seq(3 * T + 111) + b"\n>r2\n" + seq(66) + b"\n>r3\n" + seq(5) + b"\n>r4 empty, the last\n")
    put("fa_no_final_nl.fa", b">r1\n" + seq(T + 3) + b"\n>r2\n" + seq(77))
    put("fa_one.fa", b">only one\n" + seq(123) + b"\n")
    put("fa_header_only.fa", b">r1\n" + seq(12) + b"\n>r2 cut")
    put("fq_long_header.fq", b"@" + b"H" * (2 * T + 5) + b"\n" + seq(10) + b"\n+\n" + b"I" * 10 + b"\n@q2\n" + seq(4) + b"\n+\n" + b"IIII\n@q3\nA\n+\nI\n")
    put("fq_long_line.fq", b"@q1\n" + seq(3 * T + 9) + b"\n+\n" + b"F" * (3 * T + 9) + b"\n@q2\n" + seq(30) + b"\n+\n" + b"G" * 30 + b"\n@q3\nAC\n+\nII\n")
    put("fq_no_final_nl.fq", b"@q1\n" + seq(T + 1) + b"\n+\n" + b"F" * (T + 1) + b"\n@q2\n" + seq(30) + b"\n+\n" + b"G" * 30)
    put("fq_one.fq", b"@only\n" + seq(222) + b"\n+only\n" + b"E" * 222 + b"\n")
    put("fq_unequal.fq", b"@q1\nACGT\n+\nIIII\n@q2\nACGTA\n+\nIII\nII\n@q3\nAC\n+\nII\n")
    put("fq_blank_line.fq", b"@q1\nACGT\n+\nIIII\n\n@q2\nACG\n+\nIII\n")
    return out
