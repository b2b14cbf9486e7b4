"""Shared by the tests of the BAM writer (tests/test_output_bam_cpu.py on the host, tests/test_gpu_writer_bam.py on the device).

bam_of_sam is the independent expectation everywhere: the re-encoding rule of a SAM line as a BAM record, written down from the rule alone
(little endian; block_size; refID = index of RNAME among the @SQ names, -1 for '*'; pos = POS - 1; l_read_name; mapq 255; bin =
reg2bin(pos, pos + reference bases of the CIGAR); n_cigar_op; flag; l_seq; next_refID -1; next_pos -1; tlen 0; QNAME NUL; count << 4 | op
with MIDNSHP=X = 0..8; SEQ two bases per byte, high nibble first, =ACMGRSVTWYHKDBN = 0..15; l_seq bytes 0xff; 'S' 'A' 'Z' text NUL for
SA:Z:).  The shapes: writer_cases' batches without SEQ, and seq() -- writer_seq_cases-style cords and reads at the SEQ lengths at which
two bases per byte and the kernels' 4-byte words and LDS window can go wrong."""
import re
import struct

import numpy as np

from tests import writer_cases as wc, writer_seq_cases as sc

GIDS, GLEN, genome = sc.GIDS, sc.GLEN, sc.genome
OUT_WIN = sc.OUT_WIN
SEQ_LENS = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 2 * OUT_WIN - 1, 2 * OUT_WIN, 2 * OUT_WIN + 1, 200_000]      # 2 * OUT_WIN bases = OUT_WIN packed bytes
_NIB = np.zeros(256, np.uint8)
_NIB[list(b"=ACMGRSVTWYHKDBN")] = np.arange(16, dtype=np.uint8)


def reg2bin(beg, end):
    end = (end - 1) & 0xffffffff
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def bam_of_sam(sam_text: bytes, genome_ids) -> bytes:
    names = [g.encode() if isinstance(g, str) else g for g in genome_ids]
    out = []
    for line in sam_text.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        qname, flag, rname, pos, seq = f[0], int(f[1]), f[2], int(f[3]) - 1, f[9]
        ops = [(int(n), op) for n, op in re.findall(rb"(\d+)([MIDNSHP=X])", f[5])]
        reflen = sum(n for n, op in ops if op in b"=XDMN")
        l_seq = 0 if seq == b"*" else len(seq)
        nib = _NIB[np.frombuffer(seq, np.uint8)] if l_seq else np.zeros(0, np.uint8)
        if l_seq & 1:
            nib = np.concatenate([nib, np.zeros(1, np.uint8)])
        packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
        tag = b"".join(b"SAZ" + t[5:] + b"\0" for t in f[11:] if t.startswith(b"SA:Z:"))
        body = struct.pack("<iiBBHHHiiii", names.index(rname) if rname in names else -1, pos, (len(qname) + 1) & 0xff, 255, reg2bin(pos, (pos + reflen) & 0xffffffff) & 0xffff,
                           len(ops) & 0xffff, flag, l_seq, -1, -1, 0)
        body += qname + b"\0" + b"".join(struct.pack("<I", (n << 4 | b"MIDNSHP=X".index(op)) & 0xffffffff) for n, op in ops) + packed + b"\xff" * l_seq + tag
        out.append(struct.pack("<i", len(body)) + body)
    return b"".join(out)


def walk_records(raw: bytes):
    """the records of a stream as dicts; raises where a block_size does not fit its record or the stream"""
    recs, p = [], 0
    while p < len(raw):
        bs, = struct.unpack_from("<i", raw, p)
        assert bs >= 32 and p + 4 + bs <= len(raw), (p, bs, len(raw))
        ref, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", raw, p + 4)
        q = p + 36
        end = q + l_name - 1
        while raw[end] != 0:                       # l_read_name holds the low 8 bits of a longer name's length
            end += 256
        name = raw[q:end]
        q = end + 1
        cigar = [(w >> 4, "MIDNSHP=X"[w & 15]) for w in struct.unpack_from(f"<{n_cig}I", raw, q)]
        q += 4 * n_cig
        seq, qual = raw[q:q + (l_seq + 1) // 2], raw[q + (l_seq + 1) // 2:q + (l_seq + 1) // 2 + l_seq]
        q += (l_seq + 1) // 2 + l_seq
        assert q <= p + 4 + bs
        recs.append(dict(ref=ref, pos=pos, mapq=mapq, bin=bin_, flag=flag, l_seq=l_seq, next=(nref, npos, tlen), name=name, cigar=cigar, seq=seq, qual=qual, tags=raw[q:p + 4 + bs]))
        p += 4 + bs
    return recs


def split_bam(raw: bytes):
    """an inflated .bam -> (header text, [(name, length)], record stream)"""
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        name = raw[p + 4:p + 4 + l_name]
        assert name.endswith(b"\0")
        refs.append((name[:-1], struct.unpack_from("<i", raw, p + 4 + l_name)[0]))
        p += 8 + l_name
    return raw[8:8 + l_text], refs, raw[p:]


many_records = wc.many_records


def build_seq():
    """(cord_off, cords_str, cords_end, reads, read_off, ids): writer_seq_cases.build() at SEQ_LENS, QNAMEs of 1 .. 5 bytes (with the 36
    bytes before it a record's CIGAR, SEQ and tag start at every address mod 4), both strands, N, positions outside the genome, a record
    without CIGAR, reads without cords, 66 records in a read, 3 000 cords in a record (the segment table refills more than 20 times)"""
    B = wc.Batch()
    plant = {}
    B.read([(500, 0, 0, 0, False, 0)], L=0, rid="empty")         # no CIGAR element, no SEQ
    k = 0
    for L in SEQ_LENS:
        for strand in (0, 1):
            cord = (300 + L % 1000, 0, strand, 0, False, 0) if L <= 3 else (300 + L % 1000, 1, strand, 0, False, min(L // 2, 96))
            B.read([cord], L=L, rid="abcde"[:1 + k % 5])
            k += 1
    for q in range(5):
        B.read([(700, 2, q & 1, 2, False, 40)], L=66 + q, rid="vwxyz"[:q + 1])     # even and odd L, both strands, the third sequence
    B.read([(1000, 10, 0, 0, False, 96), (1050, 40, 0, 0, False, 96)])           # =30 D20
    B.read([(1000, 10, 1, 0, False, 96), (1030, 60, 1, 0, False, 96)])           # =30 I20, reverse
    for strand in (0, 1):
        B.read(sc.x_pair(strand))                               # X over random bases
        plant[len(B.rl)] = (106, 2096, 100)
        B.read(sc.x_pair(strand))                               # X where the read IS the genome: N
    B.read(sc.x_pair(0, x=69_900, y=20))                        # runs past the end of the first sequence
    B.read([(4, 3, 0, 1, False, 9)])                            # past the end of the 9-base sequence
    B.read(many_records(), rid="m")
    B.read([], dummy=False)                                     # a read without cords between reads with records
    B.read(many_records(65), rid="mm")
    coff, cs, ce, rl, ids = B.arrays()
    s_off, s_cs, s_ce, s_rl, s_ids = wc.synthetic()
    coff = np.concatenate([coff, s_off[1:] + coff[-1]])
    cs, ce, rl, ids = np.concatenate([cs, s_cs]), np.concatenate([ce, s_ce]), np.concatenate([rl, s_rl]), ids + s_ids
    rng = np.random.default_rng(11)
    off = np.zeros(rl.size + 1, np.uint64)
    off[1:] = np.cumsum(rl)
    reads = rng.integers(0, 4, int(off[-1])).astype(np.uint8)
    g = genome()
    for i in range(rl.size):
        a, L = int(off[i]), int(rl[i])
        if L >= 20:
            reads[a + L // 3:a + L // 3 + 5] = 4                # a run of N
        if L >= 10 and i % 5 == 0:
            reads[a + 7], reads[a + L - 2] = 9, 200             # no Dna5 ordinals: N
        if i in plant:
            y, x, n = plant[i]
            fwd = g[0][x:x + n]
            if (int(cs[int(coff[i]) + 1]) >> 61) & 1:
                reads[a + L - y - n:a + L - y] = sc.revcomp(fwd)
            else:
                reads[a + y:a + y + n] = fwd
    return coff, cs, ce, reads, off, ids


_cache = {}


def seq():
    if "s" not in _cache:
        _cache["s"] = build_seq()
    return _cache["s"]


def seq_batches():
    return [("seq", seq()), ("one_read", sc.one_read()), ("empty", sc.empty())]


def plain_batches():
    """(name, (cord_off, cords_str, cords_end, read_len, ids)) without SEQ; the many-record reads ride along with writer_cases' shapes"""
    coff, cs, ce, reads, off, ids = seq()
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    return [("synthetic", wc.synthetic()), ("one_read", wc.one_read()), ("empty", wc.empty()), ("seq_shapes", (coff, cs, ce, rl, ids))] + \
           [(f"{name}_dup{dup}", wc.gap_set(name, dup)) for name, dup in wc.GAP_SETS]
