"""BAM fixtures for the reader's BAM input (tests/test_reader_bam_cpu.py on the host reader and the shared record logic,
tests/test_gpu_reader_bam.py on the device).  Python's standard library only: a BAM writer over struct and tests/bgzf_cases.bgzf, and an
independent decoder (gzip.decompress + struct) that yields what a file's reads are: the ids and ordinals `samtools fastq` would print --
records with flag 0x100 / 0x800 skipped, flag 0x10 reverse-complemented, A C G T -> 0 1 2 3, every other code -> 4."""
import gzip
import os
import random
import struct

from tests import bgzf_cases as bc

CODES = "=ACMGRSVTWYHKDBN"
ORD = {1: 0, 2: 1, 4: 2, 8: 3}
TILE_DEFAULT = 65536


# ---- writer
def header(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<I", len(name) + 1) + name + b"\0" + struct.pack("<I", ln)
    return out


def record(name, codes, flag=4, refid=-1, pos=-1, cigar=(), aux=b"", next_refid=-1, next_pos=-1, mapq=0, l_seq=None, block_size=None):
    """codes: the 4-bit base codes; cigar: (length, op) pairs.  l_seq / block_size override the true values (bad files)."""
    n = len(codes)
    packed = bytes((codes[i] << 4) | (codes[i + 1] if i + 1 < n else 0) for i in range(0, n, 2))
    cig = b"".join(struct.pack("<I", (ln << 4) | op) for ln, op in cigar)
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, n if l_seq is None else l_seq, next_refid, next_pos, 0)
    body += name + b"\0" + cig + packed + b"\xff" * n + aux
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def aux_all_types():
    a = b"XAAQ" + b"Xcc" + struct.pack("<b", -5) + b"XCC" + struct.pack("<B", 250) + b"Xss" + struct.pack("<h", -300) + b"XSS" + struct.pack("<H", 60000)
    a += b"Xii" + struct.pack("<i", -70000) + b"XII" + struct.pack("<I", 4000000000) + b"Xff" + struct.pack("<f", 1.5) + b"XZZhello world\0" + b"XHH1AE301\0"
    for t, fmt, vals in ((b"c", "<b", (-1, 2)), (b"C", "<B", (1, 255)), (b"s", "<h", (-2, 3)), (b"S", "<H", (7, 65535)), (b"i", "<i", (-9, 9)), (b"I", "<I", (1, 2)), (b"f", "<f", (0.5, 2.0))):
        a += b"YBB" + t + struct.pack("<I", len(vals)) + b"".join(struct.pack(fmt, v) for v in vals)
    return a


# ---- decoder (independent of the library)
def parse(stream):
    """(header bytes, n_ref, [(offset, flag, name, codes)]) of an uncompressed BAM stream; raises on a record that ends behind the stream"""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<I", stream, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<I", stream, p)[0] + 4
    hdr, recs = p, []
    while p < len(stream):
        bs = struct.unpack_from("<i", stream, p)[0]
        assert p + 4 + bs <= len(stream), "record at %d ends behind the stream" % p
        _, _, lname, _, _, ncig, flag, l_seq = struct.unpack_from("<iiBBHHHi", stream, p + 4)
        name = stream[p + 36:p + 36 + lname - 1]
        s0 = p + 36 + lname + 4 * ncig
        codes = [(stream[s0 + (j >> 1)] >> (0 if j & 1 else 4)) & 15 for j in range(l_seq)]
        recs.append((p, flag, name, codes))
        p += 4 + bs
    return hdr, n_ref, recs


def reads_of(stream):
    """([id], [ordinals as bytes], counts) of the delivered records"""
    _, _, recs = parse(stream)
    ids, seqs, skipped, reverse = [], [], 0, 0
    for _, flag, name, codes in recs:
        if flag & 0x900:
            skipped += 1
            continue
        o = [ORD.get(c, 4) for c in codes]
        if flag & 0x10:
            reverse += 1
            o = [3 - x if x < 4 else x for x in reversed(o)]
        ids.append(name.decode("latin-1"))
        seqs.append(bytes(o))
    return ids, seqs, {"records": len(ids), "skipped": skipped, "reverse": reverse}


def blocks_of(ids, seqs, cap, mr):
    """the blocks lnr_reader_next delivers: [(off list, bases bytes, ids)]; stops at a read that alone exceeds cap (LNR_ERR_LIMIT)"""
    out, k = [], 0
    while k < len(ids):
        if len(seqs[k]) > cap:
            break
        off, used, k0 = [0], 0, k
        while k < len(ids) and k - k0 < mr and used + len(seqs[k]) <= cap:
            used += len(seqs[k])
            off.append(used)
            k += 1
        out.append((off, b"".join(seqs[k0:k]), ids[k0:k]))
    return out


def stream_of(path):
    return gzip.decompress(open(path, "rb").read())


# ---- fixtures
def rnd_records(n=200, seed=7, max_len=3000, flags=(4,)):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = 0 if i % 41 == 17 else rng.randint(0, max_len)
        codes = [rng.randrange(16) for _ in range(L)] if i % 3 else [rng.choice((1, 2, 4, 8)) for _ in range(L)]
        out.append(record(b"m64011_%d/%d/ccs" % (seed, i), codes, flag=rng.choice(flags)))
    return out


def decoy_head():
    """64 bytes that repeat: a complete plausible unmapped record (block_size 60: name "x", 4 bases, 20 bytes behind them)"""
    body = struct.pack("<iiBBHHHiiii", -1, -1, 2, 0, 4680, 0, 4, 4, -1, -1, 0) + b"x\0" + b"\x12\x48" + b"\xff" * 4
    rec = struct.pack("<i", 60) + body + b"\x07" * (64 - 4 - len(body))
    assert len(rec) == 64
    return rec


def streams(tile=TILE_DEFAULT):
    """name -> uncompressed BAM stream of every well-formed fixture (numbers: the issue's list)"""
    rng = random.Random(3)
    hdr = header()
    s = {}
    s["1_rnd200"] = hdr + b"".join(rnd_records())
    names = [b"", b"n" * 254, b"q", b"", b"z" * 254]
    s["2_names"] = hdr + b"".join(record(nm, [rng.randrange(16) for _ in range(10 + 7 * i)]) for i, nm in enumerate(names))
    s["3_aux"] = hdr + b"".join(record(b"aux%d" % i, [rng.randrange(16) for _ in range(33 * i)], aux=aux_all_types()) for i in range(6))
    long_text = b"@HD\tVN:1.6\n" + b"".join(b"@CO\t" + b"c" * 96 + b"\n" for _ in range(700))
    assert len(long_text) > 65536
    s["4_long_header"] = header(long_text) + b"".join(rnd_records(30, seed=8, max_len=400))
    refs = ((b"chr1", 248956422), (b"chr2", 242193529), (b"chrM", 16569))
    s["4_refs"] = header(b"@HD\tVN:1.6\tSO:coordinate\n", refs) + b"".join(
        record(b"r%d" % i, [rng.choice((1, 2, 4, 8, 15)) for _ in range(50 + i)], flag=0 if i % 2 else 4, refid=(i % 3) if i % 2 else -1, pos=1000 * i if i % 2 else -1,
               cigar=((50 + i, 0),) if i % 2 else ()) for i in range(12))
    flags = [0x100, 0, 0x10, 0x800, 0x910, 0x10, 0, 0x110, 0x10, 0x800]
    s["5_aligned"] = header(b"@HD\tVN:1.6\n", refs[:2]) + b"".join(
        record(b"aln%d" % i, [rng.randrange(16) for _ in range(61 + 10 * i)], flag=f, refid=i % 2, pos=77 * i, cigar=((30, 0), (1, 1), (30 + 10 * i, 0)), next_refid=i % 2, next_pos=5,
               aux=b"NMC\x01") for i, f in enumerate(flags))
    s["6_header_only"] = hdr
    s["7_long"] = hdr + record(b"long", [rng.choice((1, 2, 4, 8)) for _ in range(300_000)]) + b"".join(rnd_records(20, seed=9, max_len=200))
    # 8: tile edges, in the coordinates the kernels tile: offsets from the first record (a whole file is one window).  The first
    # record's aux pads the second record's start to the tile boundary and to 1, 2, 3 bytes in front of it (block_size straddles it)
    for d in (0, 1, 2, 3):
        extra = tile - d - len(record(b"pad", [1, 2, 4, 8] * 5, aux=b"XZZ\0"))
        first = record(b"pad", [1, 2, 4, 8] * 5, aux=b"XZZ" + b"p" * extra + b"\0")
        assert len(first) == tile - d
        s["8_edge_minus%d" % d] = hdr + first + b"".join(rnd_records(6, seed=20 + d, max_len=300))
    tail = b"".join(rnd_records(5, seed=30, max_len=300))
    first = record(b"pad", [8, 4, 2, 1] * 4)
    extra = 2 * tile - len(first) - len(tail) - len(record(b"end", [1] * 9, aux=b"XZZ\0"))
    body = first + tail + record(b"end", [1] * 9, aux=b"XZZ" + b"e" * extra + b"\0")
    assert len(body) == 2 * tile
    pay = BGZF_PAYLOAD["8_end_at_tile_end"]
    text = b"@HD\tVN:1.6\n@CO\t" + b"c" * (pay - 12 - 16) + b"\n"      # the header fills one BGZF block: header + body is a multiple of the payload
    assert len(header(text)) == pay and (2 * tile) % pay == 0
    s["8_end_at_tile_end"] = header(text) + body
    # 9: the decoy
    arr = decoy_head() * (3 * tile // 64 + 40)
    s["9_decoy"] = hdr + record(b"before", [2] * 30) + record(b"decoy", [4] * 21, aux=b"XBBC" + struct.pack("<I", len(arr)) + arr) + b"".join(rnd_records(8, seed=40, max_len=500))
    return s


# the header is padded to one whole block of this payload, so the last record ends at a tile end and at the end of a full BGZF block
BGZF_PAYLOAD = {"8_end_at_tile_end": 32768}


def bad_streams():
    """name -> (stream, ordinal of the refused record, its offset, part of the reason)"""
    rng = random.Random(5)
    hdr = header()
    good = [record(b"g%d" % i, [rng.randrange(16) for _ in range(40 + i)], flag=4 if i != 2 else 0x904) for i in range(5)]
    at = len(hdr) + sum(len(g) for g in good)
    codes = [1, 2, 4, 8] * 8
    tail = record(b"after", codes)
    out = {"block_size_8": (hdr + b"".join(good) + record(b"bad", codes, block_size=8) + tail, 5, at, "not a valid record"),
           "negative_l_seq": (hdr + b"".join(good) + record(b"bad", codes, l_seq=-3) + tail, 5, at, "not a valid record"),
           "block_size_small": (hdr + b"".join(good) + record(b"bad", codes, block_size=32 + 4 + 16 + 32 - 1) + tail, 5, at, "not a valid record")}
    whole = hdr + b"".join(good) + record(b"cut", codes * 4)
    out["truncated"] = (whole[:-40], 5, at, "the file ends inside it")
    return out


def write(tmp, tile=TILE_DEFAULT):
    """name -> path of every well-formed fixture, BGZF-wrapped"""
    os.makedirs(tmp, exist_ok=True)
    paths = {}
    for name, st in streams(tile).items():
        p = os.path.join(tmp, name + ".bam")
        with open(p, "wb") as f:
            f.write(bc.bgzf(st, payload=BGZF_PAYLOAD.get(name, 0xff00)))
        paths[name] = p
    return paths


def write_bad(tmp):
    os.makedirs(tmp, exist_ok=True)
    out = {}
    for name, (st, ordinal, off, why) in bad_streams().items():
        p = os.path.join(tmp, "bad_" + name + ".bam")
        with open(p, "wb") as f:
            f.write(bc.bgzf(st))
        out[name] = (p, ordinal, off, why)
    return out


def fastq_of(stream):
    """the delivered reads of an unaligned stream as four-line FASTQ (headers = names)"""
    _, _, recs = parse(stream)
    return b"".join(b"@" + name + b"\n" + "".join(CODES[c] for c in codes).encode() + b"\n+\n" + b"I" * len(codes) + b"\n" for _, flag, name, codes in recs)
