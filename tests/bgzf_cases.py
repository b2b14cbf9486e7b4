"""BGZF fixtures for the device inflate of the reader (tests/test_inflate_hd_cpu.py on the shared decoder, tests/test_gpu_reader_bgzf.py on
the device).  Python's standard library only: a BGZF writer over zlib.compressobj(level, DEFLATED, -15, memLevel, strategy) with the
18-byte header and the 8-byte footer per block, a block walker, the well-formed files and the corrupt blocks."""
import gzip
import os
import random
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def raw_deflate(data, level=-1, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def member(payload, isize, crc, extra_before=b""):
    """one BGZF block around a raw DEFLATE payload; extra_before = other subfields in front of 'BC'"""
    xlen = len(extra_before) + 6
    total = 12 + xlen + len(payload) + 8
    assert total <= 65536, total
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra_before + b"BC" + struct.pack("<HH", 2, total - 1) + payload +
            struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


def block(data, level=-1, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, extra_before=b""):
    return member(raw_deflate(data, level, strategy, mem_level), len(data), zlib.crc32(data), extra_before)


def bgzf(data, payload=0xff00, level=-1, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, eof=True, extra_before=b""):
    out = [block(data[i:i + payload], level, strategy, mem_level, extra_before) for i in range(0, len(data), payload)]
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def walk(raw):
    """[(file offset, payload bytes, isize, crc)] of a chain of BGZF blocks; stops at the first member that is not one"""
    out, o = [], 0
    while o + 18 <= len(raw) and raw[o:o + 4] == b"\x1f\x8b\x08\x04":
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        p, bsize = o + 12, None
        while p + 4 <= o + 12 + xlen:
            sl = struct.unpack_from("<H", raw, p + 2)[0]
            if raw[p:p + 2] == b"BC" and sl == 2:
                bsize = struct.unpack_from("<H", raw, p + 4)[0]
                break
            p += 4 + sl
        if bsize is None or o + bsize + 1 > len(raw):
            break
        end = o + bsize + 1
        crc, isize = struct.unpack_from("<II", raw, end - 8)
        out.append((o, raw[o + 12 + xlen:end - 8], isize, crc))
        o = end
    return out


def first_block_type(payload):
    return (payload[0] >> 1) & 3          # 0 stored, 1 fixed, 2 dynamic


def a_run():
    return b">x\n" + b"A" * 70000


def far_text(seed=5):
    rng = random.Random(seed)
    chunk = bytes(rng.choice(b"ACGT") for _ in range(30000))
    return b">far\n" + chunk + b"\n>far2\n" + chunk + b"\n>far3\n" + chunk[:20000] + b"\n"


def random_fasta(seed=11, n=200):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = rng.randint(1, 3000)
        s = bytes(rng.choice(b"ACGTacgtN") for _ in range(L))
        w = rng.randint(30, 120)
        out.append(b">read%d some text\n" % i + b"\n".join(s[k:k + w] for k in range(0, L, w)) + b"\n")
    return b"".join(out)


def texts(tmp):
    """name -> text of the FASTA / FASTQ inputs (the reader_gpu_cases files are written into tmp and read back)"""
    from tests import reader_gpu_cases as rg
    t = {"rnd200.fa": random_fasta(), "a_run.fa": a_run(), "far.fa": far_text()}
    for fmt in ("fastq", "fastq_multiline"):
        p = os.path.join(tmp, "src." + fmt)
        rg.random_file(p, fmt, n=400 if fmt == "fastq" else 900)       # (the multi-line records begin behind record 700)
        t["rnd." + fmt] = open(p, "rb").read()
    p = os.path.join(tmp, "src.fasta")
    rg.random_file(p, "fasta", n=400)                     # CRLF every fifth record, blanks inside lines
    t["crlf.fasta"] = open(p, "rb").read()
    return t


HANDOVER = ("rnd.fastq_multiline.gz", "plain_member.fa.gz", "plain_control.fa.gz")


def write_files(tmp):
    """name -> path of every well-formed file.  All are BGZF from the first to the last member except the three of HANDOVER."""
    os.makedirs(tmp, exist_ok=True)
    t = texts(tmp)
    fa, fq = t["rnd200.fa"], t["rnd.fastq"]
    small = fa[:3000]
    files = {name + ".gz": bgzf(text) for name, text in t.items()}
    for pay in (1, 7):
        files["pay%d.fa.gz" % pay] = bgzf(small[:700], payload=pay)
    files["pay4096.fq.gz"] = bgzf(fq, payload=4096)
    files["pay65280.fa.gz"] = bgzf(fa, payload=0xff00)
    files["pay65536.fa.gz"] = bgzf(a_run() + b"\n" + a_run().replace(b">x", b">y"), payload=65536)
    files["stored.fa.gz"] = bgzf(fa, payload=65536 - 26 - 10, level=0)         # the largest stored payload that fits BSIZE (zlib ends with an empty stored block)
    files["fixed.fq.gz"] = bgzf(fq, payload=20000, strategy=zlib.Z_FIXED)
    files["mem1.fa.gz"] = bgzf(fa, payload=0xff00, mem_level=1)                # several DEFLATE blocks per BGZF block
    files["level1.fa.gz"] = bgzf(fa, payload=30000, level=1)
    files["level9.fq.gz"] = bgzf(fq, payload=0xff00, level=9)
    blocks = [block(fa[i:i + 5000]) for i in range(0, 40000, 5000)]
    files["empty_mid_eof.fa.gz"] = b"".join(blocks[:3]) + EOF_BLOCK + block(b"") + b"".join(blocks[3:]) + EOF_BLOCK
    files["empty_end_noeof.fa.gz"] = b"".join(blocks) + block(b"") + block(b"")
    files["no_eof.fa.gz"] = bgzf(fa[:50000], payload=9000, eof=False)
    files["extra_subfield.fa.gz"] = bgzf(fa[:60000], payload=10000, extra_before=b"XY" + struct.pack("<H", 3) + b"abc")
    files["plain_member.fa.gz"] = b"".join(blocks[:2]) + gzip.compress(fa[10000:25000]) + b"".join(blocks[5:])
    files["plain_control.fa.gz"] = gzip.compress(fa[:40000])
    paths = {}
    for name, raw in files.items():
        p = os.path.join(tmp, name)
        with open(p, "wb") as f:
            f.write(raw)
        paths[name] = p
    return paths


# ---- corrupt blocks: (name, payload, isize, crc, text the block would hold or None)
def _bits(pairs):
    """LSB-first bit writer: [(value, nbits)] -> bytes"""
    acc, n = 0, 0
    for v, k in pairs:
        acc |= (v & ((1 << k) - 1)) << n
        n += k
    return acc.to_bytes((n + 7) // 8, "little")


def _dynamic_header(cl_lens):
    """BFINAL=1, BTYPE=2, HLIT=0 (257), HDIST=0 (1), HCLEN=15 (19) and the 19 code-length code lengths in RFC order"""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    return [(1, 1), (2, 2), (0, 5), (0, 5), (15, 4)] + [(cl_lens.get(s, 0), 3) for s in order]


def corrupt_blocks():
    text = random_fasta(seed=3, n=12)[:20000]
    good = raw_deflate(text)
    crc = zlib.crc32(text)
    out = [("crc_flipped", good, len(text), crc ^ 0x10, None),
           ("isize_plus_1", good, len(text) + 1, crc, None),
           ("isize_minus_1", good, len(text) - 1, crc, None),
           ("cut_short", good[: len(good) - 40], len(text), crc, None),
           ("block_type_3", _bits([(1, 1), (3, 2), (0, 5)]) + b"\0" * 8, 10, 0, None),
           ("stored_len_nlen", b"\x01\x05\x00\xfa\xfe" + b"ACGTA", 5, zlib.crc32(b"ACGTA"), None),
           # three code-length codes of length 1: over-subscribed; one of length 2 and nothing else: incomplete
           ("oversubscribed", _bits(_dynamic_header({0: 1, 1: 1, 2: 1})) + b"\0" * 8, 10, 0, None),
           ("incomplete", _bits(_dynamic_header({0: 2})) + b"\0" * 8, 10, 0, None),
           # fixed block: literal 'A' (0x41 + 0x30 = 8-bit code 0x71, sent MSB first), then length 3 (symbol 257: 7-bit code 1), distance
           # symbol 1 (distance 2): one byte before the start of the text
           ("distance_before_start", _bits([(1, 1), (1, 2), (int("{:08b}".format(0x71)[::-1], 2), 8), (int("{:07b}".format(1)[::-1], 2), 7),
                                            (int("{:05b}".format(1)[::-1], 2), 5), (0, 7)]) + b"\0" * 4, 4, 0, None)]
    return out


def bit_flips(n=200, seed=99):
    """(name, payload, isize, crc, text): a dynamic block with one bit flipped at each of n seeded positions"""
    text = random_fasta(seed=4, n=8)[:12000]
    good = raw_deflate(text)
    assert first_block_type(good) == 2
    rng = random.Random(seed)
    out = []
    for k in range(n):
        pos = rng.randrange(8 * len(good))
        bad = bytearray(good)
        bad[pos >> 3] ^= 1 << (pos & 7)
        out.append(("flip_%d" % pos, bytes(bad), len(text), zlib.crc32(text), text))
    return out


def zlib_inflate(payload, isize):
    """the bytes zlib gives for a raw DEFLATE payload, or None when it reports an error or the stream does not end"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload, isize + 1024)
    except zlib.error:
        return None
    return out if d.eof else None


def corrupt_files(tmp):
    """name -> (path, file offset of the bad block): two good blocks, the corrupt one, one good block, the EOF marker"""
    os.makedirs(tmp, exist_ok=True)
    fa = random_fasta(seed=21, n=40)
    head = block(fa[:30000]) + block(fa[30000:52000])
    out = {}
    for name, payload, isize, crc, _ in corrupt_blocks():
        p = os.path.join(tmp, "bad_" + name + ".fa.gz")
        with open(p, "wb") as f:
            f.write(head + member(payload, isize, crc) + block(fa[52000:60000]) + EOF_BLOCK)
        out[name] = (p, len(head))
    return out
