"""Plain gzip fixtures for the parallel inflate (tests/test_gunzip_hd_cpu.py on the shared logic, tests/test_gpu_reader_gzip.py on the
device).  Generated from seeds with Python's zlib / gzip only; the yardstick is zlib's own inflate, never the code under test."""
import functools
import gzip
import os
import random
import struct
import tempfile
import zlib

import numpy as np

from tests import bgzf_cases as bc

CHUNKS = (1024, 4096, 32768, 131072)


def gz(data, level=-1, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None, every=10000):
    """one gzip member; flush: zlib.Z_SYNC_FLUSH / Z_FULL_FLUSH after every `every` bytes (the empty stored blocks pigz leaves)"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem_level, strategy)
    if flush is None:
        return c.compress(data) + c.flush()
    out = []
    for i in range(0, len(data), every):
        out.append(c.compress(data[i:i + every]))
        out.append(c.flush(flush))
    return b"".join(out) + c.flush()


def fastq(n_bytes, seed=1):
    """four-line FASTQ of reads up to 10 kb"""
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        L = int(rng.integers(200, 10000))
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes()
        q = rng.integers(33, 74, L, dtype=np.uint8).tobytes()
        rec = b"@read%d len=%d\n" % (i, L) + s + b"\n+\n" + q + b"\n"
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)


def fasta(n_bytes, seed=2):
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        L = int(rng.integers(200, 10000))
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes()
        rec = b">read%d len=%d\n" % (i, L) + b"\n".join(s[k:k + 70] for k in range(0, L, 70)) + b"\n"
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)


def with_header(member, extra=b"XY\x03\x00abc", name=b"reads.fq", comment=b"made by a test"):
    """the member with FEXTRA + FNAME + FCOMMENT + FHCRC in its header"""
    assert member[:3] == b"\x1f\x8b\x08" and member[3] == 0
    head = b"\x1f\x8b\x08" + bytes([4 | 8 | 16 | 2]) + member[4:10] + struct.pack("<H", len(extra)) + extra + name + b"\0" + comment + b"\0"
    return head + struct.pack("<H", zlib.crc32(head) & 0xffff) + member[10:]


def _reader_texts():
    from tests import reader_gpu_cases as rg
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for fmt, n in (("fasta", 400), ("fastq_multiline", 900)):
            p = os.path.join(d, "src." + fmt)
            rg.random_file(p, fmt, n=n)
            out[fmt] = open(p, "rb").read()
    return out


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> (gzip bytes, text).  Every file inflates to its text with gzip.decompress."""
    fq, fa = fastq(3_000_000), fasta(2_500_000)
    fq2, fq1 = fastq(2_000_000), fastq(1_200_000)         # the same records from the start: texts that end with a whole record
    assert fq.startswith(fq2) and fq2.startswith(fq1)
    f = {}
    for lv in (1, 6, 9):
        f["fq_l%d.fq.gz" % lv] = (gz(fq, lv), fq)
        f["fa_l%d.fa.gz" % lv] = (gz(fa, lv), fa)
    f["fq_m4.fq.gz"] = (gz(fq, 6, 4), fq)
    f["fq_m1.fq.gz"] = (gz(fq2, 6, 1), fq2)
    f["fq_fixed.fq.gz"] = (gz(fq2, 6, 8, zlib.Z_FIXED), fq2)
    f["fq_huffman.fq.gz"] = (gz(fq, 6, 8, zlib.Z_HUFFMAN_ONLY), fq)
    f["fq_rle.fq.gz"] = (gz(fq, 6, 8, zlib.Z_RLE), fq)
    f["fq_l0.fq.gz"] = (gz(fq, 0), fq)
    f["fq_sync.fq.gz"] = (gz(fq2, 6, 8, flush=zlib.Z_SYNC_FLUSH), fq2)
    f["fq_full.fq.gz"] = (gz(fq2, 6, 8, flush=zlib.Z_FULL_FLUSH), fq2)
    a = bc.a_run() * (3_000_000 // len(bc.a_run()) + 1)
    f["a_run.fa.gz"] = (gz(a), a)
    far = bc.far_text() * (2_000_000 // len(bc.far_text()) + 1)
    f["far.fa.gz"] = (gz(far), far)
    for n in (0, 1, 30000):
        f["len%d.fa.gz" % n] = (gz(fa[:n]), fa[:n])
    parts = (fq1, b"", fq2[len(fq1):])
    f["two_members.fq.gz"] = (gz(parts[0]) + gz(parts[2], 9), parts[0] + parts[2])
    f["three_members.fq.gz"] = (gz(parts[0]) + gz(parts[1]) + gz(parts[2], 1), parts[0] + parts[2])
    f["header_fields.fq.gz"] = (with_header(gz(fq2)), fq2)
    rt = _reader_texts()
    f["crlf.fa.gz"] = (gz(rt["fasta"]), rt["fasta"])
    f["multiline.fq.gz"] = (gz(rt["fastq_multiline"]), rt["fastq_multiline"])
    return f


@functools.lru_cache(maxsize=None)
def false_candidate_files():
    """arbitrary bytes, for the inflate alone: (a) a level-0 gzip of the bytes of a level-6 gzip of FASTQ -- stored blocks only, every
    candidate lies inside a payload; (b) a level-6 gzip of text + those compressed bytes + text -- zlib stores the middle, the chain must
    pass the false candidates and land on a true one behind them"""
    fq = fastq(3_000_000)
    inner = gz(fq, 6)
    a = inner
    b = fq[:700_000] + inner + fq[700_000:1_400_000]
    return {"false_a.gz": (gz(a, 0), a), "false_b.gz": (gz(b, 6), b)}


@functools.lru_cache(maxsize=None)
def small_files():
    """texts of half a megabyte, for the runs in rounds of 8 KiB (sixty rounds each, not hundreds)"""
    fq, far = fastq(500_000), (bc.far_text() * 7)[:500_000]
    a = fastq(200_000)
    return {"small_l6.fq.gz": (gz(fq, 6), fq), "small_m1.fq.gz": (gz(fq, 6, 1), fq), "small_far.fa.gz": (gz(far), far),
            "small_three.fq.gz": (gz(a) + gz(b"") + gz(fq[len(a):], 1), fq)}


def cut_behind_header_files():
    """name -> (gzip bytes, text in front of the failure, compressed offset the error names): files that end directly behind a member's
    header -- what a killed gzip leaves -- alone and behind a whole member.  zlib reports an unexpected end of file on each."""
    bare = b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03"
    named = b"\x1f\x8b\x08\x08\0\0\0\0\x00\x03reads.fq\0"
    text = fastq(120_000)
    m = gz(text)
    return {"header_only.gz": (bare, b"", 10), "header_name_only.gz": (named, b"", len(named)),
            "member_then_header.fq.gz": (m + bare, text, len(m) + 10), "member_then_named_header.fq.gz": (m + named, text, len(m) + len(named))}


def host_driver():
    """the host driver of linear_amd/csrc/lnr_gunzip_hd.h, compiled by g++ from tests/gunzip_hd_shim.cpp:
    run(raw, cap, chunk, round) -> (status, text, stats, bad offset); the guard bytes around the output array are checked; run.lib = the library"""
    import ctypes as C
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    build = os.path.join(here, "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "libgunzip_hd_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, os.path.join(here, "gunzip_hd_shim.cpp"), "-lz"])
    lib = C.CDLL(so)
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    lib.gz_gunzip.argtypes = [C.c_char_p, C.c_ulonglong, u8p, C.c_ulonglong, u64p, C.c_ulonglong, C.c_ulonglong, u64p, u64p]
    lib.gz_gunzip.restype = C.c_uint
    guard = 64

    def run(raw, cap, chunk, rnd=1 << 26):
        buf = np.full(cap + 2 * guard, 0xA5, np.uint8)
        n, bad = C.c_uint64(), C.c_uint64()
        st = np.zeros(len(HOST_STATS), np.uint64)
        s = lib.gz_gunzip(raw, len(raw), buf[guard:].ctypes.data_as(u8p), cap, C.byref(n), chunk, rnd, st.ctypes.data_as(u64p), C.byref(bad))
        assert (buf[:guard] == 0xA5).all() and (buf[guard + cap:] == 0xA5).all(), "wrote outside the output array"
        assert n.value <= cap
        return s, buf[guard:guard + n.value].tobytes(), dict(zip(HOST_STATS, (int(x) for x in st))), bad.value
    run.lib = lib
    return run


HOST_STATS = ("rounds", "members", "chunks", "candidates", "pieces", "falses", "blocks", "comp_bytes", "text_bytes", "win_syms", "grown")


def flips_clean_on_host(step=1):
    """every step-th flip of bit_flips() that the host driver has just taken without a fault and with zlib's verdict (an error where zlib
    raises, zlib's text where it does not): the flips a GPU test may run.  [(name, gzip bytes, zlib's text or None)]"""
    run = host_driver()
    out = []
    for name, raw, text in bit_flips()[::step]:
        want = zlib_text(raw)
        s, got, _, _ = run(raw, len(text) + 70000, 4096)
        if (s != 0) if want is None else (s == 0 and got == want):
            out.append((name, raw, want))
    return out


def all_files():
    out = dict(fixtures())
    out.update(false_candidate_files())
    return out


def bit_flips(n=200, seed=123):
    """(name, gzip bytes, text): a level-6 FASTQ of 300 000 bytes of text with one bit of its DEFLATE data flipped"""
    text = fastq(300_000)
    good = gz(text, 6)
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        pos = rng.randrange(80, 8 * (len(good) - 8))
        bad = bytearray(good)
        bad[pos >> 3] ^= 1 << (pos & 7)
        out.append(("flip_%d" % pos, bytes(bad), text))
    return out


def zlib_text(raw):
    """the text gzread would deliver in full, or None where zlib reports an error or the stream does not end"""
    try:
        return gzip.decompress(raw)
    except (OSError, EOFError, zlib.error):
        return None
