"""CPU: the per-block logic of the writer's device deflate (linear_amd/csrc/lnr_deflate_hd.h), compiled for the host by
tests/deflate_hd_shim.cpp.  Every text of tests/deflate_cases.py: the members parse as BGZF, each inflates on its own with zlib and with
lnr_inf::inflate_block (tests/inflate_hd_shim.cpp in a library of this test's own) to its slice of the text, CRC32 and ISIZE are right,
gzip reads the whole, nothing is written outside the slot, no member exceeds isize + 31 bytes.  Bounds that follow from the format: random
bytes are stored; random DNA takes under half (a 2-bit code is a quarter, fixed Huffman cannot go below 1); a run of one byte takes under
1/20 (Huffman alone cannot go below 1/8).  The bytes depend on the block's text alone.  The same through a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import bgzf_cases as bc, deflate_cases as dc, writer_cases as wc

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "deflate_hd_shim.cpp")
GUARD = 64
BLOCK = dc.BLOCK
_u8p, _u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def shim():
    os.makedirs(BUILD, exist_ok=True)
    so, inf_so = os.path.join(BUILD, "libdeflate_hd_shim.so"), os.path.join(BUILD, "libdeflate_test_inflate.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, SRC])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", inf_so, os.path.join(HERE, "inflate_hd_shim.cpp")])
    lib, inf = C.CDLL(so), C.CDLL(inf_so)
    lib.def_member.argtypes = [C.c_char_p, C.c_uint, _u8p, _u32p]
    lib.def_member.restype = lib.def_slot_bytes.restype = C.c_uint
    lib.def_slot_bytes.argtypes = [C.c_uint]
    inf.inf_block.argtypes = [C.c_char_p, C.c_uint, _u8p, C.c_uint, C.c_uint, _u32p, _u32p]
    inf.inf_block.restype = C.c_uint

    def member(block):
        """(member bytes, stored) of one block; the guard bytes around its slot are checked here"""
        slot = lib.def_slot_bytes(len(block))
        buf = np.full(slot + 2 * GUARD, 0xA5, np.uint8)
        st = C.c_uint32()
        m = lib.def_member(block, len(block), buf[GUARD:].ctypes.data_as(_u8p), C.byref(st))
        assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + slot:] == 0xA5).all(), "wrote outside the slot"
        assert 26 <= m <= slot
        return buf[GUARD:GUARD + m].tobytes(), st.value

    def compress(text):
        """([(member, stored)] per block, the members back to back)"""
        ms = [member(text[o:o + BLOCK]) for o in range(0, len(text), BLOCK)]
        return ms, b"".join(m for m, _ in ms)

    def own_inflate(payload, isize, crc):
        out = np.zeros(isize + 1, np.uint8)
        got, blocks = C.c_uint32(), C.c_uint32()
        st = inf.inf_block(payload, len(payload), out.ctypes.data_as(_u8p), isize, crc, C.byref(got), C.byref(blocks))
        return st, out[:isize].tobytes()
    compress.own_inflate = own_inflate
    return compress


@pytest.fixture(scope="module")
def all_texts():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    w = Writer(wc.GIDS, wc.GLEN)
    sam = w.format(*wc.synthetic(), "sam")
    apf = w.format(*wc.synthetic(), "apf")
    w.close()
    assert len(sam) > 10_000 and len(apf) > BLOCK
    t = dc.texts(sam)
    t["apf"] = apf
    return t


def test_every_text(shim, all_texts):
    for name, text in all_texts.items():
        ms, raw = shim(text)
        assert len(ms) == (len(text) + BLOCK - 1) // BLOCK, name
        walked = bc.walk(raw)
        assert len(walked) == len(ms) and sum(len(m) for m, _ in ms) == len(raw), name
        for k, ((off, payload, isize, crc), (m, stored)) in enumerate(zip(walked, ms)):
            want = text[k * BLOCK:(k + 1) * BLOCK]
            d = zlib.decompressobj(-15)
            assert d.decompress(payload) == want and d.eof and d.unused_data == b"", (name, k)
            assert isize == len(want) and crc == zlib.crc32(want), (name, k)
            st, got = shim.own_inflate(payload, isize, crc)
            assert st == 0 and got == want, (name, k, st)
            assert len(m) <= isize + 31 and len(m) <= 65536, (name, k)
            assert bc.first_block_type(payload) == (0 if stored else 2), (name, k)
            if stored:
                assert len(m) == isize + 31, (name, k)
        assert gzip.decompress(raw + bc.EOF_BLOCK) == text, name
    assert shim(b"")[1] == b""


def test_derived_bounds(shim, all_texts):
    ms, _ = shim(all_texts["random_bytes"])
    assert [(len(m), st) for m, st in ms[:2]] == [(BLOCK + 31, 1)] * 2            # every full block of random bytes is stored
    (m, st), = shim(all_texts["dna"])[0]
    assert st == 0 and len(m) < BLOCK // 2
    ms, _ = shim(all_texts["a_run"])
    for k, (m, st) in enumerate(ms):
        assert st == 0 and len(m) * 20 < len(all_texts["a_run"][k * BLOCK:(k + 1) * BLOCK]), k
    for k in ("sam", "apf"):
        ms, raw = shim(all_texts[k])
        assert not any(st for _, st in ms) and len(raw) * 3 < len(all_texts[k])
    # a repeat at the largest distance is found, one byte further it is not: the first is the smaller member
    a, b = shim(all_texts["dist_32768"])[1], shim(all_texts["dist_32769"])[1]
    assert len(a) + 100 < len(b)


def test_bytes_depend_on_the_text_alone(shim, all_texts):
    text = all_texts["random_fasta"]
    assert len(text) > 2 * BLOCK
    assert shim(text)[1] == shim(text)[1]
    # the slice that is block 0 of one text and block 2 of another: the same member
    piece = text[BLOCK:2 * BLOCK]
    first = shim(piece + all_texts["random_fasta"])[0][0][0]
    third = shim((all_texts["a_run"] * 2)[:2 * BLOCK] + piece)[0][2][0]
    assert first == third == shim(piece)[0][0][0]
    # after other work in the same thread (the work space is reused)
    shim(all_texts["random_bytes"])
    assert shim(piece)[0][0][0] == first


def test_stand_alone_under_sanitizers(shim, all_texts, tmp_path):
    """host code with its own main: address + undefined-behaviour sanitizers over every text, block by block into arrays of exact size;
    the program inflates every member again and its bytes (by hash and size) are those of the library"""
    import struct
    exe = os.path.join(BUILD, "deflate_hd_shim_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DDEF_MAIN", "-o", exe, SRC])
    names = sorted(all_texts)
    p = tmp_path / "texts.bin"
    with open(p, "wb") as f:
        for n in names:
            f.write(struct.pack("<I", len(all_texts[n])) + all_texts[n])
    r = subprocess.run([exe, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(names)

    def fnv(b):
        h = 1469598103934665603
        for x in np.frombuffer(b, np.uint8).tolist():
            h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return h
    for n, line in zip(names, lines):
        members, nbytes, stored, h, status = (int(x) for x in line.split())
        ms, raw = shim(all_texts[n])
        assert status == 0 and members == len(ms) and nbytes == len(raw) and stored == sum(st for _, st in ms), (n, line)
        if len(raw) < 100_000:
            assert h == fnv(raw), n
