"""CPU: the decode logic of the reader's device inflate (linear_amd/csrc/lnr_inflate_hd.h), compiled for the host by
tests/inflate_hd_shim.cpp: every block of every fixture of tests/bgzf_cases.py against Python's zlib, with the CRC32 combined from 64
slices as the kernel does; every corrupt case returns its status and writes nothing outside the output array (guard bytes); the fixture
maker itself (block types per zlib setting); and the same cases through a stand-alone program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import bgzf_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "inflate_hd_shim.cpp")
GUARD = 64
_u8p, _u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
# the statuses of lnr_inf::Status
OK, E_INPUT_END, E_BLOCK_TYPE, E_STORED_LEN, E_OVERSUBSCRIBED, E_INCOMPLETE, E_DISTANCE, E_OUTPUT, E_ISIZE, E_CRC = 0, 1, 2, 3, 5, 6, 10, 11, 12, 13
WANT = {"crc_flipped": E_CRC, "isize_plus_1": E_ISIZE, "isize_minus_1": E_OUTPUT, "cut_short": E_INPUT_END, "block_type_3": E_BLOCK_TYPE,
        "stored_len_nlen": E_STORED_LEN, "oversubscribed": E_OVERSUBSCRIBED, "incomplete": E_INCOMPLETE, "distance_before_start": E_DISTANCE}


@pytest.fixture(scope="module")
def shim():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libinflate_hd_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.inf_block.argtypes = [C.c_char_p, C.c_uint, _u8p, C.c_uint, C.c_uint, _u32p, _u32p]
    lib.inf_block.restype = C.c_uint
    lib.inf_member.argtypes = [C.c_char_p, C.c_ulonglong, _u32p]
    lib.inf_member.restype = C.c_uint

    def run(payload, isize, crc):
        """(status, text, DEFLATE blocks); the guard bytes around the output array are checked here"""
        buf = np.full(isize + 2 * GUARD, 0xA5, np.uint8)
        got, blocks = C.c_uint32(), C.c_uint32()
        st = lib.inf_block(payload, len(payload), buf[GUARD:].ctypes.data_as(_u8p), isize, crc, C.byref(got), C.byref(blocks))
        assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + isize:] == 0xA5).all(), "wrote outside the output array"
        return st, buf[GUARD:GUARD + isize].tobytes(), blocks.value
    run.lib = lib
    return run


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return bc.write_files(str(tmp_path_factory.mktemp("bgzf")))


def test_fixture_maker():
    text = bc.random_fasta()[:50000]
    for kw, typ in ((dict(level=0), 0), (dict(strategy=zlib.Z_FIXED), 1), (dict(), 2), (dict(mem_level=1), 2)):
        raw = bc.bgzf(text, payload=20000, **kw)
        blocks = bc.walk(raw)
        assert len(blocks) == 4 and blocks[-1][2] == 0 and bc.first_block_type(blocks[0][1]) == typ, kw      # three + the EOF marker
        assert gzip.decompress(raw) == text
    raw = bc.bgzf(text[:70], payload=7)
    assert gzip.decompress(raw) == text[:70] and len(bc.walk(raw)) == 11
    assert gzip.decompress(bc.bgzf(text, eof=False)) == text
    # the A run: 70 000 bytes in two blocks of under 200 bytes -- length-258 matches at distance 1
    raw = bc.bgzf(bc.a_run(), payload=65536)
    blocks = bc.walk(raw)
    assert gzip.decompress(raw) == bc.a_run() and blocks[0][2] == 65536 and len(blocks[0][1]) < 65536 // 258 + 64
    extra = bc.bgzf(text, payload=9000, extra_before=b"XY\x03\x00abc")
    assert gzip.decompress(extra) == text and len(bc.walk(extra)) == 7


def test_every_block_of_every_fixture(shim, files):
    types, multi, far, run258 = set(), 0, 0, 0
    for name, path in files.items():
        raw = open(path, "rb").read()
        text = gzip.decompress(raw)
        blocks = bc.walk(raw)
        if name not in bc.HANDOVER or name == "rnd.fastq_multiline.gz":
            assert sum(b[2] for b in blocks) == len(text) and sum(len(b[1]) + 26 for b in blocks) <= len(raw), name
        pos = 0
        for off, payload, isize, crc in blocks:
            want = zlib.decompressobj(-15).decompress(payload)
            st, got, nb = shim(payload, isize, crc)
            assert st == OK and got == want and zlib.crc32(got) == crc and len(want) == isize, (name, off, st)
            types.add(bc.first_block_type(payload))
            multi += nb > 1
            dof = C.c_uint32()
            assert shim.lib.inf_member(raw[off:], len(raw) - off, C.byref(dof)) == 26 + len(payload) + (dof.value - 18) and raw[off + dof.value: off + dof.value + len(payload)] == payload
            pos += isize
    assert types == {0, 1, 2} and multi > 0
    # what is not a BGZF member: a plain gzip member, a cut header, a BSIZE too small, a chain past the end of the file
    dof = C.c_uint32()
    good = bc.block(b"ACGT")
    assert shim.lib.inf_member(good, len(good), C.byref(dof)) == len(good) and dof.value == 18
    for bad in (gzip.compress(b"ACGT"), good[:17], good[:-1], good[:16] + struct.pack("<H", 20) + good[18:]):
        assert shim.lib.inf_member(bad, len(bad), C.byref(dof)) == 0


def test_corrupt_blocks(shim):
    for name, payload, isize, crc, _ in bc.corrupt_blocks():
        st, _, _ = shim(payload, isize, crc)
        assert st == WANT[name], (name, st)


def test_bit_flips(shim):
    ok = 0
    for name, payload, isize, crc, text in bc.bit_flips():
        st, got, _ = shim(payload, isize, crc)
        if st == OK:                                      # a flip in bits nothing reads: the text zlib gives, and the right one
            assert got == bc.zlib_inflate(payload, isize) == text, name
            ok += 1
    assert ok < 20


def test_stand_alone_under_sanitizers(files, tmp_path):
    """host code with its own main: address + undefined-behaviour sanitizers over the blocks of the fixtures and every corrupt case"""
    exe = os.path.join(BUILD, "inflate_hd_shim_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DINF_MAIN", "-o", exe, SRC])
    recs, want = [], []
    for name in ("rnd200.fa.gz", "pay7.fa.gz", "stored.fa.gz", "fixed.fq.gz", "mem1.fa.gz", "pay65536.fa.gz", "far.fa.gz"):
        for _, payload, isize, crc in bc.walk(open(files[name], "rb").read()):
            recs.append((payload, isize, crc)); want.append(OK)
    for name, payload, isize, crc, _ in bc.corrupt_blocks():
        recs.append((payload, isize, crc)); want.append(WANT[name])
    flips = bc.bit_flips()
    for _, payload, isize, crc, _ in flips:
        recs.append((payload, isize, crc)); want.append(None)
    p = tmp_path / "blocks.bin"
    with open(p, "wb") as f:
        for payload, isize, crc in recs:
            f.write(struct.pack("<III", len(payload), isize, crc) + payload)
    r = subprocess.run([exe, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(want) and all(w is None or g == w for g, w in zip(got, want))


def clean_corrupt_cases():
    """the corrupt cases the GPU test may use: those this file has shown to be clean on the host (all of corrupt_blocks())"""
    return sorted(WANT)
