"""CPU: the parallel inflate of plain gzip (linear_amd/csrc/lnr_gunzip_hd.h), compiled for the host by tests/gunzip_hd_shim.cpp.  The host
driver runs every stage (find, measure, stitch, emit, chain, resolve) serially with the device's chunking: it equals zlib on every
fixture of tests/gzip_cases.py at four chunk sizes, again with rounds of 8 KiB (many rounds, the window carried, rounds that must grow);
the finder reports exactly zlib's non-final dynamic block starts; false candidates occur where they must and nowhere else; 200 seeded
bit flips agree with zlib; and the same through a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import gzip_cases as gc

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "gunzip_hd_shim.cpp")
_u8p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
STATS = ("rounds", "members", "chunks", "candidates", "pieces", "falses", "blocks", "comp_bytes", "text_bytes", "win_syms", "grown")
BIG = 1 << 26           # the default round: every fixture is one round


@pytest.fixture(scope="module")
def shim():
    run = gc.host_driver()
    lib = run.lib
    lib.gz_find_all.argtypes = [C.c_char_p, C.c_ulonglong, C.c_ulonglong, _u64p, C.c_ulonglong]
    lib.gz_find_all.restype = C.c_ulonglong
    lib.gz_zlib_boundaries.argtypes = [C.c_char_p, C.c_ulonglong, _u64p, C.c_ulonglong]
    lib.gz_zlib_boundaries.restype = C.c_longlong
    lib.gz_member_header.argtypes = [C.c_char_p, C.c_ulonglong, _u64p]
    lib.gz_member_header.restype = C.c_uint
    return run


def test_fixture_maker():
    for name, (raw, text) in gc.all_files().items():
        assert gc.zlib_text(raw) == text, name
    f = gc.fixtures()
    assert f["fq_l0.fq.gz"][0][10] & 6 == 0 and f["fq_fixed.fq.gz"][0][10] & 6 == 2 and f["fq_l6.fq.gz"][0][10] & 6 == 4      # stored, fixed, dynamic
    assert f["header_fields.fq.gz"][0][3] == 30


@pytest.mark.parametrize("chunk", gc.CHUNKS)
def test_driver_equals_zlib(shim, chunk):
    for name, (raw, text) in gc.all_files().items():
        s, got, st, bad = shim(raw, len(text), chunk)
        assert s == 0 and got == text, (name, chunk, s, bad)
        assert st["pieces"] + st["falses"] == st["candidates"] + st["rounds"] and st["text_bytes"] == len(text), (name, st)
        if name.startswith("false_"):
            assert st["falses"] > 0, (name, chunk, st)
        elif name.startswith(("fq_l", "fa_l", "fq_m")):
            assert st["falses"] == 0, (name, chunk, st)


@pytest.mark.parametrize("chunk", (1024, 4096, 131072))
def test_driver_in_rounds_of_8k(shim, chunk):
    grown = 0
    for name, (raw, text) in list(gc.all_files().items()) + list(gc.small_files().items()):
        s, got, st, bad = shim(raw, len(text), chunk, 8192)
        assert s == 0 and got == text, (name, chunk, s, bad)
        assert st["rounds"] > 1 or st["grown"] > 0 or len(raw) < 8300, (name, st)
        grown += st["grown"]
    assert grown > 0


@pytest.mark.parametrize("chunk", (1024, 131072))
def test_files_that_end_behind_a_header(shim, chunk):
    """a round without a single byte: the driver reports the end of the input at the end of the file, with the text in front of it"""
    for name, (raw, text, where) in gc.cut_behind_header_files().items():
        assert gc.zlib_text(raw) is None, name
        for rnd in (BIG, 8192):
            s, got, _, bad = shim(raw, len(text) + 200, chunk, rnd)
            assert s == 1 and got == text and bad == where, (name, chunk, rnd, s, bad)


def test_text_that_does_not_fit(shim):
    raw, text = gc.fixtures()["fq_l6.fq.gz"]
    for cap in (0, 1, 100000, len(text) - 1):
        s, got, _, _ = shim(raw, cap, 32768)
        assert s == 21 and text.startswith(got), cap


def zlib_block_starts(lib, raw):
    """[(bit, bfinal, btype)] of the first member, from zlib's inflate(Z_BLOCK)"""
    bits = np.zeros(1 << 16, np.uint64)
    n = lib.gz_zlib_boundaries(raw, len(raw), bits.ctypes.data_as(_u64p), bits.size)
    assert 0 < n <= bits.size
    out = []
    for b in (int(x) for x in bits[:n]):
        h = (int.from_bytes(raw[b >> 3:(b >> 3) + 2], "little") >> (b & 7)) & 7
        out.append((b, h & 1, h >> 1))
        if h & 1:
            break
    return out


def test_finder_reports_zlibs_block_starts(shim):
    for name, want_min in (("fq_l6.fq.gz", 50), ("fq_m4.fq.gz", 800), ("fa_l6.fa.gz", 10)):
        raw = gc.fixtures()[name][0]
        starts = zlib_block_starts(shim.lib, raw)
        assert all(t == 2 for _, _, t in starts), name
        want = [b for b, fin, t in starts[1:] if not fin and t == 2]          # behind the first, not the final one
        bits = np.zeros(1 << 16, np.uint64)
        n = shim.lib.gz_find_all(raw, len(raw), starts[0][0] + 1, bits.ctypes.data_as(_u64p), bits.size)
        assert [int(x) for x in bits[:n]] == want and n >= want_min, (name, n, len(want))


def test_three_quarters_of_32k_chunks_start_a_piece(shim):
    """what tests/test_gpu_reader_gzip.py relies on, shown on the host driver for the fixture it uses"""
    raw, text = gc.fixtures()["fq_l6.fq.gz"]
    s, got, st, _ = shim(raw, len(text), 32768)
    assert s == 0 and 4 * st["pieces"] >= 3 * st["chunks"] and st["chunks"] > 20, st


def test_member_header(shim):
    d = C.c_uint64()
    raw = gc.fixtures()["header_fields.fq.gz"][0]
    plain = gc.fixtures()["fq_l6.fq.gz"][0]
    assert shim.lib.gz_member_header(plain, len(plain), C.byref(d)) == 0 and d.value == 10
    assert shim.lib.gz_member_header(raw, len(raw), C.byref(d)) == 0
    assert zlib.decompress(raw[d.value:], -15) == gc.fixtures()["header_fields.fq.gz"][1]
    for cut in range(d.value):
        assert shim.lib.gz_member_header(raw[:cut], cut, C.byref(d)) == (1 if cut < 2 or raw[:2] == b"\x1f\x8b" else 20), cut
    for bad in (b"\x1f\x8c" + raw[2:], raw[:2] + b"\x07" + raw[3:], raw[:3] + b"\x20" + raw[4:]):
        assert shim.lib.gz_member_header(bad, len(bad), C.byref(d)) == 20


def flip_verdicts(shim):
    """[(name, raw, text zlib gives or None)] with the driver's result checked against it"""
    out = []
    for name, raw, text in gc.bit_flips():
        want = gc.zlib_text(raw)
        s, got, _, bad = shim(raw, len(text) + 70000, 4096)
        if want is None:
            assert s != 0, name
        else:
            assert s == 0 and got == want, (name, s, bad)
        out.append((name, raw, want))
    return out


def test_bit_flips(shim):
    v = flip_verdicts(shim)
    assert sum(w is None for _, _, w in v) > 150


def test_cut_file_and_bad_trailer(shim):
    raw, text = gc.fixtures()["fq_l6.fq.gz"]
    s, got, _, bad = shim(raw[:len(raw) // 2], len(text), 32768)
    assert s == 1 and text.startswith(got) and 0 < bad <= len(raw) // 2
    crc = raw[:-8] + struct.pack("<I", zlib.crc32(text) ^ 4) + raw[-4:]
    s, got, _, bad = shim(crc, len(text), 32768)
    assert s == 13 and got == text and bad == len(raw) - 8
    size = raw[:-4] + struct.pack("<I", len(text) + 1)
    assert shim(size, len(text), 32768)[0] == 12
    # bytes behind the last member that start no member are passed over, as gzread does; a member cut inside its header is an error
    assert shim(raw + b"\0" * 100, len(text), 32768)[:2] == (0, text)
    assert shim(raw + raw[:7], len(text), 32768)[0] == 1


def test_stand_alone_under_sanitizers(tmp_path):
    """host code with its own main: address + undefined-behaviour sanitizers over every fixture, the rounds of 8 KiB and every flip"""
    exe = os.path.join(BUILD, "gunzip_hd_shim_san")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DGZ_MAIN", "-o", exe, SRC, "-lz"])
    recs, want = [], []
    for name, (raw, text) in gc.all_files().items():
        for chunk, rnd in [(c, BIG) for c in gc.CHUNKS] + [(1024, 8192)]:
            recs.append((raw, len(text), chunk, rnd)); want.append((0, len(text), zlib.crc32(text)))
    for name, raw, text in gc.bit_flips():
        z = gc.zlib_text(raw)
        recs.append((raw, len(text) + 70000, 4096, BIG)); want.append(None if z is None else (0, len(z), zlib.crc32(z)))
    for name, (raw, text, _) in gc.cut_behind_header_files().items():
        for chunk, rnd in ((1024, BIG), (131072, BIG), (1024, 8192)):
            recs.append((raw, len(text) + 200, chunk, rnd)); want.append(None)
    p = tmp_path / "files.bin"
    with open(p, "wb") as f:
        for raw, cap, chunk, rnd in recs:
            f.write(struct.pack("<QQQQ", len(raw), cap, chunk, rnd) + raw)
    r = subprocess.run([exe, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.decode().splitlines()]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g[0] != 0) if w is None else (g[:3] == w), (g, w)
