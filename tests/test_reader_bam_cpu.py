"""CPU: BAM input of the reader.  The record logic of linear_amd/csrc/lnr_bam_hd.h, compiled for the host by tests/reader_bam_hd_shim.cpp:
the header span with its "need more" answer, rec_valid / rec_plausible, nib2ord, the take against a Python model, and the speculate /
verify / repair scheme of the kernels run on the host at 64, 256 and 4096 bytes per tile against the true record list of every fixture of
tests/ubam_cases.py.  lnr_reader_next on every fixture against the independent Python decoder under three limits, against the same reads
as FASTQ, on the bad files and on a record longer than dst_cap.  The host decode and the host model as a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tests import reader_gpu_cases as rg, ubam_cases as ub

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "reader_bam_hd_shim.cpp")
_u64p, _u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
TILES = (64, 256, 4096)
LIMITS = [(1 << 22, 100000), (5000, 7), (1000, 1)]


@pytest.fixture(scope="module")
def shim():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libreader_bam_hd_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.bh_header_span.argtypes = [C.c_char_p, C.c_uint64, _u64p, _u64p, C.POINTER(C.c_int)]
    lib.bh_rec_valid.argtypes = lib.bh_rec_plausible.argtypes = [C.c_char_p, C.c_uint64, C.c_int]
    lib.bh_rec_fields.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
    lib.bh_take.argtypes = [_u32p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _u64p]
    lib.bh_guesses.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_uint32, _u32p]
    lib.bh_scheme.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_uint32, _u64p, C.c_uint64, _u64p]
    return lib


def header_span(shim, b):
    first, need, nref = C.c_uint64(), C.c_uint64(), C.c_int()
    st = shim.bh_header_span(b, len(b), C.byref(first), C.byref(need), C.byref(nref))
    return st, first.value, need.value, nref.value


def scheme(shim, body, n_ref, tile):
    offs = np.zeros(len(body) // 37 + 2, np.uint64)
    info = np.zeros(5, np.uint64)
    shim.bh_scheme(body, len(body), n_ref, tile, offs.ctypes.data_as(_u64p), offs.size, info.ctypes.data_as(_u64p))
    return offs[: int(info[0])].tolist(), int(info[1]), int(info[2]), int(info[3])


@pytest.fixture(scope="module")
def built():
    from linear_amd import build as lb
    lb.build()
    return lb


@pytest.fixture(scope="module")
def files(built, tmp_path_factory):
    from linear_amd.api import Reader
    tile = Reader.gpu_bam_tile()
    assert tile > 0
    d = str(tmp_path_factory.mktemp("bam_cpu"))
    return ub.write(d, tile), ub.streams(tile), tile, d


def test_header_span(shim):
    refs = ((b"chr1", 1000), (b"a_longer_name", 5))
    for h, n_ref in ((ub.header(), 0), (ub.header(b""), 0), (ub.header(b"@CO\t" + b"x" * 70000 + b"\n"), 0), (ub.header(b"@HD\tVN:1.6\n", refs), 2)):
        assert header_span(shim, h + b"\x55" * 50) == (0, len(h), len(h), n_ref)
        assert header_span(shim, h)[:2] == (0, len(h))
        last = 0
        for cut in sorted(set(list(range(0, min(len(h), 80))) + [len(h) // 2, len(h) - 5, len(h) - 1])):
            st, _, need, _ = header_span(shim, h[:cut])
            assert st == 1 and cut < need <= len(h) and need >= last, (cut, need)        # asks for more, never for more than the header
            last = need
    for bad in (b"BAM\2" + b"\0" * 20, b"@r1\nACGT\n+\nIIII\n", b"BA>"):
        assert header_span(shim, bad)[0] == -1, bad
    neg = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<i", -2)
    assert header_span(shim, neg)[0] == -1


def test_rec_valid_and_plausible(shim):
    codes = [1, 2, 4, 8, 15] * 4
    good = ub.record(b"name", codes, aux=b"XZZ\0")
    out = (C.c_int64 * 9)()
    shim.bh_rec_fields(good, out)
    assert list(out) == [len(good) - 4, -1, -1, 5, 0, 4, 20, -1, -1]
    assert shim.bh_rec_valid(good, len(good), 0) == 1 and shim.bh_rec_plausible(good, len(good), 0) == 1
    assert shim.bh_rec_valid(good, 36, 0) == 1                      # the name's NUL lies outside the buffer: not looked at
    bad = {"l_read_name 0": good[:12] + b"\0" + good[13:],
           "negative l_seq": ub.record(b"name", codes, l_seq=-1),
           "parts exceed block_size": ub.record(b"name", codes, block_size=32 + 5 + 10 + 20 - 1),
           "block_size 8": ub.record(b"name", codes, block_size=8),
           "block_size at the maximum": ub.record(b"name", codes, block_size=shim.bh_max_block()),
           "negative block_size": ub.record(b"name", codes, block_size=-40),
           "refID -2": ub.record(b"name", codes, refid=-2),
           "refID == n_ref": ub.record(b"name", codes, refid=0),
           "next_refID == n_ref": ub.record(b"name", codes, next_refid=0),
           "pos -2": ub.record(b"name", codes, pos=-2),
           "next_pos -2": ub.record(b"name", codes, next_pos=-2),
           "name without NUL": good[:36 + 4] + b"x" + good[36 + 5:]}
    for what, rec in bad.items():
        assert shim.bh_rec_valid(rec, len(rec), 0) == 0 and shim.bh_rec_plausible(rec, len(rec), 0) == 0, what
    assert shim.bh_rec_valid(ub.record(b"name", codes, block_size=32 + 5 + 10 + 20), 200, 0) == 1          # exactly its parts
    assert shim.bh_rec_valid(ub.record(b"name", codes, refid=0, next_refid=1), 200, 2) == 1
    assert shim.bh_rec_valid(ub.record(b"name", codes, refid=2), 200, 2) == 0


def test_nib2ord(shim):
    want = {"A": 0, "C": 1, "G": 2, "T": 3}
    assert [shim.bh_nib2ord(n) for n in range(16)] == [want.get(ch, 4) for ch in ub.CODES]


def test_take_against_the_model(shim):
    rng = random.Random(12)
    for trial in range(300):
        count = rng.randrange(0, 12)
        lens = [rng.choice((0, 1, 5, 50, 400)) for _ in range(count)]
        free, allowed, empty = rng.choice((0, 10, 60, 500, 10000)), rng.randrange(0, 14), rng.random() < 0.5
        n, bases = 0, 0
        while n < count and n < allowed and bases + lens[n] <= free:
            bases += lens[n]
            n += 1
        full = n < count and n < allowed
        arr = np.array(lens + [0], np.uint32)
        out = np.zeros(4, np.uint64)
        shim.bh_take(arr.ctypes.data_as(_u32p), count, free, allowed, int(empty), out.ctypes.data_as(_u64p))
        assert out.tolist() == [n, bases, int(full), int(full and n == 0 and empty)], (trial, lens, free, allowed, empty)


@pytest.mark.parametrize("tile", TILES)
def test_scheme_gives_the_true_record_list(shim, files, tile):
    _, streams, _, _ = files
    for name, st in streams.items():
        hdr, n_ref, recs = ub.parse(st)
        offs, repaired, flag, consumed = scheme(shim, st[hdr:], n_ref, tile)
        assert offs == [p - hdr for p, _, _, _ in recs] and flag == 0 and consumed == len(st) - hdr, (name, tile)
        if name in ("7_long", "9_decoy"):
            assert repaired >= 1, (name, tile)
    for name, (st, ordinal, off, why) in ub.bad_streams().items():
        hdr = header_span(shim, st)[1]
        offs, _, flag, consumed = scheme(shim, st[hdr:], 0, tile)
        assert len(offs) == ordinal and consumed == off - hdr and flag == (2 if name == "truncated" else 1), (name, tile)


def test_decoy_has_a_false_first_guess(shim, files):
    """the condition the GPU test's repaired_tiles >= 1 rests on, at the device's tile size: some tile's first plausible offset is no record start"""
    _, streams, tile, _ = files
    st = streams["9_decoy"]
    hdr, n_ref, recs = ub.parse(st)
    body = st[hdr:]
    nt = (len(body) + tile - 1) // tile
    first = np.zeros(nt, np.uint32)
    shim.bh_guesses(body, len(body), n_ref, tile, first.ctypes.data_as(_u32p))
    true = {p - hdr for p, _, _, _ in recs}
    false_guess = [t for t in range(nt) if first[t] != 0xFFFFFFFF and t * tile + int(first[t]) not in true]
    assert false_guess, first.tolist()
    # ... and it lies in the tile in which the next true record starts: that tile has to be walked again
    nxt = recs[2][0] - hdr
    assert nxt // tile in false_guess


def host_blocks(path, cap, mr):
    return rg.serial_blocks(path, cap, mr, serial=False)


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0].tolist() == w[0] and g[1].tobytes() == w[1] and g[2] == w[2], (what, k)


@pytest.mark.parametrize("cap,mr", LIMITS)
def test_reader_next_equals_the_python_decoder(files, cap, mr):
    paths, streams, _, _ = files
    for name, p in paths.items():
        ids, seqs, _ = ub.reads_of(ub.stream_of(p))               # the decoder reads the written file, through its BGZF wrapping
        same(host_blocks(p, cap, mr), ub.blocks_of(ids, seqs, cap, mr), (name, cap, mr))


def test_header_only_and_limit(files):
    from linear_amd.api import LnrError, Reader
    paths, _, _, _ = files
    r = Reader(paths["6_header_only"])
    n, off, ids = r.next(np.zeros(100, np.uint8), 10)
    assert n == 0 and ids == []
    r.close()
    r = Reader(paths["7_long"])                                    # 300 kb in front of a block of 1000 bases
    with pytest.raises(LnrError) as e:
        r.next(np.zeros(1000, np.uint8), 10)
    assert e.value.status == -6 and "longer than the block" in str(e.value)
    r.close()


def test_same_blocks_as_fastq(files):
    paths, streams, _, d = files
    fq = os.path.join(d, "rnd200.fq")
    with open(fq, "wb") as f:
        f.write(ub.fastq_of(streams["1_rnd200"]))
    for cap, mr in LIMITS:
        a, b = host_blocks(paths["1_rnd200"], cap, mr), host_blocks(fq, cap, mr)
        assert len(a) == len(b) and (len(a) > 0 or cap == 1000)       # (the first read is longer than 1000 bases: LNR_ERR_LIMIT from both)
        for x, y in zip(a, b):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]


def test_bad_files(built, tmp_path):
    from linear_amd.api import LnrError, Reader
    for name, (p, ordinal, off, why) in ub.write_bad(str(tmp_path)).items():
        r = Reader(p)
        with pytest.raises(LnrError) as e:
            r.next(np.zeros(1 << 20, np.uint8), 100000)
        assert e.value.status == -1 and ("BAM record %d at offset %d " % (ordinal, off)) in str(e.value) and why in str(e.value), (name, str(e.value))
        with pytest.raises(LnrError):                              # the reader can only be closed
            r.next(np.zeros(1 << 20, np.uint8), 100000)
        r.close()
        # under limits that end a block in front of the record the blocks before it stand
        r = Reader(p)
        n, _, ids = r.next(np.zeros(1 << 20, np.uint8), 4)
        assert n == 4 and ids == ["g0", "g1", "g3", "g4"]
        with pytest.raises(LnrError):
            r.next(np.zeros(1 << 20, np.uint8), 4)
        r.close()


def test_stand_alone_under_sanitizers(files, tmp_path):
    """host code with its own main: the host decode (lnr_reader.cpp without the device half) and the host model of the device scheme"""
    paths, streams, _, _ = files
    exe = os.path.join(BUILD, "reader_bam_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "reader_bam_asan_main.cpp"), os.path.join(HERE, "..", "linear_amd", "csrc", "lnr_reader.cpp"), "-lz", "-lpthread"])
    bad = ub.write_bad(str(tmp_path))
    names = list(paths)
    p = subprocess.run([exe, "256"] + [paths[n] for n in names] + [bad[n][0] for n in bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(names) + len(bad)
    for name, line in zip(names, lines):
        ids, seqs, c = ub.reads_of(streams[name])
        want = ub.blocks_of(ids, seqs, 5000, 7)
        whole = len(want) and sum(len(b[2]) for b in want) == len(ids)
        hdr, _, recs = ub.parse(streams[name])
        assert " status %d blocks %d records %d bases %d | chain %d " % (0 if whole or not ids else -6, len(want), sum(len(b[2]) for b in want), sum(len(b[1]) for b in want), len(recs)) in line, line
        assert line.endswith("flag 0")
    for (name, (_, ordinal, _, _)), line in zip(bad.items(), lines[len(names):]):
        assert " status -1 " in line and (" chain %d " % ordinal) in line, line
