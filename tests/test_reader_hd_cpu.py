"""CPU: the logic the reader's kernels run (linear_amd/csrc/lnr_reader_hd.h), compiled for the host by tests/reader_hd_shim.cpp and run tile
by tile at 7, 64 and 4096 bytes per tile: records, ordinals, header spans and the hand-over point against the serial reader
(LNR_READER_SERIAL=1, itself pinned to SeqAn's reader by tests/golden/reader.npz) on the six fixture files and a seeded random file per
format; block after block under small limits; tile summaries combined in other groupings give the same summary; the same shim as a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import reader_cases, reader_gpu_cases as rg

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "reader_hd_shim.cpp")
_u8p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
TILES = (7, 64, 4096)


@pytest.fixture(scope="module")
def shim():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libreader_hd_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.rs_parse.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, _u8p, _u64p, _u64p, _u64p]

    def parse(text, tile, allowed, free, eof=True):
        fmt = 1 if text[:1] == b">" else 2
        out = np.zeros(free + 1, np.uint8)
        cap = min(allowed, len(text))
        off, hdr, res = np.zeros(cap + 2, np.uint64), np.zeros(2 * cap + 2, np.uint64), np.zeros(8, np.uint64)
        rc = lib.rs_parse(fmt, text, len(text), int(eof), tile, allowed, free, out.ctypes.data_as(_u8p), off.ctypes.data_as(_u64p), hdr.ctypes.data_as(_u64p), res.ctypes.data_as(_u64p))
        assert rc == 0 and res[6] == 1, "tile summaries combine differently in another grouping"
        n, bases = int(res[0]), int(res[1])
        ids = [text[int(hdr[2 * k]):int(hdr[2 * k + 1])].rstrip(b"\r").decode(errors="replace") for k in range(n)]
        return dict(n=n, off=off[: n + 1].copy(), bases=out[:bases].copy(), ids=ids, consumed=int(res[2]), handover=int(res[3]), full=int(res[4]), too_big=int(res[5]))
    return parse


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from linear_amd import build as lb
    lb.build()
    d = tmp_path_factory.mktemp("reader_hd")
    paths, _ = reader_cases.write_cases(str(d))
    hand = {}
    for fmt in ("fasta", "fastq", "fastq_multiline"):
        p = str(d / ("rnd." + fmt))
        hand[p] = rg.random_file(p, fmt)
        paths["rnd." + fmt] = p
    text = rg.plain_text(paths["multiline.fq"])
    hand[paths["multiline.fq"]] = text.index(b"@q1/1")          # the first record of more than 100 bases is the first multi-line one
    want = {name: rg.serial_blocks(p, 1 << 22, 100000)[0] for name, p in paths.items()}
    return paths, hand, want


@pytest.mark.parametrize("tile", TILES)
def test_whole_file_equals_serial_reader(shim, files, tile):
    paths, hand, want = files
    for name, p in paths.items():
        text = rg.plain_text(p)
        got = shim(text, tile, 100000, 1 << 22)
        off, bases, ids = want[name]
        h = hand.get(p)
        if h is None:
            assert got["handover"] == 0 and got["n"] == off.size - 1 and got["consumed"] == len(text), name
        else:                                                     # nothing from the hand-over point on is consumed
            assert got["handover"] == 1 and got["consumed"] == h and 0 < got["n"] < off.size - 1, name
        n = got["n"]
        assert np.array_equal(got["off"], off[: n + 1]) and np.array_equal(got["bases"], bases[: int(off[n])]) and got["ids"] == ids[:n], name
        assert got["full"] == 0 and got["too_big"] == 0


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("cap,mr", [(5000, 7), (1000, 1), (40000, 64)])
def test_blocks_under_limits_equal_serial_reader(shim, files, tile, cap, mr):
    """block after block, each window from the block's first record to the end of the file, up to the hand-over point"""
    paths, hand, _ = files
    for name in ("rnd.fasta", "rnd.fastq", "rnd.fastq_multiline", "crlf_blank.fa", "reads.fq"):
        text = rg.plain_text(paths[name])
        blocks = rg.serial_blocks(paths[name], cap, mr)
        pos, k = 0, 0
        span = len(text) if tile > 7 else 3 * cap + 400 * mr + 4096   # (7-byte tiles: a window that holds more than the block can take, not the whole file)
        while pos < len(text) and k < 40:                         # (the first 40 blocks: every kind of boundary has occurred by then)
            got = shim(text[pos:pos + span], tile, mr, cap, eof=pos + span >= len(text))
            if got["n"] == 0 and not (got["full"] or got["handover"]) and pos + span < len(text):
                span *= 2                                         # no whole record in the window: a larger one, as the reader does
                continue
            if got["too_big"]:
                break                                             # (cap 1000 / 5000 against the 12000-base record of the fixtures: LNR_ERR_LIMIT)
            off, bases, ids = blocks[k]
            if got["handover"] and got["n"] < off.size - 1:
                assert pos + got["consumed"] == hand[paths[name]]
                assert np.array_equal(got["off"], off[: got["n"] + 1]) and got["ids"] == ids[: got["n"]]
                break
            assert got["n"] == off.size - 1 and np.array_equal(got["off"], off) and np.array_equal(got["bases"], bases) and got["ids"] == ids, (name, k)
            pos += got["consumed"]
            k += 1
        assert k > 0 or name in ("crlf_blank.fa", "reads.fq")


def test_window_cut_inside_a_record(shim, files):
    """a window that is not the end of the file: only complete records are taken, and none when the first one is cut"""
    paths, _, want = files
    for name in ("rnd.fasta", "rnd.fastq"):
        text = rg.plain_text(paths[name])
        off, bases, ids = want[name]
        for cut in (10, 4096, 4097, 100001):
            got = shim(text[:cut], 64, 100000, 1 << 22, eof=False)
            n = got["n"]
            assert got["handover"] == 0 and got["full"] == 0 and got["consumed"] <= cut
            assert np.array_equal(got["off"], off[: n + 1]) and np.array_equal(got["bases"], bases[: int(off[n])]) and got["ids"] == ids[:n]
            again = shim(text[: got["consumed"] + 1], 64, 100000, 1 << 22, eof=False) if n else None
            assert (n == 0) == (cut == 10) and (again is None or again["n"] == n)          # the take ends at the last record start of the window


def test_limit_and_edges(shim, tmp_path):
    got = shim(b">a\nACGUacguRYKM-*.\n>b\n" + b"A" * 500 + b"\n", 64, 10, 100)
    assert got["n"] == 1 and got["full"] == 1 and got["too_big"] == 0 and got["bases"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 4, 4, 4, 4, 4, 4]
    got = shim(b">b\n" + b"A" * 500 + b"\n", 64, 10, 100)
    assert got["n"] == 0 and got["too_big"] == 1
    for name, p in rg.edge_files(str(tmp_path), 64).items():
        text = open(p, "rb").read()
        blocks = rg.serial_blocks(p, 1 << 20, 1000)
        off, bases, ids = blocks[0] if blocks else (np.zeros(1, np.uint64), np.zeros(0, np.uint8), [])
        for tile in (7, 64):
            got = shim(text, tile, 1000, 1 << 20)
            n = got["n"]
            assert np.array_equal(got["off"], off[: n + 1]) and np.array_equal(got["bases"], bases[: int(off[n])]) and got["ids"] == ids[:n], name
            assert got["handover"] == (name in ("fq_unequal.fq", "fq_blank_line.fq")) and (got["handover"] or n == off.size - 1), name
            if got["handover"]:
                assert n == 1 and got["consumed"] == 16, name


def test_stand_alone_under_sanitizers(files, tmp_path):
    """host code with its own main: address + undefined-behaviour sanitizers over the random files at an odd tile size"""
    paths, _, want = files
    exe = os.path.join(BUILD, "reader_hd_shim_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DRS_MAIN", "-o", exe, SRC])
    for name in ("rnd.fasta", "rnd.fastq"):
        p = subprocess.run([exe, paths[name], "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        off = want[name][0]
        assert p.stdout.decode().startswith("%d records %d bases" % (off.size - 1, int(off[-1]))), p.stdout
