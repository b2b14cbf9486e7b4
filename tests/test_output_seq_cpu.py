"""CPU: the SEQ column of the SAM writer (lnr_writer_set_genome / lnr_writer_format_seq, what the reference prints with -ss 1).
The host writer on the oracle's cords reproduces the real program's `-ss 1` text (tests/golden/cli_ss_<case>.npz, made by
tools/make_cli_ss_golden.py) byte for byte; the shared logic the kernels run (lnr_output_hd.h: head, segments, tail), compiled for the
host by tests/output_seq_shim.cpp, gives the host writer's text on the shapes of tests/writer_seq_cases.py, measured size = emitted size."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases, writer_cases as wc, writer_seq_cases as sc
from tests.test_cli_golden_cpu import MODE_OPTS

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "liboutput_seq_shim.so")
_u64p, _u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)


class In(C.Structure):
    _fields_ = [("gblob", C.c_char_p), ("goff", _u64p), ("glen", _u64p), ("nseq", C.c_uint32), ("preset", C.c_uint32), ("genome", _u8p), ("gstart", _u64p),
                ("coff", _u64p), ("cs", _u64p), ("ce", _u64p), ("n", C.c_uint32), ("reads", _u8p), ("roff", _u64p), ("ids", C.c_char_p), ("idoff", _u64p)]


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", SO, os.path.join(HERE, "output_seq_shim.cpp")])
    lib = C.CDLL(SO)
    lib.oss_measure.restype = lib.oss_emit.restype = C.c_uint64
    lib.oss_measure.argtypes = [C.POINTER(In), _u64p]
    lib.oss_emit.argtypes = [C.POINTER(In), C.c_char_p, _u64p]

    def fmt(gids, genome, coff, cs, ce, reads, off, rids, preset):
        pad = lambda a, t: np.concatenate([np.ascontiguousarray(a, dtype=t), np.zeros(1, t)])      # (never empty: a valid pointer for ctypes)
        glen = pad([g.size for g in genome], np.uint64)
        gstart = pad(np.cumsum([0] + [g.size for g in genome])[:-1], np.uint64)
        gcat = pad(np.concatenate(genome), np.uint8)
        goff = pad(np.cumsum([0] + [len(g.encode()) + 1 for g in gids]), np.uint64)
        ido = pad(np.cumsum([0] + [len(i.encode()) + 1 for i in rids]), np.uint64)
        coff, cs, ce, off, reads = pad(coff, np.uint64)[:-1], pad(cs, np.uint64), pad(ce, np.uint64), pad(off, np.uint64)[:-1], pad(reads, np.uint8)
        n = coff.size - 1
        keep = (glen, gstart, gcat, goff, ido, coff, cs, ce, off, reads)
        p = lambda a, t=_u64p: a.ctypes.data_as(t)
        a = In(b"".join(g.encode() + b"\0" for g in gids), p(goff), p(glen), len(gids), preset, p(gcat, _u8p), p(gstart), p(coff), p(cs), p(ce), n, p(reads, _u8p), p(off),
               b"".join(i.encode() + b"\0" for i in rids) + b"\0", p(ido))
        sizes, emitted = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        total = lib.oss_measure(C.byref(a), p(sizes))
        buf = C.create_string_buffer(int(total) + 16)
        assert lib.oss_emit(C.byref(a), buf, p(emitted)) == total
        assert np.array_equal(sizes, emitted), "measured and emitted sizes differ"
        assert buf.raw[total:] == b"\0" * 16 and keep
        return buf.raw[:total]
    return fmt


@pytest.fixture(scope="module")
def writer():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    made = []

    def make(preset=1, genome=True):
        w = Writer(sc.GIDS, sc.GLEN)
        w.set_preset(preset)
        if genome:
            w.set_genome(sc.genome())
        made.append(w)
        return w
    yield make
    for w in made:
        w.close()


def first_diff(want: bytes, got: bytes) -> str:
    for i, (x, y) in enumerate(zip(want.split(b"\n"), got.split(b"\n"))):
        if x != y:
            k = next((k for k, (a, b) in enumerate(zip(x, y)) if a != b), min(len(x), len(y)))
            return f"line {i} byte {k} of {len(x)} / {len(y)}: want {x[max(0, k - 40):k + 40]!r} got {y[max(0, k - 40):k + 40]!r}"
    return f"{len(want)} vs {len(got)} bytes"


@pytest.mark.parametrize("name,mode", [("edge", "g0"), ("chim", "g50dup1")])
def test_host_writer_reproduces_the_real_program_with_ss1(oracle_lib, case_inputs, name, mode):
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    refs, reads, off = case_inputs(name)
    g = np.load(os.path.join(HERE, "golden", f"cli_ss_{name}.npz"))
    assert cases.input_digest(refs, reads, off) == str(g["digest"])
    rid, gid = cases.text_ids(off.size - 1, len(refs))
    w = Writer(gid, [r.size for r in refs])
    w.set_genome(refs)
    o = oracle_lib.Checker("oracle", refs, 1)
    gl, dup = MODE_OPTS[mode]
    coff, cs, ce, _ = o.map_batch(reads, off, threads=4, gap_len=gl, dup=dup)
    got = w.sam_header("") + w.format_seq(coff, cs, ce, reads, off, rid)
    want = g[f"sam_{mode}"].tobytes()
    assert got == want, first_diff(want, got)
    seqs = [l.split(b"\t")[9] for l in want.split(b"\n") if l and not l.startswith(b"@")]
    assert len(seqs) > 50 and max(len(s) for s in seqs) > 10_000 and all(set(s) <= set(b"ACGTN") for s in seqs)
    o.close(); w.close()


@pytest.mark.parametrize("preset", [1, 2])
def test_shared_logic_equals_host_writer(shim, writer, preset):
    w = writer(preset)
    for batch in (sc.synthetic(), sc.one_read(), sc.empty()):
        want = w.format_seq(*batch)
        got = shim(sc.GIDS, sc.genome(), *batch, preset)
        assert got == want, first_diff(want, got)
    # the shapes are really in there
    import re
    recs = [l.split(b"\t") for l in w.format_seq(*sc.synthetic()).split(b"\n") if l]
    lens = {len(f[9]) for f in recs}
    assert set(sc.SEQ_LENS) <= lens and [f for f in recs if f[0] == b"empty"][0][5:10] == [b"*", b"*", b"0", b"0", b"*"]
    for f in recs:
        assert len(f[9]) == sc.seq_len_of_cigar(f[5]) or (f[9] == b"*" and f[5] == b"*"), f[:9]
    assert any(b"N" * 100 in f[9] for f in recs if f[1] == b"0") and any(b"N" * 100 in f[9] for f in recs if f[1] == b"16")     # X over equal bases, both strands
    assert bool(re.search(rb"[=XID]80[DI]", b"\n".join(f[5] for f in recs))) == (preset == 1)
    assert sum(1 for f in recs if len(f) > 11 and f[11].startswith(b"SA:Z:")) >= 8


def test_tile_and_window_shapes_are_in_the_cases(writer):
    """Counted from the host writer's output: the 70-record read of writer_cases.synthetic() gives every format of the kernels' read
    skeleton a second tile of records (records 64 .. 69, with SEQ: with bodies), a head that straddles a window edge, and a record whose
    tail lies in a later window than its head.  (Reads without cords and with the dummy cord alone: the first two of synthetic().)"""
    from tests import bam_cases as bmc
    w = writer(2)
    coff, cs, ce, reads, off, ids = sc.synthetic()
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    rid = wc.MANY.encode()
    assert ids.count(wc.MANY) == 1 and sorted(int(coff[k + 1] - coff[k]) for k in range(len(ids)))[:2] == [0, 1]
    shapes = {}
    for name, text in (("sam", w.format(coff, cs, ce, rl, ids, "sam")), ("sam_seq", w.format_seq(coff, cs, ce, reads, off, ids))):
        t0 = text.find(rid + b"\t")
        assert t0 > 0 and text[t0 - 1:t0] == b"\n"
        fields = [(l + b"\n").split(b"\t") for l in text[t0:].split(b"\n") if l.startswith(rid + b"\t")]
        whole = [len(b"\t".join(f)) for f in fields]
        if name == "sam":
            items = [(n, 0, 0) for n in whole]                                      # Text: an item is its head alone
        else:
            items = [(len(b"\t".join(f[:9])) + 1, len(f[9]), n - len(b"\t".join(f[:10]))) for f, n in zip(fields, whole)]
            assert all(b > 0 for _, b, _ in items[64:])                              # bodies in the second tile
        shapes[name] = (len(items), wc.tile_shapes(items, t0))
    for name, raw in (("bam", w.format_bam(coff, cs, ce, rl, ids)), ("bam_seq", w.format_bam(coff, cs, ce, None, ids, reads=reads, read_off=off))):
        p, t0, items = 0, None, []
        for r in bmc.walk_records(raw):
            size = 36 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + (r["l_seq"] + 1) // 2 + r["l_seq"] + len(r["tags"])
            if r["name"] == rid:
                t0 = p if t0 is None else t0
                items.append((36 + len(r["name"]) + 1 + 4 * len(r["cigar"]), (r["l_seq"] + 1) // 2 + r["l_seq"], len(r["tags"])))
            p += size
        shapes[name] = (len(items), wc.tile_shapes(items, t0))
    for name, (n, tiles) in shapes.items():
        assert n == 70 and len(tiles) == 2, name                                    # rec_carry = 64 in the second tile
        if name == "bam":                                                           # (the format Bam meets the two shapes below with SEQ)
            continue
        assert sum(st for st, _ in tiles) >= 1, (name, tiles)                        # a head across a window edge
        if name != "sam":
            assert sum(tl for _, tl in tiles) >= 1, (name, tiles)                    # a tail windows behind its head


@pytest.mark.parametrize("preset", [1, 2])
def test_seq_changes_nothing_but_column_10(writer, preset):
    w = writer(preset)
    for batch in (sc.synthetic(), sc.one_read(), sc.empty()):
        coff, cs, ce, reads, off, ids = batch
        rl = np.diff(off.astype(np.int64)).astype(np.uint64)
        assert sc.star_seq(w.format_seq(*batch)) == w.format(coff, cs, ce, rl, ids, "sam")


def test_format_seq_needs_the_genome(writer):
    from linear_amd.api import LnrError
    w = writer(genome=False)
    with pytest.raises(LnrError) as e:
        w.format_seq(*sc.one_read())
    assert e.value.status == -1 and "lnr_writer_set_genome" in str(e.value)
    w.set_genome(sc.genome())
    assert len(w.format_seq(*sc.one_read())) > 100
    w.set_genome(None)                                           # off again
    with pytest.raises(LnrError):
        w.format_seq(*sc.one_read())
