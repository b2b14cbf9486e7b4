"""CPU: the BAM writer (lnr_writer_bam_header / lnr_writer_format_bam; the records of -ot 4 / 8).
The expectation everywhere is bam_cases.bam_of_sam, the re-encoding rule applied to the SAM text the SAM writer gives for the same cords.
  - the shared logic the kernels run (lnr_output_hd.h: bam_head, packed SEQ, bam_tail), compiled for the host by tests/output_bam_shim.cpp:
    measured size = emitted size, no byte past the total, the expected bytes on every shape, without and with SEQ; the same source as a
    stand-alone program under the address and undefined-behaviour sanitizers;
  - lnr_writer_format_bam on 1 and 4 threads: the same;
  - the host writer on the oracle's cords of edge and chim in the four modes: the record stream the real program wrote with -ot 4
    (tests/golden/cli_bam_<case>.npz, made by tools/make_cli_bam_golden.py), with -ss 1 its length and sha256; bam_of_sam of the committed SAM
    goldens gives those streams too;
  - the header: the golden's text (std and pbsv) and the writer's own sequences as the reference list."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_cases as bmc, cases, writer_cases as wc, writer_seq_cases as sc
from tests.test_cli_golden_cpu import MODE_OPTS, UB_READS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "output_bam_shim.cpp")
SO = os.path.join(HERE, "_build", "liboutput_bam_shim.so")
GOLD = os.path.join(HERE, "golden")
_u64p, _u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)


class In(C.Structure):
    _fields_ = [("gblob", C.c_char_p), ("goff", _u64p), ("glen", _u64p), ("nseq", C.c_uint32), ("preset", C.c_uint32), ("genome", _u8p), ("gstart", _u64p),
                ("coff", _u64p), ("cs", _u64p), ("ce", _u64p), ("n", C.c_uint32), ("reads", _u8p), ("rlen", _u64p), ("ids", C.c_char_p), ("idoff", _u64p), ("seq", C.c_uint32)]


def arrays_of(gids, genome, coff, cs, ce, reads, rlen, rids, preset, seq):
    """the 13 arrays of one batch in the order the stand-alone program reads them (the first: nseq, preset, n, seq)"""
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    n = len(coff) - 1
    return [u64([len(gids), preset, n, int(seq)]), np.frombuffer(b"".join(g.encode() + b"\0" for g in gids), np.uint8), u64(np.cumsum([0] + [len(g.encode()) + 1 for g in gids])),
            u64([g.size for g in genome]), np.concatenate(genome).astype(np.uint8), u64(np.cumsum([0] + [g.size for g in genome])), u64(coff), u64(cs), u64(ce),
            np.ascontiguousarray(reads, dtype=np.uint8), u64(rlen), np.frombuffer(b"".join(i.encode() + b"\0" for i in rids) + b"\0", np.uint8),
            u64(np.cumsum([0] + [len(i.encode()) + 1 for i in rids]))]


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.obs_measure.restype = lib.obs_emit.restype = C.c_uint64
    lib.obs_measure.argtypes = [C.POINTER(In), _u64p]
    lib.obs_emit.argtypes = [C.POINTER(In), C.c_char_p, _u64p]

    def fmt(gids, genome, coff, cs, ce, reads, rlen, rids, preset, seq):
        arr = arrays_of(gids, genome, coff, cs, ce, reads, rlen, rids, preset, seq)
        arr = [np.concatenate([a, np.zeros(1, a.dtype)]) for a in arr]                  # (never empty: a valid pointer for ctypes)
        p = lambda i, t=_u64p: arr[i].ctypes.data_as(t)
        n = len(coff) - 1
        a = In(arr[1].tobytes(), p(2), p(3), len(gids), preset, p(4, _u8p), p(5), p(6), p(7), p(8), n, p(9, _u8p), p(10), arr[11].tobytes(), p(12), int(seq))
        sizes, emitted = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        total = lib.obs_measure(C.byref(a), sizes.ctypes.data_as(_u64p))
        buf = C.create_string_buffer(b"\xa5" * (int(total) + 16))
        assert lib.obs_emit(C.byref(a), buf, emitted.ctypes.data_as(_u64p)) == total
        assert np.array_equal(sizes, emitted), "measured and emitted sizes differ"
        assert buf.raw[total:total + 16] == b"\xa5" * 16, "bytes written past the total"
        return buf.raw[:total]
    return fmt


@pytest.fixture(scope="module")
def writer():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    made = []

    def make(preset=1, seq=False):
        w = Writer(sc.GIDS, sc.GLEN) if seq else Writer(wc.GIDS, wc.GLEN)
        w.set_preset(preset)
        if seq:
            w.set_genome(sc.genome())
        made.append(w)
        return w
    yield make
    for w in made:
        w.close()


@pytest.fixture(scope="module")
def expected(writer):
    """bam_of_sam of the SAM writer's text, once per (preset, batch)"""
    memo = {}

    def get(preset, name, batch, seq):
        key = (preset, name, seq)
        if key not in memo:
            w = writer(preset, seq)
            sam = w.format_seq(*batch) if seq else w.format(*batch, "sam")
            memo[key] = bmc.bam_of_sam(sam, sc.GIDS)
        return memo[key]
    return get


def first_diff(want: bytes, got: bytes) -> str:
    k = next((k for k, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
    return f"{len(want)} vs {len(got)} bytes, first difference at {k}: want {want[max(0, k - 24):k + 24].hex()} got {got[max(0, k - 24):k + 24].hex()}"


@pytest.mark.parametrize("preset", [1, 2])
def test_shared_logic_without_seq(shim, expected, preset):
    none = [np.zeros(1, np.uint8)]
    for name, (coff, cs, ce, rl, ids) in bmc.plain_batches():
        want = expected(preset, name, (coff, cs, ce, rl, ids), False)
        got = shim(wc.GIDS, [np.zeros(1, np.uint8)] * 3, coff, cs, ce, none[0], rl, ids, preset, False)
        assert got == want, (name, first_diff(want, got))


@pytest.mark.parametrize("preset", [1, 2])
def test_shared_logic_with_seq(shim, expected, preset):
    for name, (coff, cs, ce, reads, off, ids) in bmc.seq_batches():
        want = expected(preset, name, (coff, cs, ce, reads, off, ids), True)
        for form in (1, 2):                                      # one concatenated genome (the kernels); a pointer per sequence (the host writer)
            got = shim(sc.GIDS, sc.genome(), coff, cs, ce, reads, off, ids, preset, form)
            assert got == want, (name, form, first_diff(want, got))


def test_the_shapes_are_in_there(expected):
    recs = bmc.walk_records(expected(1, "seq", bmc.seq(), True))
    assert set(bmc.SEQ_LENS) <= {r["l_seq"] for r in recs}
    for r in recs:
        assert r["mapq"] == 255 and r["next"] == (-1, -1, 0) and r["qual"] == b"\xff" * r["l_seq"]
        assert r["l_seq"] == sum(n for n, op in r["cigar"] if op != "D")
    e = [r for r in recs if r["name"] == b"empty"][0]
    assert e["cigar"] == [] and e["l_seq"] == 0 and e["bin"] == bmc.reg2bin(500, 500)
    assert {len(r["name"]) for r in recs} >= {1, 2, 3, 4, 5}
    assert {r["flag"] & 16 for r in recs if r["l_seq"] in bmc.SEQ_LENS} == {0, 16} and any(r["ref"] == -1 for r in recs)
    m = [r for r in recs if r["name"] == b"m"]
    assert len(m) == 66 and all(r["tags"].startswith(b"SAZ") and r["tags"].endswith(b";\0") and r["tags"].count(b";") == 65 for r in m)
    assert max(len(r["cigar"]) for r in recs) > 256 and any(r["seq"].count(b"\xff") > 40 for r in recs)          # segments; N runs of an X over equal bases
    plain = bmc.walk_records(expected(1, "seq_shapes", bmc.plain_batches()[3][1], False))
    assert len(plain) == len(recs) and all(p["l_seq"] == 0 and p["seq"] == b"" and p["cigar"] == r["cigar"] and p["tags"] == r["tags"] for p, r in zip(plain, recs))


@pytest.mark.parametrize("threads", [1, 4])
def test_host_writer_equals_the_rule(writer, expected, threads):
    for preset in (1, 2):
        w, ws = writer(preset), writer(preset, seq=True)
        for name, batch in bmc.plain_batches():
            want, got = expected(preset, name, batch, False), w.format_bam(*batch, threads=threads)
            assert got == want, (name, first_diff(want, got))
        for name, (coff, cs, ce, reads, off, ids) in bmc.seq_batches():
            want = expected(preset, name, (coff, cs, ce, reads, off, ids), True)
            got = ws.format_bam(coff, cs, ce, None, ids, reads=reads, read_off=off, threads=threads)
            assert got == want, (name, first_diff(want, got))


def test_format_bam_with_seq_needs_the_genome(writer):
    from linear_amd.api import LnrError
    w = writer()
    coff, cs, ce, reads, off, ids = sc.one_read()
    with pytest.raises(LnrError) as e:
        w.format_bam(coff, cs, ce, None, ids, reads=reads, read_off=off)
    assert e.value.status == -1 and "lnr_writer_set_genome" in str(e.value)
    assert len(w.format_bam(coff, cs, ce, np.diff(off.astype(np.int64)), ids)) > 100        # without SEQ it needs none


def by_read(stream: bytes):
    recs, p = {}, 0
    while p < len(stream):
        bs, = struct.unpack_from("<i", stream, p)
        l_name = stream[p + 12]
        recs.setdefault(stream[p + 36:p + 36 + l_name - 1], []).append(stream[p:p + 4 + bs])
        p += 4 + bs
    return recs


@pytest.mark.parametrize("name", ["edge", "chim"])
def test_host_writer_reproduces_the_real_programs_bam(oracle_lib, case_inputs, name):
    """The four modes.  One read of `edge` at -g > 0 is compared with nothing: the real program's result for it depends on heap contents
    (tests/test_cli_golden_cpu.py: UB_READS); the golden streams themselves are pinned whole by bam_of_sam of the SAM goldens."""
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    refs, reads, off = case_inputs(name)
    g, gs, gss = (np.load(os.path.join(GOLD, f"{k}_{name}.npz")) for k in ("cli_bam", "cli", "cli_ss"))
    assert cases.input_digest(refs, reads, off) == str(g["digest"])
    rid, gid = cases.text_ids(off.size - 1, len(refs))
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    w = Writer(gid, [r.size for r in refs])
    w.set_genome(refs)
    o = oracle_lib.Checker("oracle", refs, 1)
    for mode, (gl, dup) in MODE_OPTS.items():
        want = g[f"recs_{mode}"].tobytes()
        assert bmc.bam_of_sam(gs[f"sam_{mode}"].tobytes(), gid) == want, mode                   # the rule IS what the program does
        if f"sam_{mode}" in gss:
            ss = bmc.bam_of_sam(gss[f"sam_{mode}"].tobytes(), gid)
            assert len(ss) == int(g[f"ss_len_{mode}"]) and hashlib.sha256(ss).hexdigest() == str(g[f"ss_sha_{mode}"]), mode
        coff, cs, ce, _ = o.map_batch(reads, off, threads=4, gap_len=gl, dup=dup)
        got, got_ss = w.format_bam(coff, cs, ce, rl, rid), w.format_bam(coff, cs, ce, None, rid, reads=reads, read_off=off)
        skip = UB_READS.get((name, mode), set())
        if not skip:
            assert got == want, (mode, first_diff(want, got))
            assert len(got_ss) == int(g[f"ss_len_{mode}"]) and hashlib.sha256(got_ss).hexdigest() == str(g[f"ss_sha_{mode}"]), mode
        else:
            a, b = by_read(got), by_read(want)
            assert list(a) == list(b) and all(a[k] == b[k] for k in b if k not in skip), mode
            if f"sam_{mode}" in gss:
                a, b = by_read(got_ss), by_read(bmc.bam_of_sam(gss[f"sam_{mode}"].tobytes(), gid))
                assert list(a) == list(b) and all(a[k] == b[k] for k in b if k not in skip), mode
        assert int(g[f"n_ref_{mode}"]) == 0
    o.close(); w.close()


@pytest.mark.parametrize("name", ["edge", "chim"])
def test_bam_header(case_inputs, name):
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    refs, reads, off = case_inputs(name)
    g = np.load(os.path.join(GOLD, f"cli_bam_{name}.npz"))
    _, gid = cases.text_ids(off.size - 1, len(refs))
    w = Writer(gid, [r.size for r in refs])
    for pbsv, key in ((False, "header_g0"), (True, "header_pbsv")):
        text, ref_list, rest = bmc.split_bam(w.bam_header("", pbsv))
        assert text == g[key].tobytes() and rest == b""
        # n_ref == nseq: the golden's n_ref is 0 (the reference hands its BAM writer an empty context) -- the one deliberate deviation, so
        # that htslib opens the file
        assert ref_list == [(i.encode(), r.size) for i, r in zip(gid, refs)] and len(ref_list) == len(refs) and int(g["n_ref_g0"]) == 0
    assert b"@RG\t ID:" in g["header_pbsv"].tobytes() and b"@RG\tID:" in g["header_g0"].tobytes()
    assert bmc.split_bam(w.bam_header("", False))[0] == w.sam_header("")
    w.close()


def test_stand_alone_under_sanitizers(expected, tmp_path):
    """host code with its own main: address + undefined-behaviour sanitizers over the shapes, output arrays of exactly the measured size"""
    exe = str(tmp_path / "obs_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DOBS_MAIN", "-o", exe, SRC])
    jobs = [(name, arrays_of(wc.GIDS, [np.zeros(1, np.uint8)] * 3, coff, cs, ce, np.zeros(0, np.uint8), rl, ids, 1, False), expected(1, name, (coff, cs, ce, rl, ids), False))
            for name, (coff, cs, ce, rl, ids) in bmc.plain_batches()[:4]]
    jobs += [(f"{name}_{form}", arrays_of(sc.GIDS, sc.genome(), coff, cs, ce, reads, off, ids, 1, form), expected(1, name, (coff, cs, ce, reads, off, ids), True))
             for name, (coff, cs, ce, reads, off, ids) in bmc.seq_batches() for form in (1, 2)]
    for name, arr, want in jobs:
        path = str(tmp_path / f"{name}.bin")
        with open(path, "wb") as f:
            for a in arr + [np.frombuffer(want, np.uint8)]:
                f.write(struct.pack("<Q", a.nbytes) + a.tobytes())
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0 and p.stdout.startswith(b"ok"), (name, p.stderr.decode()[-2000:])
