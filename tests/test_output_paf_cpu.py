"""CPU: PAF from the writer (lnr_writer_format_paf, linear_amd/csrc/lnr_output.cpp) and from the per-read logic its GPU twin runs
(paf_read of linear_amd/csrc/lnr_output_hd.h, compiled for the host by tests/output_paf_shim.cpp).
 1. An independent derivation: tests/paf_cases.py builds the line from a SAM line of the reference's own goldens (flag, RNAME, POS, CIGAR*)
    plus the read's length and the genome's lengths; the host writer equals it byte for byte on every golden that carries SAM text.
 2. The host form against the device form, on the host: the shim equals the host writer on the synthetic shapes and the gap-path cord
    sets, presets 1 and 2; measured size = emitted size, no byte past it.
 3. Every line is valid PAF, one per SAM record.
 4. paf_read as a stand-alone program under the address and undefined-behaviour sanitizers, into buffers of exactly the measured size."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases, paf_cases as pc, writer_cases as wc
from tests.test_cli_golden_cpu import MODE_OPTS, UB_READS, sam_by_read

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "liboutput_paf_shim.so")
_u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def Writer():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    return Writer


def arrays_for_c(gids, glen, coff, cs, ce, rl, rids):
    coff, cs, ce, rl = (np.ascontiguousarray(a, dtype=np.uint64) for a in (coff, cs, ce, rl))
    gblob = b"".join(g.encode() + b"\0" for g in gids)
    goff = np.array(([0] + list(np.cumsum([len(g.encode()) + 1 for g in gids])))[:len(gids)], np.uint64)
    blob = b"".join(i.encode() + b"\0" for i in rids)
    ido = np.array(([0] + list(np.cumsum([len(i.encode()) + 1 for i in rids])))[:len(rids)], np.uint64)
    return gblob, goff, np.array(list(glen), np.uint64), coff, cs, ce, rl, blob, ido


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", SO, os.path.join(HERE, "output_paf_shim.cpp")])
    lib = C.CDLL(SO)
    common = [C.c_char_p, _u64p, _u64p, C.c_uint32, C.c_uint32, _u64p, _u64p, _u64p, C.c_uint32, _u64p, C.c_char_p, _u64p]
    lib.ps_measure.restype = lib.ps_emit.restype = C.c_uint64
    lib.ps_measure.argtypes = common + [_u64p]
    lib.ps_emit.argtypes = common + [C.c_char_p, _u64p]

    def fmt(gids, glen, coff, cs, ce, rl, rids, preset=1):
        gblob, goff, gl, coff, cs, ce, rl, blob, ido = arrays_for_c(gids, glen, coff, cs, ce, rl, rids)
        pad = lambda a: np.concatenate([a, np.zeros(1, np.uint64)])                       # (never empty: a valid pointer for ctypes)
        p = lambda a: a.ctypes.data_as(_u64p)
        n = coff.size - 1
        args = [gblob, p(pad(goff)), p(pad(gl)), len(gids), preset, p(coff), p(pad(cs)), p(pad(ce)), n, p(pad(rl)), blob + b"\0", p(pad(ido))]
        sizes, emitted = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        total = lib.ps_measure(*args, p(sizes))
        buf = C.create_string_buffer(int(total) + 16)
        assert lib.ps_emit(*args, buf, p(emitted)) == total
        assert np.array_equal(sizes, emitted), "measured and emitted sizes differ"
        assert buf.raw[total:] == b"\0" * 16, "bytes written past the measured size"
        return buf.raw[:total]
    return fmt


def by_read(paf: bytes):
    recs = {}
    for l in paf.split(b"\n"):
        if l:
            recs.setdefault(l.split(b"\t")[0], []).append(l + b"\n")
    return recs


def expect_from_golden_sam(sam: bytes, rid, rl, gid, glen):
    """QNAME -> the PAF lines derived from the golden's SAM lines"""
    L = {i.encode(): int(x) for i, x in zip(rid, rl)}
    G = {g.encode(): int(x) for g, x in zip(gid, glen)}
    _, recs = sam_by_read(sam)
    return {k: [pc.paf_of_sam_line(l, L[k], G) for l in v] for k, v in recs.items()}


# ---- 1. the independent derivation
@pytest.mark.parametrize("name", list(cases.CASES_CLI))
def test_host_writer_equals_the_derivation_from_the_real_programs_sam(Writer, oracle_lib, case_inputs, name):
    """tests/golden/cli_<case>.npz: the .sam the real program wrote at -g 0, -g 50, -g 50 -dup 1 and without -g; the cords are the oracle's, as in
    tests/test_cli_golden_cpu.py (which pins that the writer's SAM on them is that text, but for the read listed there)."""
    refs, reads, off = cases.CASES_CLI[name]() if name not in cases.CASES and name not in cases.CASES_G50 else case_inputs(name)
    g = np.load(os.path.join(wc.GOLD, f"cli_{name}.npz"))
    assert cases.input_digest(refs, reads, off) == str(g["digest"])
    rid, gid = cases.text_ids(off.size - 1, len(refs))
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    glen = [r.size for r in refs]
    w = Writer(gid, glen)
    o = oracle_lib.Checker("oracle", refs, 1)
    lines = 0
    for mode, (gl, dup) in MODE_OPTS.items():
        coff, cs, ce, _ = o.map_batch(reads, off, threads=4, gap_len=gl, dup=dup)
        paf = w.format_paf(coff, cs, ce, rl, rid)
        want, got = expect_from_golden_sam(g[f"sam_{mode}"].tobytes(), rid, rl, gid, glen), by_read(paf)
        assert list(got) == list(want)
        for k in want:
            if k not in UB_READS.get((name, mode), set()):
                assert got[k] == want[k], (mode, k)
        pc.check_valid(paf, pc.sam_records(w.format(coff, cs, ce, rl, rid, "sam")))
        lines += paf.count(b"\n")
    assert lines >= 4 * 6              # (the smallest case has six reads)
    o.close(); w.close()


@pytest.mark.parametrize("name,dup", wc.GAP_SETS)
def test_host_writer_equals_the_derivation_on_the_gap_goldens(Writer, case_inputs, name, dup):
    """chim, ccs_sv and edge at -g 50, dup 0 and 1: the reference's cords of tests/golden/<case>_g50_T1.npz with the SAM text the real program
    wrote for them (cli_<case>.npz), real read lengths."""
    refs, reads, off = case_inputs(name)
    g, gs = np.load(os.path.join(wc.GOLD, f"{name}_g50_T1.npz")), np.load(os.path.join(wc.GOLD, f"cli_{name}.npz"))
    assert cases.input_digest(refs, reads, off) == str(g["digest"]) == str(gs["digest"])
    mode = "g50dup1" if dup else "g50"
    rid, gid = cases.text_ids(off.size - 1, len(refs))
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    glen = [r.size for r in refs]
    w = Writer(gid, glen)
    a = (g[f"cord_off_dup{dup}"], g[f"cords_str_dup{dup}"], g[f"cords_end_dup{dup}"], rl, rid)
    paf = w.format_paf(*a)
    want, got = expect_from_golden_sam(gs[f"sam_{mode}"].tobytes(), rid, rl, gid, glen), by_read(paf)
    assert list(got) == list(want)
    for k in want:
        if k not in UB_READS.get((name, mode), set()):
            assert got[k] == want[k], k
    pc.check_valid(paf, pc.sam_records(w.format(*a, "sam")))
    assert sum(len(v) for v in want.values()) >= 30 and any(b"\t-\t" in l for v in want.values() for l in v)
    w.close()


@pytest.mark.parametrize("name,T", [(n, T) for n, (_, Ts) in cases.CASES.items() for T in Ts])
def test_host_writer_equals_the_derivation_on_the_stage_goldens(Writer, case_inputs, name, T):
    """tests/golden/<case>_T<T>.npz hold the reference's cords at -g 0 and its SAM text for them."""
    refs, reads, off = case_inputs(name)
    g = np.load(os.path.join(wc.GOLD, f"{name}_T{T}.npz"))
    rid, gid = cases.text_ids(off.size - 1, len(refs))
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    glen = [r.size for r in refs]
    w = Writer(gid, glen)
    paf = w.format_paf(g["cord_off"], g["cords_str"], g["cords_end"], rl, rid)
    L = {i.encode(): int(x) for i, x in zip(rid, rl)}
    assert paf == pc.paf_of_sam(g["sam"].tobytes(), L, {k.encode(): v for k, v in zip(gid, glen)})
    pc.check_valid(paf, pc.sam_records(g["sam"].tobytes()))
    w.close()


def test_the_derivation_on_a_line_written_out_by_hand():
    """The Python side itself, on numbers a reader can check: 5S 100= 3I 20X 7D 50= 12S, POS 1001, read of 190 bases."""
    sam = b"r 1\t%d\tchr1\t1001\t255\t5S100=3I20X7D50=12S\t*\t0\t0\t*\t*"
    assert pc.paf_of_sam_line(sam % 0, 190, {b"chr1": 5000}) == b"r 1\t190\t5\t178\t+\tchr1\t5000\t1000\t1177\t150\t180\t255\tcg:Z:100=3I20X7D50=\n"
    assert pc.paf_of_sam_line(sam % 2064, 190, {b"chr1": 5000}) == b"r 1\t190\t12\t185\t-\tchr1\t5000\t1000\t1177\t150\t180\t255\tcg:Z:100=3I20X7D50=\n"
    assert pc.paf_of_sam_line(b"q\t16\t*\t8\t255\t*\t*\t0\t0\t*\t*", 9, {}) == b"q\t9\t0\t9\t-\t*\t0\t7\t7\t0\t0\t255\n"
    with pytest.raises(AssertionError):
        pc.paf_of_sam_line(b"q\t0\tchr1\t8\t255\t9S\t*\t0\t0\t*\t*", 9, {b"chr1": 10})


# ---- 2. host form against device form, on the host
@pytest.mark.parametrize("preset", [1, 2])
def test_shared_logic_equals_host_writer_on_synthetic_cords(Writer, shim, preset):
    w = Writer(wc.GIDS, wc.GLEN)
    w.set_preset(preset)
    for batch in (wc.synthetic(), wc.one_read(), wc.empty(), pc.strands_and_clips(), pc.tile_edges(), pc.window_lines(), pc.misaligned(), pc.target_fields()):
        want = w.format_paf(*batch)
        got = shim(wc.GIDS, wc.GLEN, *batch, preset)
        assert got == want, next((x, y) for x, y in zip(want.split(b"\n"), got.split(b"\n")) if x != y)
        assert want.count(b"\n") == pc.sam_records(w.format(*batch, "sam"))
    paf = w.format_paf(*wc.synthetic())
    # the shapes are really in there: '*' with length 0, the 10-digit length, both strands, a line without cg, splits at preset 1 alone
    import re
    assert b"\t*\t0\t" in paf and b"\tchrA\t4000000000\t" in paf and b"\t-\t" in paf and b"\t+\t" in paf and b"\t255\n" in paf
    assert bool(re.search(rb"cg:Z:\S*[=XID]80[DI]", paf)) == (preset == 1)
    assert w.format_paf(*wc.empty()) == b""
    w.close()


@pytest.mark.parametrize("preset", [1, 2])
@pytest.mark.parametrize("name,dup", wc.GAP_SETS)
def test_shared_logic_equals_host_writer_on_gap_cords(Writer, shim, name, dup, preset):
    batch = wc.gap_set(name, dup)
    w = Writer(wc.GIDS, wc.GLEN)
    w.set_preset(preset)
    want = w.format_paf(*batch)
    assert shim(wc.GIDS, wc.GLEN, *batch, preset) == want
    pc.check_valid(want, pc.sam_records(w.format(*batch, "sam")))        # 3. (the lengths here are the largest cord end + 0 .. 2)
    w.close()


# ---- 3. validity on the small shapes (the goldens: above, next to the derivation)
def test_every_line_of_the_small_shapes_is_valid(Writer):
    w = Writer(wc.GIDS, wc.GLEN)
    for batch in (wc.one_read(), pc.strands_and_clips(), pc.tile_edges(), pc.window_lines(), pc.misaligned(), pc.target_fields()):
        pc.check_valid(w.format_paf(*batch), pc.sam_records(w.format(*batch, "sam")))
    paf = w.format_paf(*pc.strands_and_clips()).split(b"\n")
    # forward: lead 17, trail 23 of L = 136; reverse: the two swap; L below the cord's end: the trail is 0 and the end is L
    assert paf[3].split(b"\t")[1:5] == [b"136", b"17", b"113", b"+"] and paf[8].split(b"\t")[1:5] == [b"136", b"23", b"119", b"-"]
    assert paf[4].split(b"\t")[1:5] == [b"100", b"17", b"100", b"+"] and paf[9].split(b"\t")[1:5] == [b"100", b"0", b"83", b"-"]
    w.close()


def test_window_shapes_are_what_they_claim(Writer):
    """tests/paf_cases.py window_lines: one line longer than the kernels' LDS window, one line across a window edge (OUT_WIN = 8192 bytes, windows
    counted from the read's first byte rounded down to 4, per tile of 64 cords)."""
    import re
    src = open(os.path.join(HERE, "..", "linear_amd", "csrc", "lnr_output_kernels.hip")).read()
    assert int(re.search(r"constexpr u32 OUT_WIN = (\d+);", src).group(1)) == 8192
    w = Writer(wc.GIDS, wc.GLEN)
    coff, cs, ce, rl, rid = pc.window_lines()
    per_read = [w.format_paf(coff[k:k + 2] - coff[k], cs[int(coff[k]):int(coff[k + 1])], ce[int(coff[k]):int(coff[k + 1])], rl[k:k + 1], rid[k:k + 1]) for k in range(len(rid))]
    assert per_read[0].count(b"\n") == 1 and len(per_read[0]) > 8192
    pos, crossing = len(per_read[0]) & 3, []
    for l in per_read[1].split(b"\n")[:-1]:
        crossing.append(pos // 8192 != (pos + len(l)) // 8192)
        assert len(l) + 1 < 8192
        pos += len(l) + 1
    assert crossing == [False, False, True, False, False, True]
    w.close()


# ---- 4. the stand-alone program under the sanitizers
def test_paf_read_under_sanitizers(Writer, tmp_path):
    exe, path = str(tmp_path / "output_paf_main"), str(tmp_path / "batches.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "output_paf_main.cpp")])
    w = Writer(wc.GIDS, wc.GLEN)
    reads, text = 0, {1: b"", 2: b""}
    with open(path, "wb") as f:
        for preset in (1, 2):
            w.set_preset(preset)
            for batch in [wc.synthetic(), wc.one_read(), wc.empty(), pc.strands_and_clips(), pc.tile_edges(), pc.window_lines(), pc.target_fields()] + [wc.gap_set(n, d) for n, d in wc.GAP_SETS]:
                gblob, goff, gl, coff, cs, ce, rl, blob, ido = arrays_for_c(wc.GIDS, wc.GLEN, *batch)
                f.write(np.array([len(wc.GIDS), coff.size - 1, cs.size, len(gblob), len(blob), preset], np.uint64).tobytes())
                for a in (goff, gl, coff, cs, ce, rl, ido):
                    f.write(a.tobytes())
                for b in (gblob, blob):
                    f.write(b + b"\0" * (-len(b) % 8))
                text[preset] += w.format_paf(*batch)
                reads += coff.size - 1
    w.close()
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    all_text = text[1] + text[2]
    h = 1469598103934665603
    for b in all_text:
        h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
    assert p.stdout.decode().split() == ["ok", str(reads), str(len(all_text)), f"{h:016x}"]
    assert text[1] != text[2]
