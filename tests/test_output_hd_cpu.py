"""CPU: the per-read formatting logic the writer's kernels run (linear_amd/csrc/lnr_output_hd.h), compiled for the host by
tests/output_shim.cpp: byte for byte the reference's text of the goldens, the host writer's text on the gap-path cord sets (many SA:Z
lines, supplementary flags, long CIGARs) and on the synthetic shapes of tests/writer_cases.py; the counting sink and the byte sink
agree read by read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases, writer_cases as wc

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "liboutput_shim.so")
_u64p = C.POINTER(C.c_uint64)
PARAMS = [(n, T) for n, (_, Ts) in cases.CASES.items() for T in Ts]


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "output_shim.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", SO, src])
    lib = C.CDLL(SO)
    common = [C.c_char_p, _u64p, _u64p, C.c_uint32, C.c_uint32, _u64p, _u64p, _u64p, C.c_uint32, _u64p, C.c_char_p, _u64p, C.c_int]
    lib.os_measure.restype = lib.os_emit.restype = C.c_uint64
    lib.os_measure.argtypes = common + [_u64p]
    lib.os_emit.argtypes = common + [C.c_char_p, _u64p]

    def fmt(gids, glen, coff, cs, ce, rl, rids, what, preset=1):
        p = lambda a: a.ctypes.data_as(_u64p)
        coff, cs, ce, rl = (np.ascontiguousarray(a, dtype=np.uint64) for a in (coff, cs, ce, rl))
        cs, ce = (np.concatenate([a, np.zeros(1, np.uint64)]) for a in (cs, ce))          # (never empty: a valid pointer for ctypes)
        n = coff.size - 1
        gblob = b"".join(g.encode() + b"\0" for g in gids)
        goff = np.array([0] + list(np.cumsum([len(g.encode()) + 1 for g in gids])), np.uint64)
        gl = np.array(list(glen) + [0], np.uint64)
        blob = b"".join(i.encode() + b"\0" for i in rids) + b"\0"
        ido = np.array([0] + list(np.cumsum([len(i.encode()) + 1 for i in rids])), np.uint64)
        args = [gblob, p(goff), p(gl), len(gids), preset, p(coff), p(cs), p(ce), n, p(np.concatenate([rl, np.zeros(1, np.uint64)])), blob, p(ido), {"sam": 1, "apf": 2}[what]]
        sizes, emitted = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        total = lib.os_measure(*args, p(sizes))
        buf = C.create_string_buffer(int(total) + 16)
        assert lib.os_emit(*args, buf, p(emitted)) == total
        assert np.array_equal(sizes, emitted), "measured and emitted sizes differ"
        assert buf.raw[total:] == b"\0" * 16
        return buf.raw[:total]
    return fmt


@pytest.fixture(scope="module")
def host_writer():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    return Writer


@pytest.mark.parametrize("name,T", PARAMS)
def test_shared_logic_equals_reference_text(shim, case_inputs, name, T):
    refs, reads, off = case_inputs(name)
    g = np.load(os.path.join(wc.GOLD, f"{name}_T{T}.npz"))
    rid, gid = cases.text_ids(off.size - 1, len(refs))
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    a = (gid, [r.size for r in refs], g["cord_off"], g["cords_str"], g["cords_end"], rl, rid)
    sam, apf = shim(*a, "sam"), shim(*a, "apf")
    want_sam, want_apf = wc.sam_body(g["sam"].tobytes()), g["apf"].tobytes()
    assert sam == want_sam and apf == want_apf


@pytest.mark.parametrize("name,dup", wc.GAP_SETS)
def test_shared_logic_equals_host_writer_on_gap_cords(shim, host_writer, name, dup):
    coff, cs, ce, rl, rid = wc.gap_set(name, dup)
    w = host_writer(wc.GIDS, wc.GLEN)
    want = {k: w.format(coff, cs, ce, rl, rid, k) for k in ("sam", "apf")}
    if name != "edge":        # what these sets are here for
        assert 30 <= want["sam"].count(b"SA:Z:") <= 44 and 16 <= want["sam"].count(b"\t2048\t") + want["sam"].count(b"\t2064\t") <= 29
    for k in ("sam", "apf"):
        assert shim(wc.GIDS, wc.GLEN, coff, cs, ce, rl, rid, k) == want[k], k
    w.close()


@pytest.mark.parametrize("preset", [1, 2])
def test_shared_logic_equals_host_writer_on_synthetic_cords(shim, host_writer, preset):
    w = host_writer(wc.GIDS, wc.GLEN)
    assert w.lib.lnr_writer_set_preset(w.h, preset) == 0
    for batch in (wc.synthetic(), wc.one_read(), wc.empty()):
        coff, cs, ce, rl, rid = batch
        for k in ("sam", "apf"):
            want = w.format(coff, cs, ce, rl, rid, k)
            got = shim(wc.GIDS, wc.GLEN, coff, cs, ce, rl, rid, k, preset)
            assert got == want, (k, next((x, y) for x, y in zip(want.split(b"\n"), got.split(b"\n")) if x != y))
    sam = w.format(*wc.synthetic(), "sam")
    # the shapes are really in there: splits only at preset 1, '*' names, five-record reads, merged '='
    import re
    assert bool(re.search(rb"[=XID]80[DI]", sam)) == (preset == 1) and b"\t*\t" in sam and sam.count(b"\t2064\t") >= 3
    w.close()


def test_decimal_conversion_by_hand():
    """put_u / put_i over the 64-bit range, the 16-digit seam and negative values, against Python's str()."""
    src = os.path.join(HERE, "_build", "dec_probe.cpp")
    exe = os.path.join(HERE, "_build", "dec_probe")
    os.makedirs(os.path.dirname(src), exist_ok=True)
    vals = [0, 9, 10, 10**15, 10**16 - 1, 10**16, 10**16 + 1, 10**17 + 5, 2**63 - 1, 2**63, 2**64 - 1]
    with open(src, "w") as f:
        f.write('#include "../../linear_amd/csrc/lnr_output_hd.h"\n#include <cstdio>\nint main(){ char b[64]; unsigned long long v[] = {' + ",".join(f"{v}ULL" for v in vals) +
                '};\nfor (auto x : v) { lnr_out::ByteSink s{b}; lnr_out::put_u(s, x); *s.p = 0; printf("%s ", b); lnr_out::ByteSink t{b}; lnr_out::put_i(t, (long long)x); *t.p = 0; printf("%s\\n", b); } }\n')
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src])
    out = subprocess.check_output([exe]).decode().split("\n")
    for v, line in zip(vals, out):
        assert line == f"{v} {v if v < 2**63 else v - 2**64}", (v, line)
