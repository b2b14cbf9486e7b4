"""Texts for the writer's device deflate, shared by tests/test_deflate_hd_cpu.py (lnr_deflate_hd.h on the host) and
tests/test_gpu_writer_bgzf.py (the kernel): the sizes at which a block begins, ends or stays empty, the degenerate code shapes (one distinct
byte, no match, a single distance, one byte), repeats at and just past the largest distance, and the kinds of text the writer produces."""
import random

from tests import bgzf_cases as bc

BLOCK = 0xff00


def _rnd(n, seed):
    return random.Random(seed).randbytes(n)


def _dna(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def distance_text(d, seed=17):
    """200 random bytes, filler without any repeat of four bytes, and the 200 bytes again at distance exactly d"""
    head = _rnd(200, seed)
    filler = b"".join(b"%06x|" % (i * 2654435761 % (1 << 24)) for i in range(d // 7 + 1))[: d - 200]
    return head + filler + head + b"tail"


def texts(sam_text=None):
    """name -> text.  sam_text: SAM text of the host writer (the caller formats it), added under 'sam'."""
    base = bc.random_fasta()
    t = {"size_%d" % n: (base * (n // len(base) + 1))[:n] for n in (0, 1, 2, 3, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17)}
    t["a_run"] = bc.a_run()
    t["one_byte_258"] = b"G" * 258
    t["one_byte_259"] = b"G" * 259
    t["single_distance"] = b"abcdefgh" * 40                    # every match at distance 8, 16, ...: few distance codes
    t["no_match"] = bytes(range(256))
    t["far"] = bc.far_text()
    t["dist_32768"] = distance_text(32768)
    t["dist_32769"] = distance_text(32769)
    t["random_bytes"] = _rnd(2 * BLOCK + 1000, 23)
    t["dna"] = _dna(BLOCK, 29)
    t["random_fasta"] = base
    if sam_text is not None:
        t["sam"] = sam_text
    return t


def host_bgzf():
    """text -> (BGZF members back to back, stored members) by lnr_deflate_hd.h compiled for the host (tests/deflate_hd_shim.cpp)"""
    import ctypes as C
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    os.makedirs(os.path.join(here, "_build"), exist_ok=True)
    so = os.path.join(here, "_build", "libdeflate_hd_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, os.path.join(here, "deflate_hd_shim.cpp")])
    lib = C.CDLL(so)
    lib.def_text.restype = C.c_ulonglong
    lib.def_text.argtypes = [C.c_char_p, C.c_ulonglong, C.c_char_p, C.POINTER(C.c_ulonglong)]

    def run(text):
        out = C.create_string_buffer(len(text) + 31 * (len(text) // BLOCK + 1) + 8)
        stored = C.c_ulonglong()
        m = lib.def_text(text, len(text), out, C.byref(stored))
        return out.raw[:m], stored.value
    return run
