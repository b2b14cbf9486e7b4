#!/usr/bin/env python3
"""tests/golden/cli_bam_<case>.npz: the BAM the program users run writes with -ot 4.

Runs the REAL `linear filter` binary (oracle/_ref/linear, see tools/make_cli_golden.py) at `-t 1 -ot 4` on FASTA dumps of the seeded
cases edge and chim of tests/cases.py for every mode of cases.CLI_MODES, inflates the .bam (a chain of BGZF members = gzip members) and
stores per mode
    header_<mode>   the header text (the bytes between l_text and n_ref)
    n_ref_<mode>    the reference's n_ref -- 0: it hands SeqAn an empty context (f_io.cpp:509-523)
    recs_<mode>     the whole inflated record stream (everything after n_ref), without SEQ
    ss_len_<mode>, ss_sha_<mode>   length and sha256 of the record stream of the same run with -ss 1 (0.8-2.8 MB each: not stored)
and once header_pbsv, the header text of an `-ot 8` run (PREFIX_pbsv.bam; mode g0).

Only runs where the reference tree exists.  The stored vectors are data (the program's output), never reference source."""
from __future__ import annotations

import gzip
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pyorc  # noqa: E402
from tests import cases  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "linear")
CASES = ("edge", "chim")


def run_bam(rp, gp, flags, td, ot=4):
    pre = os.path.join(td, "out")
    path = pre + (".bam" if ot == 4 else "_pbsv.bam")
    if os.path.exists(path):
        os.remove(path)
    p = subprocess.run([BIN, "filter", rp, gp, "-t", "1", "-ot", str(ot), "-o", pre] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=td)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return split_bam(gzip.decompress(open(path, "rb").read()))


def split_bam(raw: bytes):
    """(header text, n_ref, record stream); the reference list is walked where there is one"""
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    text = raw[8:8 + l_text]
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        p += 4 + l_name + 4
    return text, n_ref, raw[p:]


def main():
    pyorc.build(ref=True)
    assert os.path.exists(BIN), "oracle/_ref/linear not built (no reference tree?)"
    outdir = os.path.join(ROOT, "tests", "golden")
    for name in CASES:
        refs, reads, off = cases.CASES_CLI[name]()
        d = {"digest": cases.input_digest(refs, reads, off), "n_reads": off.size - 1}
        with tempfile.TemporaryDirectory() as td:
            rp, gp, _, _ = cases.write_fasta_case(td, refs, reads, off)
            for mode, flags in cases.CLI_MODES.items():
                text, n_ref, recs = run_bam(rp, gp, flags, td)
                d[f"header_{mode}"], d[f"n_ref_{mode}"], d[f"recs_{mode}"] = np.frombuffer(text, np.uint8), n_ref, np.frombuffer(recs, np.uint8)
                _, _, ss = run_bam(rp, gp, flags + ["-ss", "1"], td)
                d[f"ss_len_{mode}"], d[f"ss_sha_{mode}"] = len(ss), hashlib.sha256(ss).hexdigest()
                print(f"{name} {mode}: header {len(text)} B, n_ref {n_ref}, records {len(recs)} B, with SEQ {len(ss)} B")
            text, _, _ = run_bam(rp, gp, cases.CLI_MODES["g0"], td, ot=8)
            d["header_pbsv"] = np.frombuffer(text, np.uint8)
        path = os.path.join(outdir, f"cli_bam_{name}.npz")
        np.savez_compressed(path, **d)
        print(f"{path}: {os.path.getsize(path) / 1024:.0f} kB")


if __name__ == "__main__":
    main()
