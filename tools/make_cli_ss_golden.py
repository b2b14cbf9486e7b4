#!/usr/bin/env python3
"""tests/golden/cli_ss_<case>.npz: the .sam of the program users run, WITH the SEQ column (`-ss 1`).

Runs the real `linear filter` binary (oracle/_ref/linear, see tools/make_cli_golden.py) at `-t 1 -ss 1` on two of the seeded cases of
tests/cases.py: `edge` at -g 0 (sam_g0) and `chim` at -g 50 -dup 1 (sam_g50dup1), and stores the whole text with the case's digest.  While
making them it checks that -ss 1 changes nothing but column 10: with that column put back to `*` the text is the sam_<mode> of the
existing cli_<case>.npz.

No case is truncated: both files hold all reads' records and stay under the largest golden committed before them.

Only runs where the reference tree exists.  The stored vectors are data (the program's output text), never reference source."""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_cli_golden import BIN, run_cli  # noqa: E402
from oracle import pyorc  # noqa: E402
from tests import cases  # noqa: E402

WHAT = {"edge": "g0", "chim": "g50dup1"}
LIMIT = 651 * 1024          # tests/golden/cli_ccs_sv.npz


def without_seq(sam: bytes) -> bytes:
    out = []
    for l in sam.split(b"\n"):
        if l and not l.startswith(b"@"):
            f = l.split(b"\t")
            f[9] = b"*"
            l = b"\t".join(f)
        out.append(l)
    return b"\n".join(out)


def main():
    pyorc.build(ref=True)
    assert os.path.exists(BIN), "oracle/_ref/linear not built (no reference tree?)"
    outdir = os.path.join(ROOT, "tests", "golden")
    for name, mode in WHAT.items():
        refs, reads, off = cases.CASES_CLI[name]()
        with tempfile.TemporaryDirectory() as td:
            rp, gp, _, _ = cases.write_fasta_case(td, refs, reads, off)
            sam, _ = run_cli(rp, gp, cases.CLI_MODES[mode] + ["-ss", "1"], td)
            again, _ = run_cli(rp, gp, cases.CLI_MODES[mode] + ["-ss", "1"], td)
        assert sam == again, "two runs differ"
        plain = np.load(os.path.join(outdir, f"cli_{name}.npz"))
        assert str(plain["digest"]) == cases.input_digest(refs, reads, off)
        assert without_seq(sam) == plain[f"sam_{mode}"].tobytes(), f"{name} {mode}: -ss 1 changed more than column 10"
        recs = [l.split(b"\t") for l in sam.split(b"\n") if l and not l.startswith(b"@")]
        print(f"{name} {mode}: sam {len(sam)} B, records {len(recs)}, longest SEQ {max(len(f[9]) for f in recs)}")
        path = os.path.join(outdir, f"cli_ss_{name}.npz")
        np.savez_compressed(path, **{"digest": cases.input_digest(refs, reads, off), f"sam_{mode}": np.frombuffer(sam, np.uint8)})
        size = os.path.getsize(path)
        print(f"{path}: {size / 1024:.0f} kB")
        assert size < LIMIT, "too large: store the first N reads' records only, and say N here"


if __name__ == "__main__":
    main()
