#!/usr/bin/env python3
"""Generate tests/golden/index_layouts.npz by running the REAL reference (oracle/_ref, built from /root/reference by oracle/Makefile)
on the seeded families of tests/index_cases.py.  Only runs where /root/reference exists.

Digests and cord words only (the inputs are regenerated from their seeds):
  <key>:hs_len, <key>:dir_sha, <key>:hs_sha      the DIndex of a configuration (-i 1)
  <key>:hs_len, <key>:ysa_sha                    the HIndex block array (-i 2; key ends in _i2)
  <key>:f2_len, <key>:f2_sha                     the genome window features: entries per sequence, and one digest over the entries of all
                                                 sequences without each sequence's last
  <key>:cord_off / cords_str / cords_end         the cords of many_reads at -g 0 (the read-set families only)
  <key>:sam_sha, <key>:apf_sha                   the reference's own SAM (header + records) and APF text for them (frag_max only)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pyorc  # noqa: E402
from tests import cases, index_cases as ic  # noqa: E402


def main():
    pyorc.build(ref=True)
    assert pyorc.have_ref(), "oracle/_ref not built (no /root/reference?)"
    out = {}
    for key, make, T, it in ic.all_configs():
        refs = make()
        r = pyorc.Checker("ref", refs, T, it)
        for k, v in ic.index_digests(r, len(refs), it).items():
            out[f"{key}:{k}"] = v
        name = key[: key.rindex("_T")]
        if it == 1 and name in ic.READ_SETS:
            reads, off = ic.many_reads(refs)
            coff, cs, ce, _ = r.map_batch(reads, off, threads=1)
            out[f"{key}:cord_off"], out[f"{key}:cords_str"], out[f"{key}:cords_end"] = coff, cs, ce
            if name == "frag_max":
                rid, gid = cases.text_ids(off.size - 1, len(refs))
                sam, apf = r.format(reads, off, rid, gid, cases.CMD_LINE)
                out[f"{key}:sam_sha"], out[f"{key}:apf_sha"] = cases.sha(np.frombuffer(sam, np.uint8)), cases.sha(np.frombuffer(apf, np.uint8))
        print(key, "entries", int(out[f"{key}:hs_len"]), flush=True)
        r.close()
    path = os.path.join(ROOT, "tests", "golden", "index_layouts.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} kB")


if __name__ == "__main__":
    main()
