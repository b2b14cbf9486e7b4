"""Inputs shared by the tests of the writer's GPU twin (tests/test_output_hd_cpu.py on the host build of lnr_output_hd.h,
tests/test_gpu_writer.py on the device): the gap-path cord sets of the goldens and a synthetic batch of cord words built from the bit
layout of include/linear_amd.h -- main[63] recd[62] strand[61] blockEnd[60] id[50..59] x[20..49] y[0..19] -- holding the smallest
shapes at which a lane = cord formatter can go wrong.  Every read starts with the dummy cord 0 that carries the block-end flag, as the
pipeline emits it."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
F_END, F_STRAND = 1 << 60, 1 << 61
GAP_SETS = [(name, dup) for name in ("chim", "ccs_sv", "edge") for dup in (0, 1)]
GIDS = ["chrA", "c", "chromosome_three_with_a_long_name"]
GLEN = [4_000_000_000, 9, 1_073_741_823]           # 10 digits, 1 digit, 2^30 - 1


def cy(v):
    return np.asarray(v, np.uint64) & np.uint64(0xfffff)


def gap_set(name, dup):
    """(cord_off, cords_str, cords_end, read_len, read ids) of a -g 50 golden.  The goldens hold no read lengths: L = the read's largest
    cord end + (k mod 3), i.e. trailing clips of 0, 1 and 2 (both writers get the same L; the host writer is the reference here)."""
    g = np.load(os.path.join(GOLD, f"{name}_g50_T1.npz"))
    coff, cs, ce = g[f"cord_off_dup{dup}"], g[f"cords_str_dup{dup}"], g[f"cords_end_dup{dup}"]
    n = coff.size - 1
    rl = np.array([(int(cy(ce[int(coff[k]):int(coff[k + 1])]).max()) if coff[k + 1] > coff[k] else 100) + k % 3 for k in range(n)], np.uint64)
    return coff, cs, ce, rl, [f"read_{k} len extra={k * 3}" for k in range(n)]


class Batch:
    def __init__(self):
        self.cs, self.ce, self.off, self.rl, self.ids = [], [], [0], [], []

    def read(self, cords, L=None, rid=None, dummy=True):
        """cords: (x, y, strand, gid, end, w) tuples; w = side of the cord's window (cords_end = cords_str shifted by w in x and y)"""
        s = [F_END] if dummy else []
        e = [F_END] if dummy else []
        for (x, y, strand, gid, end, w) in cords:
            v = (gid << 50) + (x << 20) + y + (F_STRAND if strand else 0) + (F_END if end else 0)
            s.append(v)
            e.append(v + (w << 20) + w)
        self.cs += s
        self.ce += e
        self.off.append(len(self.cs))
        if L is None:
            L = max([(v & 0xfffff) for v in e[1:]] + [50]) + 7
        self.rl.append(L)
        self.ids.append(rid if rid is not None else f"syn_{len(self.ids)} x")
        return self

    def arrays(self):
        return (np.array(self.off, np.uint64), np.array(self.cs, np.uint64), np.array(self.ce, np.uint64), np.array(self.rl, np.uint64), list(self.ids))


def run(n, x0=1000, y0=5, step=100, strand=0, gid=0, w=96, ends=()):
    """n cords along one diagonal; `ends`: indices (1-based cord numbers inside the read) that carry the block-end flag"""
    return [(x0 + step * i, y0 + step * i, strand, gid, (i + 1) in ends, w) for i in range(n)]


def blocks(strands_per_block, x0=5000, gid=1):
    """one block per entry of strands_per_block, each ended by the flag on its last cord; blocks lie far apart"""
    out = []
    for b, strands in enumerate(strands_per_block):
        for i, s in enumerate(strands):
            out.append((x0 + 50_000 * b + 120 * i, 10 + 1000 * b + 120 * i, s, gid, i == len(strands) - 1, 96))
    return out


MANY = "many" + "y" * 23                                       # the QNAME of synthetic()'s 70-record read


def tile_shapes(items, t0, win=8192):
    """What the kernels' read skeleton meets in one read.  items: (head, body, tail) bytes of the read's records in order, every cord of
    the read a record; t0: the read's offset in the batch's text.  Per tile of 64 records: (heads that straddle an edge of the LDS window,
    records whose tail starts in a later window than their head) -- windows of `win` bytes from the tile's start rounded down to 4."""
    out, pos = [], t0
    for first in range(0, len(items), 64):
        wl, st, tl = pos & ~3, 0, 0
        for h, b, t in items[first:first + 64]:
            st += (pos - wl) // win != (pos + h - 1 - wl) // win
            tl += bool(t) and (pos + h + b - wl) // win > (pos - wl) // win
            pos += h + b + t
        out.append((st, tl))
    return out


def many_records(n=66):
    """one read of n records (every cord ends a block), strands alternating: two tiles of records, every record with an SA tag of n - 1 entries"""
    return [(5000 + 50_000 * b, 10 + 3 * b, b & 1, 0, True, 96) for b in range(n)]


def synthetic():
    B = Batch()
    B.read([], dummy=False)                                    # 0 cords
    B.read([])                                                 # 1 cord: the dummy alone
    B.read(run(1))                                             # 2 cords
    for n in (62, 63, 64, 65, 128, 129):                       # 63 .. 130 cords with the dummy: lane and tile borders
        B.read(run(n))
    for e in (63, 64, 65):                                     # a block border at / next to cord 64
        B.read(run(130, ends=(e,)))
    B.read(run(129, ends=(64, 128, 129)))
    B.read(blocks([[0, 0], [1, 1], [0]]))                      # 3 records
    B.read(blocks([[0], [1, 1], [0, 0, 0], [1], [0, 0]], gid=2))      # 5 records: SA:Z lines 2.. print NM 0 everywhere
    B.read(blocks([[1, 1, 1, 1]]))                             # reverse strand
    B.read(blocks([[1, 1, 0, 0]]))                             # tie main_cnt == block_len / 2, '-' first
    B.read(blocks([[0, 0, 1, 1]]))                             # tie, '+' first
    B.read(blocks([[1, 1, 1, 0], [0, 1, 0, 0], [0, 1], [1, 0]]))
    B.read([(9000, 900, 0, 0, False, 96), (8000, 700, 0, 0, False, 96), (8500, 650, 1, 0, False, 96), (100, 640, 1, 0, True, 96)])   # negative deltas
    ys = [9, 10, 99, 100, 999, 1000, 9999, 10_000, 99_999, 100_000, 999_999, 1_000_000]
    xs = [9, 10, 99, 100, 99_999, 100_000, 9_999_999, 10_000_000, 999_999_999, 1_000_000_000, (1 << 30) - 1 - 96, (1 << 30) - 1 - 96]
    B.read([(x, y, 0, 0, False, 0 if i >= 10 else 1) for i, (x, y) in enumerate(zip(xs, ys))], L=1_000_000)      # every decimal digit border
    B.read([((1 << 30) - 1, 0, 0, 2, True, 0)], L=1_048_575)
    B.read(run(3, y0=0), L=250)                                # leading clip 0; L smaller than r_end (205 + 96 + 96)
    r = run(3)
    B.read(r, L=r[-1][1] + 96)                                 # trailing clip 0
    B.read(r, L=r[-1][1] + 97)                                 # trailing clip 1
    B.read(run(2, gid=5) + run(2, x0=90_000, y0=4000, gid=3))  # sequence ids beyond the genome list: '*'
    B.read(run(2), rid="q")
    B.read(run(70), rid="I" * 300)
    for X in (201, 7999):                                      # preset 1 splits large diagonal shifts: |DI| / 80 exact and one off
        for DI in (160, 240, 8000, 161, 81):
            for sign in (1, -1):                               # shift in x, shift in y
                x, y, w = 20_000, 30, 96
                B.read([(x, y, 0, 0, False, w), (x + w + X + (DI if sign > 0 else 0), y + w + X + (DI if sign < 0 else 0), 0, 0, False, w)])
    B.read([(3000, 40, 0, 0, False, 192), (3100, 140, 0, 0, False, 192), (3200, 240, 0, 0, False, 192)])          # overlapping cords on one diagonal: '=' merges
    B.read(run(3000, step=100, w=96))                          # text 1000x that of its neighbours
    B.read(run(1))
    B.read(many_records(70), rid=MANY)                         # 70 records: a second tile of records that starts at record 64; some 150 kB of SA tags, so heads straddle
    B.read(run(2))                                             # window edges and tails lie windows behind their heads (counted in tests/test_output_seq_cpu.py)
    return B.arrays()


def one_read():
    return Batch().read(blocks([[0, 0], [1]])).arrays()


def empty():
    return Batch().arrays()


def sam_body(sam: bytes) -> bytes:
    lines = sam.split(b"\n")
    k = 0
    while k < len(lines) and lines[k].startswith(b"@"):
        k += 1
    return b"\n".join(lines[k:])
