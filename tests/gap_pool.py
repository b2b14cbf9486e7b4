"""The inputs of the gap re-mapper's worker tests (tests/test_gap_workers_cpu.py, tests/test_gpu_gap_workers.py, tests/test_gpu_gap_variants.py):
about 40 reads on one reference of 400 kb, most of them ordinary, a dozen across an expanded tandem array (linear_amd.synth
tandem_expansion_read): the gap between the flanks joins every reference copy against every read copy."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEED = 20261
# (unit length, copies in the reference, copies in the read, divergence between copies, sequencing error, flanks)
ARRAYS = [(42, 203, 609, 0.02, 0.05, (2000, 2500)), (20, 263, 798, 0.02, 0.05, (2526, 2845)), (21, 268, 671, 0.02, 0.05, (2919, 2053)),
          (20, 416, 1048, 0.02, 0.05, (2463, 2682)), (22, 254, 700, 0.02, 0.05, (2000, 2500)), (160, 52, 156, 0.02, 0.05, (2000, 2000)),
          (21, 406, 1374, 0.02, 0.05, (2868, 1507)), (32, 260, 780, 0.02, 0.05, (2000, 2500)), (20, 400, 1100, 0.02, 0.05, (1560, 1660)),
          (58, 147, 441, 0.02, 0.05, (3000, 1500)), (20, 300, 900, 0.02, 0.05, (2724, 1954)), (100, 84, 252, 0.04, 0.10, (3000, 3000)),
          (20, 410, 1050, 0.02, 0.05, (2769, 1513)), (21, 400, 1350, 0.02, 0.05, (1894, 2961))]
MODES = [(50, 1), (50, 0)]            # (-g, -dup)
MODE_IDS = ["g50dup1", "g50"]


class Pool:
    pass


def pack(read_list):
    off = np.zeros(len(read_list) + 1, np.uint64)
    off[1:] = np.cumsum([r.size for r in read_list])
    return (np.concatenate(read_list) if read_list and int(off[-1]) else np.zeros(0, np.uint8)), off


def split(coff, cs, ce):
    return [(cs[int(coff[i]):int(coff[i + 1])], ce[int(coff[i]):int(coff[i + 1])]) for i in range(coff.size - 1)]


def differing(got, want):
    """positions of the batch whose cords differ"""
    assert len(got) == len(want)
    return [i for i, (g, w) in enumerate(zip(got, want)) if not (np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]))]


def plant(ref, arrays, start=12_000, apart=9_000):
    """the arrays into ref, `apart` bases from one another -> the tandem-expansion reads.  Each array and its read come from a generator of
    their own (SEED and the array's line), so that a line added or taken out leaves the other reads as they were"""
    from linear_amd import synth
    heavy, pos = [], start
    for k, (u, c, cr, div, err, flank) in enumerate(arrays):
        rng = np.random.default_rng([SEED, u, c, cr, int(div * 1000), int(err * 1000), flank[0], flank[1]])
        unit = rng.integers(0, 4, size=u, dtype=np.uint8)
        arr = synth.tandem_array(unit, c, div, rng)
        ref[pos:pos + arr.size] = arr
        heavy.append(synth.tandem_expansion_read(ref, pos, arr.size, unit, cr, div, flank, err, rng, rc=bool(k % 3 == 2)))
        pos += arr.size + apart
    assert pos < ref.size - 60_000
    return heavy


def make_pool():
    """refs, T, reads, tandem: the positions of the tandem-expansion reads in the pool"""
    from linear_amd import synth
    import stress_parity
    ref = synth.random_ref(400_000, SEED + 1)
    heavy = plant(ref, ARRAYS)
    reads, off, _ = synth.sample_reads([ref], 28, 3500, 0.1, SEED + 2, "random", len_jitter=0.7)
    reads, off = stress_parity.plant_svs(reads, off, [ref], np.random.default_rng(SEED + 3))
    rl = [reads[int(off[i]):int(off[i + 1])].copy() for i in range(off.size - 1)]
    P = Pool()
    P.tandem = [2 + 3 * k for k in range(len(heavy))]         # spread over the pool
    for i, r in zip(P.tandem, heavy):
        rl.insert(i, r)
    rl.append(rl[5][:180].copy())                            # at most 200 bases: no cords, no weight
    P.refs, P.T, P.reads, P.n = [ref], 2, rl, len(rl)
    return P


def oracle_cords(oracle_lib, P):
    """the oracle's cords of every read in MODES, stream state 1 (a read's cords then depend on the read alone -- checked here, once)"""
    o = oracle_lib.Checker("oracle", P.refs, P.T)
    reads, off = pack(P.reads)
    want = {m: split(*o.map_batch(reads, off, threads=8, gap_len=m[0], dup=m[1], ext=1)[:3]) for m in MODES}
    plain = split(*o.map_batch(reads, off, threads=8)[:3])
    rr, ro = pack(P.reads[::-1])
    for m in MODES:
        assert not differing(split(*o.map_batch(rr, ro, threads=8, gap_len=m[0], dup=m[1], ext=1)[:3]), want[m][::-1]), "the oracle itself depends on the slot"
    o.close()
    return want, plain
