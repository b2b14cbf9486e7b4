"""Seeded reference families that aim at the layout and bucket edges of the index build (tests/test_index_layouts_cpu.py,
tests/test_gpu_index_layouts.py, tools/make_index_golden.py).  numpy only, a few hundred kilobases each; like tests/cases.py the inputs
are regenerated from their seeds wherever they are needed.

  frag     many contigs, down to lengths that have no chunk, no feature entry or empty chunks, at wide -t layouts
  nrun     N runs laid against every chunk border of one sequence, up to runs that swallow whole chunks
  planted  bucket lengths planted on the thresholds of the build and of the seed kernel's bucket view
"""
from __future__ import annotations

import numpy as np

from linear_amd import synth
from tests.cases import sha

# ---- frag: fragmented references
N_MAX = 1023          # the most sequences lnr_index_build accepts (the cord's id field; the reference refuses 1024 as well)
# lengths under 42 (no chunk at any -t), under 48 (no f2 entry), under 42 * 3 (empty chunks at -t 3): they replace the drawn length of
# the first random contigs of frag_max
SHORT = (22, 30, 41, 42, 43, 47, 48, 49, 63, 64, 83, 84, 125, 126, 127)
FRAG = {
    # name: (seed, contigs, lo, hi, short lengths, [-t layouts])
    "frag200": (1, 200, 300, 6000, (), [1, 7, 16, 64]),
    "frag40": (2, 40, 5000, 40000, (), [16, 32]),
    "frag_max": (3, N_MAX, 50, 900, SHORT, [3]),
    # contigs long enough for many_reads to map on (reads of frag_max are cut to their contig: a third of them is too short for a cord)
    "frag_map": (5, N_MAX, 300, 4000, (), [1, 16]),
}
FRAG_I2 = [("frag200", 16), ("frag40", 16)]      # -i 2 layouts
READ_SETS = ["frag_max", "frag200", "frag_map"]             # many_reads are mapped on these


def frag(seed: int, n: int, lo: int, hi: int, short=()) -> list[np.ndarray]:
    """n contigs with lengths uniform in [lo, hi): every third one cut from a repeat-rich sequence of at least 20 kb, the others random;
    every second contig longer than 400 bases gets a leading N run shorter than L/4, a trailing one shorter than L/5 and one inside.
    `short`: lengths given to the first random contigs instead of their drawn ones."""
    rng = np.random.default_rng(seed)
    short = list(short)
    out = []
    for i in range(n):
        L = int(rng.integers(lo, hi))
        if i % 3 and short:
            L = short.pop(0)
        r = synth.random_ref(L, seed * 1000 + i) if i % 3 else synth.repeat_ref(max(L, 20000), seed * 1000 + i)[:L]
        r = r.copy()
        if i % 2 == 0 and L > 400:
            a = int(rng.integers(1, max(2, L // 4)))
            r[:a] = 4
            b = int(rng.integers(1, max(2, L // 5)))
            r[L - b:] = 4
            m = int(rng.integers(L // 3, L // 2))
            r[m:m + int(rng.integers(1, L // 6))] = 4
        out.append(np.ascontiguousarray(r))
    return out


_frag_cache = {}


def frag_refs(name: str) -> list[np.ndarray]:
    if name not in _frag_cache:
        seed, n, lo, hi, short, _ = FRAG[name]
        _frag_cache[name] = frag(seed, n, lo, hi, short)
    return _frag_cache[name]


def many_reads(refs: list[np.ndarray], seed: int = 77):
    """300 reads of 1500 +- 60 % bases (never more than their contig) at 8 % errors, both strands: (bases, off)."""
    reads, off, _ = synth.sample_reads(refs, 300, 1500, 0.08, seed, "random", len_jitter=0.6)
    return reads, off


# ---- nrun: N runs against chunk borders
NRUN_T = 8
NRUN_LEN = 36 * 8 * 700       # 201 600 bases: chunks of 25 200
NRUN_LEADS = (0, 1, 20, 21, 22, 63, 64, 65, 16363, 16364, 16384, 16385, 16405, 25157, 25158, 25200, 25221, 33000)
NRUN_EMPTY = (25221, 33000)   # these runs swallow every chunk: hs_len = 0
NRUN_I2 = (21, 16384, 25157, 25158, 25200, 25221, 33000)   # from 25157 on fewer than three repeated minimizers are left: the reference gives its last block up
_nrun_base = []


def nrun(lead: int) -> np.ndarray:
    """One sequence of NRUN_LEN bases whose eight chunks each get an N run of `lead` bases that starts 0, 1, 20 or 21 bases in front of
    the chunk's first position (chunk border + 21; the offsets rotate over the chunks); for odd `lead` the last 3000 bases are N too.
    The runs end 20 or 21 bases short of a 64-position segment of the N-skip search, on its 16 384-position tile, past the chunk."""
    if not _nrun_base:
        _nrun_base.append(synth.random_ref(NRUN_LEN, 4))
    ref = _nrun_base[0].copy()
    for t in range(NRUN_T):
        s = NRUN_LEN // NRUN_T * t + 21
        d = (0, 1, 20, 21)[t % 4]
        ref[max(s - d, 0): max(s - d + lead, 0)] = 4
    if lead % 2:
        ref[NRUN_LEN - 3000:] = 4
    return ref


def nrun_reads(seed: int = 78):
    """20 reads of 1500 bases at 5 % errors from the family's sequence without its runs."""
    nrun(0)
    reads, off, _ = synth.sample_reads([_nrun_base[0]], 20, 1500, 0.05, seed, "random")
    return reads, off


# ---- planted: bucket lengths on the thresholds
# 1 | 2 a bucket that needs no sort; 15 | 16 the end of the inline bucket line (BL_INLINE); 16 | 17, 31 | 32, 47 | 48, 63 | 64 the borders of
# the 16-entry overflow lines; 32 | 33 insertion sort | bitonic sort; 64 lines per LDS round of the seed kernel; 400 | 401 kept | emptied
COUNTS = (1, 2, 14, 15, 16, 17, 30, 31, 32, 33, 34, 47, 48, 63, 64, 65, 128, 256, 399, 400, 401, 450)
PLANTED_T = (1, 4)
PLANTED_SEED = 77
UNIT, SLOT, FIRST = 90, 117, 900


def planted(seed: int = PLANTED_SEED) -> np.ndarray:
    """A random sequence (length a multiple of 288, so that the chunks of -t 4 sample in the phase of -t 1) in which unit i of twenty-two
    random 90-base units stands COUNTS[i] times, the copies at FIRST + SLOT * slot with the slots shuffled.  FIRST and SLOT are multiples
    of the sampling stride 9: every copy of a unit meets the sample grid in the same phase, so each of its minimizers collects one entry
    per copy."""
    rng = np.random.default_rng(seed)
    n_slots = sum(COUNTS)
    L = ((n_slots * SLOT + 5000) // 288 + 1) * 288
    ref = rng.integers(0, 4, L, dtype=np.uint8)
    units = [rng.integers(0, 4, UNIT, dtype=np.uint8) for _ in COUNTS]
    order = np.concatenate([np.full(c, i) for i, c in enumerate(COUNTS)])
    rng.shuffle(order)
    for s, u in enumerate(order):
        p = FIRST + s * SLOT
        ref[p:p + UNIT] = units[u]
    return ref


def planted_reads(ref: np.ndarray, seed: int = 79):
    """Error-free 3 kb windows of `ref` every 1499 bases, then the same windows at 5 % errors; every second read reverse-complemented."""
    rng = np.random.default_rng(seed)
    wins = [ref[s:s + 3000] for s in range(0, ref.size - 3000, 1499)]
    lst = [w.copy() for w in wins] + [synth.mutate(w, 0.05, rng) for w in wins]
    lst = [synth.revcomp(r) if k & 1 else r for k, r in enumerate(lst)]
    return synth.pack_reads(lst)


def config_key(name: str, T: int, index_type: int = 1) -> str:
    """Key prefix of a configuration in tests/golden/index_layouts.npz."""
    return f"{name}_T{T}" + ("_i2" if index_type == 2 else "")


def index_digests(chk, nseq: int, index_type: int) -> dict:
    """The digests of one configuration from a checker (the reference in tools/make_index_golden.py; the oracle and the host shim in the tests)."""
    d = {}
    if index_type == 2:
        ysa = chk.ysa()
        d["hs_len"], d["ysa_sha"] = ysa.size, sha(ysa)
    else:
        hs = chk.hs()
        d["hs_len"], d["dir_sha"], d["hs_sha"] = hs.size, sha(chk.dir()), sha(hs)
        f2 = [chk.f2(k) for k in range(nseq)]
        d["f2_len"] = np.array([f.shape[0] for f in f2], np.int64)
        d["f2_sha"] = sha(np.concatenate([f[:-1] for f in f2]))
    return d


def all_configs():
    """(key, builder of the sequences, T, index_type) of every configuration."""
    out = []
    for name, (_, _, _, _, _, Ts) in FRAG.items():
        for T in Ts:
            out.append((config_key(name, T), (lambda n=name: frag_refs(n)), T, 1))
    for name, T in FRAG_I2:
        out.append((config_key(name, T, 2), (lambda n=name: frag_refs(n)), T, 2))
    for lead in NRUN_LEADS:
        out.append((config_key(f"nrun{lead}", NRUN_T), (lambda l=lead: [nrun(l)]), NRUN_T, 1))
        out.append((config_key(f"nrun{lead}", NRUN_T, 2), (lambda l=lead: [nrun(l)]), NRUN_T, 2))
    for T in PLANTED_T:
        out.append((config_key("planted", T), (lambda: [planted()]), T, 1))
    return out
