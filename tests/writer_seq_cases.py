"""Inputs shared by the tests of the SAM writer's SEQ column (tests/test_output_seq_cpu.py on the host, tests/test_gpu_writer_seq.py on the
device): a small seeded genome, reads with runs of N and a few bytes that are no Dna5 ordinal, and cords built with writer_cases.Batch that
hold the smallest shapes at which a wave-cooperative SEQ writer can go wrong.  The host writer lnr_writer_format_seq is the reference."""
import numpy as np

from tests import writer_cases as wc

GIDS = wc.GIDS
GLEN = [70_000, 9, 3_000]
OUT_WIN = 8192            # bytes of LDS window per wave in linear_amd/csrc/lnr_output_kernels.hip
SEQ_LENS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, OUT_WIN - 1, OUT_WIN, OUT_WIN + 1, 200_000]


def genome():
    rng = np.random.default_rng(20260)
    g = [rng.integers(0, 4, n).astype(np.uint8) for n in GLEN]
    g[0][2100:2110] = 4                    # a run of N inside the X stretch of x_pair()
    g[0][40_000:40_003] = 4
    g[2][5] = 4
    return g


def revcomp(a):
    a = np.asarray(a, np.uint8)[::-1]
    return np.where(a > 3, 4, 3 - np.minimum(a, 3)).astype(np.uint8)


def x_pair(strand, x=2000, y=10):
    """two cords on one diagonal, 100 bases apart: =96 X100 =96"""
    return [(x, y, strand, 0, False, 96), (x + 196, y + 196, strand, 0, False, 96)]


def build():
    """(cord_off, cords_str, cords_end, reads, read_off, ids)"""
    B = wc.Batch()
    plant = {}                                                  # read index -> (y, x, n): the read equals the genome there
    B.read([(500, 0, 0, 0, False, 0)], L=0, rid="empty")         # CIGAR '*', SEQ '*'
    k = 0
    for L in SEQ_LENS:
        for strand in (0, 1):
            cord = (300 + L % 1000, 0, strand, 0, False, 0) if L <= 3 else (300 + L % 1000, 1, strand, 0, False, min(L // 2, 96))
            B.read([cord], L=L, rid="abcd"[:1 + k % 4])          # qnames of 1 .. 4 bytes: SEQ starts at every address mod 4
            k += 1
    for q in range(4):
        B.read([(700, 2, q & 1, 2, False, 40)], L=66, rid="wxyz"[:q + 1])       # even L, both strands, the third sequence
    B.read([(1000, 10, 0, 0, False, 96), (1050, 40, 0, 0, False, 96)])           # =30 D20
    B.read([(1000, 10, 1, 0, False, 96), (1030, 60, 1, 0, False, 96)])           # =30 I20, reverse
    for strand in (0, 1):
        B.read(x_pair(strand))                                  # X over random bases: about 3 in 4 differ
        plant[len(B.rl)] = (106, 2096, 100)
        B.read(x_pair(strand))                                  # X where the read IS the genome: N
    B.read(x_pair(0, x=69_900, y=20))                           # runs past the end of the first sequence
    B.read([(4, 3, 0, 1, False, 9)])                            # past the end of the 9-base sequence
    coff, cs, ce, rl, ids = B.arrays()
    s_off, s_cs, s_ce, s_rl, s_ids = wc.synthetic()             # tiles of 130 cords, 3 000 cords (the segment table refills; x runs beyond glen), 3 and 5 records with
    coff = np.concatenate([coff, s_off[1:] + coff[-1]])         # SA:Z, preset-1 splits, ids beyond the list, a cord end beyond L, no cords at all
    cs, ce, rl, ids = np.concatenate([cs, s_cs]), np.concatenate([ce, s_ce]), np.concatenate([rl, s_rl]), ids + s_ids
    rng = np.random.default_rng(7)
    off = np.zeros(rl.size + 1, np.uint64)
    off[1:] = np.cumsum(rl)
    reads = rng.integers(0, 4, int(off[-1])).astype(np.uint8)
    g = genome()
    for i in range(rl.size):
        a, L = int(off[i]), int(rl[i])
        if L >= 20:
            reads[a + L // 3:a + L // 3 + 5] = 4                # a run of N
        if L >= 10 and i % 5 == 0:
            reads[a + 7], reads[a + L - 2] = 9, 200             # no Dna5 ordinals: print as N
        if i in plant:
            y, x, n = plant[i]
            fwd = g[0][x:x + n]
            if (int(cs[int(coff[i]) + 1]) >> 61) & 1:           # reverse strand: y counts along the reverse complement
                reads[a + L - y - n:a + L - y] = revcomp(fwd)
            else:
                reads[a + y:a + y + n] = fwd
    return coff, cs, ce, reads, off, ids


_cache = {}


def synthetic():
    if "s" not in _cache:
        _cache["s"] = build()
    return _cache["s"]


def one_read():
    B = wc.Batch().read(wc.blocks([[0, 0], [1]], x0=1000, gid=0))
    coff, cs, ce, rl, ids = B.arrays()
    reads = np.random.default_rng(3).integers(0, 5, int(rl[0])).astype(np.uint8)
    return coff, cs, ce, reads, np.array([0, rl[0]], np.uint64), ids


def empty():
    coff, cs, ce, _, ids = wc.Batch().arrays()
    return coff, cs, ce, np.zeros(0, np.uint8), np.zeros(1, np.uint64), ids


def star_seq(sam: bytes) -> bytes:
    """the text with column 10 put back to '*'"""
    out = []
    for l in sam.split(b"\n"):
        if l and not l.startswith(b"@"):
            f = l.split(b"\t")
            f[9] = b"*"
            l = b"\t".join(f)
        out.append(l)
    return b"\n".join(out)


def seq_len_of_cigar(cigar: bytes) -> int:
    import re
    return sum(int(n) for n, op in re.findall(rb"(\d+)([SI=XD])", cigar) if op != b"D")
