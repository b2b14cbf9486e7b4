"""GPU (-m gpu): a read's cords must not depend on where the read sits in its batch, on the batch's size, on what lies around the
batch in host memory or on what the context ran before -- and, while the gap re-mapper's stream state is still 0, on how the batch
falls onto the chunks of the probe ladder (lnr_gap_stage.h gap_stage: 256, 1 024, 4 096 ... reads).  The oracle is the checker
throughout (pinned to the real program by tests/test_oracle_golden.py); every value is an integer word, so every comparison is exact,
and no read is left out of one."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stress_parity  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = [(50, 1), (50, 0), (0, 0)]                     # (-g, -dup)
MODE_IDS = ["g50dup1", "g50", "g0"]


def make_filter(gap_len=0, dup=0):
    from linear_amd import build as lb
    lb.build()
    from linear_amd import Filter
    return Filter(device=0, gap_len=gap_len, dup=dup)


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


# ------------------------------------------------------------------------------------------- B. the recorded stress finding
def test_gpu_stress_gap_seed31415926_cfg87(oracle_lib, monkeypatch):
    """Configuration 87 of `LNR_STRESS_GAP=1 tools/stress_parity.py 120 31415926` (profiles/r03/stress_gap_120cfg_seed31415926.log:88-89):
    1 500 reads of 20 kb on three sequences, -t 4, LNR_JOB_LDS_KB=1, -g 50 -dup 1.  The recorded run had the last cord of the last read
    x + 9 / y + 5 off the oracle."""
    c = list(stress_parity.configs(31415926, 88, True))[87]
    assert (c.kind, c.T, c.L, c.nreads, c.opt, c.gap_len, c.dup) == (2, 4, 20000, 1500, {"LNR_JOB_LDS_KB": "1"}, 50, 1)
    refs, reads, off = c.build()
    o = oracle_lib.Checker("oracle", refs, c.T)
    want = split(*o.map_batch(reads, off, threads=8, gap_len=50, dup=1)[:3])
    o.close()
    assert sum(w[0].size for w in want) == 491890
    monkeypatch.setenv("LNR_JOB_LDS_KB", "1")
    f = make_filter(50, 1)
    try:
        f.build_index(refs, c.T)
        got = split(*f.filter_batch(reads, off))
    finally:
        f.close()
    d = differing(got, want)
    for i in d[:8]:
        k = [j for j in range(min(got[i][0].size, want[i][0].size)) if got[i][0][j] != want[i][0][j] or got[i][1][j] != want[i][1][j]]
        print(f"read {i}: {got[i][0].size} cords against the oracle's {want[i][0].size}, cords that differ {k[:8]}")
    assert not d, f"reads that differ from the oracle: {d[:20]} ({len(d)} of {len(want)})"


# ------------------------------------------------------------------------------------------- C. slot invariance (stream state 1)
class Pool:
    pass


@pytest.fixture(scope="module")
def pool(oracle_lib):
    """~300 reads on the stress tool's kind-2 references (three sequences, one with N runs): lengths 201 .. ~20 000, a third with a planted
    SV, a few N-heavy, one of at most 200 bases, one empty; the oracle's cords of every read in every mode, computed once (stream state 1:
    a read's cords depend on the read alone)."""
    from linear_amd import synth
    s = 870187
    refs = [synth.repeat_ref(400_000, s), synth.add_n_runs(synth.random_ref(250_000, s + 1), s + 2, lead=1234), synth.repeat_ref(150_000, s + 3, n_families=4)]
    rl = []
    for q, (cnt, L, err) in enumerate([(70, 330, 0.03), (70, 900, 0.1), (70, 3000, 0.1), (48, 8000, 0.15), (32, 15000, 0.1)]):
        reads, off, _ = synth.sample_reads(refs, cnt, L, err, s + 10 + q, "random", len_jitter=0.4)
        rl += [reads[int(off[i]):int(off[i + 1])] for i in range(cnt)]
    rl.append(synth.sample_reads(refs, 1, 20000, 0.1, s + 20, "random")[0])
    rl += [synth.sample_reads([refs[0]], 1, 201, 0.03, s + 21, "none")[0][:201], synth.sample_reads([refs[2]], 1, 202, 0.0, s + 22, "none")[0][:202]]
    order = np.random.default_rng(s + 30).permutation(len(rl))
    reads, off = pack([rl[int(i)] for i in order])
    reads, off = stress_parity.plant_svs(reads, off, refs, np.random.default_rng(s + 31))
    rl = [reads[int(off[i]):int(off[i + 1])].copy() for i in range(off.size - 1)]
    rl.insert(77, rl[3][:150].copy())                        # at most 200 bases: no cords
    rl.insert(190, np.zeros(0, np.uint8))                    # empty
    rng = np.random.default_rng(s + 32)
    n_heavy = []
    for i in (5, 50, 120, 200):                               # N-heavy: a third of the read in N runs / one long run
        r = rl[i]
        if i % 2:
            r[r.size // 3: 2 * r.size // 3] = 4
        else:
            r[rng.random(r.size) < 0.3] = 4
        n_heavy.append(i)
    P = Pool()
    P.refs, P.T, P.reads = refs, 3, rl
    P.n = len(rl)
    lens = [r.size for r in rl]
    assert 290 <= P.n <= 310 and min(lens) == 0 and 201 in lens and max(lens) >= 19000 and sum(1 for x in lens if 0 < x <= 200) == 1
    o = oracle_lib.Checker("oracle", refs, P.T)
    reads, off = pack(rl)
    P.want = {}
    for g, d in MODES:
        P.want[(g, d)] = split(*o.map_batch(reads, off, threads=8, gap_len=g, dup=d, ext=1)[:3])
    # the checker's own premise, once: in state 1 a read's cords do not depend on its neighbours
    rr, ro = pack(rl[::-1])
    assert not differing(split(*o.map_batch(rr, ro, threads=8, gap_len=50, dup=1, ext=1)[:3]), P.want[(50, 1)][::-1])
    o.close()
    ncord = [w[0].size for w in P.want[(50, 1)]]
    P.heaviest = int(np.argmax(ncord))
    P.shortest = 190                                         # the empty read
    P.shortest_mapped = lens.index(201)
    P.n_heavy = n_heavy
    assert sum(1 for w, v in zip(P.want[(50, 1)], P.want[(0, 0)]) if not np.array_equal(w[0], v[0])) > 30, "the gap re-mapper changes too few reads of the pool"
    assert differing(P.want[(50, 1)], P.want[(50, 0)]), "-dup 1 changes no read of the pool"
    return P


class Ctx:
    """fresh: a new context for every batch; reused: one context for the whole module (buffers only grow: a smaller batch runs in front of
    stale bytes, and the context changes -g / -dup between calls)"""

    def __init__(self, pool, reused):
        self.pool, self.reused, self.f = pool, reused, None

    def get(self, mode):
        if self.reused is not None:
            f = self.reused
            f.set_gap(*mode)
        else:
            self.done()
            f = self.f = make_filter(*mode)
            f.build_index(self.pool.refs, self.pool.T)
        if mode[0]:
            assert f.gap_stream(1) == 1
        return f

    def run(self, mode, idx, keep=False):
        """the reads idx of the pool as one batch -> the positions that differ from the oracle"""
        f = self.f if keep and self.f is not None else self.get(mode)
        if keep and mode[0]:
            f.gap_stream(1)
        reads, off = pack([self.pool.reads[i] for i in idx])
        got = split(*f.filter_batch(reads, off))
        if mode[0]:
            assert f.gap_stream() == 1
        return got, differing(got, [self.pool.want[mode][i] for i in idx])

    def done(self):
        if self.f is not None and self.reused is None:
            self.f.close()
        self.f = None


@pytest.fixture(scope="module")
def reused_filter(pool):
    f = make_filter(50, 1)
    f.build_index(pool.refs, pool.T)
    yield f
    f.close()


@pytest.fixture(params=["fresh", "reused"])
def ctx(request, pool, reused_filter):
    c = Ctx(pool, reused_filter if request.param == "reused" else None)
    yield c
    c.done()


def rotations(P):
    n = P.n
    rot = lambda k: [(i + k) % n for i in range(n)]         # noqa: E731  (pool read k lands in slot 0, read k - 1 in slot n - 1)
    return {"in order": list(range(n)), "reversed": list(range(n))[::-1], "heaviest first": rot(P.heaviest), "heaviest last": rot(P.heaviest + 1),
            "shortest first": rot(P.shortest), "shortest last": rot(P.shortest + 1), "201 bases last": rot(P.shortest_mapped + 1), "by 97": rot(97)}


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gpu_cords_do_not_depend_on_the_slot(pool, ctx, mode):
    bad = {}
    for name, idx in rotations(pool).items():
        assert sorted(idx) == list(range(pool.n))
        _, d = ctx.run(mode, idx)
        if d:
            bad[name] = [(p, idx[p]) for p in d[:10]]
    assert not bad, f"(slot, pool read) that differ from the oracle: {bad}"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gpu_copies_of_the_last_read_agree(pool, ctx, mode):
    for last in (pool.heaviest, pool.n_heavy[0], 11):
        idx = [i for i in range(pool.n) if i != last]
        idx.insert(100, last)
        idx.insert(200, last)
        idx.append(last)
        got, d = ctx.run(mode, idx)
        assert not d, f"slots that differ from the oracle: {d[:10]} (the read {last} sits in 100, 200 and {len(idx) - 1})"
        assert not differing([got[100], got[200]], [got[-1], got[-1]])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gpu_a_read_alone(pool, ctx, mode):
    """(on the parent commit this met a GPU memory fault: a single read that a single wave hands over to a team made the team look one entry
    past the zeroed part of the hand-over queue)"""
    alone = sorted({pool.heaviest, pool.shortest, pool.shortest_mapped, 77, pool.n - 1, 0, *pool.n_heavy} | set(range(3, pool.n, 29)))[:20]
    assert len(alone) == 20
    bad = [i for i in alone if ctx.run(mode, [i])[1]]
    assert not bad, f"pool reads that differ from the oracle when filtered alone: {bad}"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gpu_bytes_around_the_batch_do_not_matter(pool, ctx, mode):
    """the batch as a window of a larger host array (off[0] > 0), the bytes in front of and behind it filled with 0, random bases, 4 and 200;
    from pageable memory and from a pinned block that ends with the batch"""
    idx = sorted({pool.heaviest, pool.shortest, 77, *pool.n_heavy} | set(range(0, pool.n, 7)))
    idx.append(pool.shortest_mapped)
    idx.append(idx.pop(idx.index(pool.heaviest)))           # the heaviest read ends the window
    reads, off = pack([pool.reads[i] for i in idx])
    want = [pool.want[mode][i] for i in idx]
    front, behind = 4099, 70001
    rng = np.random.default_rng(5)
    f = ctx.get(mode)
    pinned = f.host_alloc(front + reads.size)
    bad = {}
    for fill in ("0", "bases", "4", "200"):
        big = np.empty(front + reads.size + behind, np.uint8)
        big[:] = rng.integers(0, 4, big.size, dtype=np.uint8) if fill == "bases" else int(fill)
        big[front:front + reads.size] = reads
        pinned[:front] = big[:front]
        pinned[front:] = reads
        for kind, buf in (("pageable", big), ("pinned", pinned)):
            if mode[0]:
                f.gap_stream(1)
            d = differing(split(*f.filter_batch(buf, off + np.uint64(front))), want)
            if d:
                bad[(fill, kind)] = d[:10]
    assert not bad, f"slots that differ from the oracle: {bad}"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gpu_a_small_batch_between_two_large_ones(pool, ctx, mode):
    for k, idx in enumerate([list(range(pool.n)), list(range(7)), list(range(pool.n))]):
        _, d = ctx.run(mode, idx, keep=k > 0)
        assert not d, f"batch {k} of full / 7 reads / full: slots that differ from the oracle: {d[:10]}"


# ------------------------------------------------------------------------------------------- D. the probe ladder's borders (stream state 0)
LADDER = [(255, 0), (255, 254), (256, 255), (256, None), (257, 255), (257, 256), (1279, 256), (1279, 257), (1279, 1278), (1280, 1279), (1281, 1279),
          (1281, 1280), (1281, None), (1400, 0), (1400, 255), (1400, 1280), (1400, 1399), (1400, None)]


@pytest.fixture(scope="module")
def short_pool(oracle_lib):
    """cheap reads of 700 .. 3 000 bases, sorted by the oracle read by read (-g 50 -dup 1, stream state 0) into those that extend a gap --
    the stream is "extended" behind them -- and those that do not; `moved`: reads whose cords depend on the state they start from, which is
    what makes a wrong border visible"""
    from linear_amd import synth
    s = 550155
    refs = [synth.repeat_ref(400_000, s), synth.add_n_runs(synth.random_ref(250_000, s + 1), s + 2, lead=777), synth.repeat_ref(150_000, s + 3, n_families=4)]
    reads, off, _ = synth.sample_reads(refs, 2600, 1850, 0.1, s + 4, "random", len_jitter=0.6)
    reads, off = stress_parity.plant_svs(reads, off, refs, np.random.default_rng(s + 5))
    o = oracle_lib.Checker("oracle", refs, 2)
    P = Pool()
    P.refs, P.T, P.o = refs, 2, o
    P.ext, P.plain, P.moved_plain, P.moved_ext = [], [], [], []
    for i in range(off.size - 1):
        r = reads[int(off[i]):int(off[i + 1])].copy()
        if not 700 <= r.size <= 3000:
            continue
        a = o.map_read_gap(r, 50, 1, ext=0)
        e = o.ext_out
        if a[0].size <= 1:
            continue
        b = o.map_read_gap(r, 50, 1, ext=1)
        moved = not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
        (P.ext if e else P.plain).append(r)
        if moved:
            (P.moved_ext if e else P.moved_plain).append(r)
    assert len(P.plain) >= 1400 and len(P.ext) >= 40, (len(P.plain), len(P.ext))
    assert len(P.moved_plain) >= 4, "no read that does not extend has cords that depend on the stream state: a wrong border would go unseen"
    yield P
    o.close()


def ladder_batch(P, n, first):
    """n reads whose first extending one sits at `first` (None: nobody extends); reads that depend on the state sit on both sides of it and
    on both sides of the chunk borders, extending and plain reads follow it in turns"""
    mp, pl, ex = P.moved_plain, P.plain, P.ext
    out = [pl[i % len(pl)] for i in range(n)]
    for q, p in enumerate(sorted({0, 1, 254, 255, 256, 257, 1278, 1279, 1280, 1281, n - 2, n - 1} | ({first - 2, first - 1, first + 1, first + 2, first + 3} if first is not None else set()))):
        if 0 <= p < n:
            out[p] = mp[q % len(mp)]
    if first is not None:
        for q, p in enumerate(range(first, n, 5)):
            out[p] = ex[q % len(ex)]
    return out


@pytest.fixture(scope="module")
def ladder_filter(short_pool):
    f = make_filter(50, 1)
    f.build_index(short_pool.refs, short_pool.T)
    yield f
    f.close()


@pytest.mark.parametrize("n,first", LADDER)
def test_gpu_probe_ladder_borders(short_pool, ladder_filter, n, first):
    P, f, o = short_pool, ladder_filter, short_pool.o
    rl = ladder_batch(P, n, first)
    reads, off = pack(rl)
    want = split(*o.map_batch(reads, off, threads=8, gap_len=50, dup=1, ext=0)[:3])
    state_out = o.ext_out
    # the layout is what it is meant to be, by the oracle's own per-read states
    states = []
    for r in rl[: n if first is None else first + 1]:
        o.map_read_gap(r, 50, 1, ext=0)
        states.append(o.ext_out)
    assert (states.index(1) if 1 in states else None) == first and state_out == (first is not None)
    if first is not None and first + 1 < n:                  # the read behind the border shows the border: its cords differ between the states
        a, b = o.map_read_gap(rl[first + 1], 50, 1, ext=0), o.map_read_gap(rl[first + 1], 50, 1, ext=1)
        assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    assert f.gap_stream(0) == 0
    d = differing(split(*f.filter_batch(reads, off)), want)
    assert not d, f"slots that differ from the oracle: {d[:20]} ({len(d)} of {n})"
    assert f.gap_stream() == state_out
    # the same stream in three calls: cut just before, on and just after the first extending read
    p = n // 2 if first is None else first
    for a, b in ((p - 1, p), (p, p + 1), (p + 1, p + 2)):
        cuts = [0] + [c for c in (a, b) if 0 < c < n] + [n]
        assert f.gap_stream(0) == 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            r2, o2 = pack(rl[lo:hi])
            d = differing(split(*f.filter_batch(r2, o2)), want[lo:hi])
            assert not d, f"cuts {cuts}, call [{lo}, {hi}): slots that differ from the oracle: {[lo + i for i in d[:20]]}"
            assert f.gap_stream() == int(first is not None and first < hi), f"cuts {cuts}, stream state after [{lo}, {hi})"
