"""GPU (-m gpu): reads of 40 kb to 2^20 - 1 bases -- the length limit of the cord format -- on every GPU path, bit for bit against the
oracle (pinned to the reference on these lengths by tests/test_oracle_golden.py and the `long` goldens).  Everything sized by the read
length is reached with the stock build: the workgroup sorts and the dealt chaining DP of the job kernels (48 000 anchors in one DP), the
per-job scratch and capacities with their 4x / 16x re-run, the re-map round's window list of a 500 kb junk read, the gap re-mapper on gaps
of up to the whole of a 2^20 - 1 read, and reader and writer on records of a megabyte.

Inputs (tests/cases.py): set A = long_set_a (40 kb ... 2^20 - 1 with errors, 2^20 - 1 error-free, a chimera, junk), set B = long_set_b
(poly-A of 2^20 - 1, (AC)n, a 100 kb insert, a 50 kb deletion, 70 000 leading N, 65 535 / 65 536 / 65 537 bases, a mapped head with 848 kb
of poly-A behind it), on 5 Mb of reference.
The fixture checks with the oracle alone, before the GPU is used, that they are the cases meant (anchors into the DP, a read that
overflows its cord capacity twice under LNR_CAP_SHRINK=64, gaps wider than 32 768 and over a whole read of 2^20 - 1).

The library reads its knobs when a context is created, and a loop that does not end would show on inputs like these: every group of
settings runs in a child process (tests/long_reads_child.py), every batch there under an alarm of 60 s, the child under a limit of 300 s;
results come back through an .npz, and each setting is asserted on its own, so that a child that ended early is reported as such.

Measured on the MI355X (seconds per batch, as the child prints them): set A + set B 0.13 - 0.16 at every job-kernel setting, 0.35 at -i 2;
the 4 MiB scratch budget 0.27 (8 launches); LNR_CAP_SHRINK=64 0.34 (three runs of the batch); the neighbours 0.16; the gap re-mapper
2.9 s (-g 50), 4.1 s (-g 50 -dup 1) and 3.0 s (-g 200) per batch of the 17 reads, of which the gap kernels are 0.2 - 0.3 s (`gap_ms`) and
the job kernels 0.12 s -- the slowest batches here, at the edge of "a few seconds"; the three parts of the split 0.1 - 0.35 s; reader +
filter + writer of the `long` case 0.9 - 1.4 for a block of all six reads.  The file as a whole: 41 s for its 21 tests, of which 20 s are the oracle and the host writer on the CPU."""
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "long_reads_child.py")
pytestmark = pytest.mark.gpu
BATCH_LIMIT = 60          # seconds per batch (tests/test_gpu_job_five_waves.py)
CHILD_LIMIT = 300
STAT_KEYS = ("jobs", "samples", "lookups", "bucket_entries", "anchors", "remap_reads", "cords", "job_launches", "gap_second_pass", "gap_last_launch", "groups_heavy", "groups_mid", "groups_wave1")
LONG = cases.LONG_MAX
# the record of the `long` case with the most CIGAR elements (the 800 kb chimera, whose second half is error-free): the count
# linear_amd/csrc/lnr_output_hd.h quotes for the distance between real input and the 65 535 elements a BAM record's n_cigar_op holds
LONG_CASE_MAX_CIGAR = 12491

KERNEL_SETTINGS = {
    "default": {},                                                   # 4 waves from 6144 anchors, 16 waves in the re-map round
    "heavy64": {"LNR_HEAVY_CAP": "64"},                              # every read on 16 waves
    "mid64": {"LNR_MID_CAP": "64"},                                  # ... on 4 waves
    "mid64w2": {"LNR_MID_CAP": "64", "LNR_MID_WAVES": "2"},          # ... on 2 waves
    "midmax": {"LNR_MID_CAP": "4000000000"},                         # ... on a single wave: 48 000 anchors in the global half of the arena
    "lds1k": {"LNR_JOB_LDS_KB": "1"},                                # next to no LDS
}
GAP_SETTINGS = {"g50": (50, 0), "g50dup1": (50, 1), "g200": (200, 0)}


class Pool:
    pass


def _pack(lst):
    from linear_amd import synth
    return synth.pack_reads([np.ascontiguousarray(r) for r in lst])


def _per_read(off, *arrs):
    return [tuple(a[int(off[i]):int(off[i + 1])] for a in arrs) for i in range(off.size - 1)]


@pytest.fixture(scope="module")
def pool(oracle_lib, tmp_path_factory):
    from linear_amd import synth
    P = Pool()
    P.refs = refs = cases.long_refs()
    P.A, P.B = cases.long_set_a(refs), cases.long_set_b(refs)
    P.AB = P.A + P.B
    P.sets = {"A": _pack(P.A), "AB": _pack(P.AB)}
    o = oracle_lib.Checker("oracle", refs, 1)
    P.want, P.raw, P.gaps, P.counters = {}, {}, {}, {}
    # ---- the oracle alone: are the inputs the cases meant?
    P.dp = np.array([o.stage(r, 2).size for r in P.AB])
    print("anchors into the DP:", P.dp.tolist())
    assert int(np.sum(P.dp >= 2048)) >= 4 and int(np.sum(P.dp >= 20_000)) >= 2, P.dp.tolist()
    assert int(np.sum((P.dp >= 2) & (P.dp < 2048))) >= 1, P.dp.tolist()
    gaps = []
    for r in P.AB:
        o.map_read(r)
        gaps.append(o.gaps())
    P.gaps[1] = gaps
    y = lambda w: int(w) & 0xfffff
    assert any(y(b) - y(a) > 32768 for g in gaps for a, b in g), "no apx gap wider than 32 768 in y"
    assert any(r.size == LONG and any(y(a) == 0 and y(b) == LONG - 1 for a, b in g) for r, g in zip(P.AB, gaps)), "no gap over the whole of a read of 2^20 - 1"
    coff, cs, ce, st = o.map_batch(*P.sets["AB"], threads=8)
    P.want[("AB", 1, 1)], P.counters[1] = (coff, cs, ce), tuple(int(x) for x in st[:4])
    ncord = np.diff(coff.astype(np.int64))
    P.twice = [i for i, r in enumerate(P.A) if ncord[i] > (16 * (r.size // 64) + 256) // 64 * 4]
    assert P.twice, "no read of set A overflows its cord capacity twice under LNR_CAP_SHRINK=64"
    P.want[("A", 1, 1)] = o.map_batch(*P.sets["A"], threads=8)[:3]
    P.raw[1] = [o.stage(r, 0) for r in P.AB]
    # gap re-mapper: file-order stream semantics
    for name, (gl, dup) in GAP_SETTINGS.items():
        c = o.map_batch(*P.sets["AB"], threads=8, gap_len=gl, dup=dup)
        P.want[name] = (c[0], c[1], c[2], o.ext_out)
    # neighbours: forty reads of 201 to 3000 bases around the four reads of 2^20 - 1
    sr, so, _ = synth.sample_reads(refs, 39, 1600, 0.08, 7300, "random", len_jitter=0.875)
    short = [sr[int(so[i]):int(so[i + 1])] for i in range(39)] + [refs[1][500_000:500_201].copy()]
    lens = [r.size for r in short]
    assert min(lens) == 201 and 2500 < max(lens) <= 3000, sorted(lens)
    big = [r for r in P.AB if r.size == LONG]
    assert len(big) == 4
    mixed, P.short_at = [], []
    for k in range(4):
        for r in short[10 * k:10 * k + 10]:
            P.short_at.append(len(mixed)); mixed.append(r)
        mixed.append(big[k])
    P.sets["short"], P.sets["mixed"] = _pack(short), _pack(mixed)
    P.want["short"] = o.map_batch(*P.sets["short"], threads=8)[:3]
    P.want["mixed"] = o.map_batch(*P.sets["mixed"], threads=8)[:3]
    o.close()
    # the other index layouts
    o3 = oracle_lib.Checker("oracle", refs, 3)
    coff, cs, ce, st = o3.map_batch(*P.sets["AB"], threads=8)
    P.want[("AB", 3, 1)], P.counters[3] = (coff, cs, ce), tuple(int(x) for x in st[:4])
    P.raw[3], P.gaps[3] = [o3.stage(r, 0) for r in P.AB], []
    for r in P.AB:
        o3.map_read(r)
        P.gaps[3].append(o3.gaps())
    o3.close()
    oi = oracle_lib.Checker("oracle", refs, 1, index_type=2)
    cl, P.raw["i2"], P.gaps["i2"] = [], [], []
    for r in P.AB:
        cl.append(oi.map_read(r))
        P.gaps["i2"].append(oi.gaps())
        P.raw["i2"].append(oi.seed_lookup(r)[0])
    oi.close()
    coff = np.zeros(len(P.AB) + 1, np.uint64)
    coff[1:] = np.cumsum([c[0].size for c in cl])
    P.want[("AB", 1, 2)] = (coff, np.concatenate([c[0] for c in cl]), np.concatenate([c[1] for c in cl]))
    # the input file of the children
    P.dir = tmp_path_factory.mktemp("long_reads")
    P.inp = str(P.dir / "in.npz")
    d = {"ref0": refs[0], "ref1": refs[1]}
    for k, (rd, off) in P.sets.items():
        d[k + "_reads"], d[k + "_off"] = rd, off
    np.savez(P.inp, **d)
    return P


_ended_badly = []


def run_child(P, tag, specs):
    """-> (process, results so far).  After a child that did not end with status 0 (a fault, an alarm, the time limit) no further child is
    started: nothing more goes to a GPU that may be in a bad state."""
    if _ended_badly:
        pytest.fail(f"not started: the child of group {_ended_badly[0]!r} did not end clean")
    out, sp = str(P.dir / f"{tag}.npz"), str(P.dir / f"{tag}.json")
    with open(sp, "w") as f:
        json.dump(specs, f)
    try:
        p = subprocess.run([sys.executable, CHILD, P.inp, out, sp, str(BATCH_LIMIT)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired as e:
        p = subprocess.CompletedProcess(e.cmd, -9, (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""),
                                        f"the child passed its limit of {CHILD_LIMIT} s")
    print(p.stdout)
    if p.returncode != 0:
        _ended_badly.append(tag)
        print(p.stderr[-3000:])
    got = dict(np.load(out)) if os.path.exists(out) else {}
    secs = {k[:-4]: round(float(v), 2) for k, v in got.items() if k.endswith("_sec")}
    print("seconds per batch:", secs)
    return p, got


def ended(runs, name):
    p, got = runs
    assert name + "_done" in got, f"the child ended (status {p.returncode}) before or in setting {name!r}: {p.stderr[-2000:]}"
    return got


def same_cords(got, name, want, what):
    coff, cs, ce = got[name + "_off"], got[name + "_cs"], got[name + "_ce"]
    ooff, ocs, oce = want[:3]
    if not np.array_equal(coff, ooff):
        bad = np.nonzero(np.diff(coff.astype(np.int64)) != np.diff(ooff.astype(np.int64)))[0]
        raise AssertionError(f"{what}: cord counts differ from the oracle for reads {bad[:20].tolist()} ({bad.size} of {ooff.size - 1})")
    d = np.nonzero((cs != ocs) | (ce != oce))[0]
    reads = np.unique(np.searchsorted(ooff, d, side="right") - 1)
    assert d.size == 0, f"{what}: {d.size} cords differ from the oracle, in reads {reads[:20].tolist()}; first at cord {int(d[0]) - int(ooff[reads[0]])} of read {int(reads[0])}"


def stats_of(got, name):
    return dict(zip(STAT_KEYS, (int(x) for x in got[name + "_stats"])))


# ---- 1. defaults, and 2. every job kernel on the same batch
@pytest.fixture(scope="module")
def runs_defaults(pool):
    specs = [{"name": "t1", "mode": "map", "reads": "AB", "T": 1, "anchors": True, "gaps": True},
             {"name": "t3", "mode": "map", "reads": "AB", "T": 3, "anchors": True, "gaps": True},
             {"name": "i2", "mode": "map", "reads": "AB", "T": 1, "index_type": 2, "anchors": True, "gaps": True}]
    return run_child(pool, "defaults", specs)


@pytest.mark.parametrize("name,T,it", [("t1", 1, 1), ("t3", 3, 1), ("i2", 1, 2)])
def test_gpu_long_reads_defaults(pool, runs_defaults, name, T, it):
    """Set A + set B in one batch at -t 1, -t 3 and -i 2: cords, raw anchors, apx gaps read by read, the seed counters (-i 1)."""
    got = ended(runs_defaults, name)
    same_cords(got, name, pool.want[("AB", T, it)], name)
    key = "i2" if it == 2 else T
    aoff, anc = got[name + "_aoff"], got[name + "_anc"]
    for i, want in enumerate(pool.raw[key]):
        assert np.array_equal(anc[int(aoff[i]):int(aoff[i + 1])], want), f"{name}: raw anchors of read {i} ({pool.AB[i].size} bases)"
    goff, gaps = got[name + "_goff"], got[name + "_gaps"]
    for i, want in enumerate(pool.gaps[key]):
        assert np.array_equal(gaps[int(goff[i]):int(goff[i + 1])], want), f"{name}: apx gaps of read {i} ({pool.AB[i].size} bases)"
    st = stats_of(got, name)
    if it == 1:
        assert (st["samples"], st["lookups"], st["bucket_entries"], st["anchors"]) == pool.counters[T], name
    assert st["remap_reads"] > 0, st


@pytest.fixture(scope="module")
def runs_kernels(pool):
    specs = [{"name": n, "mode": "map", "reads": "AB", "T": 1, "env": env} for n, env in KERNEL_SETTINGS.items()]
    return run_child(pool, "kernels", specs)


@pytest.mark.parametrize("name", list(KERNEL_SETTINGS))
def test_gpu_long_reads_every_job_kernel(pool, runs_kernels, name):
    """The single-wave, 2-wave, 4-wave and 16-wave job kernels and the arena without LDS on reads that bring 1 000 to 56 000 anchors into
    the chaining DP: the same cords."""
    got = ended(runs_kernels, name)
    same_cords(got, name, pool.want[("AB", 1, 1)], name)
    st = stats_of(got, name)
    h, m, w1 = st["groups_heavy"], st["groups_mid"], st["groups_wave1"]
    print(name, "job groups on 16 waves:", h, " on 4 / 2 waves:", m, " on one wave:", w1, " jobs:", st["jobs"])
    # a read's weight is at least the anchors it brings into the DP, so the cuts place these reads for certain
    ge64, ge6144 = int(np.sum(pool.dp >= 64)), int(np.sum(pool.dp >= 6144))
    assert ge64 >= 12 and ge6144 >= 6
    if name in ("default", "lds1k"):
        assert m >= ge6144 and w1 >= 3, (h, m, w1)      # 4 waves from 6144 anchors, one wave below
    elif name == "heavy64":
        assert h >= ge64 and m == 0, (h, m, w1)         # 16 waves from 64 anchors, in both rounds
    elif name in ("mid64", "mid64w2"):
        assert m >= ge64, (h, m, w1)                    # 4 / 2 waves from 64 anchors (the re-map round keeps its 16-wave cut of 7000)
    else:
        assert m == 0 and w1 >= ge64, (h, m, w1)        # midmax: up to 56 000 anchors in a single wave's DP


# ---- 3. scratch slicing, 4. capacity re-runs
@pytest.fixture(scope="module")
def runs_sizing(pool):
    specs = [{"name": "budget", "mode": "map", "reads": "A", "T": 1, "scratch_budget": 4 << 20},
             {"name": "shrink64", "mode": "map", "reads": "A", "T": 1, "env": {"LNR_CAP_SHRINK": "64"}},
             {"name": "shrink4096", "mode": "map", "reads": "A", "T": 1, "env": {"LNR_CAP_SHRINK": "4096"}}]
    return run_child(pool, "sizing", specs)


def test_gpu_long_reads_scratch_slicing(pool, runs_sizing):
    """A scratch budget of 4 MiB, less than one long read's job needs: a job larger than the budget runs in a slice of its own (lnr_batch.h:
    `g1 > g0 && s2 > budget`), the batch takes several launches, the cords are unchanged."""
    got = ended(runs_sizing, "budget")
    assert "budget_off" in got, str(got.get("budget_msg"))
    same_cords(got, "budget", pool.want[("A", 1, 1)], "scratch_budget 4 MiB")
    assert stats_of(got, "budget")["job_launches"] > 1


def test_gpu_long_reads_capacity_reruns(pool, runs_sizing):
    """LNR_CAP_SHRINK=64: the error-free read of 2^20 - 1 bases has more cords than its capacity at 1x and at 4x, the batch is run a third
    time at 16x and gives the oracle's cords.  LNR_CAP_SHRINK=4096: 16x is not enough, the call fails with status -8 and names the read."""
    got = ended(runs_sizing, "shrink64")
    assert "shrink64_off" in got, str(got.get("shrink64_msg"))
    same_cords(got, "shrink64", pool.want[("A", 1, 1)], "LNR_CAP_SHRINK=64")
    got = ended(runs_sizing, "shrink4096")
    assert "shrink4096_status" in got, "LNR_CAP_SHRINK=4096 returned cords"
    ooff = pool.want[("A", 1, 1)][0]
    ncord = np.diff(ooff.astype(np.int64))
    first = next(i for i, r in enumerate(pool.A) if ncord[i] > max((16 * (r.size // 64) + 256) // 4096, 8) * 16)
    msg = str(got["shrink4096_msg"])
    assert int(got["shrink4096_status"]) == -8 and "overflow" in msg, msg
    assert f"read {first} " in msg and f"length {pool.A[first].size}" in msg, msg


# ---- 5. neighbours
@pytest.fixture(scope="module")
def runs_neighbours(pool):
    return run_child(pool, "neighbours", [{"name": "nb", "mode": "neighbours"}])


def test_gpu_long_reads_neighbours(pool, runs_neighbours):
    """Forty reads of 201 to 3000 bases between the four reads of 2^20 - 1: every short read's cords are those of the short reads submitted
    alone; the same through lnr_filter_submit / _wait with two batches in flight; a read of 2^20 bases and a reference sequence of
    2^30 - 2^20 are refused with status -6, and the context, its index untouched, maps the next batch correctly."""
    got = ended(runs_neighbours, "nb")
    same_cords(got, "nb_alone", pool.want["short"], "short reads alone")
    same_cords(got, "nb_mixed", pool.want["mixed"], "short reads between the long ones")
    alone = _per_read(got["nb_alone_off"], got["nb_alone_cs"], got["nb_alone_ce"])
    mixed = _per_read(got["nb_mixed_off"], got["nb_mixed_cs"], got["nb_mixed_ce"])
    assert len(alone) == 40 and sum(a[0].size > 0 for a in alone) >= 30
    for k, at in enumerate(pool.short_at):
        assert np.array_equal(alone[k][0], mixed[at][0]) and np.array_equal(alone[k][1], mixed[at][1]), f"short read {k}"
    same_cords(got, "nb_pipe_mixed", pool.want["mixed"], "submit / wait, first batch")
    same_cords(got, "nb_pipe_alone", pool.want["short"], "submit / wait, second batch")
    assert int(got["nb_limit_status"]) == -6, got.get("nb_limit_msg")
    assert int(got["nb_seq_limit_status"]) == -6 and "30-bit" in str(got["nb_seq_limit_msg"]), got.get("nb_seq_limit_msg")
    same_cords(got, "nb_after", pool.want["mixed"], "the batch after the refused ones")


# ---- 6. gap re-mapper
@pytest.fixture(scope="module")
def runs_gap(pool):
    specs = [{"name": n, "mode": "gap", "reads": "AB", "gap_len": gl, "dup": dup, "split": n == "g50"} for n, (gl, dup) in GAP_SETTINGS.items()]
    return run_child(pool, "gap", specs)


@pytest.mark.parametrize("name", list(GAP_SETTINGS))
def test_gpu_long_reads_gap_remapper(pool, runs_gap, name):
    """-g 50, -g 50 -dup 1 and -g 200 on set A + set B in file order: gaps of 300 kb to the whole of a read of 2^20 - 1, a gap of 848 kb of
    poly-A behind 200 kb that map (k_gap_weight: one 9-mer bucket beyond 65 535 entries, whose packed 16-bit counter carries into its
    neighbour -- the weight only ranks the reads, the cords must not depend on it), the column DP without its y buckets, the stock
    thresholds of the team forms.  Cords and stream state
    equal the oracle's; the state is carried over a split into three batches."""
    got = ended(runs_gap, name)
    want = pool.want[name]
    same_cords(got, name, want, name)
    assert int(got[name + "_ext"]) == want[3]
    st = stats_of(got, name)
    assert st["gap_second_pass"] > 0, st
    assert not np.array_equal(want[1], pool.want[("AB", 1, 1)][1]), "the gap path changed nothing"
    if name == "g50":
        assert np.array_equal(got["g50_split_n"], np.diff(want[0].astype(np.int64)))
        assert np.array_equal(got["g50_split_cs"], want[1]) and np.array_equal(got["g50_split_ce"], want[2])
        assert int(got["g50_split_ext"]) == want[3]


# ---- 7. files in, text out
FILE_BLOCKS = (23, 3)       # one block; and a block that ends in front of the read of 2^20 - 1 (the fourth of the case)


@pytest.fixture(scope="module")
def files(pool, case_inputs, oracle_lib):
    from tests import bgzf_cases as bc, gzip_cases as gc
    from linear_amd.api import Writer
    F = Pool()
    refs, reads, off = case_inputs("long")
    n = off.size - 1
    assert int(off[4] - off[3]) == LONG
    rid, gid = cases.text_ids(n, len(refs))
    d = pool.dir / "files"
    os.makedirs(d, exist_ok=True)
    fa, _, _, _ = cases.write_fasta_case(d, refs, reads, off)
    abc = np.frombuffer(b"ACGTN", np.uint8)
    rng = np.random.default_rng(7400)
    fq = str(d / "reads.fq")
    with open(fq, "wb") as f:
        for i in range(n):
            L = int(off[i + 1] - off[i])
            f.write(b"@" + rid[i].encode() + b"\n" + abc[reads[int(off[i]):int(off[i + 1])]].tobytes() + b"\n+\n" + rng.integers(33, 74, L, dtype=np.uint8).tobytes() + b"\n")
    F.paths, F.plain_gzip = {"fa": fa, "fq": fq}, {}
    for tag, src in (("fa", fa), ("fq", fq)):
        text = open(src, "rb").read()
        for kind, data in (("gz", gc.gz(text)), ("bgzf", bc.bgzf(text))):
            p = str(d / f"reads.{tag}.{kind}")
            with open(p, "wb") as f:
                f.write(data)
            F.paths[f"{tag}_{kind}"] = p
            F.plain_gzip[f"{tag}_{kind}"] = kind == "gz"
    F.dst_cap = 1 << 22
    o = oracle_lib.Checker("oracle", refs, 1)
    coff, cs, ce, _ = o.map_batch(reads, off, threads=8)
    o.close()
    w = Writer(gid, [r.size for r in refs])
    w.set_genome(refs)
    F.want = {}
    for mr in FILE_BLOCKS:
        for k, a in enumerate(range(0, n, mr)):
            b = min(a + mr, n)
            c0 = (coff[a:b + 1] - coff[a]).astype(np.uint64)
            s, e = cs[int(coff[a]):int(coff[b])], ce[int(coff[a]):int(coff[b])]
            rd, ro = np.ascontiguousarray(reads[int(off[a]):int(off[b])]), (off[a:b + 1] - off[a]).astype(np.uint64)
            rl = np.diff(ro.astype(np.int64)).astype(np.uint64)
            F.want[(mr, k)] = {"sam": w.format_seq(c0, s, e, rd, ro, rid[a:b]), "apf": w.format(c0, s, e, rl, rid[a:b], "apf"),
                               "bam": w.format_bam(c0, s, e, None, rid[a:b], reads=rd, read_off=ro)}
    w.close()
    F.gid = gid
    return F


@pytest.fixture(scope="module")
def runs_files(pool, files):
    spec = {"name": "files", "mode": "files", "files": files.paths, "plain_gzip": files.plain_gzip, "block_reads": list(FILE_BLOCKS), "dst_cap": files.dst_cap, "full": "fa"}
    return run_child(pool, "files", [spec])


def _sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.mark.parametrize("tag", ["fa", "fq", "fa_gz", "fq_gz", "fa_bgzf", "fq_bgzf"])
def test_gpu_long_reads_files_in_text_out(files, runs_files, tag):
    """The `long` case as FASTA and four-line FASTQ, plain, gzip and BGZF (records of up to a megabyte) -> GPU reader -> filter_batch_dev ->
    GPU writer: the blocks are the serial reader's; SAM with SEQ, APF and BAM with SEQ are the host writer's bytes on the oracle's cords
    (a CIGAR from 3 456 cords, a BAM record of 0.8 MB that spans a dozen BGZF blocks); the BAM goes through tests/bam_cases.py."""
    from tests import bam_cases as bmc, reader_gpu_cases as rg
    p, got = runs_files
    for mr in FILE_BLOCKS:
        assert f"files_{tag}_{mr}_blocks" in got, f"the child ended (status {p.returncode}) before file {tag!r} at {mr} reads per block: {p.stderr[-2000:]}"
        blocks = rg.serial_blocks(files.paths[tag], files.dst_cap, mr)
        assert int(got[f"files_{tag}_{mr}_blocks"]) == len(blocks) == (1 if mr == 23 else 2)
        for k, (off, bases, ids) in enumerate(blocks):
            key = f"files_{tag}_{mr}_{k}"
            assert np.array_equal(got[key + "_off"], off) and str(got[key + "_ids"]).split("\n") == ids, key
            assert str(got[key + "_bases_sha"]) == _sha(bases.tobytes()), f"{key}: bases differ from the serial reader's"
            want = files.want[(mr, k)]
            for what in ("sam", "apf", "bam"):
                assert int(got[f"{key}_{what}_len"]) == len(want[what]) and str(got[f"{key}_{what}_sha"]) == _sha(want[what]), f"{key}: {what} differs from the host writer's on the oracle's cords"
            raw = gzip.decompress(got[key + "_bgz"].tobytes() + got["files_eof"].tobytes())
            assert raw == want["bam"], f"{key}: BGZF members of the BAM records"
            if tag == "fa":
                bam = got[key + "_bam"].tobytes()
                assert bam == bmc.bam_of_sam(got[key + "_sam"].tobytes(), files.gid)
                recs = bmc.walk_records(bam)
                lines = [l for l in want["sam"].split(b"\n") if l]
                assert len(recs) == len(lines)
                assert [r["l_seq"] for r in recs] == [len(l.split(b"\t")[9]) for l in lines]
    # the distance between real input and the 65 535 CIGAR elements of a BAM record (linear_amd/csrc/lnr_output_hd.h)
    sam = files.want[(23, 0)]["sam"]
    ncig = [len(re.findall(rb"\d+[MIDNSHP=X]", l.split(b"\t")[5])) for l in sam.split(b"\n") if l]
    lseq = [len(l.split(b"\t")[9]) for l in sam.split(b"\n") if l]
    print("CIGAR elements per record:", ncig, "SEQ lengths:", lseq)
    assert max(lseq) == LONG
    assert max(ncig) == LONG_CASE_MAX_CIGAR
