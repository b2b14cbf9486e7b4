"""GPU (-m gpu): the stretch between two bulk rounds of the two lanes -- the order of the job launches (lnr_handover.h), the merged
read-backs and the multi-segment single-wave copies.  None of it changes a result: every batch through lnr_filter_submit / lnr_filter_wait
must come back word for word as the same batch through lnr_filter_batch on a fresh one-lane context (computed once, shared by the tests).
That reference runs the same copy and read-back code; what pins it from outside is the golden file of the `edge` batch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = {"LNR_HEAVY_CAP": "900", "LNR_MID_CAP": "300"}      # all three job classes and the re-map round on the small references


class _Env:
    """environment for the contexts made inside (the knobs are read in lnr_create), restored on the way out"""
    def __init__(self, **kv):
        self.kv = dict(CUTS, **kv)

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _batches(refs, reads, off):
    """The read counts are the sizes of the copies: 1, 63, 64, 65 words and 257 (five single-wave workgroups, the last one ragged)."""
    from linear_amd import synth
    out = [synth.sample_reads(refs, n, 450, 0.08, 9200 + n, "random", len_jitter=0.33)[:2] for n in (1, 63, 64, 65, 257)]   # 300-600 bases
    out.append((reads, off))                                                                 # 5: the `edge` case (golden edge_T3)
    out.append((np.zeros(0, np.uint8), np.zeros(1, np.uint64)))                              # 6: empty
    out.append(synth.pack_reads([refs[0][1000 * k:1000 * k + L].copy() for k, L in enumerate((50, 200, 0, 199, 120, 1, 200))]))   # 7: nothing above 200 bases
    out.append(synth.sample_reads([refs[1]], 48, 10000, 0.10, 9001, "random")[:2])           # 8: repeat-rich: every job class, re-map round
    return [(np.ascontiguousarray(r, np.uint8), np.ascontiguousarray(o, np.uint64)) for r, o in out]


EDGE = 5


@pytest.fixture(scope="module")
def world(case_inputs):
    from linear_amd import Filter
    refs, reads, off = case_inputs("edge")
    batches = _batches(refs, reads, off)
    want, remap = [], []
    for b in batches:       # a fresh one-lane context for every batch: nothing sticky (capacities, estimates) goes from batch to batch
        with _Env(LNR_LANES="1"):
            one = Filter(device=0)
        one.build_index(refs, 3)
        want.append(one.filter_batch(*b))
        remap.append(one.stats()["remap_reads"])
        one.close()
    g = np.load(os.path.join(GOLD, "edge_T3.npz"))
    assert np.array_equal(want[EDGE][0], g["cord_off"]) and np.array_equal(want[EDGE][1], g["cords_str"]) and np.array_equal(want[EDGE][2], g["cords_end"])
    assert remap[EDGE] > 0 and sum(remap[:5]) > 0, remap        # the re-map round runs, on the case and on the short reads
    assert sum(want[k][1].size for k in range(5)) > 0, "short reads should map"
    return refs, batches, want, remap


def _pipeline(f, batches):
    """submit(0); submit(1); loop { submit(k + 2); wait(k) }; the re-map reads of every batch beside its result"""
    got, remap = [], []
    for k in range(min(2, len(batches))):
        f.filter_submit(*batches[k])
    for k in range(len(batches)):
        if k + 2 < len(batches):
            f.filter_submit(*batches[k + 2])
        got.append(f.filter_wait())
        remap.append(f.stats()["remap_reads"])
    return got, remap


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _two_rounds(world, **env):
    from linear_amd import Filter
    refs, batches, want, remap = world
    with _Env(**env):       # (for the whole run: LNR_DEBUG_TIMES is looked up whenever a stamp is due)
        f = Filter(device=0)
        f.build_index(refs, 3)
        for rnd in range(2):
            got, rm = _pipeline(f, batches)
            for k, (w, c) in enumerate(zip(want, got)):
                assert _same(w, c), (env, rnd, k)
            assert rm == remap, (env, rnd, rm, remap)
        f.close()


def test_gpu_pipeline_parity(world):
    _two_rounds(world)
    g = np.load(os.path.join(GOLD, "edge_T3.npz"))
    assert np.array_equal(world[2][EDGE][1], g["cords_str"])


@pytest.mark.parametrize("spec", ["1", "100000000"])
def test_gpu_gap_readback_sizes(world, spec):
    """LNR_GAPS_SPEC=1: one gap entry travels with the flags, so the second trip is always taken; a value above every batch's gap count: never."""
    assert world[3][EDGE] > 0                                   # stats()["remap_reads"]: the re-map round ran (and _two_rounds compares it per batch)
    _two_rounds(world, LNR_GAPS_SPEC=spec)


_STAMP = re.compile(r"\[lnr\] handover lane (\d) (\S+) ([0-9.]+)")


def test_gpu_order_of_the_launches(world, capfd):
    """The phase stamps are wired to the right places: every hand-over that opens ends, both lanes go through them, and no lane's "round-0
    enqueued" lies inside the other lane's hand-over (from its own "round-0 enqueued" to its "handover-end").  The hand-overs of these
    small batches last about a millisecond, so a broken gate would seldom show here: the protocol itself is checked by
    tests/handover_gate_main.cpp under the thread sanitizer."""
    capfd.readouterr()
    _two_rounds(world, LNR_DEBUG_TIMES="1")
    err = capfd.readouterr().err
    ev = [(int(m.group(1)), m.group(2), float(m.group(3))) for m in _STAMP.finditer(err)]
    spans, r0 = {0: [], 1: []}, {0: [], 1: []}
    open_ = {}
    for lane, what, t in ev:
        if what == "round0-enqueued":
            r0[lane].append(t)
            open_[lane] = t
        elif what == "handover-end":
            spans[lane].append((open_.pop(lane), t))
    assert not open_, "a hand-over that never ended"
    assert len(spans[0]) >= 6 and len(spans[1]) >= 6, "both lanes must have gone through hand-overs"
    for lane in (0, 1):
        for t in r0[lane]:
            for a, b in spans[lane ^ 1]:
                assert not (a < t < b), (lane, t, a, b)
    m = re.findall(r"copy launches of this batch (\d+)", err)
    assert m and max(map(int, m)) <= 20, m      # (one launch per round trip: 15 on a batch with a re-map round, 55 before)


def test_gpu_gate_changes_order_only(world, capfd):
    capfd.readouterr()
    _two_rounds(world, LNR_HANDOVER_GATE="0", LNR_DEBUG_TIMES="1")
    err = capfd.readouterr().err
    assert "[lnr] handover" not in err and "copy launches of this batch" in err


_EXITS = """
import os, sys
sys.path.insert(0, {root!r})
import numpy as np
from linear_amd import Filter, LnrError, synth
os.environ.update(LNR_HEAVY_CAP="900", LNR_MID_CAP="300")
ref = synth.repeat_ref(300_000, 4)
good = [tuple(np.ascontiguousarray(a) for a in synth.sample_reads([ref], n, 6000, 0.1, 70 + n, "random")[:2]) for n in (40, 33, 48)]
os.environ["LNR_LANES"] = "1"
one = Filter(device=0)
one.build_index([ref], 2)
want = [one.filter_batch(*b) for b in good]
one.close()
del os.environ["LNR_LANES"]
same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
mode = sys.argv[1]
if mode == "nomem":
    os.environ["LNR_LANE1_NOMEM"] = "1"
f = Filter(device=0)
f.build_index([ref], 2)
if mode == "bad":
    # offsets not monotone: refused when submitted (the pipeline never sees them), with good batches in flight around it
    f.filter_submit(*good[0])
    try:
        f.filter_submit(good[1][0], np.array([0, 500, 400, 900], np.uint64)); raise SystemExit("not refused")
    except LnrError as e:
        assert e.status == -1, e.status
    # a read of 2^20 bases: passes the submit and fails in prepare_batch, on lane 1, between good batches
    long_read = (np.zeros(1 << 20, np.uint8), np.array([0, 1 << 20], np.uint64))
    f.filter_submit(*long_read)
    f.filter_submit(*good[1])
    assert same(want[0], f.filter_wait())
    try:
        f.filter_wait(); raise SystemExit("no error")
    except LnrError as e:
        assert e.status == -6, e.status
    f.filter_submit(*good[2]); f.filter_submit(*good[0])
    assert same(want[1], f.filter_wait()) and same(want[2], f.filter_wait()) and same(want[0], f.filter_wait())
if mode == "nomem":
    for rnd in range(2):
        for b in good: f.filter_submit(*b)
        for w in want: assert same(w, f.filter_wait())
if mode == "close":
    for b in good: f.filter_submit(*b)
f.close()
print("done", mode)
"""


@pytest.mark.parametrize("mode", ["bad", "nomem", "close"])
def test_gpu_exits_leave_the_gate(mode):
    """Ways out of a batch that must let go of the hand-over: an error in prepare_batch, lane 1 out of memory, a context closed with batches
    in flight.  In a child process under a time limit: a missed wake-up fails instead of hanging."""
    p = subprocess.run([sys.executable, "-c", _EXITS.format(root=ROOT), mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and ("done " + mode).encode() in p.stdout, (p.returncode, p.stdout.decode()[-300:], p.stderr.decode()[-1500:])
