"""GPU (-m gpu): two batches computed side by side inside one context (the lanes behind lnr_filter_submit / lnr_filter_wait at
gap_len == 0), through the C ABI.  Every batch must come back word for word as the same batch through lnr_filter_batch on a fresh
context that runs one batch at a time (LNR_LANES=1), in submission order; -g > 0 stays serial and carries its stream state."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batches(case_inputs):
    """Batches of different sizes and contents on the references of the `edge` case (three sequences, N runs, a repeat-rich one)."""
    from linear_amd import synth
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    h = n // 3
    out = [(reads, off)]                                                                    # 0: the whole case (golden edge_T3)
    out.append((np.zeros(0, np.uint8), np.zeros(1, np.uint64)))                             # 1: empty
    out.append(synth.pack_reads([refs[0][1000 * k:1000 * k + L].copy() for k, L in enumerate((50, 200, 0, 199, 120, 1, 200))]))   # 2: nothing above 200 bases
    out.append(synth.sample_reads([refs[1]], 48, 10000, 0.10, 9001, "random")[:2])          # 3: repeat-rich: every job class, re-map round
    out.append(synth.sample_reads(refs, 40, 8000, 0.10, 9002, "random")[:2])                # 4
    out.append(synth.pack_reads([refs[2][100:100 + 12000].copy()]))                         # 5: one read
    out.append(synth.sample_reads(refs, 150, 3000, 0.08, 9003, "random", len_jitter=0.8)[:2])   # 6: many ragged reads
    out.append((np.ascontiguousarray(reads[int(off[h]):]), np.ascontiguousarray((off[h:] - off[h]).astype(np.uint64))))          # 7: a window of the case
    return refs, [(np.ascontiguousarray(r, np.uint8), np.ascontiguousarray(o, np.uint64)) for r, o in out]


def _pipeline(f, batches):
    """submit(0); submit(1); loop { submit(k + 2); wait(k) }"""
    got = []
    for k in range(min(2, len(batches))):
        f.filter_submit(*batches[k])
    for k in range(len(batches)):
        if k + 2 < len(batches):
            f.filter_submit(*batches[k + 2])
        got.append(f.filter_wait())
    return got


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _one_at_a_time(refs, batches, monkeypatch):
    """Every batch through lnr_filter_batch on a fresh context with one lane; also the re-map reads of each batch."""
    from linear_amd import Filter
    monkeypatch.setenv("LNR_LANES", "1")
    one = Filter(device=0)
    monkeypatch.delenv("LNR_LANES")
    one.build_index(refs, 3)
    want, remap = [], []
    for b in batches:
        want.append(one.filter_batch(*b))
        remap.append(one.stats()["remap_reads"])
    one.close()
    return want, remap


def test_gpu_two_lanes_equal_one_batch_at_a_time(case_inputs, oracle_lib, monkeypatch, capfd):
    from linear_amd import Filter, LnrError
    # (size-class cuts scaled to the small references, as in test_gpu_other_size_class_paths: 16-wave, 4-wave and single-wave kernels in one
    #  launch; LNR_HEAVY_CAP / LNR_MID_CAP set the cuts of the re-map round as well)
    monkeypatch.setenv("LNR_HEAVY_CAP", "900")
    monkeypatch.setenv("LNR_MID_CAP", "300")
    refs, batches = _batches(case_inputs)
    assert len(batches) >= 7
    want, remap = _one_at_a_time(refs, batches, monkeypatch)
    print("re-map reads per batch:", remap)
    assert remap[0] > 0, "the edge case should send reads through the re-map round"
    g = np.load(os.path.join(GOLD, "edge_T3.npz"))
    assert np.array_equal(want[0][0], g["cord_off"]) and np.array_equal(want[0][1], g["cords_str"]) and np.array_equal(want[0][2], g["cords_end"])
    o = oracle_lib.Checker("oracle", refs, 3)
    for k in (3, 6):
        ooff, ocs, oce, _ = o.map_batch(*batches[k], threads=8)
        assert np.array_equal(want[k][0], ooff) and np.array_equal(want[k][1], ocs) and np.array_equal(want[k][2], oce), k
    o.close()
    assert want[1][0].tolist() == [0] and want[2][1].size == 0 and want[3][1].size > 0
    monkeypatch.setenv("LNR_DEBUG_TIMES", "1")      # (every batch then reports the lane it ran on)
    f = Filter(device=0)
    f.build_index(refs, 3)
    capfd.readouterr()
    for rnd in range(2):
        got = _pipeline(f, batches)
        for k, (w, c) in enumerate(zip(want, got)):
            assert _same(w, c), (rnd, k)
        assert f.stats()["reads"] == batches[-1][1].size - 1          # lnr_last_stats: the batch handed out last
    err = capfd.readouterr().err
    assert err.count("| lane 1 allocations") >= 4 and err.count("| lane 0 allocations") >= 4, "both lanes must have computed batches"
    assert "lane 1 out of memory" not in err
    monkeypatch.delenv("LNR_DEBUG_TIMES")
    with pytest.raises(LnrError):
        f.filter_wait()
    # three in flight, a fourth refused, order kept when the batches differ wildly in cost
    order = [3, 1, 0]
    for k in order:
        f.filter_submit(*batches[k])
    with pytest.raises(LnrError):
        f.filter_submit(*batches[2])
    for k in order:
        assert _same(want[k], f.filter_wait()), k
    # a drained pipeline leaves a usable context
    assert _same(want[4], f.filter_batch(*batches[4]))
    f.close()


def test_gpu_lane_1_follows_an_index_rebuilt_between_pipelines(case_inputs, oracle_lib, monkeypatch, capfd):
    """Both lanes read the one index of their context: after lane 1 has computed on a first index, lnr_index_build with nothing in flight
    on another, larger reference set (the index buffers are sized anew) must reach lane 1 as well -- sizes, offsets, device pointers.
    Every batch of a pipeline on the second index equals the same batch through lnr_filter_batch on a fresh one-lane context."""
    from linear_amd import Filter, synth
    refs, batches = _batches(case_inputs)
    monkeypatch.setenv("LNR_DEBUG_TIMES", "1")
    f = Filter(device=0)
    f.build_index(refs, 3)
    capfd.readouterr()
    first = _pipeline(f, [batches[k] for k in (0, 3, 4, 6)])
    err = capfd.readouterr().err
    assert err.count("| lane 1 allocations") >= 1 and err.count("| lane 0 allocations") >= 1, "both lanes must have computed on the first index"
    g = np.load(os.path.join(GOLD, "edge_T3.npz"))
    assert np.array_equal(first[0][0], g["cord_off"]) and np.array_equal(first[0][1], g["cords_str"]) and np.array_equal(first[0][2], g["cords_end"])
    refs2 = case_inputs("rep")[0]
    assert sum(r.size for r in refs2) != sum(r.size for r in refs) and max(r.size for r in refs2) > max(r.size for r in refs)
    batches2 = [synth.sample_reads(refs2, 40, 8000, 0.10, 9100 + k, "random")[:2] for k in range(4)]
    batches2 = [(np.ascontiguousarray(r, np.uint8), np.ascontiguousarray(o, np.uint64)) for r, o in batches2]
    f.build_index(refs2, 1)
    capfd.readouterr()
    got = _pipeline(f, batches2)
    err = capfd.readouterr().err
    assert err.count("| lane 1 allocations") >= 1 and err.count("| lane 0 allocations") >= 1, "both lanes must have computed on the second index"
    assert "lane 1 out of memory" not in err
    f.close()
    monkeypatch.delenv("LNR_DEBUG_TIMES")
    monkeypatch.setenv("LNR_LANES", "1")
    one = Filter(device=0)
    monkeypatch.delenv("LNR_LANES")
    one.build_index(refs2, 1)
    want = [one.filter_batch(*b) for b in batches2]
    one.close()
    assert all(w[1].size > 0 for w in want)
    for k, (w, c) in enumerate(zip(want, got)):
        assert _same(w, c), k
    o = oracle_lib.Checker("oracle", refs2, 1)
    ooff, ocs, oce, _ = o.map_batch(*batches2[1], threads=8)
    o.close()
    assert np.array_equal(got[1][0], ooff) and np.array_equal(got[1][1], ocs) and np.array_equal(got[1][2], oce)


def test_gpu_lane_1_out_of_memory_falls_back_to_one_lane(case_inputs, monkeypatch, capfd):
    """A workload that fits once but not twice: LNR_LANE1_NOMEM=1 makes lane 1's first batch fail with LNR_ERR_NOMEM, as a full device would.
    The batch is run again on lane 0 and handed out in its place, no batch reports an error, and every later batch runs on lane 0."""
    from linear_amd import Filter
    refs, batches = _batches(case_inputs)
    want, _ = _one_at_a_time(refs, batches, monkeypatch)
    monkeypatch.setenv("LNR_LANE1_NOMEM", "1")
    monkeypatch.setenv("LNR_DEBUG_TIMES", "1")
    f = Filter(device=0)
    f.build_index(refs, 3)
    capfd.readouterr()
    got = _pipeline(f, batches)
    for k, (w, c) in enumerate(zip(want, got)):
        assert _same(w, c), k
    err = capfd.readouterr().err
    assert err.count("lane 1 out of memory") == 1 and "| lane 1 allocations" not in err
    for k in (3, 0, 5):                         # three in flight on the one lane that is left
        f.filter_submit(*batches[k])
    for k in (3, 0, 5):
        assert _same(want[k], f.filter_wait()), k
    got = _pipeline(f, batches)
    for k, (w, c) in enumerate(zip(want, got)):
        assert _same(w, c), k
    err = capfd.readouterr().err
    assert "lane 1" not in err
    f.close()


def test_gpu_gap_path_stays_serial_and_keeps_its_stream_state(case_inputs):
    """gap_len = 50, dup = 1: the same submit / wait sequence equals the one-by-one run, the stream state (lnr_gap_stream) after
    every batch included -- checked by running every prefix of the sequence as a new stream and reading the state once it has drained."""
    from linear_amd import Filter
    refs, batches = _batches(case_inputs)
    f = Filter(device=0, gap_len=50, dup=1)
    f.build_index(refs, 1)
    want, state = [], []
    assert f.gap_stream(0) == 0
    for b in batches:
        want.append(f.filter_batch(*b))
        state.append(f.gap_stream())
    assert state[-1] == 1, "the sequence should contain a read that extends"
    for m in range(1, len(batches) + 1):
        assert f.gap_stream(0) == 0
        got = _pipeline(f, batches[:m])
        for k in range(m):
            assert _same(want[k], got[k]), (m, k)
        assert f.gap_stream() == state[m - 1], m
    f.close()


def test_gpu_capacity_rerun_inside_the_pipeline(case_inputs, monkeypatch):
    """LNR_CAP_SHRINK as in test_gpu_batch_rerun_on_per_read_overflow: every batch of the context overflows first and is run again with
    larger capacities, on whichever lane it is; three batches through submit / wait equal the same batches through lnr_filter_batch."""
    from linear_amd import Filter
    refs, reads, off = case_inputs("ont")
    g = np.load(os.path.join(GOLD, "ont_T1.npz"))
    n = off.size - 1
    cuts = [0, n // 4, n // 2, n]
    parts = [(np.ascontiguousarray(reads[int(off[a]):int(off[b])]), np.ascontiguousarray((off[a:b + 1] - off[a]).astype(np.uint64))) for a, b in zip(cuts[:-1], cuts[1:])]
    monkeypatch.setenv("LNR_CAP_SHRINK", "64")
    one = Filter(device=0)
    one.build_index(refs, 1)
    want = [one.filter_batch(*p) for p in parts]
    one.close()
    assert np.array_equal(np.concatenate([w[1] for w in want]), g["cords_str"]) and np.array_equal(np.concatenate([w[2] for w in want]), g["cords_end"])
    f = Filter(device=0)
    f.build_index(refs, 1)
    for p in parts:
        f.filter_submit(*p)
    for k in range(3):
        assert _same(want[k], f.filter_wait()), k
    f.close()


_DESTROY = """
import sys
sys.path.insert(0, {root!r})
import numpy as np
from linear_amd import Filter, synth
ref = synth.random_ref(300_000, 77)
reads, off, _ = synth.sample_reads([ref], 60, 6000, 0.1, 78, "random")
f = Filter(device=0)
f.build_index([ref], 1)
f.filter_submit(reads, off)
f.filter_submit(reads, off)
f.close()
print("destroyed")
"""


def test_gpu_destroy_with_batches_in_flight_returns():
    """lnr_destroy with two batches submitted and never waited for gives them up and returns (a child process under a time limit)."""
    from linear_amd import build as lb
    lb.build()
    p = subprocess.run([sys.executable, "-c", _DESTROY.format(root=ROOT)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and b"destroyed" in p.stdout, (p.returncode, p.stderr.decode()[-500:])
