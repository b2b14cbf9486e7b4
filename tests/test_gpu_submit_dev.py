"""GPU (-m gpu): the device form of the filter in halves, lnr_filter_submit_dev / lnr_filter_wait_dev, through the C ABI.  Input that lies on
the device already goes through the same lanes as lnr_filter_submit's, and the result is handed out as device arrays.  Every batch must come
back word for word as the same batch through lnr_filter_batch on a fresh context that runs one batch at a time (LNR_LANES=1), in submission
order; a device result stays valid until the second next wait is called; the halves of both forms combine; limits, errors, -g > 0 and the
one-lane fall-back behave as they do behind lnr_filter_submit / lnr_filter_wait."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_hip = None


def d2h(ptr, nbytes, dtype=np.uint64):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(max(nbytes, 8), np.uint8)
    if nbytes:
        assert _hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
    return out[:nbytes].view(dtype).copy()


def dev_np(dev):
    """(cord_off, cords_str, cords_end) of a lnr_cords_dev, copied off the device now"""
    assert dev.d_cord_off
    coff = d2h(dev.d_cord_off, (dev.n_reads + 1) * 8)
    assert int(coff[-1]) == dev.n_cords and int(coff[0]) == 0
    if not dev.n_cords:
        return coff, np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    assert dev.d_cords_str and dev.d_cords_end
    return coff, d2h(dev.d_cords_str, dev.n_cords * 8), d2h(dev.d_cords_end, dev.n_cords * 8)


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


class Dev:
    """A batch on the device: bases (16 spare bytes behind them, as the GPU reader leaves) and the n + 1 offsets, complete when made"""

    def __init__(self, reads, off):
        import torch
        self.h_off = np.ascontiguousarray(off, np.uint64)
        self.n = off.size - 1
        self.reads = torch.from_numpy(np.concatenate([np.ascontiguousarray(reads, np.uint8), np.zeros(16, np.uint8)])).cuda()
        self.off = torch.from_numpy(self.h_off.view(np.int64)).cuda()
        torch.cuda.synchronize()

    def submit(self, f, h_off=True):
        f.filter_submit_dev(self.reads.data_ptr(), self.off.data_ptr(), self.n, self.h_off if h_off else None)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


def _pipeline(f, dbs, h_off=True):
    """submit(0); submit(1); loop { submit(k + 2); wait(k) }, every result copied off the device before the next wait"""
    got = []
    for k in range(min(2, len(dbs))):
        dbs[k].submit(f, h_off)
    for k in range(len(dbs)):
        if k + 2 < len(dbs):
            dbs[k + 2].submit(f, h_off)
        got.append(dev_np(f.filter_wait_dev()))
    return got


@pytest.fixture(scope="module")
def ref_run(case_inputs):
    """(refs, batches, the batches on the device, every batch through lnr_filter_batch on a fresh LNR_LANES=1 context): computed once, with
    the size-class cuts scaled to the small references (16-wave, 4-wave and single-wave job kernels in one launch, in both rounds)"""
    from linear_amd import Filter
    old = {k: os.environ.get(k) for k in ("LNR_HEAVY_CAP", "LNR_MID_CAP", "LNR_LANES")}
    os.environ.update(LNR_HEAVY_CAP="900", LNR_MID_CAP="300", LNR_LANES="1")
    try:
        refs, batches = _batches(case_inputs)
        one = Filter(device=0)
        one.build_index(refs, 3)
        want, stats = [], []
        for b in batches:
            want.append(one.filter_batch(*b))
            stats.append(one.stats())
        one.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    for w in want:
        for a in w:
            a.setflags(write=False)
    return refs, batches, [Dev(*b) for b in batches], want, stats


@pytest.fixture
def cuts(monkeypatch):
    monkeypatch.setenv("LNR_HEAVY_CAP", "900")
    monkeypatch.setenv("LNR_MID_CAP", "300")


@pytest.mark.parametrize("h_off", [True, False], ids=["h_off", "null"])
def test_gpu_device_pipeline_equals_the_synchronous_call(ref_run, cuts, monkeypatch, capfd, h_off):
    from linear_amd import Filter
    refs, batches, dbs, want, stats = ref_run
    assert len(batches) == 8
    g = np.load(os.path.join(GOLD, "edge_T3.npz"))
    assert np.array_equal(want[0][0], g["cord_off"]) and np.array_equal(want[0][1], g["cords_str"]) and np.array_equal(want[0][2], g["cords_end"])
    print("per batch:", [{k: s[k] for k in ("remap_reads", "groups_heavy", "groups_mid", "groups_wave1")} for s in stats])
    for key in ("remap_reads", "groups_heavy", "groups_mid", "groups_wave1"):      # the re-map round and every job kernel are reached
        assert any(s[key] > 0 for s in stats), key
    assert want[1][0].tolist() == [0] and want[2][1].size == 0 and want[3][1].size > 0
    monkeypatch.setenv("LNR_DEBUG_TIMES", "1")      # (every batch then reports the lane it ran on)
    f = Filter(device=0)
    f.build_index(refs, 3)
    capfd.readouterr()
    for rnd in range(2):
        got = _pipeline(f, dbs, h_off)
        for k, (w, c) in enumerate(zip(want, got)):
            assert _same(w, c), (rnd, k)
        assert f.stats()["reads"] == batches[-1][1].size - 1          # lnr_last_stats: the batch handed out last
    err = capfd.readouterr().err
    assert err.count("| lane 1 allocations") >= 4 and err.count("| lane 0 allocations") >= 4, "both lanes must have computed batches"
    assert "lane 1 out of memory" not in err
    f.close()


@pytest.mark.parametrize("lanes", [2, 1])
def test_gpu_device_result_lives_until_the_second_next_wait(ref_run, cuts, monkeypatch, lanes):
    """result k's arrays, read again after wait(k + 1) has returned (batch k + 2 and k + 3 are submitted by then and the lanes compute), equal
    the copy taken right after wait(k) -- and that copy is the expected result"""
    from linear_amd import Filter
    refs, batches, dbs, want, _ = ref_run
    if lanes == 1:
        monkeypatch.setenv("LNR_LANES", "1")
    f = Filter(device=0)
    f.build_index(refs, 3)
    n = len(dbs)
    for k in range(2):
        dbs[k].submit(f)
    prev = None
    for k in range(n):
        if k + 2 < n:
            dbs[k + 2].submit(f)
        dev = f.filter_wait_dev()
        now_ = dev_np(dev)
        assert _same(want[k], now_), k
        if prev is not None:
            assert _same(prev[1], dev_np(prev[0])), ("result %d after wait(%d)" % (k - 1, k))
        prev = (dev, now_)
    assert _same(prev[1], dev_np(prev[0]))
    f.close()


def test_gpu_mixed_halves(ref_run, cuts):
    """submit_dev + lnr_filter_wait and lnr_filter_submit + lnr_filter_wait_dev alternate within one round"""
    from linear_amd import Filter
    refs, batches, dbs, want, _ = ref_run
    f = Filter(device=0)
    f.build_index(refs, 3)
    n = len(dbs)

    def submit(k):
        dbs[k].submit(f, h_off=k % 4 == 0) if k % 2 == 0 else f.filter_submit(*batches[k])

    def wait(k):
        # (k % 4: device input + download, host input + device result, device input + device result, host input + download)
        return f.filter_wait() if k % 4 in (0, 3) else dev_np(f.filter_wait_dev())

    for rnd in range(2):
        for k in range(2):
            submit(k)
        for k in range(n):
            if k + 2 < n:
                submit(k + 2)
            assert _same(want[k], wait(k)), (rnd, k)
    f.close()


def test_gpu_limits_and_errors(ref_run, cuts):
    import torch
    from linear_amd import Filter, LnrError
    refs, batches, dbs, want, _ = ref_run
    f = Filter(device=0)
    f.build_index(refs, 3)
    with pytest.raises(LnrError) as e:
        f.filter_wait_dev()
    assert e.value.status == -1
    # three in flight, a fourth refused, the synchronous device call refused, order kept when the batches differ wildly in cost
    order = [3, 1, 0]
    for k in order:
        dbs[k].submit(f)
    with pytest.raises(LnrError) as e:
        dbs[2].submit(f)
    assert e.value.status == -1
    with pytest.raises(LnrError) as e:
        f.filter_batch_dev(dbs[2].reads.data_ptr(), dbs[2].off.data_ptr(), dbs[2].n)
    assert e.value.status == -1
    for k in order:
        assert _same(want[k], dev_np(f.filter_wait_dev())), k
    # a read of 2^20 bases between two good batches: LNR_ERR_LIMIT from the wait that takes it, with and without the host offsets
    big = Dev(np.zeros((1 << 20) + 300, np.uint8), np.array([0, 300, 300 + (1 << 20)], np.uint64))
    for h_off in (True, False):
        dbs[4].submit(f)
        big.submit(f, h_off)
        dbs[6].submit(f)
        assert _same(want[4], dev_np(f.filter_wait_dev()))
        with pytest.raises(LnrError) as e:
            f.filter_wait_dev()
        assert e.value.status == -6 and "2^20" in str(e.value)
        assert _same(want[6], dev_np(f.filter_wait_dev()))
    # the context is usable afterwards, in both forms
    assert _same(want[5], f.filter_batch(*batches[5]))
    dev = f.filter_batch_dev(dbs[7].reads.data_ptr(), dbs[7].off.data_ptr(), dbs[7].n)
    assert _same(want[7], dev_np(dev)) and _same(want[7], f.cords_to_host())
    got = _pipeline(f, dbs[:4])
    for k in range(4):
        assert _same(want[k], got[k]), k
    f.close()
    torch.cuda.synchronize()


_DESTROY = """
import sys
sys.path.insert(0, {root!r})
import numpy as np
import torch
from linear_amd import Filter, synth
ref = synth.random_ref(300_000, 77)
reads, off, _ = synth.sample_reads([ref], 60, 6000, 0.1, 78, "random")
off = np.ascontiguousarray(off, np.uint64)
d_reads = torch.from_numpy(np.ascontiguousarray(reads, np.uint8)).cuda()
d_off = torch.from_numpy(off.view(np.int64)).cuda()
torch.cuda.synchronize()
f = Filter(device=0)
f.build_index([ref], 1)
for k in range(3):
    f.filter_submit_dev(d_reads.data_ptr(), d_off.data_ptr(), off.size - 1, off if k else None)
f.close()
torch.cuda.synchronize()
print("destroyed")
"""


def test_gpu_destroy_with_device_batches_in_flight_returns():
    """lnr_destroy with three device batches submitted and never waited for gives them up and returns (a child process under a time limit;
    the device inputs outlive the context)"""
    from linear_amd import build as lb
    lb.build()
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _DESTROY.format(root=ROOT)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and b"destroyed" in p.stdout, (p.returncode, p.stderr.decode()[-500:])


def test_gpu_gap_path_through_the_device_halves(case_inputs):
    """-g 50 -dup 1 on the inputs of golden edge_g50_T1, split into three batches: through the device halves (serial by design) the batches
    and the stream state after each equal the same batches through lnr_filter_batch_dev on a second context; together they are the golden"""
    from linear_amd import Filter
    refs, reads, off = case_inputs("edge")
    g = np.load(os.path.join(GOLD, "edge_g50_T1.npz"))
    n = off.size - 1
    cut = [0, n // 3, 2 * n // 3, n]
    dbs = [Dev(reads[int(off[a]):int(off[b])], (off[a:b + 1] - off[a]).astype(np.uint64)) for a, b in zip(cut[:-1], cut[1:])]
    one = Filter(device=0, gap_len=50, dup=1)
    one.build_index(refs, 1)
    want, state = [], []
    for d in dbs:
        want.append(dev_np(one.filter_batch_dev(d.reads.data_ptr(), d.off.data_ptr(), d.n)))
        state.append(one.gap_stream())
    one.close()
    assert state[-1] == 1, "the case should contain a read that extends"
    assert np.array_equal(np.concatenate([w[1] for w in want]), g["cords_str_dup1"]) and np.array_equal(np.concatenate([w[2] for w in want]), g["cords_end_dup1"])
    f = Filter(device=0, gap_len=50, dup=1)
    f.build_index(refs, 1)
    for h_off in (True, False):
        assert f.gap_stream(0) == 0
        for d in dbs:
            d.submit(f, h_off)
        for k in range(3):
            assert _same(want[k], dev_np(f.filter_wait_dev())), k
            assert f.gap_stream() == state[k], k
    f.close()


def test_gpu_lane_1_out_of_memory_with_device_batches(ref_run, cuts, monkeypatch, capfd):
    """LNR_LANE1_NOMEM=1 makes lane 1's first batch fail as a full device would: it is run again on lane 0 while results of lane 0 are still
    handed out, no batch reports an error, the results are unchanged and later batches are served by the one lane that is left"""
    from linear_amd import Filter
    refs, batches, dbs, want, _ = ref_run
    monkeypatch.setenv("LNR_LANE1_NOMEM", "1")
    monkeypatch.setenv("LNR_DEBUG_TIMES", "1")
    f = Filter(device=0)
    f.build_index(refs, 3)
    capfd.readouterr()
    got = _pipeline(f, dbs)
    for k, (w, c) in enumerate(zip(want, got)):
        assert _same(w, c), k
    err = capfd.readouterr().err
    assert err.count("lane 1 out of memory") == 1 and "| lane 1 allocations" not in err
    for k in (3, 0, 5):                         # three in flight on the one lane that is left
        dbs[k].submit(f)
    for k in (3, 0, 5):
        assert _same(want[k], dev_np(f.filter_wait_dev())), k
    got = _pipeline(f, dbs)
    for k, (w, c) in enumerate(zip(want, got)):
        assert _same(w, c), k
    assert "lane 1" not in capfd.readouterr().err
    f.close()
