"""GPU (-m gpu): the single-wave job kernel at five waves per SIMD (96 VGPRs, 20 workgroups per CU).  What changed with it in the job
code is reached by these settings, each compared with the oracle bit for bit:

  default               one wave per read: the value-type arena (LDS first, the job's global scratch behind it), the block arrays placed
                        in LDS after the anchor traceback (`in_lds`)
  LNR_JOB_LDS_KB=1      next to no LDS: every array falls through to the global region, and the `in_lds` placement is given up -- the
                        arrays are carved again from the arena's marks
  LNR_MID_CAP=64 (+ LNR_MID_WAVES=2), LNR_HEAVY_CAP=64
                        reads of 64 anchors and more on 4, 2 and 16 waves: the shared objects that exist only for NW > 1 (JobShare)

The fixture checks with the oracle alone, on the CPU, that the reads are the cases meant: at least 20 bring more than 140 anchors into
the chaining DP (52 B per anchor: beyond 6 KB, so their DP arrays straddle LDS and global scratch at every arena size up to that), at
least 20 bring fewer than 100, and at least 20 fewer than 64 (all arrays in LDS at the 4 KB the kernel is launched with).  One more test
reads the line LNR_DEBUG_OCC=1 prints: the runtime's count of k_job workgroups per CU at the launch configuration must be 20.
The library reads its knobs when a context is created, so they are set in a child process that creates one context per setting; every
batch there runs under an alarm, the child under a time limit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SETTINGS = {
    "default": {"LNR_DEBUG_OCC": "1"},
    "lds1k": {"LNR_JOB_LDS_KB": "1"},
    "waves2": {"LNR_MID_CAP": "64", "LNR_MID_WAVES": "2"},
    "waves4": {"LNR_MID_CAP": "64"},
    "waves16": {"LNR_HEAVY_CAP": "64"},
}
KNOBS = sorted({k for s in SETTINGS.values() for k in s} | {"LNR_MID_LDS_KB", "LNR_HEAVY_LDS_KB", "LNR_MID_CAP_R1", "LNR_HEAVY_CAP_R1", "LNR_STOP_AFTER", "LNR_LANES"})
T = 2
WORKGROUPS_PER_CU = 20    # five waves on each of a CU's four SIMDs
BATCH_LIMIT = 60          # seconds per batch; the stock library takes well under one
CHILD_LIMIT = 300

_CHILD = r"""
import os, signal, sys
sys.path.insert(0, {root!r})
import numpy as np
from linear_amd import build as lb
lb.build()
from linear_amd import Filter
inp, out = sys.argv[1], sys.argv[2]
d = np.load(inp)
res = {{}}
for spec in sys.argv[3:]:
    name, *kv = spec.split(",")
    for k in {knobs!r}:
        os.environ.pop(k, None)
    os.environ.update(dict(x.split("=") for x in kv))
    signal.alarm({limit})          # no handler: a batch that does not come back ends the child here
    f = Filter(device=0)
    f.build_index([d["ref"]], {T})
    coff, cs, ce = f.filter_batch(d["reads"], d["off"])
    st = f.stats()
    f.close()
    signal.alarm(0)
    res[name + "_off"], res[name + "_cs"], res[name + "_ce"] = coff, cs, ce
    print(name, "cords", cs.size, {{k: v for k, v in st.items() if "job" in k or "heavy" in k or "mid" in k}}, flush=True)
    np.savez(out, **res)
"""


class Pool:
    pass


@pytest.fixture(scope="module")
def pool(oracle_lib):
    from linear_amd import synth
    ref = synth.repeat_ref(2_000_000, 99)
    rl = []
    for q, (cnt, L, err) in enumerate([(120, 500, 0.05), (100, 3000, 0.1), (60, 10000, 0.1), (8, 10000, 0.0)]):
        reads, off, _ = synth.sample_reads([ref], cnt, L, err, 9900 + q, "random")
        rl += [reads[int(off[i]):int(off[i + 1])] for i in range(cnt)]
    order = np.random.default_rng(99).permutation(len(rl))
    rl = [rl[int(i)] for i in order]
    P = Pool()
    P.ref = ref
    P.off = np.zeros(len(rl) + 1, np.uint64)
    P.off[1:] = np.cumsum([r.size for r in rl])
    P.reads = np.concatenate(rl)
    assert len(rl) <= 300
    o = oracle_lib.Checker("oracle", [ref], T)
    P.want = o.map_batch(P.reads, P.off, threads=8)[:3]
    # the checker alone, on the CPU: anchors that enter the chaining DP (the x-descending list), per read
    P.m = np.array([o.stage(r, 2).size for r in rl])
    o.close()
    print("anchors into the DP: > 140:", int(np.sum(P.m > 140)), " < 100:", int(np.sum(P.m < 100)), " < 64:", int(np.sum(P.m < 64)))
    assert int(np.sum(P.m > 140)) >= 20, f"reads whose DP arrays straddle LDS and global scratch: {int(np.sum(P.m > 140))}"
    assert int(np.sum((P.m >= 2) & (P.m < 100))) >= 20, f"reads with fewer than 100 anchors in the DP: {int(np.sum((P.m >= 2) & (P.m < 100)))}"
    assert int(np.sum((P.m >= 2) & (P.m < 64))) >= 20, f"reads whose DP arrays are all in LDS: {int(np.sum((P.m >= 2) & (P.m < 64)))}"
    return P


@pytest.fixture(scope="module")
def runs(pool, tmp_path_factory):
    td = tmp_path_factory.mktemp("five_waves")
    inp, out = str(td / "in.npz"), str(td / "out.npz")
    np.savez(inp, ref=pool.ref, reads=pool.reads, off=pool.off)
    specs = [",".join([name] + [f"{k}={v}" for k, v in env.items()]) for name, env in SETTINGS.items()]
    code = _CHILD.format(root=ROOT, knobs=KNOBS, limit=BATCH_LIMIT, T=T)
    p = subprocess.run([sys.executable, "-c", code, inp, out] + specs, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)
    print(p.stdout)
    got = dict(np.load(out)) if os.path.exists(out) else {}
    return p, got


@pytest.mark.parametrize("name", list(SETTINGS))
def test_gpu_job_five_waves_match_the_oracle(pool, runs, name):
    p, got = runs
    assert name + "_off" in got, f"the child ended (status {p.returncode}) before setting {name!r}: {p.stderr[-2000:]}"
    coff, cs, ce = got[name + "_off"], got[name + "_cs"], got[name + "_ce"]
    ooff, ocs, oce = pool.want
    assert ocs.size > 10000
    if not np.array_equal(coff, ooff):
        bad = np.nonzero(np.diff(coff.astype(np.int64)) != np.diff(ooff.astype(np.int64)))[0]
        raise AssertionError(f"{name}: cord counts differ from the oracle for reads {bad[:20].tolist()} ({bad.size} of {ooff.size - 1})")
    d = np.nonzero((cs != ocs) | (ce != oce))[0]
    reads = np.unique(np.searchsorted(ooff, d, side="right") - 1)
    assert d.size == 0, f"{name}: {d.size} cords differ from the oracle, in reads {reads[:20].tolist()} ({reads.size} of {ooff.size - 1})"


def test_gpu_job_five_waves_workgroups_per_cu(runs):
    p, _ = runs
    found = re.findall(r"\[lnr\] k_job: (-?\d+) workgroups per CU at (\d+) B of dynamic LDS", p.stderr)
    print(found)
    assert len(found) == 1, f"one context ran with LNR_DEBUG_OCC=1, lines seen: {found}; stderr: {p.stderr[-1000:]}"
    assert int(found[0][0]) == WORKGROUPS_PER_CU, found


def test_gpu_job_five_waves_child_ended_clean(runs):
    p, _ = runs
    assert p.returncode == 0, p.stderr[-2000:]
