"""GPU (-m gpu): the job kernels address their arrays through typed pointers (global / LDS, lnr_hd.h LNR_GLOBAL / LNR_LDS) wherever the
array's place is fixed by construction, and a pointer typed for the wrong space reads or writes a wrong address.  Every setting that selects
another typed instantiation or another branch of the arena runs the same reads against the oracle, bit for bit:

  default               one wave per read, sorted anchors / DP arrays / block arrays in LDS where they fit
  LNR_JOB_LDS_KB=1      no room in LDS: sorted anchors and block arrays in the job's global scratch (the fallback of `in_lds`)
  LNR_MID_CAP=64 (+ LNR_MID_WAVES=2), LNR_HEAVY_CAP=64
                        reads of 64 anchors and more on 4, 2 and 16 waves: the workgroup radix sort with its LDS cursors

The reads: 500 bases (nearly all with at most 256 anchors: binning's direct exact histogram, in place on the global anchors), 3 kb and
10 kb (more than 256 anchors where they meet a repeat: the hashed pre-filter into the radix buffer first), and 10 kb reads without errors,
which bring more than 128 hits to the window walk (the first 128 live in registers, the rest is read from memory).  The fixture checks
these counts with the oracle alone, on the CPU, so no case passes by being empty.  The library reads its knobs when a context is created, so they are set in a child process
that creates one context per setting; every batch there runs under an alarm, the child under a time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SETTINGS = {
    "default": {},
    "lds1k": {"LNR_JOB_LDS_KB": "1"},
    "waves2": {"LNR_MID_CAP": "64", "LNR_MID_WAVES": "2"},
    "waves4": {"LNR_MID_CAP": "64"},
    "waves16": {"LNR_HEAVY_CAP": "64"},
}
KNOBS = sorted({k for s in SETTINGS.values() for k in s} | {"LNR_MID_LDS_KB", "LNR_HEAVY_LDS_KB", "LNR_MID_CAP_R1", "LNR_HEAVY_CAP_R1", "LNR_STOP_AFTER", "LNR_LANES"})
T = 2
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
    # the checker alone, on the CPU: the cases are not empty, and they are the cases the settings are meant for
    ncords = np.diff(P.want[0].astype(np.int64))
    lens = np.diff(P.off.astype(np.int64))
    for L, least in ((500, 100), (3000, 90), (10000, 60)):
        assert int(np.sum((lens == L) & (ncords > 0))) >= least, f"reads of {L} bases with cords: {int(np.sum((lens == L) & (ncords > 0)))}"
    nanc = np.array([o.stage(r, 0).size for r in rl])
    assert int(np.sum(nanc[lens == 500] <= 256)) >= 100                               # the direct exact histogram
    assert int(np.sum(nanc > 256)) >= 40                                              # the hashed pre-filter
    assert int(np.sum((nanc >= 64) & (nanc < 1000))) >= 20                            # small reads for the multi-wave classes (caps of 64)
    P.max_hits = max(o.stage(rl[i], 5).size for i in np.nonzero(lens == 10000)[0])
    assert P.max_hits > 128, f"no read brings more than 128 hits to the window walk (most: {P.max_hits})"
    o.close()
    return P


@pytest.fixture(scope="module")
def runs(pool, tmp_path_factory):
    td = tmp_path_factory.mktemp("pointer_kinds")
    inp, out = str(td / "in.npz"), str(td / "out.npz")
    np.savez(inp, ref=pool.ref, reads=pool.reads, off=pool.off)
    specs = [",".join([name] + [f"{k}={v}" for k, v in env.items()]) for name, env in SETTINGS.items()]
    code = _CHILD.format(root=ROOT, knobs=KNOBS, limit=BATCH_LIMIT, T=T)
    p = subprocess.run([sys.executable, "-c", code, inp, out] + specs, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)
    print(p.stdout)
    got = dict(np.load(out)) if os.path.exists(out) else {}
    return p, got


@pytest.mark.parametrize("name", list(SETTINGS))
def test_gpu_job_pointer_kinds_match_the_oracle(pool, runs, name):
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


def test_gpu_job_pointer_kinds_child_ended_clean(runs):
    p, _ = runs
    assert p.returncode == 0, p.stderr[-2000:]
