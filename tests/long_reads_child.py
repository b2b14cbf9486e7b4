"""Child process of tests/test_gpu_long_reads.py: the library reads its LNR_* knobs when a context is created, and long inputs are where a
loop that does not end would show -- so every group of settings runs here, each batch under an alarm (no handler: a batch that does not come
back ends the child), and the results go to the parent through an .npz that is written again after every setting.

    long_reads_child.py <in.npz> <out.npz> <specs.json> <seconds per batch>

specs.json: [{"name": ..., "mode": ..., "env": {...}, ...}].  Keys of the output carry the spec's name in front."""
import ctypes as C
import hashlib
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from linear_amd import build as lb  # noqa: E402

lb.build()
from linear_amd import Filter  # noqa: E402
from linear_amd.api import LnrError, Reader, Writer  # noqa: E402

KNOBS = ["LNR_HEAVY_CAP", "LNR_MID_CAP", "LNR_MID_WAVES", "LNR_JOB_LDS_KB", "LNR_CAP_SHRINK", "LNR_MID_LDS_KB", "LNR_HEAVY_LDS_KB", "LNR_MID_CAP_R1",
         "LNR_HEAVY_CAP_R1", "LNR_STOP_AFTER", "LNR_LANES"]
STAT_KEYS = ("jobs", "samples", "lookups", "bucket_entries", "anchors", "remap_reads", "cords", "job_launches", "gap_second_pass", "gap_last_launch", "groups_heavy", "groups_mid", "groups_wave1")

inp, outp, specp, LIMIT = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
D = np.load(inp)
REFS = [D["ref0"], D["ref1"]]
res = {}
_hip = None


def d2h(ptr, nbytes):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(max(nbytes, 1), np.uint8)
    if nbytes:
        assert _hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
    return out[:nbytes]


class batch:
    """one batch under the alarm; its wall time goes to the output"""

    def __init__(self, key):
        self.key = key

    def __enter__(self):
        signal.alarm(LIMIT)
        self.t = time.time()

    def __exit__(self, *exc):
        signal.alarm(0)
        res[self.key + "_sec"] = np.float64(time.time() - self.t)
        return False


def put_cords(key, c):
    res[key + "_off"], res[key + "_cs"], res[key + "_ce"] = c


def put_stats(key, f):
    st = f.stats()
    res[key + "_stats"] = np.array([st[k] for k in STAT_KEYS], np.uint64)
    print(key, {k: st[k] for k in STAT_KEYS}, f"job_ms {st['job_ms']:.1f} total_ms {st['total_ms']:.1f} gap_ms {st['gap_ms']:.1f}", flush=True)


def reads_of(tag):
    return D[tag + "_reads"], D[tag + "_off"]


def mode_map(s):
    """build the index, [raw anchors], the cords, the counters, [apx gaps]"""
    name = s["name"]
    reads, off = reads_of(s["reads"])
    f = Filter(device=0, scratch_budget=s.get("scratch_budget", 0), index_type=s.get("index_type", 1))
    with batch(name + "_index"):
        f.build_index(REFS, s.get("T", 1))
    if s.get("anchors"):
        with batch(name + "_seed"):
            res[name + "_aoff"], res[name + "_anc"] = f.seed_lookup_batch(reads, off)
    try:
        with batch(name):
            put_cords(name, f.filter_batch(reads, off))
    except LnrError as e:
        res[name + "_status"], res[name + "_msg"] = np.int64(e.status), np.array(str(e))
        print(name, "refused:", e, flush=True)
        f.close()
        return
    put_stats(name, f)
    if s.get("gaps"):
        res[name + "_goff"], res[name + "_gaps"] = f.last_gaps()
    f.close()


def mode_neighbours(s):
    name = s["name"]
    mixed, alone = reads_of("mixed"), reads_of("short")
    f = Filter(device=0)
    with batch(name + "_index"):
        f.build_index(REFS, 1)
    with batch(name + "_alone"):
        put_cords(name + "_alone", f.filter_batch(*alone))
    with batch(name + "_mixed"):
        put_cords(name + "_mixed", f.filter_batch(*mixed))
    # lnr_filter_submit / _wait, two batches in flight
    with batch(name + "_pipe"):
        f.filter_submit(*mixed)
        f.filter_submit(*alone)
        put_cords(name + "_pipe_mixed", f.filter_wait())
        put_cords(name + "_pipe_alone", f.filter_wait())
    # a read of 2^20 bases is refused, and the context goes on
    try:
        with batch(name + "_limit"):
            f.filter_batch(np.zeros(1 << 20, np.uint8), np.array([0, 1 << 20], np.uint64))
        res[name + "_limit_status"] = np.int64(0)
    except LnrError as e:
        res[name + "_limit_status"], res[name + "_limit_msg"] = np.int64(e.status), np.array(str(e))
    # ... and so is a reference sequence of 2^30 - 2^20 bases (the length is checked before a base is read); the index stays
    try:
        f.build_index_ptrs([REFS[0].ctypes.data], [(1 << 30) - (1 << 20)], 1)
        res[name + "_seq_limit_status"] = np.int64(0)
    except LnrError as e:
        res[name + "_seq_limit_status"], res[name + "_seq_limit_msg"] = np.int64(e.status), np.array(str(e))
    with batch(name + "_after"):
        put_cords(name + "_after", f.filter_batch(*mixed))
    f.close()


def mode_gap(s):
    name = s["name"]
    reads, off = reads_of(s["reads"])
    f = Filter(device=0, gap_len=s["gap_len"], dup=s["dup"])
    with batch(name + "_index"):
        f.build_index(REFS, 1)
    with batch(name):
        put_cords(name, f.filter_batch(reads, off))
    put_stats(name, f)
    res[name + "_ext"] = np.int64(f.gap_stream())
    if s.get("split"):
        n = off.size - 1
        cuts = [0, 2, n // 3, n]
        assert f.gap_stream(0) == 0
        parts = []
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            with batch(f"{name}_part{k}"):
                parts.append(f.filter_batch(np.ascontiguousarray(reads[int(off[a]):int(off[b])]), (off[a:b + 1] - off[a]).astype(np.uint64)))
        res[name + "_split_cs"] = np.concatenate([p[1] for p in parts])
        res[name + "_split_ce"] = np.concatenate([p[2] for p in parts])
        res[name + "_split_n"] = np.concatenate([np.diff(p[0].astype(np.int64)) for p in parts])
        res[name + "_split_ext"] = np.int64(f.gap_stream())
    f.close()


def put_bytes(key, data, full):
    res[key + "_len"] = np.int64(len(data))
    res[key + "_sha"] = np.array(hashlib.sha256(data).hexdigest())
    if full:
        res[key] = np.frombuffer(data, np.uint8)


def mode_files(s):
    """GPU reader -> filter_batch_dev -> GPU writer (SAM with SEQ, APF, BAM with SEQ) on the files of the `long` case"""
    name = s["name"]
    gid = [f"chr{k + 1}" for k in range(len(REFS))]
    f = Filter(device=0)
    with batch(name + "_index"):
        f.build_index(REFS, 1)
    w = Writer(gid, [r.size for r in REFS])
    w.gpu_open(0)
    w.set_genome(REFS)
    for tag, path in s["files"].items():
        for mr in s["block_reads"]:
            r = Reader(path)
            r.gpu_open(0, 2)
            if s["plain_gzip"].get(tag):
                r.gpu_gzip(True)
            k = 0
            while True:
                key = f"{name}_{tag}_{mr}_{k}"
                with batch(key):
                    n, dr, dof, off, ids = r.next_dev(s["dst_cap"], mr)
                    if n:
                        bases = d2h(dr, int(off[n])).copy()
                        dev = f.filter_batch_dev(dr, dof, n)
                        w.set_bgzf(False)
                        sam = w.format_seq_dev(dev, dr, dof, ids)
                        apf = w.format_dev(dev, dof, ids, "apf")
                        bam = w.format_bam_dev(dev, dof, ids, dr)
                        w.set_bgzf(True)
                        bgz = w.format_bam_dev(dev, dof, ids, dr)
                        w.set_bgzf(False)
                if n == 0:
                    break
                full = tag == s["full"]
                res[key + "_off"], res[key + "_ids"] = off, np.array("\n".join(ids))
                put_bytes(key + "_bases", bases.tobytes(), False)
                put_bytes(key + "_sam", sam, full)
                put_bytes(key + "_apf", apf, full)
                put_bytes(key + "_bam", bam, full)
                put_bytes(key + "_bgz", bgz, True)
                k += 1
            res[f"{name}_{tag}_{mr}_blocks"] = np.int64(k)
            r.close()
            print(name, tag, mr, "blocks", k, flush=True)
    res[name + "_eof"] = np.frombuffer(w.bgzf_eof(), np.uint8)
    w.close()
    f.close()


MODES = {"map": mode_map, "neighbours": mode_neighbours, "gap": mode_gap, "files": mode_files}

for spec in json.load(open(specp)):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(spec.get("env", {}))
    MODES[spec["mode"]](spec)
    res[spec["name"] + "_done"] = np.int64(1)
    np.savez(outp, **res)
