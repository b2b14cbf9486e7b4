#!/usr/bin/env python3
"""What the compact hold and the host tier of the GPU writer's sort mode cost, on the bench workload's cords: one lnr_filter_batch_dev of
--reads synthetic 10 kb reads, then, without SEQ and with it, in rotating order within this process, the whole sorted file's record
members and its index (lnr_writer_sort_begin + lnr_writer_format_bam_gpu + lnr_writer_sort_finish + every lnr_writer_sort_next piece +
lnr_writer_sort_bai + lnr_writer_sort_end: leg B of tools/measure/writer_sort_ab.py) these ways:
    P   the PARENT commit's library (--parent-lib PATH: liblinear_amd.so built from a checkout of the parent)
    B   this tree's library, everything on the device
    S   this tree's library, lnr_writer_sort_begin(1) + lnr_writer_sort_spill: every record goes to pinned host memory and comes back over
        the bus in k_sort_gather
    T   S with the parent's library, where that has the host tier
--reps timed rotations (at least 3) after --warmup; medians and the range (min .. max).  Before any timing the pieces of every leg are
inflated and compared with lnr_writer_sort_host of the host form's records byte for byte, and P's, B's and S's file bytes with each
other.  Prints one JSON line (also written to --out FILE): times, B over P against the range of P's own runs, the per-stage milliseconds
of lnr_sort_info and lnr_sort_hold_info, the bytes held against the record bytes, and what the gather reaches in GB/s.  No ratio is
promised.  NOT measured here: the front-end's write phase to a real file, and a run large enough to need the host tier in earnest."""
import argparse, ctypes as C, gzip, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from linear_amd import build as lb, api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True, metavar="PATH", help="liblinear_amd.so of the parent commit")
ap.add_argument("--workload", choices=["grch38", "chr22"], default="grch38")
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--host-bytes", type=int, default=8 << 30, help="max_host_bytes of leg S")
ap.add_argument("--out", metavar="FILE", help="also write the JSON line to FILE")
a = ap.parse_args()
assert a.reps >= 3 and os.path.exists(a.parent_lib), a.parent_lib
lb.build()
dev = torch.device("cuda", 0)
flt = api.Filter(device=0)
t0 = time.time()
if a.workload == "grch38":
    from linear_amd.synth_torch import grch38_like_cuda, sample_reads_multi_cuda
    gen, offs = grch38_like_cuda(dev, seed=38)
    glen = [int(offs[i + 1] - offs[i]) for i in range(24)]
    flt.build_index_ptrs([gen.data_ptr() + int(o) for o in offs[:-1]], glen, 16)
    d_reads, d_off = sample_reads_multi_cuda(gen, offs, a.reads, 10_000, 0.10, 777)
    h_gen = gen.cpu().numpy()
    genome = [h_gen[int(offs[i]):int(offs[i + 1])] for i in range(24)]
else:
    from linear_amd.synth_torch import sample_reads_cuda
    ref = synth.chr22_like()
    glen = [int(ref.size)]
    flt.build_index([ref], 1)
    d_ref = torch.from_numpy(ref).cuda()
    d_reads, d_off = sample_reads_cuda(d_ref, a.reads, 10_000, 0.10, 777, non_n_start=10_510_000)
    genome = [ref]
torch.cuda.synchronize()
print(f"[writer_sort_hold_ab] {a.workload}: genome, index and {a.reads} reads in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
n = a.reads
flt.filter_batch_dev(d_reads.data_ptr(), d_off.data_ptr(), n)
coff, cs, ce = flt.cords_to_host()
h_reads = np.ascontiguousarray(d_reads.cpu().numpy(), dtype=np.uint8)
h_off = np.ascontiguousarray(d_off.cpu().numpy().view(np.uint64))
rl = np.diff(h_off.astype(np.int64)).astype(np.uint64)
rids = [f"read_{i} len extra={i * 3}" for i in range(n)]
gids = [f"chr{k + 1}" for k in range(len(glen))]


def parent_writer():
    """a Writer over the parent's library: the calls it shares with this tree's, with this tree's prototypes"""
    lib = C.CDLL(a.parent_lib)
    mine = api.load_library()
    for name in api.EXPORTS:
        if hasattr(lib, name):
            getattr(lib, name).argtypes, getattr(lib, name).restype = getattr(mine, name).argtypes, getattr(mine, name).restype
    w = api.Writer.__new__(api.Writer)
    w.lib = lib
    arr = (C.c_char_p * len(gids))(*[g.encode() for g in gids])
    lens = np.array(glen, dtype=np.uint64)
    h = C.c_void_p()
    assert lib.lnr_writer_create(arr, lens.ctypes.data_as(api._u64p), len(gids), C.byref(h)) == 0
    w.h = h
    return w


writers = {"P": parent_writer(), "B": api.Writer(gids, glen)}
writers["S"] = writers["B"]
PARENT_SPILLS = hasattr(writers["P"].lib, "lnr_writer_sort_spill")
if PARENT_SPILLS:
    writers["T"] = writers["P"]                   # T: the parent's library with every record spilled, S's counterpart
for w in (writers["P"], writers["B"]):
    w.set_genome(genome)
    w.gpu_open(0)
    w.set_bgzf(True)
blob, ido = api.Writer._ids(rids)                 # the id blob once: the timed calls go to the library with it
hc = api.LnrCords()
hc.n_reads, hc.n_cords = n, cs.size
hc.cord_off, hc.cords_str, hc.cords_end = (x.ctypes.data_as(api._u64p) for x in (coff, cs, ce))
p_ido, p_off, p_reads, p_rl = ido.ctypes.data_as(api._u64p), h_off.ctypes.data_as(api._u64p), h_reads.ctypes.data_as(api._u8p), rl.ctypes.data_as(api._u64p)
data, size = C.c_void_p(), C.c_uint64()
out = (C.byref(data), C.byref(size))
info, hold = api.LnrSortInfo(), api.LnrSortHoldInfo()


def call(leg, seq, keep=False):
    """the whole sorted file's record members and its index; keep: the pieces' bytes are copied out (the check), else they are only produced"""
    w = writers[leg]
    L = w.lib

    def ck(st):
        assert st == 0, (leg, st, L.lnr_writer_error(w.h))
    ck(L.lnr_writer_sort_begin(w.h, 1 if leg in "ST" else 0))
    if leg in "ST":
        ck(L.lnr_writer_sort_spill(w.h, a.host_bytes))
    ck(L.lnr_writer_format_bam_gpu(w.h, C.byref(hc), p_reads if seq else None, p_off if seq else p_rl, blob, p_ido, *out))
    assert size.value == 0
    ck(L.lnr_writer_sort_finish(w.h, 0, None))
    pieces, total = [], 0
    while True:
        ck(L.lnr_writer_sort_next(w.h, *out))
        if not size.value:
            break
        total += size.value
        if keep:
            pieces.append(C.string_at(data, size.value))
    ck(L.lnr_writer_sort_bai(w.h, 0, *out))
    bai = C.string_at(data, size.value) if keep else size.value
    ck(L.lnr_writer_sort_info_get(w.h, C.byref(info)))
    st = {k: getattr(info, k) for k, _ in api.LnrSortInfo._fields_}
    if hasattr(L, "lnr_writer_sort_hold_info_get"):      # (a parent from before the compact hold has no such call)
        ck(L.lnr_writer_sort_hold_info_get(w.h, C.byref(hold)))
        st.update({k: getattr(hold, k) for k, _ in api.LnrSortHoldInfo._fields_})
    ck(L.lnr_writer_sort_end(w.h))
    return (total, bai, st, pieces) if keep else (total, bai, st)


def med(v):
    return {"ms_median": round(statistics.median(v) * 1e3, 2), "ms_min": round(min(v) * 1e3, 2), "ms_max": round(max(v) * 1e3, 2), "ms": [round(x * 1e3, 2) for x in v]}


LEGS = "PBST" if PARENT_SPILLS else "PBS"
res = {"workload": a.workload, "reads": n, "cords": int(cs.size), "reps": a.reps, "warmup": a.warmup, "write_phase_to_a_file_measured": False, "a_run_that_needs_the_host_tier_measured": False}
for seq in (False, True):
    tag = "seq" if seq else "plain"
    wb = writers["B"]
    want = wb.sort_host(wb.format_bam(coff, cs, ce, None, rids, reads=h_reads, read_off=h_off, threads=16) if seq else wb.format_bam(coff, cs, ce, rl, rids, threads=16))
    files = {}
    for leg in LEGS:
        total, bai, st, pieces = call(leg, seq, keep=True)
        files[leg] = (b"".join(pieces), bai)
        assert gzip.decompress(files[leg][0] + wb.bgzf_eof()) == want, f"{tag} {leg}: the pieces are not sort_host of the host form's records"
        print(f"[writer_sort_hold_ab] {tag} {leg}: pieces checked", file=sys.stderr, flush=True)
    assert all(files[leg] == files["P"] for leg in LEGS), f"{tag}: the legs' file bytes or indexes differ"
    del files, want, pieces
    for _ in range(a.warmup):
        for leg in LEGS:
            call(leg, seq)
    t, stages = {k: [] for k in LEGS}, {k: [] for k in LEGS}
    for rep in range(a.reps):
        for leg in (LEGS[rep % len(LEGS):] + LEGS[:rep % len(LEGS)]):
            t0 = time.perf_counter()
            total, bai, st = call(leg, seq)
            t[leg].append(time.perf_counter() - t0)
            stages[leg].append(st)
        print(f"[writer_sort_hold_ab] {tag}: rotation {rep + 1} of {a.reps}", file=sys.stderr, flush=True)
    r = {}
    for leg in LEGS:
        r[leg] = med(t[leg])
        last = stages[leg][-1]
        r[leg]["info"] = {k: (round(statistics.median(s[k] for s in stages[leg]), 3) if k.endswith("_ms") else last[k]) for k in last}
        r[leg]["info_reps"] = {k: [round(s[k], 4) for s in stages[leg]] for k in last if k.endswith("_ms")}      # every repetition: a spread can be taken
    sB, sS = r["B"]["info"], r["S"]["info"]
    r["record_bytes"], r["held_bytes"] = sB["record_bytes"], sB["held_device_bytes"]
    r["held_over_record_bytes"] = round(sB["held_device_bytes"] / sB["record_bytes"], 4)
    r["B_over_P_time"] = round(r["B"]["ms_median"] / r["P"]["ms_median"], 4)
    r["B_median_above_P_slowest"] = r["B"]["ms_median"] > r["P"]["ms_max"]
    r["S_over_B_time"] = round(r["S"]["ms_median"] / r["B"]["ms_median"], 4)
    for leg, s in [(leg, r[leg]["info"]) for leg in LEGS]:     # bytes written by the gather (S) and bytes it reads (held) per second
        r[leg]["gather_GBps_written"] = round(s["record_bytes"] / s["gather_ms"] / 1e6, 1)
    r["S"]["gather_GBps_read_from_host"] = round(sS["held_host_bytes"] / sS["gather_ms"] / 1e6, 1)
    r["S"]["spill_GBps"] = round(sS["held_host_bytes"] / sS["spill_ms"] / 1e6, 1)
    res[tag] = r
    print(f"[writer_sort_hold_ab] {tag}: {json.dumps(r)}", file=sys.stderr, flush=True)
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
writers["P"].close()
writers["B"].close()
flt.close()
