#!/usr/bin/env python3
"""What the coordinate sort of the GPU writer costs, on the bench workload's cords: one lnr_filter_batch_dev of --reads synthetic 10 kb reads,
then, without SEQ and with it, in alternating order within this process,
    A   lnr_writer_format_bam_gpu with lnr_writer_set_bgzf(1): today's unsorted file's record members (the behaviour the sort leaves alone)
    B   lnr_writer_sort_begin + the same call + lnr_writer_sort_finish + every lnr_writer_sort_next piece + lnr_writer_sort_bai + lnr_writer_sort_end
and, --host-reps times, the host yardstick
    H   lnr_writer_format_bam (16 threads) + lnr_writer_sort_host + zlib level 1 per 0xff00 bytes on 16 host threads
--reps timed alternations (at least 3) after --warmup; medians and the range (min .. max).  Before any timing B's pieces are inflated and
compared with lnr_writer_sort_host of the host form's records byte for byte.  Prints one JSON line (also written to --out FILE): times,
B over A, the per-stage milliseconds of lnr_sort_info and the device bytes held.  No ratio is promised.  The front-end's write phase to a
real file is NOT measured here."""
import argparse, ctypes as C, gzip, json, os, statistics, sys, time, zlib
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from linear_amd import build as lb, api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=["grch38", "chr22"], default="grch38")
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--host-reps", type=int, default=2)
ap.add_argument("--out", metavar="FILE", help="also write the JSON line to FILE")
a = ap.parse_args()
assert a.reps >= 3
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
print(f"[writer_sort_ab] {a.workload}: genome, index and {a.reads} reads in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
n = a.reads
cdev = flt.filter_batch_dev(d_reads.data_ptr(), d_off.data_ptr(), n)
coff, cs, ce = flt.cords_to_host()
h_reads = np.ascontiguousarray(d_reads.cpu().numpy(), dtype=np.uint8)
h_off = np.ascontiguousarray(d_off.cpu().numpy().view(np.uint64))
rl = np.diff(h_off.astype(np.int64)).astype(np.uint64)
rids = [f"read_{i} len extra={i * 3}" for i in range(n)]
w = api.Writer([f"chr{k + 1}" for k in range(len(glen))], glen)
w.set_genome(genome)
w.gpu_open(0)
dr, do = C.c_void_p(d_reads.data_ptr()), C.c_void_p(d_off.data_ptr())
blob, ido = w._ids(rids)                          # the id blob once: the timed calls go to the library with it
hc = api.LnrCords()
hc.n_reads, hc.n_cords = n, cs.size
hc.cord_off, hc.cords_str, hc.cords_end = (x.ctypes.data_as(api._u64p) for x in (coff, cs, ce))
p_ido, p_off, p_reads, p_rl = ido.ctypes.data_as(api._u64p), h_off.ctypes.data_as(api._u64p), h_reads.ctypes.data_as(api._u8p), rl.ctypes.data_as(api._u64p)
data, size = C.c_void_p(), C.c_uint64()
out = (C.byref(data), C.byref(size))
L = w.lib
BLOCK = 0xff00
info = api.LnrSortInfo()


def ck(st):
    assert st == 0, (st, L.lnr_writer_error(w.h))


def bam(seq):
    ck(L.lnr_writer_format_bam_gpu(w.h, C.byref(hc), p_reads if seq else None, p_off if seq else p_rl, blob, p_ido, *out))


def call_a(seq, keep=False):
    bam(seq)
    return size.value


def call_b(seq, keep=False):
    """the whole sorted file's record members and its index; keep: the pieces' bytes are copied out (the check), else they are only produced"""
    ck(L.lnr_writer_sort_begin(w.h, 0))
    bam(seq)
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
    bai = size.value
    ck(L.lnr_writer_sort_info_get(w.h, C.byref(info)))
    st = {k: getattr(info, k) for k, _ in api.LnrSortInfo._fields_}
    ck(L.lnr_writer_sort_end(w.h))
    return (total, bai, st, pieces) if keep else (total, bai, st)


def host_form(seq):
    return w.format_bam(coff, cs, ce, None, rids, reads=h_reads, read_off=h_off, threads=16) if seq else w.format_bam(coff, cs, ce, rl, rids, threads=16)


def call_h(seq):
    srt = w.sort_host(host_form(seq))
    view = memoryview(srt)

    def member(i):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        return len(c.compress(view[i:i + BLOCK]) + c.flush()) + 26
    with ThreadPoolExecutor(16) as ex:
        return sum(ex.map(member, range(0, len(srt), BLOCK)))


w.set_bgzf(True)
res = {"workload": a.workload, "reads": n, "cords": int(cs.size), "reps": a.reps, "host_reps": a.host_reps, "write_phase_to_a_file_measured": False}
for seq in (False, True):
    tag = "seq" if seq else "plain"
    want = w.sort_host(host_form(seq))
    total, bai, st, pieces = call_b(seq, keep=True)
    assert gzip.decompress(b"".join(pieces) + w.bgzf_eof()) == want, f"{tag}: the pieces are not sort_host of the host form's records"
    del pieces, want
    for _ in range(a.warmup):
        call_a(seq), call_b(seq)
    t, stages, winners = {"A": [], "B": []}, [], []
    for rep in range(a.reps):
        for k in ("AB", "BA")[rep % 2]:
            t0 = time.perf_counter()
            r = (call_a if k == "A" else call_b)(seq)
            t[k].append(time.perf_counter() - t0)
            if k == "A":
                a_bytes = r
            else:
                b_bytes, bai_bytes, st = r
                stages.append(st)
        winners.append("A" if t["A"][-1] < t["B"][-1] else "B")
    th = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        h_bytes = call_h(seq)
        th.append(time.perf_counter() - t0)
    r = {"fastest_per_alternation": winners}
    for k, v in (("A", t["A"]), ("B", t["B"]), ("H", th)):
        r[k] = {"reads_per_s": round(n / statistics.median(v)), "ms_median": round(statistics.median(v) * 1e3, 2), "ms_min": round(min(v) * 1e3, 2), "ms_max": round(max(v) * 1e3, 2),
                "ms": [round(x * 1e3, 2) for x in v]}
    r["A"]["file_bytes"], r["B"]["file_bytes"], r["B"]["bai_bytes"], r["H"]["file_bytes"] = a_bytes, b_bytes, bai_bytes, h_bytes
    r["B_over_A_time"] = round(statistics.median(t["B"]) / statistics.median(t["A"]), 4)
    r["H_over_B_time"] = round(statistics.median(th) / statistics.median(t["B"]), 4)
    r["sort_info"] = {k: (round(statistics.median(s[k] for s in stages), 3) if k.endswith("_ms") else stages[-1][k]) for k in stages[-1]}
    res[tag] = r
    print(f"[writer_sort_ab] {tag}: {json.dumps(r)}", file=sys.stderr, flush=True)
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
w.close()
flt.close()
