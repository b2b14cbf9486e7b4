#!/usr/bin/env python3
"""A/B of the GPU writer's BAM output against its SAM + BGZF output on the bench workload's cords: one lnr_filter_batch_dev of --reads
synthetic 10 kb reads, then, with lnr_writer_set_bgzf(1) throughout and in alternating order within this process, the pairs
    sam      lnr_writer_format_gpu(SAM)       against  bam      lnr_writer_format_bam_gpu without SEQ        (host cords uploaded)
    sam_seq  lnr_writer_format_seq_gpu        against  bam_seq  lnr_writer_format_bam_gpu with SEQ
    and the _dev forms of the four on the device cords and reads of the filter call (nothing uploaded but the read ids)
--reps timed repetitions (at least 3) after --warmup, medians and the spread (min .. max) reported.  Before any timing every BAM call's
members are inflated and compared with the host form lnr_writer_format_bam byte for byte.  Prints one JSON line (also written to --out
FILE where given): reads/s, the five gpu_times parts plus deflate_ms and pack_ms, bytes before and after compression, and who won each
alternation.  The SAM + BGZF calls are the comparison target; this tool changes nothing about them.  The front-end's write phase to a
real file is NOT measured here."""
import argparse, ctypes as C, gzip, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from linear_amd import build as lb, api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=["grch38", "chr22"], default="grch38")
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
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
print(f"[writer_bam_ab] {a.workload}: genome, index and {a.reads} reads in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
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
CALLS = {
    "sam": lambda: L.lnr_writer_format_gpu(w.h, C.byref(hc), p_rl, blob, p_ido, 1, *out),
    "bam": lambda: L.lnr_writer_format_bam_gpu(w.h, C.byref(hc), None, p_rl, blob, p_ido, *out),
    "sam_seq": lambda: L.lnr_writer_format_seq_gpu(w.h, C.byref(hc), p_reads, p_off, blob, p_ido, *out),
    "bam_seq": lambda: L.lnr_writer_format_bam_gpu(w.h, C.byref(hc), p_reads, p_off, blob, p_ido, *out),
    "sam_dev": lambda: L.lnr_writer_format_dev(w.h, C.byref(cdev), do, blob, p_ido, 1, *out),
    "bam_dev": lambda: L.lnr_writer_format_bam_dev(w.h, C.byref(cdev), None, do, blob, p_ido, *out),
    "sam_seq_dev": lambda: L.lnr_writer_format_seq_dev(w.h, C.byref(cdev), dr, do, blob, p_ido, *out),
    "bam_seq_dev": lambda: L.lnr_writer_format_bam_dev(w.h, C.byref(cdev), dr, do, blob, p_ido, *out),
}
PAIRS = [("sam", "bam"), ("sam_seq", "bam_seq"), ("sam_dev", "bam_dev"), ("sam_seq_dev", "bam_seq_dev")]


def call(k):
    st = CALLS[k]()
    assert st == 0, (k, st, L.lnr_writer_error(w.h))


# every BAM call's members inflate to the host form
w.set_bgzf(True)
for keys, host in ((("bam", "bam_dev"), w.format_bam(coff, cs, ce, rl, rids, threads=16)),
                   (("bam_seq", "bam_seq_dev"), w.format_bam(coff, cs, ce, None, rids, reads=h_reads, read_off=h_off, threads=16))):
    for k in keys:
        call(k)
        assert gzip.decompress(C.string_at(data, size.value) + w.bgzf_eof()) == host, f"{k}: not the host form's records"
del host


def timed(k):
    t = time.perf_counter()
    call(k)
    dt = time.perf_counter() - t
    parts = w.gpu_times()
    st = w.bgzf_stats()
    parts.update(deflate_ms=st["deflate_ms"], pack_ms=st["pack_ms"])
    return dt, parts, st["text_bytes"], size.value


res = {"workload": a.workload, "reads": n, "cords": int(cs.size), "reps": a.reps, "bgzf": True, "write_phase_to_a_file_measured": False}
for sam, bam in PAIRS:
    for _ in range(a.warmup):
        timed(sam), timed(bam)
    t, parts, sizes = {sam: [], bam: []}, {sam: [], bam: []}, {}
    winners = []
    for rep in range(a.reps):
        for k in ((sam, bam), (bam, sam))[rep % 2]:
            dt, p, raw, comp = timed(k)
            t[k].append(dt)
            parts[k].append(p)
            sizes[k] = (raw, comp)
        winners.append(min((sam, bam), key=lambda k: t[k][-1]))
    r = {"fastest_per_alternation": winners, "bam_faster_in_every_alternation": all(x < y for x, y in zip(t[bam], t[sam]))}
    for k in (sam, bam):
        r[k] = {"reads_per_s": round(n / statistics.median(t[k])), "ms_median": round(statistics.median(t[k]) * 1e3, 2), "ms_min": round(min(t[k]) * 1e3, 2),
                "ms_max": round(max(t[k]) * 1e3, 2), "ms": [round(x * 1e3, 2) for x in t[k]], "bytes_before_deflate": sizes[k][0], "file_bytes": sizes[k][1],
                "parts_ms": {key: round(statistics.median(p[key] for p in parts[k]), 3) for key in parts[k][0]}}
    r["bam_over_sam_time"] = round(statistics.median(t[bam]) / statistics.median(t[sam]), 4)
    r["bam_over_sam_file_bytes"] = round(sizes[bam][1] / sizes[sam][1], 4)
    res[f"{sam}_vs_{bam}"] = r
    print(f"[writer_bam_ab] {sam} vs {bam}: {json.dumps(r)}", file=sys.stderr, flush=True)
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
w.close()
flt.close()
