#!/usr/bin/env python3
"""The writer's PAF output measured on the bench workload's cords: one lnr_filter_batch_dev of --reads synthetic 10 kb reads, then, in one
process and after --warmup rounds, --reps alternations (at least 3; the order rotates from alternation to alternation) of three calls on
the downloaded cords:
    sam       lnr_writer_format_gpu(SAM)      host cords uploaded, text downloaded: the GPU writer's existing text form, for scale
    paf       lnr_writer_format_paf_gpu       the same way
    paf_host  lnr_writer_format_paf           the host writer on --threads host threads (16)
Before any timing the GPU's PAF bytes (the host-cord form and the device form) are compared with the host writer's.  Medians and the
range (min .. max) are reported, with the five lnr_writer_gpu_times parts of the two GPU calls.  Prints one JSON line (also written to
--out FILE where given).  Nothing is measured against a threshold.  The front-end's write phase to a real file is NOT measured here."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from linear_amd import build as lb, api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=["grch38", "chr22"], default="grch38")
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--threads", type=int, default=16)
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
else:
    from linear_amd.synth_torch import sample_reads_cuda
    ref = synth.chr22_like()
    glen = [int(ref.size)]
    flt.build_index([ref], 1)
    d_ref = torch.from_numpy(ref).cuda()
    d_reads, d_off = sample_reads_cuda(d_ref, a.reads, 10_000, 0.10, 777, non_n_start=10_510_000)
torch.cuda.synchronize()
print(f"[writer_paf_ab] {a.workload}: genome, index and {a.reads} reads in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
n = a.reads
cdev = flt.filter_batch_dev(d_reads.data_ptr(), d_off.data_ptr(), n)
coff, cs, ce = flt.cords_to_host()
h_off = np.ascontiguousarray(d_off.cpu().numpy().view(np.uint64))
rl = np.diff(h_off.astype(np.int64)).astype(np.uint64)
rids = [f"read_{i} len extra={i * 3}" for i in range(n)]
w = api.Writer([f"chr{k + 1}" for k in range(len(glen))], glen)
w.gpu_open(0)
blob, ido = w._ids(rids)                          # the id blob once: the timed calls go to the library with it
hc = api.LnrCords()
hc.n_reads, hc.n_cords = n, cs.size
hc.cord_off, hc.cords_str, hc.cords_end = (x.ctypes.data_as(api._u64p) for x in (coff, cs, ce))
p_ido, p_rl = ido.ctypes.data_as(api._u64p), rl.ctypes.data_as(api._u64p)
data, size = C.c_void_p(), C.c_uint64()
out = (C.byref(data), C.byref(size))
L = w.lib
CALLS = {
    "sam": lambda: L.lnr_writer_format_gpu(w.h, C.byref(hc), p_rl, blob, p_ido, 1, *out),
    "paf": lambda: L.lnr_writer_format_paf_gpu(w.h, C.byref(hc), p_rl, blob, p_ido, *out),
    "paf_host": lambda: L.lnr_writer_format_paf(w.h, C.byref(hc), p_rl, blob, p_ido, a.threads, *out),
}
ORDER = ["sam", "paf", "paf_host"]


def call(k):
    st = CALLS[k]()
    assert st == 0, (k, st, L.lnr_writer_error(w.h))


# the bytes first: both GPU forms against the host writer
call("paf_host")
host = C.string_at(data, size.value)
call("paf")
assert C.string_at(data, size.value) == host, "lnr_writer_format_paf_gpu: not the host writer's bytes"
assert w.format_paf_dev(cdev, d_off.data_ptr(), rids) == host, "lnr_writer_format_paf_dev: not the host writer's bytes"
paf_lines = host.count(b"\n")
del host


def timed(k):
    t = time.perf_counter()
    call(k)
    dt = time.perf_counter() - t
    return dt, (w.gpu_times() if k != "paf_host" else None), size.value


for _ in range(a.warmup):
    for k in ORDER:
        timed(k)
t, parts, sizes, fastest = {k: [] for k in ORDER}, {k: [] for k in ORDER}, {}, []
for rep in range(a.reps):
    for k in ORDER[rep % 3:] + ORDER[:rep % 3]:
        dt, p, z = timed(k)
        t[k].append(dt)
        parts[k].append(p)
        sizes[k] = z
    fastest.append(min(ORDER, key=lambda k: t[k][-1]))
res = {"workload": a.workload, "reads": n, "cords": int(cs.size), "paf_lines": paf_lines, "reps": a.reps, "warmup": a.warmup, "host_threads": a.threads,
       "gpu_bytes_equal_host_bytes": True, "write_phase_to_a_file_measured": False, "fastest_per_alternation": fastest}
for k in ORDER:
    med = statistics.median(t[k])
    res[k] = {"reads_per_s": round(n / med), "ms_median": round(med * 1e3, 2), "ms_min": round(min(t[k]) * 1e3, 2), "ms_max": round(max(t[k]) * 1e3, 2),
              "ms": [round(x * 1e3, 2) for x in t[k]], "text_bytes": sizes[k]}
    if parts[k][0] is not None:
        res[k]["parts_ms"] = {key: round(statistics.median(p[key] for p in parts[k]), 3) for key in parts[k][0]}
res["paf_gpu_over_sam_gpu_time"] = round(statistics.median(t["paf"]) / statistics.median(t["sam"]), 4)
res["paf_host_over_paf_gpu_time"] = round(statistics.median(t["paf_host"]) / statistics.median(t["paf"]), 4)
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
w.close()
flt.close()
