#!/usr/bin/env python3
"""A/B/C of the SAM writer WITH the SEQ column on the bench workload's cords: one lnr_filter_batch_dev of --reads synthetic 10 kb reads,
then in alternating order within this process
    A  lnr_writer_format_seq, 16 host threads (the baseline)
    B  lnr_writer_format_seq_gpu (host cords and reads uploaded, text in pinned memory)
    C  lnr_writer_format_seq_dev (the batch's device result and device reads in place)
--reps timed repetitions after --warmup, medians reported; the three texts are compared byte for byte first.  Prints one JSON line (also
written to --out FILE where given): reads/s, bytes of text, the GPU side's upload / measure / scan / emit / download milliseconds, the
gate "B faster than A in every alternation", and the emit kernel's traffic figure: (text bytes written + source bytes read) / emit time,
where the source bytes are the SEQ bases (text with SEQ minus text without; an X base reads genome and read, counted once here)."""
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
print(f"[writer_seq_ab] {a.workload}: genome, index and {a.reads} reads in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
n = a.reads
cords_dev = flt.filter_batch_dev(d_reads.data_ptr(), d_off.data_ptr(), n)
coff, cs, ce = flt.cords_to_host()
h_reads = np.ascontiguousarray(d_reads.cpu().numpy(), dtype=np.uint8)
h_off = np.ascontiguousarray(d_off.cpu().numpy().view(np.uint64))
rl = np.diff(h_off.astype(np.int64)).astype(np.uint64)
rids = [f"read_{i} len extra={i * 3}" for i in range(n)]
w = api.Writer([f"chr{k + 1}" for k in range(len(glen))], glen)
w.set_genome(genome)
w.gpu_open(0)
blob, ido = w._ids(rids)
hc = api.LnrCords()
hc.n_reads, hc.n_cords = n, cs.size
hc.cord_off, hc.cords_str, hc.cords_end = (x.ctypes.data_as(api._u64p) for x in (coff, cs, ce))
text, size = C.c_void_p(), C.c_uint64()
p_ido, p_off, p_reads = ido.ctypes.data_as(api._u64p), h_off.ctypes.data_as(api._u64p), h_reads.ctypes.data_as(api._u8p)


def call(which):
    t = time.perf_counter()
    if which == "A":
        st = w.lib.lnr_writer_format_seq(w.h, C.byref(hc), p_reads, p_off, blob, p_ido, a.threads, C.byref(text), C.byref(size))
    elif which == "B":
        st = w.lib.lnr_writer_format_seq_gpu(w.h, C.byref(hc), p_reads, p_off, blob, p_ido, C.byref(text), C.byref(size))
    else:
        st = w.lib.lnr_writer_format_seq_dev(w.h, C.byref(cords_dev), d_reads.data_ptr(), d_off.data_ptr(), blob, p_ido, C.byref(text), C.byref(size))
    dt = time.perf_counter() - t
    assert st == 0, (which, st, w.lib.lnr_writer_error(w.h))
    return dt


res = {"workload": a.workload, "reads": n, "cords": int(cs.size), "reps": a.reps, "host_threads": a.threads}
t_first = call("B")                                           # includes the upload of the writer's own copy of the genome
res["first_B_call_with_genome_upload_ms"] = round(t_first * 1e3, 1)
assert w.lib.lnr_writer_format(w.h, C.byref(hc), rl.ctypes.data_as(api._u64p), blob, p_ido, 1, a.threads, C.byref(text), C.byref(size)) == 0
plain_bytes = size.value
call("A"); ref_text = C.string_at(text, size.value)
for which in "BC":
    call(which)
    assert C.string_at(text, size.value) == ref_text, f"{which}: text differs from lnr_writer_format_seq"
for _ in range(a.warmup):
    for which in "ABC":
        call(which)
t = {k: [] for k in "ABC"}
parts = {k: [] for k in "BC"}
gate = True
for rep in range(a.reps):
    for which in ("ABC", "CBA")[rep % 2]:
        t[which].append(call(which))
        if which != "A":
            parts[which].append(w.gpu_times())
    gate = gate and t["B"][-1] < t["A"][-1]
r = {"text_bytes": len(ref_text), "text_bytes_without_seq": plain_bytes}
for k in "ABC":
    r[k + "_reads_per_s"] = round(n / statistics.median(t[k]))
    r[k + "_ms"] = [round(x * 1e3, 2) for x in t[k]]
for k in "BC":
    r[k + "_parts_ms"] = {key: round(statistics.median(p[key] for p in parts[k]), 3) for key in parts[k][0]}
emit_s = r["C_parts_ms"]["emit_ms"] / 1e3
r["emit_traffic_bytes"] = 2 * len(ref_text) - plain_bytes
r["emit_TB_per_s"] = round(r["emit_traffic_bytes"] / emit_s / 1e12, 3) if emit_s > 0 else None
res["sam_seq"] = r
res["gate_B_faster_than_A_in_every_alternation"] = gate
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
w.close()
flt.close()
