#!/usr/bin/env python3
"""A/B/C of the GPU writer's BGZF output on the bench workload's cords: one lnr_filter_batch_dev of --reads synthetic 10 kb reads, then for
each kind of text (SAM, APF, SAM with SEQ), in alternating order within this process
    A  the _gpu format call with the switch off (plain text in pinned memory: the call as it was before the switch existed)
    B  the same call after lnr_writer_set_bgzf(1) (BGZF members in pinned memory)
    C  A, then the text cut into the same 0xff00-byte blocks and compressed by zlib level 1 on --threads host threads (what a user of
       the plain text could do)
--reps timed repetitions after --warmup, medians reported.  Before any timing B's members are inflated and compared with A's text byte for
byte, and so are C's.  Prints one JSON line (also written to --out FILE where given): reads/s of A, B and C and which won each
alternation, text GB/s of the deflate kernel, the five gpu_times parts plus deflate_ms and pack_ms, and the compressed size against C's
and against zlib level 6 on the same blocks.  The front-end's write phase to a real file is NOT measured here."""
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
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--kinds", default="sam,apf,sam_seq")
ap.add_argument("--out", metavar="FILE", help="also write the JSON line to FILE")
a = ap.parse_args()
lb.build()
BLOCK = 0xff00
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
print(f"[writer_bgzf_ab] {a.workload}: genome, index and {a.reads} reads in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
n = a.reads
flt.filter_batch_dev(d_reads.data_ptr(), d_off.data_ptr(), n)
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
p_ido, p_off, p_reads, p_rl = ido.ctypes.data_as(api._u64p), h_off.ctypes.data_as(api._u64p), h_reads.ctypes.data_as(api._u8p), rl.ctypes.data_as(api._u64p)
pool = ThreadPoolExecutor(a.threads)


def fmt(kind):
    if kind == "sam_seq":
        st = w.lib.lnr_writer_format_seq_gpu(w.h, C.byref(hc), p_reads, p_off, blob, p_ido, C.byref(text), C.byref(size))
    else:
        st = w.lib.lnr_writer_format_gpu(w.h, C.byref(hc), p_rl, blob, p_ido, 1 if kind == "sam" else 2, C.byref(text), C.byref(size))
    assert st == 0, (kind, st, w.lib.lnr_writer_error(w.h))


def zblock(view, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(view) + c.flush()


def host_deflate(level):
    """the bytes of the last call's text in 0xff00 blocks by zlib on the pool; returns the payloads"""
    buf = (C.c_char * size.value).from_address(text.value)
    mv = memoryview(buf)
    return list(pool.map(lambda o: zblock(mv[o:o + BLOCK], level), range(0, size.value, BLOCK)))


def call(kind, which):
    w.set_bgzf(which == "B")
    t = time.perf_counter()
    fmt(kind)
    out = host_deflate(1) if which == "C" else None
    return time.perf_counter() - t, out


res = {"workload": a.workload, "reads": n, "cords": int(cs.size), "reps": a.reps, "host_threads": a.threads, "write_phase_to_a_file_measured": False}
for kind in a.kinds.split(","):
    _, _ = call(kind, "A")
    plain = C.string_at(text, size.value)
    call(kind, "B")
    members = C.string_at(text, size.value)
    assert gzip.decompress(members + w.bgzf_eof()) == plain, f"{kind}: B does not inflate to A's text"
    stats = w.bgzf_stats()
    _, c_payloads = call(kind, "C")
    assert b"".join(zlib.decompress(p, -15) for p in c_payloads) == plain, f"{kind}: C does not inflate to A's text"
    c_bytes = sum(len(p) + 26 for p in c_payloads)
    z6_bytes = sum(len(p) + 26 for p in host_deflate(6))
    for _ in range(a.warmup):
        for which in "ABC":
            call(kind, which)
    t = {k: [] for k in "ABC"}
    parts, bz = {k: [] for k in "AB"}, []
    winners = []
    for rep in range(a.reps):
        for which in ("ABC", "CBA")[rep % 2]:
            t[which].append(call(kind, which)[0])
            if which in parts:
                parts[which].append(w.gpu_times())
            if which == "B":
                bz.append(w.bgzf_stats())
        winners.append(min("ABC", key=lambda k: t[k][-1]))
    r = {"text_bytes": len(plain), "B_compressed_bytes": len(members), "C_zlib1_bytes": c_bytes, "zlib6_bytes": z6_bytes,
         "B_over_C_size": round(len(members) / c_bytes, 4), "B_over_zlib6_size": round(len(members) / z6_bytes, 4),
         "blocks": stats["blocks"], "stored_blocks": stats["stored_blocks"], "fastest_per_alternation": winners,
         "B_faster_than_C_in_every_alternation": all(x < y for x, y in zip(t["B"], t["C"])),
         "B_faster_than_A_in_every_alternation": all(x < y for x, y in zip(t["B"], t["A"]))}
    for k in "ABC":
        r[k + "_reads_per_s"] = round(n / statistics.median(t[k]))
        r[k + "_ms"] = [round(x * 1e3, 2) for x in t[k]]
    for k in "AB":
        r[k + "_parts_ms"] = {key: round(statistics.median(p[key] for p in parts[k]), 3) for key in parts[k][0]}
    d_ms, p_ms = statistics.median(b["deflate_ms"] for b in bz), statistics.median(b["pack_ms"] for b in bz)
    r["B_parts_ms"].update(deflate_ms=round(d_ms, 3), pack_ms=round(p_ms, 3))
    r["deflate_text_GB_per_s"] = round(len(plain) / d_ms / 1e6, 2)
    r["deflate_reads_per_s"] = round(n / (d_ms / 1e3))
    res[kind] = r
    print(f"[writer_bgzf_ab] {kind}: {json.dumps(r)}", file=sys.stderr, flush=True)
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
w.close()
flt.close()
