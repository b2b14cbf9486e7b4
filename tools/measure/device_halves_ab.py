#!/usr/bin/env python3
"""A/B/C of the device form of the filter on the bench workload's reads (the GRCh38 stand-in, --reads synthetic 10 kb reads per batch,
--distinct different batches resident on the device), one process, one GPU, in alternating order:
    A   a loop of lnr_filter_batch_dev, one batch at a time
    B   submit_dev(0); submit_dev(1); loop { submit_dev(k + 2); wait_dev(k) }
    CA  A, each result followed by lnr_writer_format_dev (SAM)
    CB  B, each result followed by the same call while the lanes compute the next batches
Before any timing the results of A and B are compared with each other, batch by batch.  A leg is --batches batches; after --warmup untimed
legs of each kind, --reps alternations (ABCACB / CBCABA in turn); ms per batch as median and range, and who won each alternation.  Then the
same with -g 50 (serial by design: A and B are expected level) on --gap-batches batches of --gap-reads reads.  Prints one JSON line (also
written to --out FILE)."""
import argparse, ctypes as C, hashlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from linear_amd import build as lb, api

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--distinct", type=int, default=4)
ap.add_argument("--batches", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--gap-reads", type=int, default=20_000)
ap.add_argument("--gap-batches", type=int, default=4)
ap.add_argument("--no-gap", action="store_true")
ap.add_argument("--out", metavar="FILE", help="also write the JSON line to FILE")
a = ap.parse_args()
lb.build()
dev = torch.device("cuda", 0)
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
flt = api.Filter(device=0)
t0 = time.time()
from linear_amd.synth_torch import grch38_like_cuda, sample_reads_multi_cuda
gen, offs = grch38_like_cuda(dev, seed=38)
glen = [int(offs[i + 1] - offs[i]) for i in range(24)]
flt.build_index_ptrs([gen.data_ptr() + int(o) for o in offs[:-1]], glen, 16)
w = api.Writer([f"chr{k + 1}" for k in range(len(glen))], glen)
w.gpu_open(0)
text, size = C.c_void_p(), C.c_uint64()


def make(n, seed0):
    out = []
    for b in range(a.distinct):
        r, o = sample_reads_multi_cuda(gen, offs, n, 10_000, 0.10, seed0 + b)
        out.append((r, o, np.ascontiguousarray(o.cpu().numpy().view(np.uint64))))
    torch.cuda.synchronize()
    return out


def digest(d):
    h = hashlib.sha256()
    for p, k in ((d.d_cord_off, d.n_reads + 1), (d.d_cords_str, d.n_cords), (d.d_cords_end, d.n_cords)):
        buf = np.zeros(max(k, 1), np.uint64)
        if k:
            assert hip.hipMemcpy(buf.ctypes.data, p, k * 8, 2) == 0
        h.update(buf[:k].tobytes())
    return h.hexdigest(), int(d.n_cords)


def run(batches, n, nb, ids):
    blob, p_ido = ids

    def fmt(d, k):
        st = w.lib.lnr_writer_format_dev(w.h, C.byref(d), batches[k % len(batches)][1].data_ptr(), blob, p_ido, 1, C.byref(text), C.byref(size))
        assert st == 0, w.lib.lnr_writer_error(w.h)

    def leg_a(post=None, keep=None):
        t = time.perf_counter()
        for k in range(nb):
            r, o, _ = batches[k % len(batches)]
            d = flt.filter_batch_dev(r.data_ptr(), o.data_ptr(), n)
            if post:
                post(d, k)
            if keep is not None:
                keep.append(digest(d))
        return (time.perf_counter() - t) * 1e3 / nb

    def leg_b(post=None, keep=None):
        def sub(k):
            r, o, ho = batches[k % len(batches)]
            flt.filter_submit_dev(r.data_ptr(), o.data_ptr(), n, ho)
        t = time.perf_counter()
        for k in range(min(2, nb)):
            sub(k)
        for k in range(nb):
            if k + 2 < nb:
                sub(k + 2)
            d = flt.filter_wait_dev()
            if post:
                post(d, k)
            if keep is not None:
                keep.append(digest(d))
        return (time.perf_counter() - t) * 1e3 / nb

    legs = {"A": lambda: leg_a(), "B": lambda: leg_b(), "CA": lambda: leg_a(fmt), "CB": lambda: leg_b(fmt)}
    ka, kb = [], []
    leg_a(keep=ka); leg_b(keep=kb)
    assert ka == kb and all(c > 0 for _, c in ka), "the device halves and lnr_filter_batch_dev disagree"
    for _ in range(a.warmup):
        for k in legs:
            legs[k]()
    t = {k: [] for k in legs}
    wins = {"B_over_A": [], "CB_over_CA": []}
    for rep in range(a.reps):
        for k in (("A", "B", "CA", "CB"), ("CB", "CA", "B", "A"))[rep % 2]:
            t[k].append(legs[k]())
        wins["B_over_A"].append(t["B"][-1] < t["A"][-1])
        wins["CB_over_CA"].append(t["CB"][-1] < t["CA"][-1])
    res = {"reads_per_batch": n, "batches_per_leg": nb, "cords_per_batch": [c for _, c in ka[:len(batches)]]}
    for k in legs:
        res[k] = {"ms_per_batch": [round(x, 2) for x in t[k]], "median": round(statistics.median(t[k]), 2), "min": round(min(t[k]), 2), "max": round(max(t[k]), 2),
                  "reads_per_s": round(n / statistics.median(t[k]) * 1e3)}
    res["wins"] = wins
    res["B_wins_every_alternation"] = all(wins["B_over_A"])
    res["CB_wins_every_alternation"] = all(wins["CB_over_CA"])
    return res


def ids_of(n):
    blob, ido = w._ids([f"read_{i}" for i in range(n)])
    return blob, ido, ido.ctypes.data_as(api._u64p)


out = {"script": "device_halves_ab", "distinct_batches": a.distinct, "reps": a.reps, "warmup": a.warmup}
batches = make(a.reads, 777)
print(f"[device_halves_ab] genome, index and {a.distinct} batches of {a.reads} reads in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
blob, ido, p_ido = ids_of(a.reads)
out["g0"] = run(batches, a.reads, a.batches, (blob, p_ido))
print("[device_halves_ab] -g 0:", json.dumps(out["g0"]), file=sys.stderr, flush=True)
if not a.no_gap:
    del batches
    flt.set_gap(50, 0)
    batches = make(a.gap_reads, 1777)
    blob, ido, p_ido = ids_of(a.gap_reads)
    out["g50"] = run(batches, a.gap_reads, a.gap_batches, (blob, p_ido))
line = json.dumps(out)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
w.close()
flt.close()
