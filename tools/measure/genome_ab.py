#!/usr/bin/env python3
"""What loading the reference genome costs, host loader against lnr_genome_load_gpu, from opening the files to an index that is ready.
One process, warm page cache.  Input: a synthetic genome of 24 sequences with the human chromosome lengths (GRCh38 primary assembly, scaled
by --scale), 60-column FASTA, half of it lower case in stretches, runs of N at both ends of every sequence; written as plain text, as gzip
level 6 (one member) and as BGZF.
    A   what the front-end does without --gpu-genome: lnr_reader_open, lnr_reader_next(max_reads = 1) into a 1 GiB buffer, every sequence
        copied into an array of its own, lnr_index_build from the host pointers (the upload is inside)
    B   lnr_genome_load_gpu + lnr_index_build from the device pointers; on the gzip file also with LNR_GENOME_GPU_GZIP (leg "B_gpu_gzip")
--warmup rotations, then --reps (at least 3) timed alternations A, B(, B_gpu_gzip); per leg the median and the range, and who won every
alternation.  Before timing, B's sequences are compared with A's byte for byte.  After it, one instrumented pass per file with the calls
the loader makes (lnr_reader_gpu_open(1 slot) + lnr_reader_next_dev) collects the reader's own stage times: lnr_reader_gpu_times summed over
the blocks, lnr_reader_gpu_inflate_stats, lnr_reader_gpu_gzip_stats.  Prints one JSON line (also written to --out FILE).  No ratio is
promised.  NOT measured here: a cold page cache, a real assembly's text (its compression ratio and N layout), several genome files."""
import argparse, gzip, json, os, statistics, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from linear_amd import build as lb, api

GRCH38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309,
          114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468, 156040895, 57227415]
ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0, help="factor on the 24 chromosome lengths (1.0 = 3.09 Gb)")
ap.add_argument("--dir", default="/tmp/genome_ab", help="where the three files are written (about 1.6 bytes per base)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--threads", type=int, default=16, help="layout_threads of the index")
ap.add_argument("--out", metavar="FILE")
a = ap.parse_args()
assert a.reps >= 3
lb.build()
lens = [max(1000, int(n * a.scale)) for n in GRCH38]
os.makedirs(a.dir, exist_ok=True)
paths = {k: os.path.join(a.dir, f"genome_{a.scale:g}.{ext}") for k, ext in (("plain", "fa"), ("gzip", "fa.gz"), ("bgzf", "bgzf.fa.gz"))}
note = lambda m: print(f"[genome_ab] {m}", file=sys.stderr, flush=True)


def bgzf_block(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    p = c.compress(data) + c.flush()
    total = 18 + len(p) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (total - 1).to_bytes(2, "little") + p + zlib.crc32(data).to_bytes(4, "little") +
            len(data).to_bytes(4, "little"))


def bgzf_piece(data):
    return b"".join(bgzf_block(data[i:i + 0xff00]) for i in range(0, len(data), 0xff00))


def write_files():
    from concurrent.futures import ProcessPoolExecutor
    rng = np.random.default_rng(38)
    upper, lower = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"acgt", np.uint8)
    t0 = time.time()
    gz = zlib.compressobj(6, zlib.DEFLATED, 31)
    PIECE = 0xff00 * 512
    with open(paths["plain"], "wb") as fp, open(paths["gzip"], "wb") as fg, open(paths["bgzf"], "wb") as fb, ProcessPoolExecutor(min(16, os.cpu_count() or 4)) as pool:
        carry = b""
        for k, n in enumerate(lens):
            o = rng.integers(0, 4, n, dtype=np.uint8)
            s = upper[o]
            for _ in range(max(1, n // 200_000)):                # soft-masked stretches: about half of the sequence
                p = int(rng.integers(0, n)); m = int(rng.integers(1, 200_000))
                s[p:p + m] = lower[o[p:p + m]]
            cap = min(10_000, n // 10)
            s[:cap] = ord("N"); s[n - cap:] = ord("N")
            rows = -(-n // 60)
            pad = np.zeros(rows * 60, np.uint8)
            pad[:n] = s
            t = np.full((rows, 61), ord("\n"), np.uint8)
            t[:, :60] = pad.reshape(rows, 60)
            flat = t.reshape(-1)
            body = flat.tobytes() if n % 60 == 0 else flat[: (rows - 1) * 61 + n % 60].tobytes() + b"\n"
            text = b">chr%d synthetic, GRCh38 length scaled by %g\n" % (k + 1, a.scale) + body
            fp.write(text)
            for i in range(0, len(text), 64 << 20):
                fg.write(gz.compress(text[i:i + (64 << 20)]))
            text = carry + text
            whole = len(text) // PIECE * PIECE
            for piece in pool.map(bgzf_piece, [text[i:i + PIECE] for i in range(0, whole, PIECE)]):
                fb.write(piece)
            carry = text[whole:]
            note(f"wrote chr{k + 1} ({n} bases), {time.time() - t0:.0f} s")
        fg.write(gz.flush())
        fb.write(bgzf_piece(carry) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


if not all(os.path.exists(p) for p in paths.values()):
    write_files()
sizes = {k: os.path.getsize(p) for k, p in paths.items()}
note(f"files: {sizes}")
BUF = np.zeros(max(lens) + 4096, np.uint8)                # (the front-end's buffer is 1 GiB; a record never fills it)


def leg_a(path, keep=False):
    flt = api.Filter(device=0)
    t0 = time.perf_counter()
    r = api.Reader(path)
    seqs = []
    while True:
        n, off, _ = r.next(BUF, 1)
        if n == 0:
            break
        seqs.append(BUF[: int(off[1])].copy())
    r.close()
    t1 = time.perf_counter()
    flt.build_index(seqs, a.threads)
    t2 = time.perf_counter()
    flt.close()
    return {"total_s": t2 - t0, "load_s": t1 - t0, "index_s": t2 - t1}, (seqs if keep else None)


def leg_b(path, gpu_gzip=False, check=None):
    flt = api.Filter(device=0)
    t0 = time.perf_counter()
    g = api.Genome.load_gpu(path, device=0, gpu_gzip=gpu_gzip)
    t1 = time.perf_counter()
    g.build_index(flt, a.threads)
    t2 = time.perf_counter()
    if check is not None:
        host = g.to_host()
        assert g.lens == [s.size for s in check] and all(np.array_equal(x, y) for x, y in zip(host, check)), "B's sequences differ from A's"
    g.close(); flt.close()
    return {"total_s": t2 - t0, "load_s": t1 - t0, "index_s": t2 - t1}


def reader_stages(path, gpu_gzip):
    r = api.Reader(path)
    r.gpu_open(0, 1)
    if gpu_gzip:
        r.gpu_gzip(True)
    sums, blocks = {}, 0
    while True:
        n = r.next_dev(1 << 30, 1024)[0]
        if n == 0:
            break
        blocks += 1
        for k, v in r.gpu_times().items():
            sums[k] = sums.get(k, 0.0) + v
    out = {"blocks": blocks, "gpu_times_ms": sums, "inflate": r.gpu_inflate_stats()["total"]}
    if gpu_gzip:
        out["gzip"] = r.gpu_gzip_stats()["total"]
    r.close()
    return out


result = {"tool": "genome_ab", "scale": a.scale, "bases": sum(lens), "sequences": len(lens), "file_bytes": sizes, "reps": a.reps, "warmup": a.warmup,
          "layout_threads": a.threads, "forms": {}}
for form, path in paths.items():
    legs = {"A": lambda p=path: leg_a(p)[0], "B": lambda p=path: leg_b(p)}
    if form == "gzip":
        legs["B_gpu_gzip"] = lambda p=path: leg_b(p, gpu_gzip=True)
    _, seqs = leg_a(path, keep=True)                      # warms the page cache; the yardstick of the comparison
    leg_b(path, check=seqs)
    if form == "gzip":
        leg_b(path, gpu_gzip=True, check=seqs)
    del seqs
    note(f"{form}: B's sequences equal A's")
    for _ in range(a.warmup):
        for f in legs.values():
            f()
    runs = {k: [] for k in legs}
    winners = []
    for rep in range(a.reps):
        for k, f in legs.items():
            runs[k].append(f())
        winners.append(min(legs, key=lambda k: runs[k][-1]["total_s"]))
        note(f"{form} rep {rep}: " + ", ".join(f"{k} {runs[k][-1]['total_s']:.3f} s" for k in legs))
    summary = {}
    for k, rs in runs.items():
        summary[k] = {f: {"median": statistics.median(r[f] for r in rs), "min": min(r[f] for r in rs), "max": max(r[f] for r in rs)} for f in ("total_s", "load_s", "index_s")}
    stages = {"B": reader_stages(path, False)}
    if form == "gzip":
        stages["B_gpu_gzip"] = reader_stages(path, True)
    result["forms"][form] = {"legs": summary, "winner_of_every_alternation": winners, "reader_stages": stages,
                             "B_over_A": summary["B"]["total_s"]["median"] / summary["A"]["total_s"]["median"]}
line = json.dumps(result)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
