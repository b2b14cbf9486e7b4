"""A/B of the reader and its GPU twin on the bench workload's reads written as FASTA, four-line FASTQ and gzip -> profiles/r08/reader_ab.json.

All in one process, page cache warm (every file is read once before anything is timed), REPS alternating repetitions, medians and ranges:
  host    lnr_reader_next on 16 threads into a pinned block
  dev     lnr_reader_next_dev from the file to a device-resident block, with the five lnr_reader_gpu_times fields
  d2d     a plain device-to-device copy of as many bytes as the window's text, in the same run: the yardstick for measure + scan + emit
  cli     the front-end's read phase (-g 0, --gpu-writer) with and without --gpu-reader, alternating, each run under a time limit

python tools/measure/reader_ab.py [--reads 100000] [--len 10000] [--reps 5] [--out profiles/r08/reader_ab.json]"""
import argparse
import gzip
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def write_files(d, n, L, seed=5):
    rng = np.random.default_rng(seed)
    paths = {k: os.path.join(d, "reads." + k) for k in ("fa", "fq", "fa.gz")}
    abc = np.frombuffer(b"ACGT", np.uint8)
    with open(paths["fa"], "wb") as fa, open(paths["fq"], "wb") as fq:
        q = b"I" * L
        for i in range(n):
            s = abc[rng.integers(0, 4, L)].tobytes()
            fa.write(b">read%d\n" % i + s + b"\n")
            fq.write(b"@read%d\n" % i + s + b"\n+\n" + q + b"\n")
    with open(paths["fa"], "rb") as src, gzip.open(paths["fa.gz"], "wb", compresslevel=1) as dst:
        while True:
            b = src.read(1 << 24)
            if not b:
                break
            dst.write(b)
    for p in paths.values():                     # warm page cache
        with open(p, "rb") as f:
            while f.read(1 << 26):
                pass
    return paths


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--len", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--genome", default=None, help="a FASTA genome for the front-end's read phase (default: a random 20 Mb stand-in)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "reader_ab.json"))
    a = ap.parse_args()
    import torch
    from linear_amd import Filter, build as lb
    from linear_amd.api import Reader
    lb.build()
    os.environ["LNR_READER_THREADS"] = "16"
    res = {"reads": a.reads, "read_len": a.len, "reps": a.reps, "files": {}}
    with tempfile.TemporaryDirectory() as d:
        paths = write_files(d, a.reads, a.len)
        cap = a.reads * (a.len + 8) + (1 << 20)
        flt = Filter(device=0)
        dst = flt.host_alloc(cap)
        for kind, path in paths.items():
            host, dev, times, d2d = [], [], [], []
            text_bytes = os.path.getsize(path) if not kind.endswith(".gz") else os.path.getsize(paths["fa"])
            src = torch.empty(text_bytes, dtype=torch.uint8, device="cuda")
            dcp = torch.empty_like(src)
            for rep in range(a.reps + 1):        # repetition 0 warms buffers and is dropped
                r = Reader(path)
                t0 = time.perf_counter()
                n, _, _ = r.next(dst, a.reads)
                th = time.perf_counter() - t0
                r.close()
                r = Reader(path)
                r.gpu_open(0, 1)
                if rep == 0:
                    r.next_dev(cap, 1)           # buffers of the GPU side
                    r.close()
                    r = Reader(path)
                    r.gpu_open(0, 1)
                    r.next_dev(cap, a.reads)
                    r.close()
                    continue
                t0 = time.perf_counter()
                nd = r.next_dev(cap, a.reads)[0]
                td = time.perf_counter() - t0
                tm = r.gpu_times()
                r.close()
                assert n == nd == a.reads
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); dcp.copy_(src); e1.record(); torch.cuda.synchronize()
                host.append(a.reads / th); dev.append(a.reads / td); times.append(tm); d2d.append(e0.elapsed_time(e1))
            res["files"][kind] = {"text_bytes": text_bytes, "host_reads_per_s": med(host), "dev_reads_per_s": med(dev),
                                  "gpu_times_ms": {k: med([t[k] for t in times]) for k in times[0]},
                                  "kernels_ms": med([t["measure_ms"] + t["scan_ms"] + t["emit_ms"] for t in times]), "d2d_copy_ms": med(d2d)}
            del src, dcp
        flt.close()
        genome = a.genome
        if not genome:                           # a stand-in: four random sequences of 5 Mb (the read phase does not depend on what maps)
            genome = os.path.join(d, "genome.fa")
            rng = np.random.default_rng(9)
            with open(genome, "wb") as f:
                for i in range(4):
                    f.write(b">chr%d\n" % i + np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 5_000_000)].tobytes() + b"\n")
        cli = {"default": [], "gpu_reader": []}
        for rep in range(a.reps):                # alternating: one run of each per repetition
            for tag, extra in (("default", []), ("gpu_reader", ["--gpu-reader"])):
                p = subprocess.run(["timeout", "-k", "10", "300", lb.CLI, "filter", paths["fa"], genome, "-g", "0", "-o", os.path.join(d, "o_" + tag), "--gpu-writer"] + extra,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                assert p.returncode == 0, p.stderr.decode()[-500:]
                m = re.search(rb"output files out: ([0-9.]+) s", p.stderr)
                b = re.search(rb"reader ([0-9.]+), GPU", p.stderr)
                cli[tag].append((float(m.group(1)), float(b.group(1))))
        res["front_end"] = {tag: {"read_phase_s": med([t[0] for t in ts]), "reader_busy_s": med([t[1] for t in ts])} for tag, ts in cli.items()}
        res["front_end"]["same_output"] = all(open(os.path.join(d, "o_default" + e), "rb").read() == open(os.path.join(d, "o_gpu_reader" + e), "rb").read() for e in (".sam",))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
