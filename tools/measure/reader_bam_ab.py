"""A/B of BAM input: the bench workload's reads (qualities included) as unaligned BAM and as four-line FASTQ, both BGZF (zlib's default
level, 0xff00-byte payloads) -> profiles/r12/reader_bam_ab.json.  The method of tools/measure/reader_bgzf_ab.py: one process, page cache
warm, one warm-up that also compares the legs' blocks for identity, then alternating repetitions, medians with ranges.

  B   lnr_reader_next_dev on the uBAM (device inflate, k_bam_find / k_bam_stitch / k_bam_emit), with its parts
      (lnr_reader_gpu_times + lnr_reader_gpu_inflate_stats + lnr_reader_gpu_bam_stats)
  Q   lnr_reader_next_dev on the same reads as BGZF four-line FASTQ: the best path there was for the same information
  A   lnr_reader_next on the uBAM (host, gzread; 16 host threads available -- the BAM decode is one inflate stream and uses one)

No rate is fixed in advance; the JSON says which side won every alternation.

--tile-libs name=path,...: variant libraries built with another -DLNR_BAM_TILE (linear_amd.build.build(defines=..., out=...,
only=("lnr_reader_kernels.hip",))).  Leg B is repeated on the same uBAM with each of them, one child process per library (LNR_LIB),
after the alternations: the tile-size comparison.

python tools/measure/reader_bam_ab.py [--reads 100000] [--len 10000] [--reps 3] [--tile-libs ...] [--out profiles/r12/reader_bam_ab.json]"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from reader_bgzf_ab import EOF_BLOCK, PAYLOAD, bgzf_chunk, d2h, med  # noqa: E402


def write_files(d, n, L, seed=5):
    rng = np.random.default_rng(seed)
    paths = {"fq": os.path.join(d, "reads.fq"), "bam": os.path.join(d, "reads.ubam")}
    abc, code = np.frombuffer(b"ACGT", np.uint8), np.array([1, 2, 4, 8], np.uint8)
    hdr_text = b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:bench\tPL:PACBIO\n"
    qual = b"I" * L
    with open(paths["fq"], "wb") as fq, open(paths["bam"], "wb") as bam:
        bam.write(b"BAM\1" + struct.pack("<I", len(hdr_text)) + hdr_text + struct.pack("<i", 0))
        for i in range(n):
            o = rng.integers(0, 4, L)
            name = b"read%d" % i
            fq.write(b"@" + name + b"\n" + abc[o].tobytes() + b"\n+\n" + qual + b"\n")
            c = code[o]
            if L & 1:
                c = np.append(c, np.uint8(0))
            packed = ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes()
            body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 4, L, -1, -1, 0) + name + b"\0" + packed + b"\x28" * L + b"RGZbench\0"
            bam.write(struct.pack("<i", len(body)) + body)
    step = PAYLOAD * 64
    with ProcessPoolExecutor(16) as ex:
        for k in ("fq", "bam"):
            text = open(paths[k], "rb").read()
            paths[k + ".gz"] = paths[k] + ".gz"
            with open(paths[k + ".gz"], "wb") as f:
                for part in ex.map(bgzf_chunk, (text[i:i + step] for i in range(0, len(text), step))):
                    f.write(part)
                f.write(EOF_BLOCK)
            del text
    for p in (paths["fq.gz"], paths["bam.gz"]):  # warm page cache
        with open(p, "rb") as f:
            while f.read(1 << 26):
                pass
    return paths


def child_b(path, reads, length, reps):
    """leg B alone on an existing uBAM with the library LNR_LIB names: one JSON line"""
    from linear_amd.api import Reader
    cap = reads * (length + 8) + (1 << 20)
    out = []
    for rep in range(reps + 1):                  # the first run warms up
        r = Reader(path)
        r.gpu_open(0, 1)
        t0 = time.perf_counter()
        n = r.next_dev(cap, reads)[0]
        t = time.perf_counter() - t0
        assert n == reads
        out.append(dict(r.gpu_bam_stats()["last"], seconds=t, inflate_ms=r.gpu_inflate_stats()["last"]["inflate_ms"]))
        r.close()
    out = out[1:]
    print(json.dumps({"bam_tile": Reader.gpu_bam_tile(), "reads_per_s": med([reads / p["seconds"] for p in out]),
                      "parts": {k: med([p[k] for p in out]) for k in out[0]}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile-libs", default="")
    ap.add_argument("--child-b", default="")
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--len", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "reader_bam_ab.json"))
    a = ap.parse_args()
    if a.child_b:
        return child_b(a.child_b, a.reads, a.len, a.reps)
    from linear_amd import Filter, build as lb
    from linear_amd.api import Reader
    lb.build()
    os.environ["LNR_READER_THREADS"] = "16"
    res = {"reads": a.reads, "read_len": a.len, "reps": a.reps, "payload": PAYLOAD, "bam_tile": Reader.gpu_bam_tile()}
    with tempfile.TemporaryDirectory() as d:
        paths = write_files(d, a.reads, a.len)
        print("files written", {k: os.path.getsize(v) for k, v in paths.items()}, file=sys.stderr, flush=True)
        cap = a.reads * (a.len + 8) + (1 << 20)
        flt = Filter(device=0)
        dst = flt.host_alloc(cap)

        def leg(how):
            r = Reader(paths["fq.gz"] if how == "Q" else paths["bam.gz"])
            if how == "A":
                t0 = time.perf_counter()
                out = r.next(dst, a.reads)
                return time.perf_counter() - t0, out, r
            r.gpu_open(0, 1)
            t0 = time.perf_counter()
            out = r.next_dev(cap, a.reads)
            return time.perf_counter() - t0, out, r

        _, (n, off, ids), r = leg("A")           # warm-up + identity
        r.close()
        want = dst[: int(off[n])].copy()
        for how in ("B", "Q"):
            _, (nd, dr, dof, doff, dids), r = leg(how)
            assert nd == n == a.reads and np.array_equal(doff, off) and dids == ids and np.array_equal(d2h(dr, int(off[n])), want), how
            st = r.gpu_inflate_stats()["last"]
            assert st["blocks"] > 0 and st["gzread_bytes"] == 0
            r.close()
        del want
        T = {k: [] for k in "BQA"}
        parts = {"B": [], "Q": []}
        for rep in range(a.reps):                # alternating: one run of each leg per repetition
            for how in ("B", "Q", "A"):
                t, out, r = leg(how)
                assert out[0] == a.reads
                T[how].append(t)
                if how != "A":
                    tm, st = r.gpu_times(), r.gpu_inflate_stats()["last"]
                    p = dict(tm, inflate_ms=st["inflate_ms"], gather_ms=st["gather_ms"], blocks=st["blocks"], compressed_bytes=st["compressed_bytes"], text_bytes=st["text_bytes"])
                    if how == "B":
                        p.update({k: v for k, v in r.gpu_bam_stats()["last"].items()})
                    parts[how].append(p)
                r.close()
            print("repetition", rep, {k: round(T[k][-1], 3) for k in T}, file=sys.stderr, flush=True)
        flt.close()
        res["tile_sizes"] = {}
        for item in filter(None, a.tile_libs.split(",")):
            name, lib = item.split("=")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-b", paths["bam.gz"], "--reads", str(a.reads), "--len", str(a.len), "--reps", str(a.reps)],
                               env=dict(os.environ, LNR_LIB=os.path.abspath(lib)), stdout=subprocess.PIPE, timeout=600)
            assert p.returncode == 0, name
            res["tile_sizes"][name] = json.loads(p.stdout.decode().splitlines()[-1])
            print("tile variant", name, res["tile_sizes"][name]["reads_per_s"], file=sys.stderr, flush=True)
        res.update({
            "file_bytes": {k: os.path.getsize(paths[k]) for k in paths},
            "reads_per_s": {k: med([a.reads / t for t in T[k]]) for k in T},
            "seconds": T,
            "winner_B_vs_Q_per_alternation": ["B" if b < q else "Q" for b, q in zip(T["B"], T["Q"])],
            "winner_B_vs_A_per_alternation": ["B" if b < x else "A" for b, x in zip(T["B"], T["A"])],
            "B_parts": {k: med([p[k] for p in parts["B"]]) for k in parts["B"][0]},
            "Q_parts": {k: med([p[k] for p in parts["Q"]]) for k in parts["Q"][0]},
            "B_find_plus_stitch_over_inflate": med([(p["find_ms"] + p["stitch_ms"]) / p["inflate_ms"] for p in parts["B"]]),
            "not_measured": "the front-end's read phase (linear_filter with a BAM read file, with and without --gpu-reader)"})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
