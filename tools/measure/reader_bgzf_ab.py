"""A/B of BGZF input: the bench workload's reads as FASTA and four-line FASTQ, written as BGZF (zlib's default level, 0xff00-byte payloads)
-> profiles/r09/reader_bgzf_ab.json.  The method of tools/measure/reader_ab.py: one process, page cache warm, one warm-up, then
alternating repetitions, medians with ranges; the blocks of the legs are compared for identity before anything is timed.

  A   lnr_reader_next on the BGZF file (host, gzread)
  C   lnr_reader_next_dev with LNR_READER_BGZF=0 (gzread into the pinned staging buffer, parse on the device)
  B   lnr_reader_next_dev with the device inflate, with its parts (lnr_reader_gpu_times + lnr_reader_gpu_inflate_stats)
  D   lnr_reader_next_dev on the plain file
  Z   context, not a leg: 16 Python threads inflate the same blocks with zlib.decompressobj(-15)

Gate: B is faster than A and than C in every alternation.

python tools/measure/reader_bgzf_ab.py [--reads 100000] [--len 10000] [--reps 3] [--out profiles/r09/reader_bgzf_ab.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PAYLOAD = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_chunk(data):
    out = []
    for i in range(0, len(data), PAYLOAD):
        d = data[i:i + PAYLOAD]
        c = zlib.compressobj(-1, zlib.DEFLATED, -15)
        p = c.compress(d) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(p) + 25) + p + struct.pack("<II", zlib.crc32(d), len(d)))
    return b"".join(out)


def write_files(d, n, L, seed=5):
    rng = np.random.default_rng(seed)
    paths = {k: os.path.join(d, "reads." + k) for k in ("fa", "fq")}
    abc = np.frombuffer(b"ACGT", np.uint8)
    with open(paths["fa"], "wb") as fa, open(paths["fq"], "wb") as fq:
        q = b"I" * L
        for i in range(n):
            s = abc[rng.integers(0, 4, L)].tobytes()
            fa.write(b">read%d\n" % i + s + b"\n")
            fq.write(b"@read%d\n" % i + s + b"\n+\n" + q + b"\n")
    step = PAYLOAD * 64
    with ProcessPoolExecutor(16) as ex:
        for k in ("fa", "fq"):
            text = open(paths[k], "rb").read()
            paths[k + ".gz"] = paths[k] + ".gz"
            with open(paths[k + ".gz"], "wb") as f:
                for part in ex.map(bgzf_chunk, (text[i:i + step] for i in range(0, len(text), step))):
                    f.write(part)
                f.write(EOF_BLOCK)
            del text
    for p in paths.values():                     # warm page cache
        with open(p, "rb") as f:
            while f.read(1 << 26):
                pass
    return paths


def payloads(path):
    raw = open(path, "rb").read()
    out, o = [], 0
    while o < len(raw):
        size = struct.unpack_from("<H", raw, o + 16)[0] + 1
        out.append(raw[o + 18:o + size - 8])
        o += size
    return out


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def d2h(ptr, nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(max(nbytes, 1), np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
    return out[:nbytes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--len", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "reader_bgzf_ab.json"))
    a = ap.parse_args()
    from linear_amd import Filter, build as lb
    from linear_amd.api import Reader
    lb.build()
    os.environ["LNR_READER_THREADS"] = "16"
    res = {"reads": a.reads, "read_len": a.len, "reps": a.reps, "payload": PAYLOAD, "files": {}}
    with tempfile.TemporaryDirectory() as d:
        paths = write_files(d, a.reads, a.len)
        cap = a.reads * (a.len + 8) + (1 << 20)
        flt = Filter(device=0)
        dst = flt.host_alloc(cap)

        def leg(path, how):
            """(seconds, n, reader) of one block of the whole file; the reader stays open for its times and its block"""
            os.environ.pop("LNR_READER_BGZF", None)
            if how == "C":
                os.environ["LNR_READER_BGZF"] = "0"
            r = Reader(path)
            os.environ.pop("LNR_READER_BGZF", None)
            if how == "A":
                t0 = time.perf_counter()
                out = r.next(dst, a.reads)
                return time.perf_counter() - t0, out, r
            r.gpu_open(0, 1)
            t0 = time.perf_counter()
            out = r.next_dev(cap, a.reads)
            return time.perf_counter() - t0, out, r

        for kind in ("fa", "fq"):
            gz, plain = paths[kind + ".gz"], paths[kind]
            text_bytes, comp_bytes = os.path.getsize(plain), os.path.getsize(gz)
            # warm-up + identity: the blocks of B, C and D against A's
            _, (n, off, ids), r = leg(gz, "A")
            r.close()
            want = dst[: int(off[n])].copy()
            for how, path in (("B", gz), ("C", gz), ("D", plain)):
                _, (nd, dr, dof, doff, dids), r = leg(path, how)
                assert nd == n == a.reads and np.array_equal(doff, off) and dids == ids and np.array_equal(d2h(dr, int(off[n])), want), (kind, how)
                st = r.gpu_inflate_stats()["last"]
                assert (st["blocks"] > 0 and st["gzread_bytes"] == 0) if how == "B" else st["blocks"] == 0
                r.close()
            del want
            T = {k: [] for k in "ACBD"}
            parts = []
            for rep in range(a.reps):            # alternating: one run of each leg per repetition
                for how, path in (("A", gz), ("C", gz), ("B", gz), ("D", plain)):
                    t, out, r = leg(path, how)
                    assert out[0] == a.reads
                    T[how].append(t)
                    if how == "B":
                        tm, st = r.gpu_times(), r.gpu_inflate_stats()["last"]
                        parts.append(dict(tm, inflate_ms=st["inflate_ms"], gather_ms=st["gather_ms"], blocks=st["blocks"], compressed_bytes=st["compressed_bytes"],
                                          stage_upload_ms=tm["upload_ms"] - st["inflate_ms"]))      # upload_ms is wall time up to the end of the inflate
                    r.close()
            pl = payloads(gz)
            t0 = time.perf_counter()
            with ThreadPoolExecutor(16) as ex:
                total = sum(ex.map(lambda p: len(zlib.decompressobj(-15).decompress(p)), pl, chunksize=64))
            tz = time.perf_counter() - t0
            assert total == text_bytes
            res["files"][kind] = {
                "text_bytes": text_bytes, "compressed_bytes": comp_bytes, "blocks": len(pl),
                "reads_per_s": {k: med([a.reads / t for t in T[k]]) for k in T},
                "seconds": {k: T[k] for k in T},
                "gate_B_faster_than_A_and_C_in_every_alternation": all(b < x and b < c for b, x, c in zip(T["B"], T["A"], T["C"])),
                "B_parts_ms": {k: med([p[k] for p in parts]) for k in parts[0]},
                "inflate_output_GB_per_s": med([text_bytes / p["inflate_ms"] / 1e6 for p in parts]),
                "B_over_D": med([dd / b for b, dd in zip(T["B"], T["D"])]),
                "zlib_16_python_threads_s": tz, "zlib_16_python_threads_reads_per_s": a.reads / tz}
            del pl
        flt.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
