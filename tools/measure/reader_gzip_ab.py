"""A/B of plain gzip input: the bench workload's reads as FASTA and four-line FASTQ, compressed with zlib's default level as ONE plain gzip
member -> profiles/r16/reader_gzip_ab.json.  The method of tools/measure/reader_bgzf_ab.py: one process, page cache warm, the blocks of
every leg compared with A's before anything is timed, one warm-up, then rotations of the legs, medians with ranges.

  A   lnr_reader_next on the .gz (host, gzread)
  B   lnr_reader_next_dev with the switch off (gzread into the pinned staging buffer, parse on the device): the parent's behaviour
  C   lnr_reader_next_dev with lnr_reader_gpu_gzip: the parallel inflate on the device, with its stage times (lnr_reader_gpu_gzip_stats)
  Q   lnr_reader_next_dev on the same reads as BGZF (device inflate of whole blocks)

Reported: the winner of every rotation of C against B and against Q.  No rate is a gate.

python tools/measure/reader_gzip_ab.py [--reads 100000] [--len 10000] [--reps 5] [--out profiles/r16/reader_gzip_ab.json]"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tools.measure.reader_bgzf_ab import EOF_BLOCK, PAYLOAD, bgzf_chunk, d2h, med  # noqa: E402


def gzip_one_member(path):
    c = zlib.compressobj(-1, zlib.DEFLATED, 31)
    with open(path, "rb") as f, open(path + ".gz", "wb") as g:
        while True:
            b = f.read(1 << 24)
            if not b:
                break
            g.write(c.compress(b))
        g.write(c.flush())
    return path + ".gz"


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
    with ProcessPoolExecutor(16) as ex:
        plain = [ex.submit(gzip_one_member, paths[k]) for k in ("fa", "fq")]      # one member each: serial by nature, the two side by side
        step = PAYLOAD * 64
        for k in ("fa", "fq"):
            text = open(paths[k], "rb").read()
            paths[k + ".bgzf"] = paths[k] + ".bgzf.gz"
            with open(paths[k + ".bgzf"], "wb") as f:
                for part in ex.map(bgzf_chunk, (text[i:i + step] for i in range(0, len(text), step))):
                    f.write(part)
                f.write(EOF_BLOCK)
            del text
        for k, fut in zip(("fa", "fq"), plain):
            paths[k + ".gz"] = fut.result()
    for p in paths.values():                     # warm page cache
        with open(p, "rb") as f:
            while f.read(1 << 26):
                pass
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--len", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "reader_gzip_ab.json"))
    a = ap.parse_args()
    from linear_amd import Filter, build as lb
    from linear_amd.api import Reader
    lb.build()
    os.environ["LNR_READER_THREADS"] = "16"
    res = {"reads": a.reads, "read_len": a.len, "reps": a.reps, "chunk": os.environ.get("LNR_READER_GZ_CHUNK", "131072 (default)"),
           "round": os.environ.get("LNR_READER_GZ_ROUND", "67108864 (default)"), "files": {}}
    with tempfile.TemporaryDirectory() as d:
        paths = write_files(d, a.reads, a.len)
        cap = a.reads * (a.len + 8) + (1 << 20)
        flt = Filter(device=0)
        dst = flt.host_alloc(cap)

        def leg(path, how):
            """(seconds, result of one block of the whole file, reader); the reader stays open for its times and its block"""
            r = Reader(path)
            if how == "A":
                t0 = time.perf_counter()
                out = r.next(dst, a.reads)
                return time.perf_counter() - t0, out, r
            r.gpu_open(0, 1)
            if how == "C":
                r.gpu_gzip()
            t0 = time.perf_counter()
            out = r.next_dev(cap, a.reads)
            return time.perf_counter() - t0, out, r

        for kind in ("fa", "fq"):
            gz, bg, plain = paths[kind + ".gz"], paths[kind + ".bgzf"], paths[kind]
            text_bytes, comp_bytes = os.path.getsize(plain), os.path.getsize(gz)
            legs = (("A", gz), ("B", gz), ("C", gz), ("Q", bg))
            # warm-up + identity: the blocks of B, C and Q against A's
            _, (n, off, ids), r = leg(gz, "A")
            r.close()
            want = dst[: int(off[n])].copy()
            for how, path in legs[1:]:
                _, (nd, dr, dof, doff, dids), r = leg(path, how)
                assert nd == n == a.reads and np.array_equal(doff, off) and dids == ids and np.array_equal(d2h(dr, int(off[n])), want), (kind, how)
                if how == "C":
                    st = r.gpu_gzip_stats()["last"]
                    assert st["rounds"] > 0 and st["gzread_bytes"] == 0 and st["text_bytes"] == text_bytes, st
                r.close()
            del want
            T = {k: [] for k, _ in legs}
            parts = []
            for rep in range(a.reps):            # rotations: one run of each leg per repetition, the first leg moving on
                for how, path in legs[rep % 4:] + legs[:rep % 4]:
                    t, out, r = leg(path, how)
                    assert out[0] == a.reads
                    T[how].append(t)
                    if how == "C":
                        st = r.gpu_gzip_stats()["last"]
                        parts.append({k: st[k] for k in ("find_ms", "measure_ms", "stitch_ms", "emit_ms", "chain_ms", "resolve_ms", "parse_ms", "upload_ms", "download_ms",
                                                         "rounds", "chunks", "true_pieces", "false_candidates", "deflate_blocks", "window_symbols", "grown_rounds")})
                    r.close()
            dec = [sum(p[k] for k in ("find_ms", "measure_ms", "stitch_ms", "emit_ms", "chain_ms", "resolve_ms")) for p in parts]
            res["files"][kind] = {
                "text_bytes": text_bytes, "compressed_bytes": comp_bytes,
                "reads_per_s": {k: med([a.reads / t for t in T[k]]) for k in T},
                "seconds": T,
                "C_beats_B_per_rotation": [c < b for c, b in zip(T["C"], T["B"])],
                "C_beats_Q_per_rotation": [c < q for c, q in zip(T["C"], T["Q"])],
                "C_parts": {k: med([p[k] for p in parts]) for k in parts[0]},
                "C_decode_text_GB_per_s": med([text_bytes / ms / 1e6 for ms in dec])}
        flt.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
