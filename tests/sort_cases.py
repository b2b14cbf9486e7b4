"""Shared by the tests of the coordinate sort and the BAI index (tests/test_output_sort_cpu.py on the host, tests/test_gpu_writer_sort.py
on the device).  An independent yardstick in plain Python, written down from the rules of include/linear_amd.h alone:

  the order     (uint32)refID, (uint32)pos, the reverse-strand bit (forward first), the record's byte offset in the stream as it was added
  the end       pos + max(1, sum of the counts of M D N = X)
  voffset(s)    (first_offset + member_off[s // 0xff00]) << 16 | s % 0xff00; a record spans [voffset(start), voffset(start + 4 + block_size))
  the index     "BAI\\1", n_ref, per reference: n_bin, bins ascending (bin, n_chunk, chunks), n_intv, ioffset; n_no_coor.  bin = reg2bin(pos, end);
                a record whose predecessor in the file has the same refID and bin extends that chunk, else it opens one; pseudo-bin 37450 last
                (first start .. last end; mapped, unmapped counts); ioffset[w] = smallest start over window w, an empty window takes the next
                higher one's; refID < 0 counts in n_no_coor; refID >= 0 with pos < 0 or end > 2^29: Unindexable

and the cases: the batches of tests/bam_cases.py added call after call, a tie batch, the degenerate ones."""
import struct
import zlib

import numpy as np

from tests import bam_cases as bmc, bgzf_cases as bc, writer_cases as wc, writer_seq_cases as sc

BLOCK = 0xff00
HD = b"@HD\tVN:1.6\tSO:coordinate\n"


class Unindexable(Exception):
    pass


def records(raw: bytes):
    """[(start, size, ref, pos, flag, end)] of a record stream"""
    recs, out, p = bmc.walk_records(raw), [], 0
    for r in recs:
        bs, = struct.unpack_from("<i", raw, p)
        ref_bases = sum(n for n, op in r["cigar"] if op in "MDN=X")
        out.append((p, 4 + bs, r["ref"], r["pos"], r["flag"], r["pos"] + max(1, ref_bases)))
        p += 4 + bs
    assert p == len(raw)
    return out


def sorted_stream(raw: bytes) -> bytes:
    recs = records(raw)
    order = sorted(recs, key=lambda r: (r[2] & 0xffffffff, r[3] & 0xffffffff, 1 if r[4] & 16 else 0, r[0]))
    return b"".join(raw[s:s + z] for s, z, *_ in order)


def is_sorted(raw: bytes) -> bool:
    k = [(r[2] & 0xffffffff, r[3] & 0xffffffff, 1 if r[4] & 16 else 0) for r in records(raw)]
    return k == sorted(k)


def voffset(s, first_offset, member_off):
    return (first_offset + int(member_off[s // BLOCK])) << 16 | s % BLOCK


def bai_of(sorted_raw: bytes, first_offset: int, member_off, n_ref: int) -> bytes:
    assert len(member_off) == (len(sorted_raw) + BLOCK - 1) // BLOCK + 1
    refs = [dict(bins={}, lin={}, first=None, last=None, mapped=0, unmapped=0) for _ in range(n_ref)]
    no_coor, prev = 0, None
    for i, (start, size, ref, pos, flag, end) in enumerate(records(sorted_raw)):
        if ref < 0:
            no_coor, prev = no_coor + 1, None
            continue
        if pos < 0 or end > 1 << 29:
            raise Unindexable(i)
        vs, ve = voffset(start, first_offset, member_off), voffset(start + size, first_offset, member_off)
        b = bmc.reg2bin(pos, end)
        x = refs[ref]
        chunks = x["bins"].setdefault(b, [])
        if prev == (ref, b):
            chunks[-1][1] = ve
        else:
            chunks.append([vs, ve])
        prev = (ref, b)
        if x["first"] is None:
            x["first"] = vs
        x["last"] = ve
        x["unmapped" if flag & 4 else "mapped"] += 1
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            x["lin"][w] = min(x["lin"].get(w, vs), vs)
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for x in refs:
        if x["first"] is None:
            out.append(struct.pack("<II", 0, 0))
            continue
        out.append(struct.pack("<I", len(x["bins"]) + 1))
        for b in sorted(x["bins"]):
            out.append(struct.pack("<II", b, len(x["bins"][b])) + b"".join(struct.pack("<QQ", *c) for c in x["bins"][b]))
        out.append(struct.pack("<IIQQQQ", 37450, 2, x["first"], x["last"], x["mapped"], x["unmapped"]))
        n_intv = max(x["lin"]) + 1
        lin, nxt = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            nxt = x["lin"].get(w, nxt)
            lin[w] = nxt
        out.append(struct.pack("<I", n_intv) + struct.pack(f"<{n_intv}Q", *lin))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def bai_parse(bai: bytes):
    """[(bins {bin: [(beg, end)]}, pseudo or None, ioffset list)] per reference, n_no_coor"""
    assert bai[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", bai, 4)
    p, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<I", bai, p)
        p += 4
        bins, pseudo, order = {}, None, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<II", bai, p)
            ch = [struct.unpack_from("<QQ", bai, p + 8 + 16 * c) for c in range(n_chunk)]
            p += 8 + 16 * n_chunk
            order.append(b)
            if b == 37450:
                pseudo = ch
            else:
                bins[b] = ch
        assert order == sorted(order) and (not order or order[-1] == 37450)
        n_intv, = struct.unpack_from("<I", bai, p)
        lin = list(struct.unpack_from(f"<{n_intv}Q", bai, p + 4))
        p += 4 + 8 * n_intv
        refs.append((bins, pseudo, lin))
    no_coor, = struct.unpack_from("<Q", bai, p)
    assert p + 8 == len(bai)
    return refs, no_coor


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(base + (beg >> shift), base + (end >> shift) + 1)
    return out


def bai_query(bai: bytes, ref: int, beg: int, end: int):
    """the chunks a reader looks at for [beg, end) of reference `ref`: those of reg2bins, minus the ones that end at or before ioffset[beg >> 14]"""
    bins, _pseudo, lin = bai_parse(bai)[0][ref]
    w = beg >> 14
    if w >= len(lin):
        return []                                  # no record reaches this window
    return [c for b in reg2bins(beg, end) for c in bins.get(b, []) if c[1] > lin[w]]


def check_queries(bai: bytes, sorted_raw: bytes, first_offset, member_off, ref_len, seed=5, n=200):
    """about n seeded regions per case: every record that overlaps by brute force lies inside a chunk bai_query returns"""
    recs = [r for r in records(sorted_raw) if r[2] >= 0]
    rng = np.random.default_rng(seed)
    regions = []
    for ref, length in enumerate(ref_len):
        length = min(int(length), 1 << 29)
        regions += [(ref, 0, length), (ref, 0, 1), (ref, 16384, 16385), (ref, 16383, 16384), (ref, 16383, 16385), (ref, length - 1, length)]
    for s, z, ref, pos, flag, end in recs[:: max(1, len(recs) // 40)]:
        regions += [(ref, pos, pos + 1), (ref, end - 1, end), (ref, end, end + 1), (ref, max(0, pos - 1), pos), (ref, (pos >> 14) << 14, ((pos >> 14) << 14) + 1),
                    (ref, ((end >> 14) + 1) << 14, (((end >> 14) + 1) << 14) + 5)]
    top = max([r[5] for r in recs] + [1 << 15]) + 40_000
    while len(regions) < n:
        ref = int(rng.integers(0, len(ref_len)))
        a = int(rng.integers(0, top))
        regions.append((ref, a, a + int(rng.choice([1, 7, 100, 16384, 100_000, 5_000_000]))))
    hits = empty = 0
    for ref, a, b in regions:
        b = min(b, 1 << 29)
        if a >= b:
            continue
        chunks = bai_query(bai, ref, a, b)
        over = [r for r in recs if r[2] == ref and r[3] < b and r[5] > a]
        for s, z, *_ in over:
            vs, ve = voffset(s, first_offset, member_off), voffset(s + z, first_offset, member_off)
            assert any(c0 <= vs and ve <= c1 for c0, c1 in chunks), ("a record the index misses", ref, a, b, s)
        hits += bool(over)
        empty += not over
    return hits, empty


def parse_bgzf(raw: bytes):
    """a chain of BGZF members -> (offsets of the members + the end of the last, inflated bytes)"""
    members = bc.walk(raw)
    text = []
    for o, payload, isize, crc in members:
        t = zlib.decompressobj(-15).decompress(payload)
        assert len(t) == isize and zlib.crc32(t) == crc
        text.append(t)
    end = members[-1][0] + struct.unpack_from("<H", raw, members[-1][0] + 16)[0] + 1 if members else 0      # (BSIZE of the writer's members: the BC subfield comes first)
    assert end == len(raw), "bytes after the last member"
    return [m[0] for m in members] + [end], b"".join(text)


def pad_to_boundary(raw: bytes):
    """(stream whose records i - 1 / i meet exactly at byte 0xff00, that stream's first 0xff00 bytes): zero bytes appended to record i - 1 as aux data"""
    recs = records(raw)
    i = next(k for k, r in enumerate(recs) if r[0] + r[1] > BLOCK)
    assert i >= 1
    s, z = recs[i - 1][0], recs[i - 1][1]
    gap = BLOCK - recs[i][0]
    padded = raw[:s] + struct.pack("<i", z - 4 + gap) + raw[s + 4:s + z] + b"\0" * gap + raw[s + z:]
    assert any(r[0] == BLOCK for r in records(padded))
    return padded, padded[:BLOCK]


# ---- the cases: lists of batches, added call after call
def _keep_reads(batch, keep):
    """the reads k with keep[k] of a batch of either form"""
    coff, cs, ce = (np.asarray(a, np.uint64) for a in batch[:3])
    idx = [k for k in range(coff.size - 1) if keep[k]]
    spans = [(int(coff[k]), int(coff[k + 1])) for k in idx]
    ncs = np.concatenate([cs[a:b] for a, b in spans] + [np.zeros(0, np.uint64)])
    nce = np.concatenate([ce[a:b] for a, b in spans] + [np.zeros(0, np.uint64)])
    noff = np.cumsum([0] + [b - a for a, b in spans]).astype(np.uint64)
    if len(batch) == 5:
        return noff, ncs, nce, np.asarray(batch[3], np.uint64)[idx], [batch[4][k] for k in idx]
    reads, off, ids = batch[3], np.asarray(batch[4], np.uint64), batch[5]
    nreads = np.concatenate([reads[int(off[k]):int(off[k + 1])] for k in idx] + [np.zeros(0, np.uint8)])
    nro = np.cumsum([0] + [int(off[k + 1] - off[k]) for k in idx]).astype(np.uint64)
    return noff, ncs, nce, nreads, nro, [ids[k] for k in idx]


def indexable(batch):
    """without the reads that have a cord beyond 2^28 on its sequence (a BAI indexes positions below 2^29)"""
    coff, cs = np.asarray(batch[0], np.uint64), np.asarray(batch[1], np.uint64)
    x = (cs >> np.uint64(20)) & np.uint64((1 << 30) - 1)
    keep = [not bool((x[int(coff[k]) + 1:int(coff[k + 1])] >= (1 << 28)).any()) if coff[k + 1] > coff[k] else True for k in range(coff.size - 1)]
    return _keep_reads(batch, keep)


def tie_batches():
    """the same cords under the ids a and b, on both strands: (refID, pos) repeat with equal and with different strand bits inside a batch and across two"""
    def cords(flip):
        return [(x, 10 + 200 * i, s ^ flip, 0, True, 96) for i, (x, s) in enumerate([(7000, 0), (7000, 1), (7000, 0), (6000, 1), (6000, 1), (7000, 1), (6000, 0)])]
    one = wc.Batch().read(cords(0), rid="a").read(cords(0), rid="b").read(cords(1), rid="a")
    two = wc.Batch().read(cords(1), rid="b").read(cords(0), rid="a").read(cords(0), rid="b")
    return [one.arrays(), two.arrays()]


def one_record():
    return wc.Batch().read(wc.blocks([[0]]), rid="r").arrays()


def plain_cases(index_only=False):
    """(name, [batches]) without SEQ.  index_only: what a BAI can hold of them"""
    f = indexable if index_only else (lambda b: b)
    all_ = [f(b) for _, b in bmc.plain_batches()]
    return [("three_calls", all_[:1] + all_[3:5]), ("every_batch", all_), ("tie", tie_batches()), ("empty_only", [wc.empty()]), ("one_record", [one_record()]), ("no_batch", [])]


def seq_cases(index_only=False):
    f = indexable if index_only else (lambda b: b)
    return [("seq_three_calls", [f(b) for _, b in bmc.seq_batches()]), ("seq_empty_only", [sc.empty()])]
