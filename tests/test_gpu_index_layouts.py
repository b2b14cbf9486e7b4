"""GPU (-m gpu): the index build (k_ix_chunk_const, k_ix_sample, k_ix_start_blk / k_max_top / k_ix_rec, k_ix_omit, k_ix_sort_small /
k_ix_sort_big, build_hindex) and the seed kernel's bucket view (k_ix_ovcount, k_ix_lines, the line walk of k_seed_fused) on the families
of tests/index_cases.py: up to 1023 contigs at -t up to 64, N runs against every chunk border, bucket lengths on every threshold.  Every
index is built through Filter.build_index, exported whole and compared with the oracle's arrays, and its digests with the real
reference's (tests/golden/index_layouts.npz, tools/make_index_golden.py); tests/test_index_layouts_cpu.py holds the chain reference ==
oracle == host shim on the same inputs."""
import os

import numpy as np
import pytest

from tests import cases, index_cases as ic

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "index_layouts.npz")
LNR_ERR_NO_INDEX, LNR_ERR_LIMIT = -5, -6


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def flt():
    from linear_amd import build as lb
    lb.build()
    from linear_amd import Filter
    f = Filter(device=0)
    yield f
    f.close()


class Exported:
    """lnr_index_export seen as the checkers are (dir / hs / ysa / f2 per sequence), so that ic.index_digests digests it the same way."""

    def __init__(self, f):
        self.info = f.index_info()
        self._dir, self._hs, self._f2, self.f2_off = f.index_export()

    def dir(self):
        return self._dir

    def hs(self):
        return self._hs

    ysa = hs

    def f2(self, k):
        return self._f2[int(self.f2_off[k]):int(self.f2_off[k + 1])]


def same_index(f, o, gold, key, nseq, it=1):
    """The exported index against the oracle's arrays (whole) and the reference's digests."""
    e = Exported(f)
    if it == 2:
        want = o.ysa()
        assert e.info.hs_len == want.size, f"{key}: ysa_len {e.info.hs_len}, oracle {want.size}"
        bad = np.nonzero(e.ysa() != want)[0]
        assert bad.size == 0, f"{key}: {bad.size} words of ysa differ from the oracle, first at {int(bad[0])}"
    else:
        want = o.hs()
        assert e.info.hs_len == want.size, f"{key}: hs_len {e.info.hs_len}, oracle {want.size}"
        d, od = e.dir(), o.dir()
        bad = np.nonzero(d != od)[0]
        assert bad.size == 0, f"{key}: {bad.size} dir entries differ from the oracle, first at bucket {int(bad[0])}: {int(d[bad[0]])} / {int(od[bad[0]])}"
        bad = np.nonzero(e.hs() != want)[0]
        assert bad.size == 0, f"{key}: {bad.size} hs entries differ from the oracle, first at {int(bad[0])} (bucket {int(np.searchsorted(od, bad[0], side='right')) - 1})"
        for k in range(nseq):
            a, b = e.f2(k), o.f2(k)
            assert a.shape == b.shape, f"{key}: f2 of sequence {k} has {a.shape[0]} entries, oracle {b.shape[0]}"
            assert np.array_equal(a[:-1], b[:-1]), f"{key}: f2 of sequence {k}"
    for k, v in ic.index_digests(e, nseq, it).items():
        assert np.array_equal(np.asarray(v), gold[f"{key}:{k}"]), f"{key}: {k} differs from the reference's"
    return e


def same_anchors(f, o, reads, off, what):
    aoff, anc = f.seed_lookup_batch(reads, off)
    n_anc = 0
    for i in range(off.size - 1):
        want = o.seed_lookup(reads[int(off[i]):int(off[i + 1])])[0]
        got = anc[int(aoff[i]):int(aoff[i + 1])]
        assert np.array_equal(got, want), f"{what}: raw anchors of read {i} ({got.size} / {want.size})"
        n_anc += want.size
    return n_anc


def same_cords(got, want, what):
    coff, cs, ce = got
    ooff, ocs, oce = want[:3]
    assert np.array_equal(coff, ooff), f"{what}: cord counts differ for reads {np.nonzero(np.diff(coff.astype(np.int64)) != np.diff(ooff.astype(np.int64)))[0][:20].tolist()}"
    bad = np.nonzero((cs != ocs) | (ce != oce))[0]
    assert bad.size == 0, f"{what}: {bad.size} cords differ, first in read {int(np.searchsorted(ooff, bad[0], side='right')) - 1}"


def cords_by_read(o, reads, off):
    """The oracle's cords read by read (the form -i 2 has) as a CSR triple."""
    lst = [o.map_read(reads[int(off[i]):int(off[i + 1])]) for i in range(off.size - 1)]
    coff = np.zeros(len(lst) + 1, np.uint64)
    coff[1:] = np.cumsum([c[0].size for c in lst])
    return coff, np.concatenate([c[0] for c in lst]), np.concatenate([c[1] for c in lst])


# ---- 1. fragmented references, -i 1
FRAG_PARAMS = [(name, T) for name, v in ic.FRAG.items() for T in v[5]]


@pytest.mark.parametrize("name,T", FRAG_PARAMS)
def test_gpu_frag_index_and_seed_view(flt, oracle_lib, gold, name, T):
    """200 contigs at -t 1 .. 64, 40 contigs at -t 16 / 32, 1023 contigs down to 22 bases at -t 3, 1023 contigs of 300 .. 4000 bases at
    -t 1 / 16: hundreds to thousands of chunks under k_ix_sample's search, most 1024-sample blocks of the max-scan holding many chunk
    starts, contigs without a chunk or an f2 entry.  On the read sets: raw anchors read by read, cords against the reference's, and the
    seed counters."""
    refs = ic.frag_refs(name)
    key = ic.config_key(name, T)
    o = oracle_lib.Checker("oracle", refs, T)
    info = flt.build_index(refs, T)
    assert info.nseq == len(refs) and info.layout_threads == T
    same_index(flt, o, gold, key, len(refs))
    if name in ic.READ_SETS:
        reads, off = ic.many_reads(refs)
        assert same_anchors(flt, o, reads, off, key) > 1000
        got = flt.filter_batch(reads, off)
        same_cords(got, [gold[f"{key}:{k}"] for k in ("cord_off", "cords_str", "cords_end")], key + " against the reference")
        st = flt.stats()
        ost = o.map_batch(reads, off, threads=8)[3]
        assert (st["samples"], st["lookups"], st["bucket_entries"], st["anchors"]) == tuple(int(x) for x in ost[:4])
        if name != "frag200":
            ids = (got[1] >> np.uint64(50)) & np.uint64(1023)
            assert int(ids.max()) > 1000 and np.unique(ids).size > 100, "cords on contigs up to the last ids"
    o.close()


# ---- 2. the receiver path with 1023 sequences
def test_gpu_frag_max_receiver_path(gold):
    """tests/test_gpu_parity.py::test_gpu_index_receiver_path with 1023 seq_len entries: alloc from the owner's metadata, the four blobs
    copied device to device, adopt (the bucket view rebuilt from the received dir / hs) -- the same index out, the reference's cords."""
    import torch
    from linear_amd import Filter
    from linear_amd.dist import blob_tensor
    refs = ic.frag_refs("frag_max")
    T = ic.FRAG["frag_max"][5][0]
    key = ic.config_key("frag_max", T)
    reads, off = ic.many_reads(refs)
    owner = Filter(device=0)
    owner.build_index(refs, T)
    assert owner.seq_len().size == ic.N_MAX
    recv = Filter(device=0)
    recv.index_alloc_from(owner.index_info_vec(), owner.seq_len())
    src, dst = owner.index_blobs(), recv.index_blobs()
    for (ps, bs), (pd, bd) in zip(src, dst):
        assert bs == bd and bs
        blob_tensor(pd, bd, "cuda:0").copy_(blob_tensor(ps, bs, "cuda:0"))
    torch.cuda.synchronize()
    recv.index_adopt()
    owner.close()
    e = Exported(recv)
    for k, v in ic.index_digests(e, len(refs), 1).items():
        assert np.array_equal(np.asarray(v), gold[f"{key}:{k}"]), f"{key}: {k} of the receiver differs from the reference's"
    same_cords(recv.filter_batch(reads, off), [gold[f"{key}:{k}"] for k in ("cord_off", "cords_str", "cords_end")], "receiver")
    recv.close()


# ---- 3. N runs against chunk borders, one context
NRUN_GROUPS = [ic.NRUN_LEADS[0:6], ic.NRUN_LEADS[6:12], ic.NRUN_LEADS[12:18] + (0,)]


@pytest.mark.parametrize("leads", NRUN_GROUPS, ids=["-".join(str(x) for x in g) for g in NRUN_GROUPS])
def test_gpu_nrun_family_on_one_context(flt, oracle_lib, gold, leads):
    """All eighteen run lengths at -t 8, one index after the other on the module's context: runs that end 20 / 21 bases in front of a
    segment border of k_ix_chunk_const, on its 16 384-position tile, and past the chunk (ks beyond the chunk's end; for odd leads the
    run of the last chunk goes to the end of the sequence and ks into the padding).  The last two leave no entry at all: such an index
    builds, exports an all-equal dir and answers with what the oracle gives; the good index built right after it maps."""
    reads, off = ic.nrun_reads()
    for lead in leads:
        ref = ic.nrun(lead)
        key = ic.config_key(f"nrun{lead}", ic.NRUN_T)
        o = oracle_lib.Checker("oracle", [ref], ic.NRUN_T)
        info = flt.build_index([ref], ic.NRUN_T)
        e = same_index(flt, o, gold, key, 1)
        n_anc = same_anchors(flt, o, reads, off, key)
        got = flt.filter_batch(reads, off)
        same_cords(got, o.map_batch(reads, off, threads=4), key)
        if lead in ic.NRUN_EMPTY:
            assert info.hs_len == 0 and e.dir().min() == e.dir().max() and got[1].size == 0
            assert n_anc == off.size - 1, "nothing but the head word of every read"
        elif lead < 100:
            assert n_anc > 200 and got[1].size > 100
        o.close()


# ---- 4. planted bucket lengths
@pytest.mark.parametrize("T,bm", [(1, None), (4, None), (1, "0"), (4, "0")], ids=["T1", "T4", "T1-LNR_SEED_BM-0", "T4-LNR_SEED_BM-0"])
def test_gpu_planted_bucket_lengths(oracle_lib, gold, monkeypatch, T, bm):
    """Buckets of 1, 2, 14 .. 17, 30 .. 34, 47, 48, 63 .. 65, 128, 256, 399, 400 entries, and 401 / 450 emptied: k_ix_omit's bound, insertion
    sort | bitonic sort, the end of the inline bucket line, the borders of the overflow lines, the seed kernel's 64 lines per round.  The
    index arrays; the raw anchors of planted_reads read by read (the tests on the CPU assert that they look every one of those lengths
    up); the cords.  Once with the defaults and once with the lookup path without the bucket bitmap."""
    from linear_amd import Filter
    if bm is not None:
        monkeypatch.setenv("LNR_SEED_BM", bm)
    ref = ic.planted()
    key = ic.config_key("planted", T)
    reads, off = ic.planted_reads(ref)
    o = oracle_lib.Checker("oracle", [ref], T)
    f = Filter(device=0)
    f.build_index([ref], T)
    e = same_index(f, o, gold, key, 1)
    ln = np.diff(e.dir())
    assert all(int((ln == c).sum()) >= 1 for c in ic.COUNTS if c <= 400) and int(ln.max()) == 400
    assert same_anchors(f, o, reads, off, key) > 100_000
    same_cords(f.filter_batch(reads, off), o.map_batch(reads, off, threads=8), key)
    f.close()
    o.close()


# ---- 5. -i 2
I2_PARAMS = [(name, T, None) for name, T in ic.FRAG_I2] + [("nrun", ic.NRUN_T, lead) for lead in ic.NRUN_I2]


@pytest.mark.parametrize("name,T,lead", I2_PARAMS, ids=[f"{n}{'' if l is None else l}_T{T}" for n, T, l in I2_PARAMS])
def test_gpu_hindex_layouts(oracle_lib, gold, name, T, lead):
    """build_hindex on 200 and 40 contigs at -t 16 (3200 and 640 chunks; it had seen 3 sequences and -t 4) and on four of the N-run
    sequences at -t 8: ysa whole, raw anchors and cords read by read."""
    from linear_amd import Filter
    if lead is None:
        refs = ic.frag_refs(name)
        reads, off = ic.many_reads(refs)
        key = ic.config_key(name, T, 2)
    else:
        refs = [ic.nrun(lead)]
        reads, off = ic.nrun_reads()
        key = ic.config_key(f"nrun{lead}", T, 2)
    o = oracle_lib.Checker("oracle", refs, T, index_type=2)
    f = Filter(device=0, index_type=2)
    f.build_index(refs, T)
    same_index(f, o, gold, key, len(refs), it=2)
    same_anchors(f, o, reads, off, key)
    same_cords(f.filter_batch(reads, off), cords_by_read(o, reads, off), key)
    f.close()
    o.close()


# ---- 6. the limit
def test_gpu_1024_sequences_are_refused_and_the_context_goes_on(oracle_lib, gold):
    """nseq = 1024 is LNR_ERR_LIMIT (the cord's id field) and leaves no index behind: the next call is LNR_ERR_NO_INDEX; a build of
    frag200 on the same context then works."""
    from linear_amd import Filter
    from linear_amd.api import LnrError
    refs = ic.frag_refs("frag_max")
    f = Filter(device=0)
    with pytest.raises(LnrError) as ei:
        f.build_index(refs + [refs[0]], 3)
    assert ei.value.status == LNR_ERR_LIMIT
    with pytest.raises(LnrError) as ei:
        f.index_info()
    assert ei.value.status == LNR_ERR_NO_INDEX
    with pytest.raises(LnrError) as ei:
        f.filter_batch(*ic.many_reads(refs))
    assert ei.value.status == LNR_ERR_NO_INDEX
    refs = ic.frag_refs("frag200")
    o = oracle_lib.Checker("oracle", refs, 7)
    f.build_index(refs, 7)
    same_index(f, o, gold, ic.config_key("frag200", 7), len(refs))
    f.close()
    o.close()


# ---- 7. the writer on 1023 sequences
def test_gpu_writer_on_1023_sequences(gold):
    """SAM and APF of the reference's cords of many_reads over frag_max: lnr_writer_format_gpu == lnr_writer_format == the reference's own
    text (its digests) -- 1023 @SQ lines, RNAME for ids up to the last."""
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    refs = ic.frag_refs("frag_max")
    key = ic.config_key("frag_max", ic.FRAG["frag_max"][5][0])
    reads, off = ic.many_reads(refs)
    coff, cs, ce = (gold[f"{key}:{k}"] for k in ("cord_off", "cords_str", "cords_end"))
    rid, gid = cases.text_ids(off.size - 1, len(refs))
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    w = Writer(gid, [r.size for r in refs])
    w.gpu_open(0)
    head = w.sam_header(cases.CMD_LINE)
    assert head.count(b"@SQ") == ic.N_MAX
    sam, apf = w.format(coff, cs, ce, rl, rid, "sam"), w.format(coff, cs, ce, rl, rid, "apf")
    assert w.format_gpu(coff, cs, ce, rl, rid, "sam") == sam
    assert w.format_gpu(coff, cs, ce, rl, rid, "apf") == apf
    assert cases.sha(np.frombuffer(head + sam, np.uint8)) == str(gold[f"{key}:sam_sha"])
    assert cases.sha(np.frombuffer(apf, np.uint8)) == str(gold[f"{key}:apf_sha"])
    names = {l.split(b"\t")[2] for l in sam.split(b"\n") if l}
    assert len(names) >= 100 and max(int(s[3:]) for s in names) > 1000
    w.close()
