"""CPU: the index chain -- real reference == oracle == host shim -- on the families of tests/index_cases.py: fragmented references of
up to 1023 contigs at -t up to 64, N runs laid against every chunk border, and bucket lengths planted on the thresholds of the build.
The oracle and the shim are compared with tests/golden/index_layouts.npz (the reference's digests, tools/make_index_golden.py) everywhere;
with the reference itself where it can be built.  tests/test_gpu_index_layouts.py puts the HIP kernels on the same inputs."""
import os

import numpy as np
import pytest

from tests import index_cases as ic, shimlib

GOLD = os.path.join(os.path.dirname(__file__), "golden", "index_layouts.npz")
CONFIGS = {key: (make, T, it) for key, make, T, it in ic.all_configs()}
live = pytest.mark.skipif(not os.path.exists("/root/reference/src/pmpfinder.cpp"), reason="reference tree not present (GPU box)")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def same_digests(d, gold, key, who):
    for k, v in d.items():
        want = gold[f"{key}:{k}"]
        assert np.array_equal(np.asarray(v), want), f"{key}: {k} of {who} differs from the reference's"


@pytest.mark.parametrize("key", list(CONFIGS))
def test_oracle_and_shim_match_reference_golden(oracle_lib, gold, key):
    """dir, hs (ysa for -i 2), f2 and hs_len of the oracle, and dir / hs / f2 of the product's stage logic on the host (-i 1), against the
    reference's digests."""
    make, T, it = CONFIGS[key]
    refs = make()
    o = oracle_lib.Checker("oracle", refs, T, it)
    same_digests(ic.index_digests(o, len(refs), it), gold, key, "the oracle")
    if it == 1:
        assert o.lib.orc_fill_mismatch(o.h) == 0
        s = shimlib.Shim(refs, T)
        same_digests(ic.index_digests(s, len(refs), 1), gold, key, "the host shim")
        s.close()
    o.close()


@live
@pytest.mark.parametrize("key", list(CONFIGS))
def test_oracle_matches_live_reference(oracle_lib, key):
    """The same arrays whole, against the reference itself."""
    make, T, it = CONFIGS[key]
    refs = make()
    o, r = oracle_lib.Checker("oracle", refs, T, it), oracle_lib.Checker("ref", refs, T, it)
    if it == 2:
        assert np.array_equal(o.ysa(), r.ysa())
    else:
        assert np.array_equal(o.dir(), r.dir()), "dir"
        assert np.array_equal(o.hs(), r.hs()), "hs"
        for k in range(len(refs)):
            a, b = o.f2(k), r.f2(k)
            assert a.shape == b.shape and np.array_equal(a[:-1], b[:-1]), f"f2 of sequence {k}"
    o.close(); r.close()


def test_frag_max_holds_the_contigs_it_is_for(oracle_lib):
    """1023 contigs is what lnr_index_build accepts, and the reference and the oracle agree there (1022 was what had been tried before).
    Among them: contigs under 42 bases (no chunk), under 48 (no f2 entry) and under 42 * 3 (empty chunks at -t 3)."""
    refs = ic.frag_refs("frag_max")
    lens = np.array([r.size for r in refs])
    assert lens.size == ic.N_MAX == 1023
    assert (lens < 42).sum() >= 3 and ((lens >= 42) & (lens < 48)).sum() >= 3 and ((lens >= 48) & (lens < 126)).sum() >= 50
    o = oracle_lib.Checker("oracle", refs, 3)
    ids = np.unique((o.hs() >> np.uint64(50)) & np.uint64(1023))    # hs entries are cord words: the id field
    k = int(np.nonzero(lens < 48)[0][0])
    assert o.f2(k).shape[0] == 0
    assert int(ids.max()) >= 1020, "entries up to the last contigs"
    assert not set(np.nonzero(lens < 42)[0].tolist()) & set(ids.tolist()), "a contig without a chunk has no entry"
    o.close()


@pytest.mark.parametrize("name", ic.READ_SETS)
def test_many_reads_cords(oracle_lib, gold, name):
    """The whole path on the many-contig references: the oracle's cords of many_reads equal the reference's (golden at -g 0; live at -g 0
    and -g 50 where the reference is there)."""
    refs = ic.frag_refs(name)
    reads, off = ic.many_reads(refs)
    for T in ic.FRAG[name][5]:
        key = ic.config_key(name, T)
        o = oracle_lib.Checker("oracle", refs, T)
        a = o.map_batch(reads, off, threads=8)
        for x, k in zip(a[:3], ("cord_off", "cords_str", "cords_end")):
            assert np.array_equal(x, gold[f"{key}:{k}"]), f"{key}: {k}"
        if oracle_lib.have_ref() and T == ic.FRAG[name][5][-1]:
            r = oracle_lib.Checker("ref", refs, T)
            for g in (0, 50):
                a, b = o.map_batch(reads, off, threads=8, gap_len=g), r.map_batch(reads, off, threads=1, gap_len=g)
                assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])), f"{key}: cords at -g {g}"
            r.close()
        o.close()


def test_many_reads_map(oracle_lib):
    """A condition of the inputs, not a measurement: at least 80 % of many_reads get more than one cord (a cord beside the head) in the
    oracle.  It holds on frag_map (82 % at -t 1, 85 % at -t 16) and frag200 (89 %).  It cannot hold on frag_max, whose contigs of 50 to
    900 bases cut the reads to 82 .. 902 bases (median 623; a read of 200 bases or fewer is never mapped): 55 % there.  frag_map -- as many
    contigs, of 300 to 4000 bases -- is in the families for that reason; frag_max keeps the layouts nothing else has."""
    for name, T in (("frag_map", 1), ("frag_map", 16), ("frag200", 16)):
        refs = ic.frag_refs(name)
        reads, off = ic.many_reads(refs)
        o = oracle_lib.Checker("oracle", refs, T)
        coff = o.map_batch(reads, off, threads=8)[0]
        share = float((np.diff(coff.astype(np.int64)) > 1).mean())
        print(name, T, share)
        assert share >= 0.8, (name, T, share)
        o.close()


@pytest.mark.parametrize("T", ic.PLANTED_T)
def test_planted_bucket_lengths_are_there_and_are_looked_up(oracle_lib, T):
    """Conditions of the planted family, from the oracle alone: every planted length up to 400 is the length of a bucket, no bucket is
    longer than 400 (401 and 450 were emptied), and planted_reads look a bucket of each of those lengths up."""
    ref = ic.planted()
    assert ref.size % 288 == 0
    o = oracle_lib.Checker("oracle", [ref], T)
    ln = np.diff(o.dir())
    for c in ic.COUNTS:
        assert int((ln == c).sum()) >= (1 if c <= 400 else 0), f"no bucket of {c} entries"
    assert int(ln.max()) == 400
    reads, off = ic.planted_reads(ref)
    hist = np.zeros(401, np.uint64)
    for i in range(off.size - 1):
        o.lookup_hist(reads[int(off[i]):int(off[i + 1])], hist)
    for c in ic.COUNTS:
        if c <= 400:
            assert int(hist[c]) > 0, f"no lookup of a bucket of {c} entries"
    o.close()


def test_nrun_family_reaches_the_empty_index(oracle_lib):
    """The two longest runs swallow every chunk (hs_len = 0, dir all equal); every other lead leaves entries."""
    for lead in ic.NRUN_LEADS:
        o = oracle_lib.Checker("oracle", [ic.nrun(lead)], ic.NRUN_T)
        assert (o.hs().size == 0) == (lead in ic.NRUN_EMPTY), lead
        if lead in ic.NRUN_EMPTY:
            d = o.dir()
            assert d.min() == d.max() == 0
        o.close()
