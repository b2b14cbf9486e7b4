"""GPU: the reference genome loaded on the device (lnr_genome_load_gpu in linear_amd/csrc/lnr_genome.cpp over the reader's GPU twin; blocks
kept device to device by lnr_rdgpu_keep in lnr_reader_kernels.hip) against what the front-end did before: the lnr_reader_next(max_reads = 1)
loop on the same files.

 1. parity on chromosome-shaped records -- one record over many tiles and windows, 60-column lines, lower case, N runs, IUPAC letters, CRLF,
    blank lines, header lines with blanks and tabs, a last line without a newline -- as plain FASTA, gzip (host and device inflate), BGZF
    and split over two files; with the default block, with blocks just above the longest sequence, and with small windows;
 2. lnr_index_build from the device pointers: the index of the host arrays, which is the reference's (tests/golden), -i 1 and -i 2;
 3. lnr_writer_set_genome_dev: the bytes of lnr_writer_set_genome;
 4. linear_filter --gpu-genome: the bytes of the run without it, which are the real program's (tests/golden/cli_*);
 5. the error paths."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from tests import bgzf_cases as bc, cases
from tests.test_gpu_writer import diff

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
LONG = 40 * 1024 + 1                                   # the record of about 40 KiB of bases


@pytest.fixture(scope="module")
def lib():
    from linear_amd import build as lb
    lb.build()
    return lb


def seq_lengths():
    from linear_amd.api import Reader
    T = Reader.gpu_tile()
    assert T > 61
    return [0, 1, 59, 60, 61, T - 1, T, T + 1, 2 * T, 3 * T + 17, LONG]


def bases(rng, n, n_ends=False):
    """n sequence characters: mixed case, IUPAC letters, runs of N (n_ends: the sequence starts and ends in one)"""
    out = bytearray()
    while len(out) < n:
        k = rng.random()
        if k < 0.06:
            out += (b"N" if rng.random() < 0.7 else b"n") * rng.randint(1, 200)
        elif k < 0.10:
            out += bytes(rng.choice(b"RYKMSWBDHVrykmswbdhvUu") for _ in range(rng.randint(1, 9)))
        else:
            out += bytes(rng.choice(b"ACGTacgt") for _ in range(rng.randint(1, 300)))
    out = out[:n]
    if n_ends and n >= 40:
        out[:17] = b"N" * 17
        out[n - 23:] = b"N" * 23
    return bytes(out)


def records(seed=20):
    """[(header line without '>', text of the record behind the header line)] at 60 columns"""
    rng = random.Random(seed)
    out = []
    for k, n in enumerate(seq_lengths()):
        s = bases(rng, n, n_ends=(k == 8))
        eol = b"\r\n" if k == 7 else b"\n"              # CRLF line ends in one record (its header line too)
        head = b"seq%d  two blanks\tand a tab len=%d " % (k, n) if k % 2 else b"chr%d" % k
        body = b"".join(s[i:i + 60] + eol for i in range(0, n, 60))
        gap = b"\n" * (k % 3)                           # blank lines between records
        out.append(b">" + head + eol + body + gap)
    return out


@pytest.fixture(scope="module")
def forms(lib, tmp_path_factory):
    """form -> list of paths; the same records in every form, the last line of every file without its newline"""
    tmp = tmp_path_factory.mktemp("gpu_genome")
    recs = records()
    whole = b"".join(recs).rstrip(b"\n")
    assert not whole.endswith(b"\n") and whole.count(b">") == len(recs)
    cut = 5
    parts = (b"".join(recs[:cut]).rstrip(b"\n"), b"".join(recs[cut:]).rstrip(b"\n"))
    raw = {"plain.fa": whole, "one.fa.gz": gzip.compress(whole, 6), "bgzf.fa.gz": bc.bgzf(whole), "split_a.fa": parts[0], "split_b.fa": parts[1]}
    assert len(list(bc.walk(raw["bgzf.fa.gz"]))) > 1
    for name, data in raw.items():
        with open(tmp / name, "wb") as f:
            f.write(data)
    p = lambda n: str(tmp / n)
    return {"plain": [p("plain.fa")], "gzip": [p("one.fa.gz")], "bgzf": [p("bgzf.fa.gz")], "split": [p("split_a.fa"), p("split_b.fa")]}


def host_loader(paths):
    """what the front-end holds without the switch: (lens, ids, sequences) of the lnr_reader_next(max_reads = 1) loop"""
    from linear_amd.api import Reader
    buf = np.zeros(1 << 20, np.uint8)
    lens, ids, seqs = [], [], []
    for path in paths:
        r = Reader(path)
        while True:
            n, off, rid = r.next(buf, 1)
            if n == 0:
                break
            lens.append(int(off[1])); ids.append(rid[0]); seqs.append(buf[: int(off[1])].copy())
        r.close()
    return lens, ids, seqs


@pytest.fixture(scope="module")
def want(forms):
    out = {form: host_loader(paths) for form, paths in forms.items()}
    assert out["plain"][0] == seq_lengths()
    for form in out:                                    # the forms hold the same genome
        assert out[form][0] == out["plain"][0] and out[form][1] == out["plain"][1]
        assert all(np.array_equal(a, b) for a, b in zip(out[form][2], out["plain"][2]))
    return out


def same_genome(g, want, what):
    lens, ids, seqs = want
    assert g.nseq == len(lens) and g.lens == lens, what
    assert g.ids == ids, what
    ptrs = g.device_ptrs()
    assert len(ptrs) == g.nseq and all(ptrs), what
    host = g.to_host()
    for k in range(g.nseq):
        assert np.array_equal(host[k], seqs[k]), (what, k, lens[k])
    again = g.to_host()                                 # one download: the same memory again
    assert all(a.ctypes.data == b.ctypes.data for a, b in zip(host, again) if a.size)


@pytest.mark.parametrize("mode", ["default", "blocks", "windows"])
@pytest.mark.parametrize("form,gpu_gzip", [("plain", False), ("gzip", False), ("gzip", True), ("bgzf", False), ("split", False)])
def test_parity_with_the_host_loader(forms, want, form, gpu_gzip, mode, monkeypatch):
    import torch
    from linear_amd.api import Genome
    if mode == "windows":
        monkeypatch.setenv("LNR_READER_GPU_WINDOW", "4096")           # the 40 KiB record: a window is doubled until it holds it
    before = torch.cuda.current_device()
    g = Genome.load_gpu(forms[form], device=0, gpu_gzip=gpu_gzip, block_bases=LONG + 3 if mode == "blocks" else 0)
    same_genome(g, want[form], (form, gpu_gzip, mode))
    assert torch.cuda.current_device() == before
    g.close()


def big_bgzf(rows=1020, small=50, big=1800, nbig=10):
    """(BGZF bytes without the end marker, the line, lengths, ids): a 3 MB record and nbig records of 110 Mb, 1.12 GB of text from copies of
    two compressed blocks (4.9 MB)"""
    rng = random.Random(7)
    line = bytes(rng.choice(b"ACGTacgtNn") for _ in range(60))
    unit = (line + b"\n") * rows                       # one block's text: 62 220 bytes, whole lines
    body = bc.block(unit)
    raw = bc.block(b">first\n") + body * small
    for k in range(nbig):
        raw += bc.block(b">big%d of %d\n" % (k + 1, nbig)) + body * big
    assert (small + nbig * big) * len(unit) > (1 << 30) + (32 << 20) and len(raw) < (32 << 20)
    return raw, line, [small * rows * 60] + [big * rows * 60] * nbig, ["first"] + ["big%d of %d" % (k + 1, nbig) for k in range(nbig)]


def test_bgzf_windows_at_their_largest(lib, tmp_path):
    """Chromosome-sized records in a BGZF file of more than 2^30 bytes of text: the first record (3 MB) doubles the window twice, so every
    window after it asks for the largest a window can be and the chain of blocks stops 64 KiB short of it.  That window holds nine whole
    records; the reader used to refuse it as "a record is longer than the reader's window" before parsing it.  This size is the smallest
    at which it shows: the file is 18 050 copies of two compressed blocks, a few megabytes."""
    from linear_amd.api import Genome
    from tests.test_gpu_reader import d2h
    raw, line, lens, ids = big_bgzf()
    rows = 1020
    path = str(tmp_path / "big.fa.gz")
    with open(path, "wb") as f:
        f.write(raw + bc.EOF_BLOCK)
    g = Genome.load_gpu(path, device=0)
    assert g.lens == lens and g.ids == ids
    tab = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        tab[c] = tab[c + 32] = i
    want_unit = np.tile(tab[np.frombuffer(line, np.uint8)], rows)
    ptrs = g.device_ptrs()
    nbig = len(lens) - 1
    for k in (0, 1, nbig - 1, nbig):                    # head and tail of the first sequences and of the last two (the last lies in a second block)
        assert np.array_equal(d2h(ptrs[k], want_unit.size), want_unit), k
        assert np.array_equal(d2h(ptrs[k] + g.lens[k] - want_unit.size, want_unit.size), want_unit), k
    g.close()


def test_failed_load_leaves_no_device_memory(lib, tmp_path):
    """A load that fails after it has kept blocks: the big file, whole, then a second file with a corrupt block.  By then the genome holds
    the first file's eleven sequences in two allocations (1.1 GB).  Afterwards the device has its memory back: the kept blocks, and the
    readers' block slots (1.25 GiB each) and text buffers.  The bound of 256 MiB is far below any of these and far above what this
    process allocates otherwise in between (nothing)."""
    import torch
    from linear_amd.api import Genome, LnrError
    raw, line, lens, ids = big_bgzf()
    path = str(tmp_path / "big.fa.gz")
    with open(path, "wb") as f:
        f.write(raw + bc.EOF_BLOCK)
    bad, bad_off = bc.corrupt_files(str(tmp_path / "bad"))["crc_flipped"]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    with pytest.raises(LnrError) as e:
        Genome.load_gpu([path, bad], device=0)
    assert e.value.status == -1 and os.path.basename(bad) in str(e.value) and "offset %d" % bad_off in str(e.value), str(e.value)
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free1 > free0 - (256 << 20), (free0, free1)
    # the same after a load that succeeds and is closed
    g = Genome.load_gpu(path, device=0)
    held = torch.cuda.mem_get_info(0)[0]
    assert held < free0 - (900 << 20), (free0, held)   # (the measure sees the genome's blocks: 1.1 GB)
    g.drop_dev()
    with pytest.raises(LnrError) as e:                  # no device pointers any more: an error of the library's kind
        g.build_index(None)
    assert e.value.status == -1
    g.close()
    assert torch.cuda.mem_get_info(0)[0] > free0 - (256 << 20)


@pytest.fixture(scope="module")
def edge_genome(lib, case_inputs, tmp_path_factory):
    """the genome of the golden case `edge` as a 60-column FASTA, loaded on the GPU"""
    from linear_amd.api import Genome
    refs, reads, off = case_inputs("edge")
    tmp = tmp_path_factory.mktemp("gpu_genome_edge")
    _, gp, _, _ = cases.write_fasta_case(tmp, refs, reads, off, width=60)
    g = Genome.load_gpu(gp, device=0)
    yield g
    g.close()


@pytest.mark.parametrize("index_type", [1, 2])
def test_index_from_device_pointers(case_inputs, edge_genome, index_type):
    from linear_amd import Filter
    refs, reads, off = case_inputs("edge")
    T = 3
    assert edge_genome.lens == [r.size for r in refs]
    got, want_ix = Filter(device=0, index_type=index_type), Filter(device=0, index_type=index_type)
    info = edge_genome.build_index(got, T)
    winfo = want_ix.build_index(refs, T)
    assert (info.nseq, info.dir_len, info.hs_len, info.f2_len) == (winfo.nseq, winfo.dir_len, winfo.hs_len, winfo.f2_len)
    a, b = got.index_export(), want_ix.index_export()
    for name, x, y in zip(("dir", "hs", "f2", "f2_off"), a, b):
        assert np.array_equal(x, y), name
    if index_type == 1:                                 # ... which is the reference's
        gold = np.load(os.path.join(GOLD, f"edge_T{T}.npz"))
        assert cases.sha(a[0]) == str(gold["dir_sha"]) and cases.sha(a[1]) == str(gold["hs_sha"])
    else:
        gold = np.load(os.path.join(GOLD, f"edge_i2_T{T}.npz"))
        assert cases.sha(a[1]) == str(gold["ysa_sha"])
    got.close(); want_ix.close()


def test_writer_genome_from_device(case_inputs, edge_genome):
    from linear_amd import Filter
    from linear_amd.api import LnrError, Writer
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    rid, gid = cases.text_ids(n, len(refs))
    flt = Filter(device=0)
    edge_genome.build_index(flt, 3)
    coff, cs, ce = flt.filter_batch(reads, off)
    flt.close()
    w_host = Writer(gid, [r.size for r in refs])
    w_host.set_genome(refs)
    w_host.gpu_open(0)
    want_sam = w_host.format_seq_gpu(coff, cs, ce, reads, off, rid)
    assert want_sam == w_host.format_seq(coff, cs, ce, reads, off, rid) and len(want_sam) > 300_000
    w = Writer(gid, edge_genome.lens)
    with pytest.raises(LnrError) as e:                  # before gpu_open
        w.set_genome_dev(edge_genome.device_ptrs())
    assert e.value.status == -1 and "lnr_writer_gpu_open" in str(e.value)
    w.gpu_open(0)
    w.set_genome_dev(edge_genome.device_ptrs())
    got = w.format_seq_gpu(coff, cs, ce, reads, off, rid)
    assert got == want_sam, diff(want_sam, got)
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    assert w.format_bam_gpu(coff, cs, ce, rl, rid, reads=reads, read_off=off) == w_host.format_bam_gpu(coff, cs, ce, rl, rid, reads=reads, read_off=off)
    with pytest.raises(LnrError) as e:                  # the host forms have no bases
        w.format_seq(coff, cs, ce, reads, off, rid)
    assert e.value.status == -1
    w.set_genome(refs)                                  # host pointers as well: now they have
    assert w.format_seq(coff, cs, ce, reads, off, rid) == want_sam
    w.close(); w_host.close()


@pytest.fixture(scope="module")
def chim_files(lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gpu_genome_cli")
    refs, reads, off = cases.CASES_CLI["chim"]()
    rp, gp, _, _ = cases.write_fasta_case(tmp, refs, reads, off, width=60)
    gz = str(tmp / "ref_bgzf.fa.gz")
    with open(gz, "wb") as f:
        f.write(bc.bgzf(open(gp, "rb").read()))
    return tmp, rp, gp, gz


def run_cli(lib, args):
    p = subprocess.run(["timeout", "-k", "10", "240", lib.CLI, "filter"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-1000:]
    return p.stderr


@pytest.fixture(scope="module")
def base_runs(lib, chim_files):
    """mode -> {".sam", ".apf"} of the run without the switch, once per mode; they are the real program's bytes"""
    from tests.test_cli_golden_cpu import apf_by_read
    tmp, rp, gp, gz = chim_files
    g = np.load(os.path.join(GOLD, "cli_chim.npz"))
    done = {}

    def get(mode):
        if mode not in done:
            err = run_cli(lib, [rp, gp, "-o", str(tmp / ("base_" + mode)), "-t", "1", "-ot", "3"] + cases.CLI_MODES[mode])
            assert b"Genome loaded in" in err
            base = {ext: open(tmp / ("base_" + mode + ext), "rb").read() for ext in (".sam", ".apf")}
            assert base[".sam"] == g[f"sam_{mode}"].tobytes()
            assert apf_by_read(base[".apf"]) == apf_by_read(g[f"apf_{mode}"].tobytes())
            done[mode] = base
        return done[mode]
    return get


@pytest.mark.parametrize("tag", ["fa", "bgzf"])
@pytest.mark.parametrize("mode", ["g0", "gdef"])
def test_front_end_gpu_genome(lib, chim_files, base_runs, mode, tag):
    tmp, rp, gp, gz = chim_files
    base = base_runs(mode)
    out = str(tmp / f"gg_{tag}_{mode}")
    err = run_cli(lib, [rp, gz if tag == "bgzf" else gp, "-o", out, "--gpu-genome", "-t", "1", "-ot", "3"] + cases.CLI_MODES[mode])
    assert b"Genome loaded in" in err and b"--gpu-genome" in err
    for ext in (".sam", ".apf"):
        got = open(out + ext, "rb").read()
        assert got == base[ext], (tag, ext, diff(base[ext], got))


def test_front_end_gpu_genome_device_chain(lib, chim_files):
    """--gpu-genome in front of --gpu-reader --gpu-writer --sam-seq: the writer's genome comes from device memory; the real program's -ss 1 text"""
    tmp, rp, gp, gz = chim_files
    want_sam = np.load(os.path.join(GOLD, "cli_ss_chim.npz"))["sam_g50dup1"].tobytes()
    out = str(tmp / "chain")
    run_cli(lib, [rp, gz, "-t", "1", "-o", out, "--gpu-genome", "--gpu-reader", "--gpu-writer", "--sam-seq"] + cases.CLI_MODES["g50dup1"])
    got = open(out + ".sam", "rb").read()
    assert got == want_sam, diff(want_sam, got)


def test_errors(lib, forms, want, tmp_path):
    from linear_amd.api import Genome, LnrError
    from tests import ubam_cases
    # a BAM as genome
    bam = str(tmp_path / "genome.bam")
    with open(bam, "wb") as f:
        f.write(bc.bgzf(ubam_cases.header() + ubam_cases.record(b"r1", [1, 2, 4, 8, 1, 2, 4, 8])))
    with pytest.raises(LnrError) as e:
        Genome.load_gpu([forms["plain"][0], bam])
    assert e.value.status == -1 and "genome.bam" in str(e.value) and "BAM" in str(e.value)
    # a missing file
    with pytest.raises(LnrError) as e:
        Genome.load_gpu(str(tmp_path / "nothing_here.fa"))
    assert e.value.status == -1 and "nothing_here.fa" in str(e.value)
    # blocks below the longest sequence: LNR_ERR_LIMIT names the file and the record; nothing stays behind (a load after it is clean)
    for form in ("plain", "bgzf"):
        with pytest.raises(LnrError) as e:
            Genome.load_gpu(forms[form], block_bases=LONG - 1)
        assert e.value.status == -6 and os.path.basename(forms[form][0]) in str(e.value) and "record %d" % (len(seq_lengths()) - 1) in str(e.value), str(e.value)
    # a BGZF file with one corrupt block: the reader's LNR_ERR_ARG with the block's file offset
    path, bad_off = bc.corrupt_files(str(tmp_path / "bad"))["crc_flipped"]
    with pytest.raises(LnrError) as e:
        Genome.load_gpu(path)
    assert e.value.status == -1 and "offset %d" % bad_off in str(e.value), str(e.value)
    # drop_dev: no device pointers any more, lengths and ids stay; a host copy taken before stays, too
    g = Genome.load_gpu(forms["plain"])
    host = g.to_host()
    g.drop_dev()
    assert g.device_ptrs() is None
    g2 = Genome(g.lib, g.h)                             # info again, from the object
    assert g2.lens == want["plain"][0] and g2.ids == want["plain"][1]
    g2.h = None
    assert all(np.array_equal(a, b) for a, b in zip(g.to_host(), want["plain"][2])) and len(host) == g.nseq
    g.drop_dev()                                        # again: nothing to do
    g.close()
    g = Genome.load_gpu(forms["plain"])
    g.drop_dev()
    with pytest.raises(LnrError) as e:                  # no host copy was taken before
        g.to_host()
    assert e.value.status == -1
    g.close()
    # no sequence at all: LNR_OK and nseq == 0
    empty = str(tmp_path / "empty.fa")
    open(empty, "wb").write(b"\n\n")
    g = Genome.load_gpu(empty)
    assert g.nseq == 0 and g.lens == [] and g.ids == []
    g.close()
