"""GPU: BAM records encoded on the device (lnr_writer_format_bam_gpu / _dev, k_out_measure<Bam> / k_out_emit<Bam> in
linear_amd/csrc/lnr_output_kernels.hip).  On every shape of tests/bam_cases.py, without and with SEQ: the kernel's bytes == the host form
(lnr_writer_format_bam) == bam_cases.bam_of_sam of the text format_gpu gives; the device form behind a Filter result; with the BGZF switch
on the members walk and inflate to the switch-off bytes; buffer reuse; set_genome / gpu_open in either order; a whole file; the front-end's
-ot 4 / 6 / 8 against the real program's .bam (tests/golden/cli_bam_<case>.npz) and its .sam."""
import gzip
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import bam_cases as bmc, bgzf_cases as bc, cases, deflate_cases as dc, writer_cases as wc, writer_seq_cases as sc
from tests.test_cli_golden_cpu import UB_READS, sam_by_read
from tests.test_output_bam_cpu import by_read, first_diff

pytestmark = pytest.mark.gpu
BLOCK = dc.BLOCK
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TIMES = {"upload_ms", "measure_ms", "scan_ms", "emit_ms", "download_ms"}


@pytest.fixture(scope="module")
def writers():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    made = []

    def make(seq=False, preset=1, open_first=False):
        w = Writer(sc.GIDS, sc.GLEN) if seq else Writer(wc.GIDS, wc.GLEN)
        w.set_preset(preset)
        if open_first:
            w.gpu_open(0)
        if seq:
            w.set_genome(sc.genome())
        if not open_first:
            w.gpu_open(0)
        made.append(w)
        return w
    yield make
    for w in made:
        w.close()


def seq_call(f, batch, **kw):
    coff, cs, ce, reads, off, ids = batch
    return f(coff, cs, ce, None, ids, reads=reads, read_off=off, **kw)


def plain_of(raw, eof):
    return gzip.decompress(raw + eof) if raw else b""


@pytest.mark.parametrize("preset", [1, 2])
def test_without_seq_on_every_shape(writers, preset):
    w = writers(preset=preset)
    for name, batch in bmc.plain_batches():
        host, got = w.format_bam(*batch), w.format_bam_gpu(*batch)
        assert got == host, (name, first_diff(host, got))
        want = bmc.bam_of_sam(w.format_gpu(*batch, "sam"), wc.GIDS)
        assert got == want, (name, first_diff(want, got))
        assert set(w.gpu_times()) == TIMES
    assert w.format_bam_gpu(*wc.empty()) == b""


@pytest.mark.parametrize("preset", [1, 2])
def test_with_seq_on_every_shape(writers, preset):
    w = writers(seq=True, preset=preset)
    for name, batch in bmc.seq_batches():
        host, got = seq_call(w.format_bam, batch), seq_call(w.format_bam_gpu, batch)
        assert got == host, (name, first_diff(host, got))
        want = bmc.bam_of_sam(w.format_seq_gpu(*batch), sc.GIDS)
        assert got == want, (name, first_diff(want, got))
    assert seq_call(w.format_bam_gpu, sc.empty()) == b""
    assert set(bmc.SEQ_LENS) <= {r["l_seq"] for r in bmc.walk_records(seq_call(w.format_bam_gpu, bmc.seq()))}


def test_device_form(case_inputs):
    """behind a Filter result, on device cords and device reads: the host form's bytes, without and with SEQ, switch off and on"""
    import torch
    from linear_amd import Filter
    from linear_amd.api import Writer
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    rid, gid = cases.text_ids(n, len(refs))
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    flt = Filter(device=0)
    flt.build_index(refs, 3)
    d_reads = torch.from_numpy(np.ascontiguousarray(reads, dtype=np.uint8)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = flt.filter_batch_dev(d_reads.data_ptr(), d_off.data_ptr(), n)
    coff, cs, ce = flt.cords_to_host()
    w = Writer(gid, [r.size for r in refs])
    w.gpu_open(0)
    w.set_genome(refs)
    for seq in (False, True):
        host = w.format_bam(coff, cs, ce, None, rid, reads=reads, read_off=off) if seq else w.format_bam(coff, cs, ce, rl, rid)
        call = lambda: w.format_bam_dev(dev, d_off.data_ptr(), rid, d_reads.data_ptr() if seq else None)
        w.set_bgzf(False)
        got = call()
        assert len(host) > 10_000 and got == host, (seq, first_diff(host, got))
        assert got == bmc.bam_of_sam(w.format_seq_dev(dev, d_reads.data_ptr(), d_off.data_ptr(), rid) if seq else w.format_dev(dev, d_off.data_ptr(), rid, "sam"), gid)
        w.set_bgzf(True)
        raw = call()
        assert plain_of(raw, w.bgzf_eof()) == host and w.bgzf_stats()["text_bytes"] == len(host)
    w.close(); flt.close()


def test_switch_on_members_and_stats(writers):
    eof = bc.EOF_BLOCK
    for seq in (False, True):
        w = writers(seq=seq)
        batches = bmc.seq_batches() if seq else bmc.plain_batches()[:4]
        for name, batch in batches:
            call = (lambda: seq_call(w.format_bam_gpu, batch)) if seq else (lambda: w.format_bam_gpu(*batch))
            w.set_bgzf(False)
            want = call()
            w.set_bgzf(True)
            got = call()
            assert plain_of(got, eof) == want, (name, len(got))
            st = w.bgzf_stats()
            assert st["blocks"] == (len(want) + BLOCK - 1) // BLOCK and st["text_bytes"] == len(want) and st["compressed_bytes"] == len(got), (name, st)
            members = bc.walk(got) if got else []
            assert len(members) == st["blocks"] and all(isize <= BLOCK for _, _, isize, _ in members), name
            if want:
                assert st["deflate_ms"] > 0 and st["pack_ms"] > 0 and set(w.gpu_times()) == TIMES
        w.set_bgzf(False)


def test_buffer_reuse(writers):
    """big call, small call, big call, SAM and SEQ forms in between: what a fresh writer gives"""
    big, small = bmc.seq(), sc.one_read()
    fresh = {}
    for b in (big, small):
        f = writers(seq=True)
        fresh[id(b), False] = seq_call(f.format_bam_gpu, b)
        f.set_bgzf(True)
        fresh[id(b), True] = seq_call(f.format_bam_gpu, b)
    w = writers(seq=True)
    for b, on in ((big, False), (small, False), (big, False), (small, True), (big, True), (small, False)):
        w.set_bgzf(on)
        assert seq_call(w.format_bam_gpu, b) == fresh[id(b), on], on
        if b is small:
            w.set_bgzf(False)
            w.format_seq_gpu(*big)                                    # another form through the same buffers
    coff, cs, ce, reads, off, ids = big
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    w.set_bgzf(False)
    assert w.format_bam_gpu(coff, cs, ce, rl, ids) == w.format_bam(coff, cs, ce, rl, ids)        # without SEQ after with


def test_order_of_set_genome_and_gpu_open(writers):
    from linear_amd.api import LnrError, Writer
    batch = sc.one_read()
    a, b = writers(seq=True, open_first=False), writers(seq=True, open_first=True)
    want = seq_call(a.format_bam, batch)
    assert seq_call(a.format_bam_gpu, batch) == want and seq_call(b.format_bam_gpu, batch) == want
    w = Writer(sc.GIDS, sc.GLEN)
    coff, cs, ce, reads, off, ids = batch
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    with pytest.raises(LnrError) as e:                               # before gpu_open
        w.format_bam_gpu(coff, cs, ce, rl, ids)
    assert e.value.status == -1 and "gpu_open" in str(e.value)
    w.gpu_open(0)
    with pytest.raises(LnrError) as e:                               # SEQ without a genome
        seq_call(w.format_bam_gpu, batch)
    assert e.value.status == -1 and "lnr_writer_set_genome" in str(e.value)
    assert w.format_bam_gpu(coff, cs, ce, rl, ids) == w.format_bam(coff, cs, ce, rl, ids)
    w.close()


def test_a_whole_file(writers):
    """header + records + EOF of a batch as the front-end puts them together: inflated, bam_header + the host records"""
    w = writers(seq=True)
    w.set_bgzf(True)
    for pbsv in (False, True):
        raw = w.bgzf_bytes_gpu(w.bam_header("", pbsv)) + seq_call(w.format_bam_gpu, bmc.seq()) + w.bgzf_eof()
        got = gzip.decompress(raw)
        assert got == w.bam_header("", pbsv) + seq_call(w.format_bam, bmc.seq())
        text, refs, recs = bmc.split_bam(got)
        assert refs == [(g.encode(), n) for g, n in zip(sc.GIDS, sc.GLEN)] and (b"@RG\t ID:" in text) == pbsv
        assert len(bmc.walk_records(recs)) > 200 and raw.endswith(bc.EOF_BLOCK)
    w.set_bgzf(False)


# the four combinations of --sam-seq and --gpu-reader in every mode on every case; -ot 6 throughout, -ot 14 (.sam, .bam and _pbsv.bam) once per case
COMBOS = [[], ["--gpu-reader"], ["--sam-seq"], ["--sam-seq", "--gpu-reader"]]
SS_SAM = {"edge": "g0", "chim": "g50dup1"}        # the one mode per case whose `-ss 1` .sam is a golden (cli_ss_<case>.npz); the other modes have the BAM stream's length and sha256


@pytest.mark.parametrize("mode", list(cases.CLI_MODES))
@pytest.mark.parametrize("name", ["edge", "chim"])
def test_front_end(case_inputs, tmp_path, name, mode):
    """linear_filter -ot 6 --gpu-writer [--sam-seq] [--gpu-reader]: the inflated .bam minus its header is the real program's record stream (with
    SEQ: its length and sha256), the header lists the genome, the .sam next to it is the SAM golden; -ot 8: the golden's pbsv header.  One read
    of `edge` at -g > 0 is compared with nothing (tests/test_cli_golden_cpu.py: UB_READS); with --sam-seq that leaves, for `edge` at -g > 0, the
    agreement of the run's .bam with its own .sam (the stream's sha256 covers the excluded read) -- the same records without SEQ are pinned whole
    in the runs without the switch.  The SAM golden with SEQ exists for one mode per case (SS_SAM)."""
    from linear_amd import build as lb
    lb.build()
    refs, reads, off = case_inputs(name)
    g, gs, gss = (np.load(os.path.join(GOLD, f"{k}_{name}.npz")) for k in ("cli_bam", "cli", "cli_ss"))
    rp, gp, _, gid = cases.write_fasta_case(tmp_path, refs, reads, off)
    skip = UB_READS.get((name, mode), set())
    assert f"sam_{SS_SAM[name]}" in gss and f"sam_{mode}" in gs
    for k, extra in enumerate(COMBOS):
        seq, ot = "--sam-seq" in extra, "14" if mode == "g0" and k == 3 else "6"
        pre = str(tmp_path / f"o{k}")
        p = subprocess.run(["timeout", "-k", "10", "240", lb.CLI, "filter", rp, gp, "-t", "1", "-ot", ot, "-o", pre, "--gpu-writer"] + cases.CLI_MODES[mode] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        raw = open(pre + ".bam", "rb").read()
        assert raw.endswith(bc.EOF_BLOCK) and raw.count(bc.EOF_BLOCK) == 1
        text, ref_list, recs = bmc.split_bam(gzip.decompress(raw))
        assert text == g[f"header_{mode}"].tobytes() and ref_list == [(i.encode(), r.size) for i, r in zip(gid, refs)]
        sam = open(pre + ".sam", "rb").read()
        assert recs == bmc.bam_of_sam(sam, gid)                          # the two files of one run say the same
        if not seq:
            want = g[f"recs_{mode}"].tobytes()
            a, b = by_read(recs), by_read(want)
            assert (recs == want or skip) and list(a) == list(b) and all(a[q] == b[q] for q in b if q not in skip), first_diff(want, recs)
            wsam = gs[f"sam_{mode}"].tobytes()
        else:
            if not skip:
                assert len(recs) == int(g[f"ss_len_{mode}"]) and hashlib.sha256(recs).hexdigest() == str(g[f"ss_sha_{mode}"])
            wsam = gss[f"sam_{mode}"].tobytes() if mode == SS_SAM[name] else None
        if wsam is not None:
            (head, got_r), (whead, want_r) = sam_by_read(sam), sam_by_read(wsam)
            assert head == whead and list(got_r) == list(want_r) and all(got_r[q] == want_r[q] for q in want_r if q not in skip)
        if ot == "14":
            raw8 = open(pre + "_pbsv.bam", "rb").read()
            text8, refs8, recs8 = bmc.split_bam(gzip.decompress(raw8))
            assert text8 == g["header_pbsv"].tobytes() and refs8 == ref_list and recs8 == recs and raw8.endswith(bc.EOF_BLOCK)
        if shutil.which("samtools"):                                     # (where it happens to be there: htslib reads the file)
            v = subprocess.run(["samtools", "view", "-h", "--no-PG", pre + ".bam"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert v.returncode == 0 and v.stdout == sam, v.stderr.decode()[-500:]
